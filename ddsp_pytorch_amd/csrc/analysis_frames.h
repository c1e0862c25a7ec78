// What the analysis kernels share (features.hip: loudness, MFCC; pitch.hip: YIN f0): where a frame's samples come
// from, offline (reflect padding) and per call of a stream (the carried ring), the call arithmetic of a stream and its
// opening (open_stream_call), how a workgroup's threads split over its transforms, the identities
// by which two real sequences ride one complex fp64 transform, and that transform's twiddle table.  Written once, so
// that the features cannot disagree about a frame.  (analysis_bodies.h holds what is computed per frame: the
// workgroup roles.)
//
// Why fft_n runs on double2 here ("Why the transform is fp64"): the features take the LOG of single bins,
// so a bin near a spectral zero multiplies the transform's absolute error by 1/|X|, and reflect padding makes such
// bins common.  In fp64 the transform's error vanishes beside the fp32 input's; MI355X issues fp64 FMAs at the rate
// of unpacked fp32 ones, so the cost is LDS traffic (16-byte elements) and registers, not arithmetic.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"
#include "fft_radix.h"
#include "stft_frames.h"
#include "twiddle4096_f64.inc"

namespace ddsp {
namespace {

// W_4096^m in fp64 (tools/gen_twiddles.py 4096 f64), each twiddle read from the table
template <>
struct TwiddleTable<double2> {
  static __device__ __forceinline__ const double2* data() { return reinterpret_cast<const double2*>(kTwiddle4096D); }
};

template <int N>
constexpr int kPoints = N == 4096 ? 4096 : 2048;  // points per workgroup; threads = points / 16

// A workgroup's threads split over its kPoints<N>/N transforms, Q = N/16 threads each: thread t = threadIdx.x - tr * Q
// of transform tr = threadIdx.x / Q, whose LDS slots (N + N/16 double2: lds_idx's padding) start at
// lds_all + tr * (N + N/16).  The roles of analysis_bodies.h spell this line out: gathered in a struct, handed back
// through references, or with t behind a function, the same arithmetic came out of the compiler with other register
// counts in kernels around it (gfx950: loudness_kernel<32> and the kernels of N = 512).

// Where a frame's samples come from: fetch(f, i) is sample i (0 <= i < N) of frame f's N-sample window, 0.0f for a
// frame the caller does not have.  Offline: frame f of row xr[T] is centred at f * hop with reflect padding.
template <int N>
struct ReflectFetch {
  const float* __restrict__ xr;
  int64_t T;
  int hop, frames;
  __device__ __forceinline__ float operator()(int f, int i) const {
    return f < frames ? reflect_load(xr, T, (int64_t)f * hop + i - N / 2) : 0.0f;
  }
};

// One call of a stream (include/ddsp_hip.h, "streaming analysis"): call k holds the samples [kN, (k+1)N) of the
// stream in xc; the hs samples before them are in the item's ring of len >= hs + n floats, sample s at s mod len;
// samples before the stream's start are zero.  The call's frame j (0 <= j < frames) starts rel0 + j * hop samples
// from the call's first sample (rel0 = -hs), so every index rel below lies in [-hs, n).
struct StreamFetch {
  const float* __restrict__ ring;  // the item's ring
  const float* __restrict__ xc;    // the item's call input [n]
  int base;                        // (k n) mod len: the ring position of the call's first sample
  int len, first;                  // first: the smallest rel that lies inside the stream, max(-hs, -k n)
  int rel0, hop, frames;
  __device__ __forceinline__ float operator()(int j, int i) const {
    if (j >= frames) return 0.0f;
    const int rel = rel0 + j * hop + i;
    if (rel >= 0) return xc[rel];
    if (rel < first) return 0.0f;
    const int p = base + rel;
    return ring[p < 0 ? p + len : p];
  }
};

// Frames fa and fa + 1 of fetch, windowed (periodic Hann(N) from the fp64 table), through one complex FFT;
// on return this transform's LDS slots hold Z (index k at lds_idx(k)) and the workgroup is synchronised.
template <int N, class Fetch>
__device__ __forceinline__ void packed_spectrum(const Fetch& fetch, int fa, int t, double2* lds) {
  constexpr int Q = N / 16, STEP = 4096 / N;
  double2 v[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = t + Q * r;
    const double w = 0.5 - 0.5 * kTwiddle4096D[2 * ((m * STEP) & 4095)];
    const double a = (double)fetch(fa, m) * w;
    const double b = (double)fetch(fa + 1, m) * w;
    v[r] = make_double2(a, b);
  }
  fft_n<N, false, false>(v, lds, t);  // lds untouched so far
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) lds[lds_idx(t + Q * r)] = v[r];
  __syncthreads();
}

// The spectra of the two real sequences packed as z = a + i b, from zk = Z[k] and zn = Z[N-k]:
// X_a = (Z[k] + conj(Z[N-k])) / 2,  X_b = (Z[k] - conj(Z[N-k])) / (2i)
__device__ __forceinline__ void packed_split(double2 zk, double2 zn, double2& xa, double2& xb) {
  xa = make_double2(0.5 * (zk.x + zn.x), 0.5 * (zk.y - zn.y));
  xb = make_double2(0.5 * (zk.y + zn.y), -0.5 * (zk.x - zn.x));
}

// |X_a[k]|^2 and |X_b[k]|^2 of the two packed frames
template <int N>
__device__ __forceinline__ double2 packed_power(const double2* lds, int k) {
  double2 xa, xb;
  packed_split(lds[lds_idx(k)], lds[lds_idx((N - k) & (N - 1))], xa, xb);
  return make_double2(fma(xa.x, xa.x, xa.y * xa.y), fma(xb.x, xb.x, xb.y * xb.y));
}

// ---------------- streaming analysis: one call of a stream (include/ddsp_hip.h) ----------------
// Call k = *counter holds samples [k n, (k+1) n) and emits the frames = n / hop frames f = k frames - d + 1 + j,
// d = ceil((N/2) / hop): those whose windows the call completes.  Frame j's window starts hs = (d-1) hop + N/2
// samples before the call plus j hop, so a call reads [k n - hs, k n) from the item's ring (len = hs + n floats,
// sample s at s mod len) and the rest from its input, and writes its input over the ring's [k n, (k+1) n) — n
// positions that, modulo len, are exactly the ones the hs read positions leave free.  No workgroup reads what
// another writes: the copy needs no ordering, and a call run twice before the advance reads and writes the same
// values.  The kernels read the counter; ddsp_hip_stream_advance moves it.
constexpr int kStreamMaxFrames = 32;  // frames per call (the MFCC keeps the call's D in LDS)

struct StreamCall {
  uint64_t k;
  int n, len, hs, hop, frames;
  // the ring position of the call's first sample: (k n) mod len without a 64-bit overflow
  __device__ __forceinline__ int base() const {
    return (int)(((k % (uint64_t)len) * (uint64_t)n) % (uint64_t)len);
  }
  __device__ __forceinline__ StreamFetch fetch(const float* ring_b, const float* x_b) const {
    // k n >= hs once k >= ceil(hs / n); before that the stream starts k n (< hs + n) samples back
    const int first = k >= (uint64_t)((hs + n - 1) / n) ? -hs : -(int)k * n;
    return StreamFetch{ring_b, x_b, base(), len, first, -hs, hop, frames};
  }
  // thread `i0` of `stride` copies its share of the call's input into the ring
  __device__ __forceinline__ void store(float* ring_b, const float* __restrict__ x_b, int i0, int stride) const {
    const int p0 = base();
    for (int i = i0; i < n; i += stride) {
      const int p = p0 + i;
      ring_b[p >= len ? p - len : p] = x_b[i];
    }
  }
};

// How every streamed kernel opens call k (the counter's value) for item b: thread `i0` of the `stride` that share the
// item copies its share of the call's input into the ring, and the item's fetch comes back.  A role whose window is
// shorter than the ring's moves the fetch's rel0 forward.
__device__ __forceinline__ StreamFetch open_stream_call(uint64_t k, float* ring, const float* __restrict__ x, int n,
                                                        int len, int hs, int hop, int frames, int b, int i0,
                                                        int stride) {
  const StreamCall call{k, n, len, hs, hop, frames};
  float* rb = ring + (int64_t)b * len;
  const float* xb = x + (int64_t)b * n;
  call.store(rb, xb, i0, stride);
  return call.fetch(rb, xb);
}

// The streaming envelope (include/ddsp_hip.h) and the sizes it implies.
struct StreamSizes {
  int64_t frames, hs, len;  // frames per call, carried samples, ring floats per item
};

inline int check_stream_features(int64_t B, int64_t n, int64_t n_fft, int64_t hop, StreamSizes* sz) {
  if (B < 0 || n < 1 || hop < 1 || n_fft < 1 || n % hop) return DDSP_HIP_EINVAL;
  if (n_fft < 16 || n_fft > 4096 || (n_fft & (n_fft - 1))) return DDSP_HIP_ERANGE;
  if (n / hop > kStreamMaxFrames || B > 65535 || n > (1 << 24)) return DDSP_HIP_ERANGE;
  const int64_t d = (n_fft / 2 + hop - 1) / hop;
  sz->frames = n / hop;
  sz->hs = (d - 1) * hop + n_fft / 2;  // < n_fft: (d - 1) hop < n_fft / 2
  sz->len = sz->hs + n;
  return DDSP_HIP_OK;
}

inline size_t stream_features_bytes(int64_t B, const StreamSizes& sz) {  // the rings, then one float per item
  return (sizeof(float) * (size_t)B * (size_t)(sz.len + 1) + 15) / 16 * 16;
}

struct StreamArgs {
  const float* x;
  const uint64_t* counter;
  float* ring;
  int64_t B;
  int n, len, hs, hop, frames;
  void* stream;
};

// One call's StreamArgs from the sizes check_stream_features gave (host); the ring starts the state.
inline StreamArgs stream_args(const float* x, const uint64_t* counter, void* state, int64_t B, int64_t n, int64_t hop,
                              const StreamSizes& sz, void* stream) {
  return {x, counter, reinterpret_cast<float*>(state), B, (int)n, (int)sz.len, (int)sz.hs, (int)hop, (int)sz.frames,
          stream};
}

}  // namespace
}  // namespace ddsp
