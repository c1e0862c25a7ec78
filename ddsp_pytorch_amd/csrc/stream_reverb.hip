// The reverb of a realtime stream (ddsp_hip_stream_reverb): Reverb.forward (modules.py:28-35) over a stream of
// N-sample calls with the impulse response at its full length L, so that the calls' outputs laid end to end are
// (x_all * h)[0 : K N].  Reverb.forward itself crops the IR to the length of its input (a 1024-sample call would
// keep 1024 of 48000 taps), and the reference's realtime chain therefore leaves the reverb to a CPU convolver
// behind the model (export.py:67-72, patches/example.pd:17-19).
//
// Uniformly partitioned overlap-save with the call as the partition (block N, transform 2N, P = ceil(L / N)):
//   IR:      G_p = FFT_2N([h_p, 0]) / 2N                      once per IR (stream_spectrum_kernel)
//   call k:  X_k = FFT_2N([x_{k-1}, x_k])                      written to slot k mod P of the item's ring
//            Y   = sum_{p<P} X_{k-p} G_p                       bins 0..N (real signals: the rest is the conjugate)
//            y_k = last N points of IFFT_2N(Y)
// One launch per call, one workgroup per item: at batch 1 the call is 47 x 1025 complex products at config 3,
// bound by the latency of three dependent phases, not by work.  The workgroup is G thread groups of 2N/16
// threads.  Every group runs the transforms on the same data in the same LDS region (the Stockham passes
// synchronise the whole workgroup, and identical values land on identical addresses), so each group ends with
// X_k in registers in the layout the products need; group g then sums the partitions p = g, g + G, ... from HBM
// and the groups' partial sums meet in LDS, where every thread gathers the inverse transform's input.
// The kernel only reads the call counter (slot = counter mod P); ddsp_hip_stream_advance moves it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "fft_radix.h"
#include "stream_state.h"

namespace ddsp {
namespace {

template <int N2>
struct StreamShape {
  static constexpr int N = N2 / 2;                            // samples per call
  static constexpr int Q = N2 / 16;                           // threads per transform
  static constexpr int NT = Q * 8 < 512 ? (Q * 8 < 64 ? 64 : Q * 8) : 512;  // workgroup
  static constexpr int G = NT / Q;                            // thread groups
  static constexpr int kFft = N2 + N2 / 16;                   // LDS float2 slots of one transform
  static constexpr int kPart = G * (N + 1);                   // the groups' partial sums
  static constexpr int kLds = kFft > kPart ? kFft : kPart;
};

// spec[p][f] = FFT_2N([h[pN, (p+1)N), 0])[f] / 2N for f <= N (taps at or past L are zero); grid (P)
template <int N2>
__global__ void __launch_bounds__(StreamShape<N2>::Q < 64 ? 64 : StreamShape<N2>::Q)
    stream_spectrum_kernel(const float* __restrict__ h, int64_t L, float2* __restrict__ spec) {
  using Sh = StreamShape<N2>;
  constexpr int N = Sh::N, Q = Sh::Q;
  __shared__ float2 lds[Sh::kFft];
  const int t = threadIdx.x % Q, g = threadIdx.x / Q;
  const int64_t p = blockIdx.x;
  const float inv = 1.0f / (float)N2;
  float2 v[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t s = p * N + t + Q * r;
    v[r] = make_float2((r < 8 && s < L) ? h[s] * inv : 0.0f, 0.0f);
  }
  fft_n<N2, false>(v, lds, t);
  if (g != 0) return;
  float2* out = spec + p * (N + 1) + t;
#pragma unroll
  for (int i = 0; i < 8; ++i) out[Q * i] = v[i];
  if (t == 0) out[N] = v[8];
}

// one call of the stream for item blockIdx.x; x and y may be the same buffer (neither is __restrict__, and the
// call's samples are in registers before the first store)
template <int N2>
__global__ void __launch_bounds__(StreamShape<N2>::NT)
    stream_reverb_kernel(const float* x, const float2* __restrict__ spec, const uint64_t* __restrict__ counter,
                         float* __restrict__ hist, float2* __restrict__ ring, float* y, int P) {
  using Sh = StreamShape<N2>;
  constexpr int N = Sh::N, Q = Sh::Q, G = Sh::G, NB1 = N + 1;
  __shared__ float2 lds[Sh::kLds];
  const int t = threadIdx.x % Q, g = threadIdx.x / Q;
  const int64_t b = blockIdx.x;
  const int slot = (int)(*counter % (uint64_t)P);
  float* hb = hist + b * N;
  const float* xb = x + b * N;
  float2* rb = ring + b * (int64_t)P * NB1;

  // X_k = FFT([x_{k-1}, x_k]): v[r] = in[t + Q r], and 8 Q = N
  float2 v[16];
  float xs[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    xs[r] = xb[t + Q * r];
    v[r] = make_float2(hb[t + Q * r], 0.0f);
    v[r + 8] = make_float2(xs[r], 0.0f);
  }
  fft_n<N2, false>(v, lds, t);  // v[i] = X_k[t + Q i]

  // the products: this thread's bins f = t + Q i, i < 8, and bin N at t == 0 (i = 8)
  float2 acc[9];
  if (g == 0) {
    float2* zs = rb + (int64_t)slot * NB1 + t;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      zs[Q * i] = v[i];
      acc[i] = cmul(v[i], spec[t + Q * i]);
    }
    acc[8] = make_float2(0.0f, 0.0f);
    if (t == 0) {
      zs[N] = v[8];
      acc[8] = cmul(v[8], spec[N]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = make_float2(0.0f, 0.0f);
  }
#pragma unroll 2
  for (int p = g == 0 ? G : g; p < P; p += G) {
    const int sp = slot - p < 0 ? slot - p + P : slot - p;  // block k - p (p < P)
    const float2* z = rb + (int64_t)sp * NB1 + t;
    const float2* hp = spec + (int64_t)p * NB1 + t;
    float2 zv[8], hv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      zv[i] = z[Q * i];
      hv[i] = hp[Q * i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float2 m = cmul(zv[i], hv[i]);
      acc[i] = make_float2(acc[i].x + m.x, acc[i].y + m.y);
    }
    if (t == 0) {
      const float2 m = cmul(z[N], hp[N]);
      acc[8] = make_float2(acc[8].x + m.x, acc[8].y + m.y);
    }
  }

  // the groups' partial sums meet in LDS (the transform's region: its last reads are behind the barrier)
  __syncthreads();
  float2* part = lds + g * NB1;
#pragma unroll
  for (int i = 0; i < 8; ++i) part[t + Q * i] = acc[i];
  if (t == 0) part[N] = acc[8];
  __syncthreads();
  // the inverse transform's input Y[t + Q r]: bins past N are the conjugates of their mirror
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int f = t + Q * r, fm = f <= N ? f : N2 - f;
    float2 s = lds[fm];
    for (int gg = 1; gg < G; ++gg) {
      const float2 w = lds[gg * NB1 + fm];
      s = make_float2(s.x + w.x, s.y + w.y);
    }
    v[r] = make_float2(s.x, f <= N ? s.y : -s.y);
  }
  fft_n<N2, true>(v, lds, t);  // (its entry barrier closes the reads above)
  if (g != 0) return;
  float* yb = y + b * N + t;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    yb[Q * r] = v[r + 8].x;
    hb[t + Q * r] = xs[r];
  }
}

int64_t stream_partitions(int64_t N, int64_t L) { return (L + N - 1) / N; }

}  // namespace
}  // namespace ddsp

using namespace ddsp;

extern "C" {

size_t ddsp_hip_stream_state_bytes(int64_t batch, int64_t call_samples, int64_t ir_length) {
  if (batch < 0 || ir_length < 0) return 0;
  if (ir_length > 0 && !stream_block_ok(call_samples)) return 0;
  return stream_layout(batch, call_samples, ir_length).bytes;
}

size_t ddsp_hip_stream_spectrum_floats(int64_t call_samples, int64_t ir_length) {
  if (ir_length < 1 || !stream_block_ok(call_samples)) return 0;
  return (size_t)stream_partitions(call_samples, ir_length) * (size_t)(call_samples + 1) * 2;
}

int ddsp_hip_stream_spectrum(const float* impulse, int64_t ir_length, int64_t call_samples, float* spectrum,
                             size_t spectrum_floats, void* stream) {
  if (!impulse || !spectrum || ir_length < 1 || call_samples < 1) return DDSP_HIP_EINVAL;
  if (!stream_block_ok(call_samples)) return DDSP_HIP_ERANGE;
  const int64_t P = stream_partitions(call_samples, ir_length);
  if (P > INT32_MAX) return DDSP_HIP_ERANGE;
  if (spectrum_floats < ddsp_hip_stream_spectrum_floats(call_samples, ir_length)) return DDSP_HIP_EWORKSPACE;
  return for_frame_length<128>(2 * call_samples, [&](auto size) {  // the transform: two calls long
    constexpr int N2 = decltype(size)::value;
    hipLaunchKernelGGL(stream_spectrum_kernel<N2>, dim3((unsigned)P),
                       dim3(StreamShape<N2>::Q < 64 ? 64 : StreamShape<N2>::Q), 0, S(stream), impulse, ir_length,
                       reinterpret_cast<float2*>(spectrum));
    return launch_status();
  });
}

int ddsp_hip_stream_reverb(const float* x, const float* spectrum, size_t spectrum_floats, const uint64_t* counter,
                           void* state, size_t state_bytes, float* y, int64_t batch, int64_t call_samples,
                           int64_t ir_length, void* stream) {
  if (batch < 0 || call_samples < 1 || ir_length < 1) return DDSP_HIP_EINVAL;
  if (!stream_block_ok(call_samples)) return DDSP_HIP_ERANGE;
  const StreamLayout lay = stream_layout(batch, call_samples, ir_length);
  if (lay.P > INT32_MAX || batch > INT32_MAX) return DDSP_HIP_ERANGE;
  if (batch == 0) return DDSP_HIP_OK;
  if (!x || !spectrum || !counter || !state || !y) return DDSP_HIP_EINVAL;
  if (state_bytes < lay.bytes || spectrum_floats < ddsp_hip_stream_spectrum_floats(call_samples, ir_length))
    return DDSP_HIP_EWORKSPACE;
  char* st = reinterpret_cast<char*>(state);
  return for_frame_length<128>(2 * call_samples, [&](auto size) {
    constexpr int N2 = decltype(size)::value;
    hipLaunchKernelGGL(stream_reverb_kernel<N2>, dim3((unsigned)batch), dim3(StreamShape<N2>::NT), 0, S(stream), x,
                       reinterpret_cast<const float2*>(spectrum), counter, reinterpret_cast<float*>(st + lay.hist),
                       reinterpret_cast<float2*>(st + lay.ring), y, (int)lay.P);
    return launch_status();
  });
}

}  // extern "C"
