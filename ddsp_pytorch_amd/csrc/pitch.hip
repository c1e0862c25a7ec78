// On-device pitch tracking: YIN (de Cheveigne & Kawahara 2002) f0 from raw audio x[B, T], frame by frame, offline
// (reflect-padded frames, the loudness's frame count) and per call of a stream (the frames of "streaming analysis").
// include/ddsp_hip.h ("pitch") holds the definition; tests/pitch_ref.py restates it in numpy.
//
// One frame per transform, N = L = frame_length points, W = L/2:
//   E(tau)  from an inclusive fp64 prefix scan of y^2 in LDS: E(tau) = P[tau + W - 1] - P[tau - 1];
//   r(tau)  through the fp64 transform.  One complex FFT of a + i y (a = y[0..W) zero-padded) gives A and Y by the
//           packed split; C = conj(A) Y; r is real, so r = Re FFT(conj C) / N: a second forward transform, one per
//           frame (no pairing of two frames' C in one inverse: two transforms per frame instead of three per two,
//           for a body that has no cross-frame state).  With N = L nothing wraps: j < W and tau <= W keep
//           j + tau < L.  Where E(0) or E(tau) is exactly zero the window is all zeros and r(tau) is exactly zero;
//           it is set so, since the transform returns ~1e-16 of the FRAME's energy there, which no floor relative
//           to E(0) + E(tau) = E(tau) can tell from a small difference (frames that begin before an onset or before
//           the stream);
//   d, S    d = E(0) + E(tau) - 2 r with the 2^-40 floor; S from the same scan; d' = d tau / S;
//   tau*    two index reductions (the smallest candidate under the threshold; the smallest index of the minimum),
//           wave shuffles, then whole waves through LDS; one thread finishes the parabola.
// All of it in fp64 on the fp32 input; outputs fp32 and int32.  Fixed orders, no atomics: two runs give the same
// bits and an item's bits do not depend on the batch around it.  No workgroup loops over frames (one straight pass
// per workgroup), so the transform body is inlined as in loudness_kernel.
//
// A workgroup holds kPoints<N> points as features.hip does: 2048 (128 threads, 2048/N frames) or, for N = 4096, one
// frame of 4096 (256 threads); 34 KB / 68 KB of LDS, used in turn by the transforms, the two scans and d'.  Nothing
// but the transform's own registers lives across the transforms (230 VGPRs at N = 2048: two waves per SIMD).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "analysis_frames.h"

namespace ddsp {
namespace {

constexpr int kPitchMinFrame = 64;  // frame_length envelope [64, 4096]

struct PitchParams {
  int tau_min, tau_max;
  float sample_rate, threshold;
};

// In-place inclusive prefix sums of buf[lds_idx(j)], j < N, by the transform's Q = N/16 threads: thread t sums its
// 16 consecutive entries in order, the threads' totals are scanned (a shuffle scan inside the wave; Q > 64: the
// transform is the whole workgroup and the waves' totals pass through wsum in wave order), and every entry becomes
// (the sum of the threads before) + (the thread's own running sum).  The caller synchronises before and after;
// every thread of the workgroup calls this.
template <int N>
__device__ __forceinline__ void frame_scan(double* buf, double* wsum, int t) {
  constexpr int Q = N / 16, WIDTH = Q < 64 ? Q : 64;
  double x[16], s = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    s += buf[lds_idx(16 * t + i)];
    x[i] = s;
  }
  double incl = s;
  const int lane = t & (WIDTH - 1);
#pragma unroll
  for (int o = 1; o < WIDTH; o <<= 1) {
    const double u = __shfl_up(incl, o, WIDTH);
    if (lane >= o) incl += u;
  }
  const double before = __shfl_up(incl, 1, WIDTH);
  double excl = lane > 0 ? before : 0.0;
  if constexpr (Q > 64) {
    const int wid = t >> 6;
    if (lane == 63) wsum[wid] = incl;
    __syncthreads();
    double off = 0.0;
    for (int i = 0; i < wid; ++i) off += wsum[i];
    excl = off + excl;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) buf[lds_idx(16 * t + i)] = excl + x[i];
}

// The smaller of two (value, index) pairs: the smaller value, the smaller index among equals.
__device__ __forceinline__ void take_min(double& v, int& i, double ov, int oi) {
  if (ov < v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

// Over the transform's Q threads: first <- the smallest `first`, (best, besti) <- the smallest pair; valid in the
// transform's thread t == 0.  Q > 64: whole waves through LDS (one barrier); every thread of the workgroup calls it.
template <int Q>
__device__ __forceinline__ void transform_argmin(int& first, double& best, int& besti, double* rbest, int* rint,
                                                 int t) {
  constexpr int WIDTH = Q < 64 ? Q : 64;
#pragma unroll
  for (int o = WIDTH / 2; o > 0; o >>= 1) {
    first = min(first, __shfl_down(first, o, WIDTH));
    const double ov = __shfl_down(best, o, WIDTH);
    const int oi = __shfl_down(besti, o, WIDTH);
    take_min(best, besti, ov, oi);
  }
  if constexpr (Q > 64) {
    const int lane = t & 63, wid = t >> 6;
    if (lane == 0) {
      rbest[wid] = best;
      rint[2 * wid] = besti;
      rint[2 * wid + 1] = first;
    }
    __syncthreads();
    if (t == 0) {
#pragma unroll
      for (int i = 1; i < Q / 64; ++i) {
        take_min(best, besti, rbest[i], rint[2 * i]);
        first = min(first, rint[2 * i + 1]);
      }
    }
  }
}

// Frame f of fetch by the transform's Q threads (thread t, LDS slots lds); the transform's thread 0 writes the
// frame's outputs to slot o of f0 / conf / period when `write`.  Every thread of the workgroup calls this.
template <int N, class Fetch>
__device__ __forceinline__ void yin_frame(const Fetch& fetch, int f, int t, double2* lds, double* wsum, int* rint,
                                          const PitchParams& p, bool write, int64_t o, float* __restrict__ f0,
                                          float* __restrict__ conf, int32_t* __restrict__ period) {
  constexpr int Q = N / 16, W = N / 2, PAD = N + N / 16;
  double* buf = reinterpret_cast<double*>(lds);  // the scans' PAD doubles (entry j at lds_idx(j))
  double* dp = buf + PAD;                        // d'(tau), tau <= W, in the second half
  // r(tau): Z = FFT(a + i y), C = conj(A) Y, r = Re FFT(conj C) / N
  double2 v[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const double yr = (double)fetch(f, t + Q * r);
    v[r] = make_double2(r < 8 ? yr : 0.0, yr);
  }
  fft_n_f64<N>(v, lds, t);
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) lds[lds_idx(t + Q * r)] = v[r];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int k = t + Q * r;
    double2 a, b;
    packed_split(v[r], lds[lds_idx((N - k) & (N - 1))], a, b);
    v[r] = make_double2(fma(a.x, b.x, a.y * b.y), -fma(a.x, b.y, -(a.y * b.x)));  // conj(conj(A) Y)
  }
  fft_n_f64<N>(v, lds, t);  // (its entry barrier: Z is read)
  double rc[9];             // r(tau) for this thread's lags tau = t + Q r (r <= 8: tau <= W)
#pragma unroll
  for (int r = 0; r < 9; ++r) rc[r] = v[r].x * (1.0 / N);
  __syncthreads();  // the transform's LDS is free

  // E(tau) for the same lags, and E(0).  The samples are fetched a second time (cache hits) rather than kept:
  // anything live across the transforms costs the registers that decide the occupancy
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const double yr = (double)fetch(f, t + Q * r);
    buf[lds_idx(t + Q * r)] = yr * yr;
  }
  __syncthreads();
  frame_scan<N>(buf, wsum, t);
  __syncthreads();
  const double e0 = buf[lds_idx(W - 1)];
  double e[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const int tau = t + Q * r;
    e[r] = 0.0;
    if (tau <= W) e[r] = buf[lds_idx(tau + W - 1)] - (tau > 0 ? buf[lds_idx(tau - 1)] : 0.0);
  }
  __syncthreads();  // the sums are read before d takes their place

  // d(tau) with the floor; 0 at tau = 0 and beyond tau_max + 1, so that the scan gives S(tau) = sum_{k=1..tau} d(k)
  double d[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const int tau = t + Q * r;
    const double rr = (e0 == 0.0 || e[r] == 0.0) ? 0.0 : rc[r];
    const double sum = e0 + e[r];
    double dd = sum - 2.0 * rr;
    if (dd < 0x1p-40 * sum) dd = 0.0;
    d[r] = (tau >= 1 && tau <= p.tau_max + 1) ? dd : 0.0;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) buf[lds_idx(t + Q * r)] = r < 9 ? d[r < 9 ? r : 0] : 0.0;
  __syncthreads();
  frame_scan<N>(buf, wsum, t);
  __syncthreads();

  // d'(tau), tau <= tau_max + 1
  double dn[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const int tau = t + Q * r;
    dn[r] = 1.0;
    if (tau <= p.tau_max + 1) {
      const double s = buf[lds_idx(tau)];
      if (tau > 0 && s > 0.0) dn[r] = d[r] * (double)tau / s;
      dp[tau] = dn[r];
    }
  }
  __syncthreads();

  // tau*: the smallest candidate under the threshold, else the smallest index of the minimum
  const double thr = (double)p.threshold;
  int first = INT_MAX, besti = INT_MAX;
  double best = INFINITY;
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const int tau = t + Q * r;
    if (tau >= p.tau_min && tau <= p.tau_max) {
      const double b = dn[r];
      if (b < dp[tau - 1] && b <= dp[tau + 1] && b < thr) first = min(first, tau);
      take_min(best, besti, b, tau);
    }
  }
  transform_argmin<Q>(first, best, besti, wsum, rint, t);
  if (t != 0 || !write) return;
  const int ts = first != INT_MAX ? first : besti;
  const double a = dp[ts - 1], b = dp[ts], c = dp[ts + 1];
  const double curv = a - 2.0 * b + c;
  double s = 0.0;
  if (b <= a && b <= c && curv > 0.0) s = 0.5 * (a - c) / curv;
  f0[o] = (float)((double)p.sample_rate / ((double)ts + s));
  if (conf) conf[o] = (float)(1.0 - fmin(1.0, b - 0.25 * (a - c) * s));
  if (period) period[o] = ts;
}

// grid (ceil(frames / (kPoints/N)), B), kPoints/16 threads; f0 / conf / period [B, frames]
template <int N>
__global__ void __launch_bounds__(kPoints<N> / 16) pitch_kernel(const float* __restrict__ x, int64_t T, int hop,
                                                                int frames, PitchParams p, float* __restrict__ f0,
                                                                float* __restrict__ conf,
                                                                int32_t* __restrict__ period) {
  constexpr int Q = N / 16, TPW = kPoints<N> / N;
  __shared__ double2 lds_all[TPW * (N + N / 16)];
  __shared__ double wsum[4];
  __shared__ int rint[8];
  const int tr = threadIdx.x / Q, t = threadIdx.x - tr * Q;
  const int b = blockIdx.y;
  const int f = blockIdx.x * TPW + tr;
  yin_frame<N>(ReflectFetch<N>{x + (int64_t)b * T, T, hop, frames}, f, t, lds_all + tr * (N + N / 16), wsum, rint, p,
               f < frames, (int64_t)b * frames + f, f0, conf, period);
}

// grid (ceil(frames / (kPoints/N)), B), kPoints/16 threads; outputs [B, frames].  The item's workgroups share the
// ring copy (analysis_frames.h: no workgroup reads what another writes).
template <int N>
__global__ void __launch_bounds__(kPoints<N> / 16) stream_pitch_kernel(const float* __restrict__ x,
                                                                       const uint64_t* __restrict__ counter,
                                                                       float* ring, int n, int len, int hs, int hop,
                                                                       int frames, PitchParams p,
                                                                       float* __restrict__ f0,
                                                                       float* __restrict__ conf,
                                                                       int32_t* __restrict__ period) {
  constexpr int Q = N / 16, TPW = kPoints<N> / N;
  __shared__ double2 lds_all[TPW * (N + N / 16)];
  __shared__ double wsum[4];
  __shared__ int rint[8];
  const int tr = threadIdx.x / Q, t = threadIdx.x - tr * Q;
  const int b = blockIdx.y;
  const int j = blockIdx.x * TPW + tr;
  const StreamCall call{*counter, n, len, hs, hop, frames};
  float* rb = ring + (int64_t)b * len;
  const float* xb = x + (int64_t)b * n;
  call.store(rb, xb, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
  yin_frame<N>(call.fetch(rb, xb), j, t, lds_all + tr * (N + N / 16), wsum, rint, p, j < frames,
               (int64_t)b * frames + j, f0, conf, period);
}

// The parameters both entry points share (include/ddsp_hip.h), checked before any HIP call.
int check_pitch_params(int64_t L, int64_t tau_min, int64_t tau_max, float sample_rate) {
  if (L < kPitchMinFrame || L > 4096 || (L & (L - 1))) return DDSP_HIP_ERANGE;
  if (tau_min < 1 || tau_min > tau_max || tau_max > L / 2 - 1) return DDSP_HIP_EINVAL;
  if (!(sample_rate > 0.0f)) return DDSP_HIP_EINVAL;
  return DDSP_HIP_OK;
}

unsigned pitch_blocks(int64_t L, int64_t frames) {
  const int64_t per = (L == 4096 ? 4096 : 2048) / L;  // one frame per transform, kPoints/N transforms
  return (unsigned)((frames + per - 1) / per);
}

template <int N>
int pitch_launch(const float* x, int64_t B, int64_t T, int hop, int frames, const PitchParams& p, float* f0,
                 float* conf, int32_t* period, void* stream) {
  hipLaunchKernelGGL(pitch_kernel<N>, dim3(pitch_blocks(N, frames), (unsigned)B), dim3(kPoints<N> / 16), 0, S(stream),
                     x, T, hop, frames, p, f0, conf, period);
  return launch_status();
}

template <int N>
int stream_pitch_launch(const StreamArgs& a, const PitchParams& p, float* f0, float* conf, int32_t* period) {
  hipLaunchKernelGGL(stream_pitch_kernel<N>, dim3(pitch_blocks(N, a.frames), (unsigned)a.B), dim3(kPoints<N> / 16), 0,
                     S(a.stream), a.x, a.counter, a.ring, a.n, a.len, a.hs, a.hop, a.frames, p, f0, conf, period);
  return launch_status();
}

#define DDSP_FOR_FRAME_LENGTH(L, CALL) \
  switch (L) {                         \
    case 64: return CALL(64);          \
    case 128: return CALL(128);        \
    case 256: return CALL(256);        \
    case 512: return CALL(512);        \
    case 1024: return CALL(1024);      \
    case 2048: return CALL(2048);      \
    default: return CALL(4096);        \
  }

int pitch_dispatch(const float* x, int64_t B, int64_t T, int64_t L, int hop, int frames, const PitchParams& p,
                   float* f0, float* conf, int32_t* period, void* stream) {
#define DDSP_CALL(N) pitch_launch<N>(x, B, T, hop, frames, p, f0, conf, period, stream)
  DDSP_FOR_FRAME_LENGTH(L, DDSP_CALL)
#undef DDSP_CALL
}

int stream_pitch_dispatch(const StreamArgs& a, int64_t L, const PitchParams& p, float* f0, float* conf,
                          int32_t* period) {
#define DDSP_CALL(N) stream_pitch_launch<N>(a, p, f0, conf, period)
  DDSP_FOR_FRAME_LENGTH(L, DDSP_CALL)
#undef DDSP_CALL
}

}  // namespace
}  // namespace ddsp

using namespace ddsp;

extern "C" {

int ddsp_hip_pitch(const float* x, float* f0, float* confidence, int32_t* period, int64_t batch, int64_t n_samples,
                   int64_t frame_length, int64_t hop, int64_t tau_min, int64_t tau_max, float sample_rate,
                   float threshold, void* stream) {
  if (batch < 0 || n_samples < 1 || hop < 1 || frame_length < 1) return DDSP_HIP_EINVAL;
  const int st = check_pitch_params(frame_length, tau_min, tau_max, sample_rate);
  if (st) return st;
  if (frame_length / 2 >= n_samples) return DDSP_HIP_EINVAL;  // reflect padding, as ddsp_hip_loudness
  if (batch > 65535 || n_samples / hop + 1 > INT32_MAX) return DDSP_HIP_ERANGE;
  if (batch == 0) return DDSP_HIP_OK;
  if (!x || !f0) return DDSP_HIP_EINVAL;
  const int frames = (int)(n_samples / hop);
  if (frames == 0) return DDSP_HIP_OK;
  const PitchParams p{(int)tau_min, (int)tau_max, sample_rate, threshold};
  return pitch_dispatch(x, batch, n_samples, frame_length, (int)hop, frames, p, f0, confidence, period, stream);
}

int ddsp_hip_stream_pitch(const float* x, float* f0, float* confidence, int32_t* period, const uint64_t* counter,
                          void* state, size_t state_bytes, int64_t batch, int64_t call_samples, int64_t frame_length,
                          int64_t hop, int64_t tau_min, int64_t tau_max, float sample_rate, float threshold,
                          void* stream) {
  StreamSizes sz;
  int st = check_stream_features(batch, call_samples, frame_length, hop, &sz);
  if (st) return st;
  st = check_pitch_params(frame_length, tau_min, tau_max, sample_rate);
  if (st) return st;
  if (batch == 0) return DDSP_HIP_OK;
  if (!x || !f0 || !counter || !state) return DDSP_HIP_EINVAL;
  if (state_bytes < stream_features_bytes(batch, sz)) return DDSP_HIP_EWORKSPACE;
  const StreamArgs a{x, counter, reinterpret_cast<float*>(state), batch, (int)call_samples, (int)sz.len, (int)sz.hs,
                     (int)hop, (int)sz.frames, stream};
  const PitchParams p{(int)tau_min, (int)tau_max, sample_rate, threshold};
  return stream_pitch_dispatch(a, frame_length, p, f0, confidence, period);
}

}  // extern "C"
