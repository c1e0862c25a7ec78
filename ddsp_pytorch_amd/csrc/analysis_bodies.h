// The per-frame bodies of the analysis kernels, written once: the loudness's reduction over a packed spectrum
// (features.hip's loudness kernels) and the YIN estimator of one frame (pitch.hip's kernels), with the envelope and
// the grid arithmetic that go with them.  stream_analysis.hip runs both side by side in one launch, in different
// workgroups; since the bodies are these, its bits are those of the separate launches.
#pragma once

#include <climits>
#include <cmath>

#include "analysis_frames.h"

namespace ddsp {
namespace {

// ---------------- loudness: the bins of two packed frames ----------------
// Sums of a and b over the Q threads of one transform, valid in its thread t == 0; fixed order.
// Q < 64: a shuffle tree inside the wave.  Q >= 64: whole waves (group_sum_double2, one barrier — every
// thread of the workgroup calls this either way).
template <int Q>
__device__ __forceinline__ void transform_sum2(double& a, double& b, double* scratch, int tr) {
  if constexpr (Q >= 64) {
    group_sum_double2(a, b, scratch, tr * (Q / 64), Q / 64);
  } else {
#pragma unroll
    for (int o = Q / 2; o > 0; o >>= 1) {
      a += __shfl_down(a, o, Q);
      b += __shfl_down(b, o, Q);
    }
  }
}

// The two packed frames' sums over the bins of ln(|X[k]| + 1e-7) + w[k] (fp32 log, fp64 sum in a fixed order), valid
// in the transform's thread t == 0; every thread of the workgroup calls this.
template <int N>
__device__ __forceinline__ void loudness_sums(const double2* lds, const float* __restrict__ w, int t, int tr,
                                              double* red, double& sa, double& sb) {
  constexpr int Q = N / 16, BINS = N / 2 + 1;
  sa = 0.0;
  sb = 0.0;
  for (int k = t; k < BINS; k += Q) {
    const double2 p = packed_power<N>(lds, k);
    const float wk = w ? w[k] : 0.0f;
    sa += (double)(logf((float)sqrt(p.x) + 1e-7f) + wk);
    sb += (double)(logf((float)sqrt(p.y) + 1e-7f) + wk);
  }
  transform_sum2<Q>(sa, sb, red, tr);
}

// two frames per transform, kPoints/N transforms per workgroup
inline unsigned frame_blocks(int64_t n_fft, int64_t frames) {
  const int64_t per = 2 * ((n_fft == 4096 ? 4096 : 2048) / n_fft);
  return (unsigned)((frames + per - 1) / per);
}

// ---------------- pitch: YIN of one frame (include/ddsp_hip.h, "pitch") ----------------
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

// The parameters the pitch entry points share (include/ddsp_hip.h), checked before any HIP call.
inline int check_pitch_params(int64_t L, int64_t tau_min, int64_t tau_max, float sample_rate) {
  if (L < kPitchMinFrame || L > 4096 || (L & (L - 1))) return DDSP_HIP_ERANGE;
  if (tau_min < 1 || tau_min > tau_max || tau_max > L / 2 - 1) return DDSP_HIP_EINVAL;
  if (!(sample_rate > 0.0f)) return DDSP_HIP_EINVAL;
  return DDSP_HIP_OK;
}

// one frame per transform, kPoints/N transforms per workgroup
inline unsigned pitch_blocks(int64_t L, int64_t frames) {
  const int64_t per = (L == 4096 ? 4096 : 2048) / L;
  return (unsigned)((frames + per - 1) / per);
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

}  // namespace
}  // namespace ddsp
