// The workgroup roles of the analysis kernels, written once; the kernels are shells around them, each with its own
// __shared__ arrays and its own source of frames (analysis_frames.h):
//   loudness_role    packed_spectrum + loudness_sums   features.hip's loudness kernels, both fused kernels
//   pitch_role       yin_frame                         pitch.hip's kernels, both fused kernels
//   salience_role    yin_dprime + salience_bins (+ yin_pick)   the two salience kernels
//   stream_mfcc_body the streamed MFCC of one call     features.hip's stream_mfcc_kernel, stream_analysis_mfcc.hip
//   mel_rows, workgroup_max                            mel_db_kernel and stream_mfcc_body
//   viterbi_rows                                       the two decode kernels
//   wave_argmin                                        transform_argmin (YIN's pick) and the streamed decode
// with the envelopes and the grid arithmetic that go with them.  stream_analysis.hip and stream_analysis_mfcc.hip
// run the roles side by side in one launch, in different workgroups; since a role has one definition, their bits are
// those of the separate launches.
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

// The loudness role of a workgroup: workgroup `block` of the role takes frames fa = 2 (block TPW + tr) and fa + 1 of
// item b's fetch through one packed transform per transform tr (lds_all: the workgroup's kPoints<N> + kPoints<N>/16
// slots) and writes their loudness to out[b, fa], out[b, fa + 1] (out [B, frames]; red: 8 doubles).  Every thread
// of the workgroup calls this.
template <int N, class Fetch>
__device__ __forceinline__ void loudness_role(const Fetch& fetch, unsigned block, const float* w,
                                              double2* lds_all, double* red, float* out, int b) {
  constexpr int Q = N / 16, TPW = kPoints<N> / N, BINS = N / 2 + 1;
  const int tr = threadIdx.x / Q, t = threadIdx.x - tr * Q;  // thread t of the workgroup's transform tr
  double2* lds = lds_all + tr * (N + N / 16);
  const int frames = fetch.frames;
  const int fa = 2 * (block * TPW + tr);
  packed_spectrum<N>(fetch, fa, t, lds);
  double sa, sb;
  loudness_sums<N>(lds, w, t, tr, red, sa, sb);
  if (t != 0 || fa >= frames) return;
  float* o = out + (int64_t)b * frames + fa;
  o[0] = (float)(sa / (double)BINS);
  if (fa + 1 < frames) o[1] = (float)(sb / (double)BINS);
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

inline PitchParams pitch_params(int64_t tau_min, int64_t tau_max, float sample_rate, float threshold) {
  return {(int)tau_min, (int)tau_max, sample_rate, threshold};
}

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

// The smallest pair over each WIDTH lanes of a wave, valid in the first of them; a fixed order.  Any ints in `mins`
// are each reduced to their smallest beside it, step by step in the same loop (YIN's first candidate).
template <int WIDTH, class... Ints>
__device__ __forceinline__ void wave_argmin(double& v, int& vi, Ints&... mins) {
#pragma unroll
  for (int o = WIDTH / 2; o > 0; o >>= 1) {
    ((mins = min(mins, __shfl_down(mins, o, WIDTH))), ...);
    const double ov = __shfl_down(v, o, WIDTH);
    const int oi = __shfl_down(vi, o, WIDTH);
    take_min(v, vi, ov, oi);
  }
}

// Over the transform's Q threads: first <- the smallest `first`, (best, besti) <- the smallest pair; valid in the
// transform's thread t == 0.  Q > 64: whole waves through LDS (one barrier); every thread of the workgroup calls it.
template <int Q>
__device__ __forceinline__ void transform_argmin(int& first, double& best, int& besti, double* rbest, int* rint,
                                                 int t) {
  constexpr int WIDTH = Q < 64 ? Q : 64;
  wave_argmin<WIDTH>(best, besti, first);
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

// Where yin_dprime leaves d'(tau), tau <= tau_max + 1, in the transform's LDS slots: the second half (the scans' PAD
// doubles come first).
template <int N>
__device__ __forceinline__ double* yin_dp(double2* lds) {
  return reinterpret_cast<double*>(lds) + (N + N / 16);
}

// d'(tau) of frame f of fetch by the transform's Q threads (thread t, LDS slots lds): dn[r] for this thread's lags
// tau = t + Q r, and every tau <= tau_max + 1 at yin_dp<N>(lds)[tau], published by the closing barrier.  Every
// thread of the workgroup calls this.
template <int N, class Fetch>
__device__ __forceinline__ void yin_dprime(const Fetch& fetch, int f, int t, double2* lds, double* wsum,
                                           const PitchParams& p, double (&dn)[9]) {
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
  fft_n<N, false>(v, lds, t);
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
  fft_n<N, false>(v, lds, t);  // (its entry barrier: Z is read)
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
}

// tau* of the frame whose d' yin_dprime left (dn, and LDS): the smallest candidate under the threshold, else the
// smallest index of the minimum; the transform's thread 0 finishes the parabola and writes the frame's outputs to
// slot o of f0 / conf / period when `write`.  Every thread of the workgroup calls this.
template <int N>
__device__ __forceinline__ void yin_pick(const double (&dn)[9], int t, double2* lds, double* wsum, int* rint,
                                         const PitchParams& p, bool write, int64_t o, float* __restrict__ f0,
                                         float* __restrict__ conf, int32_t* __restrict__ period) {
  constexpr int Q = N / 16;
  const double* dp = yin_dp<N>(lds);
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

// Frame f of fetch by the transform's Q threads (thread t, LDS slots lds); the transform's thread 0 writes the
// frame's outputs to slot o of f0 / conf / period when `write`.  Every thread of the workgroup calls this.
template <int N, class Fetch>
__device__ __forceinline__ void yin_frame(const Fetch& fetch, int f, int t, double2* lds, double* wsum, int* rint,
                                          const PitchParams& p, bool write, int64_t o, float* __restrict__ f0,
                                          float* __restrict__ conf, int32_t* __restrict__ period) {
  double dn[9];
  yin_dprime<N>(fetch, f, t, lds, wsum, p, dn);
  yin_pick<N>(dn, t, lds, wsum, rint, p, write, o, f0, conf, period);
}

// The pitch role of a workgroup: workgroup `block` of the role runs yin_frame on frame f = block TPW + tr of item
// b's fetch, one frame per transform tr of lds_all, into slot [b, f] of f0 / conf / period [B, frames] (wsum: 4
// doubles, rint: 8 ints).  Every thread of the workgroup calls this.
template <int N, class Fetch>
__device__ __forceinline__ void pitch_role(const Fetch& fetch, unsigned block, double2* lds_all, double* wsum,
                                           int* rint, const PitchParams& p, int b, float* f0, float* conf,
                                           int32_t* period) {
  constexpr int Q = N / 16;
  const int tr = threadIdx.x / Q, t = threadIdx.x - tr * Q;  // thread t of the workgroup's transform tr
  const int f = block * (kPoints<N> / N) + tr;
  yin_frame<N>(fetch, f, t, lds_all + tr * (N + N / 16), wsum, rint, p, f < fetch.frames,
               (int64_t)b * fetch.frames + f, f0, conf, period);
}

// ---------------- pitch_viterbi: the salience of one frame (include/ddsp_hip.h, "pitch_viterbi") ----------------
constexpr int kMaxBins = 1024;  // n_bins cap: the decodes run one thread per bin
constexpr int kMaxJump = 127;   // max_jump cap: the back-offsets are int8

// The salience of one frame from its d' in LDS (yin_dprime's): bins t, t + Q, ... of the transform's Q threads; the
// offline and the streamed salience kernels (pitch_viterbi.hip, stream_pitch_viterbi.hip) share it.
template <int N>
__device__ __forceinline__ void salience_bins(const double* dp, int t, const PitchParams& p,
                                              const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                              int n_bins, int64_t o, float* __restrict__ cost,
                                              float* __restrict__ f0c, int32_t* __restrict__ lag) {
  constexpr int Q = N / 16;
  for (int i = t; i < n_bins; i += Q) {
    const int l = min(max(lo[i], p.tau_min), p.tau_max);
    const int h = min(max(hi[i], l), p.tau_max);
    int ts = l;
    double b = dp[l];
    for (int tau = l + 1; tau <= h; ++tau) {
      const double v = dp[tau];
      if (v < b) {
        b = v;
        ts = tau;
      }
    }
    const double a = dp[ts - 1], c = dp[ts + 1];
    const double curv = a - 2.0 * b + c;
    double s = 0.0;
    if (b <= a && b <= c && curv > 0.0) s = 0.5 * (a - c) / curv;
    cost[o + i] = (float)fmin(1.0, b);
    f0c[o + i] = (float)((double)p.sample_rate / ((double)ts + s));
    if (lag) lag[o + i] = ts;
  }
}

// The salience role of a workgroup: workgroup `block` takes frame f = block TPW + tr of item b's fetch, one frame per
// transform tr of lds_all: its d', then its bins into cost / f0c / lag [B, frames, n_bins], and, when f0 is given,
// yin_pick on the same d' into f0 / conf / period [B, frames] (the pitch role's bits).  f0 is uniform over the grid,
// as it has to be: yin_pick holds a barrier.  Every thread of the workgroup calls this.
template <int N, class Fetch>
__device__ __forceinline__ void salience_role(const Fetch& fetch, unsigned block, double2* lds_all, double* wsum,
                                              int* rint, const PitchParams& p, int b, const int32_t* lo,
                                              const int32_t* hi, int n_bins, float* cost, float* f0c, int32_t* lag,
                                              float* f0, float* conf, int32_t* period) {
  constexpr int Q = N / 16;
  const int tr = threadIdx.x / Q, t = threadIdx.x - tr * Q;  // thread t of the workgroup's transform tr
  const int f = block * (kPoints<N> / N) + tr;
  double2* lds = lds_all + tr * (N + N / 16);
  double dn[9];
  yin_dprime<N>(fetch, f, t, lds, wsum, p, dn);
  const int64_t o = (int64_t)b * fetch.frames + f;
  if (f < fetch.frames) salience_bins<N>(yin_dp<N>(lds), t, p, lo, hi, n_bins, o * n_bins, cost, f0c, lag);
  if (f0) yin_pick<N>(dn, t, lds, wsum, rint, p, f < fetch.frames, o, f0, conf, period);
}

// ---------------- the decodes' shared pieces (pitch_viterbi.hip, stream_pitch_viterbi.hip) ----------------
constexpr int kViterbiStride = kMaxBins + 2 * kMaxJump;  // doubles per padded row of delta

// The two padded rows (rows: 2 kViterbiStride doubles) set to +inf by the workgroup's nt threads and published.
// Returns the first row's prev: delta(i) lives at prev[i], with prev[-R .. -1] and prev[NB .. NB + R - 1] left +inf
// (no bounds branch in the neighbour loop); the second row's is prev + kViterbiStride.
__device__ __forceinline__ double* viterbi_rows(double* rows, int j, int nt, int R) {
  for (int i = j; i < 2 * kViterbiStride; i += nt) rows[i] = INFINITY;
  __syncthreads();
  return rows + R;
}

// (The neighbour loop of the recursion, min over |k| <= R of prev[j + k] + lam |k|, and the fold of the waves' pairs
// stay written out in the two decode kernels.  The offline decode is latency-bound per frame, and each of its pieces
// tried as a function here changed its code: the neighbour loop, in every form, came out with its exit block after
// the body and a commuted v_add_f64; pitch_viterbi.hip says what wave_argmin and the fold did.)

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

// ---------------- MFCC: mel dB of packed frames, the causal clamp, the DCT ----------------
constexpr int kMaxMels = 256;  // n_mels cap (the band tables live in LDS)
constexpr int kDctFrames = 8;  // frames per workgroup of the DCT launch
constexpr int kDctChunk = 32;  // mel columns of the DCT table staged per pass

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o, 64));
  return v;
}

// The mel rows' band tables into LDS for a workgroup of THREADS threads: s_start / s_count, cut to the spectrum's
// BINS bins, and s_off, the rows' offsets into band_w (an exclusive scan of the counts; thread tid holds rows
// RPT tid ..).  The caller's next barrier publishes them.
template <int THREADS, int BINS>
__device__ __forceinline__ void stage_bands(const int* __restrict__ band_start, const int* __restrict__ band_count,
                                            int n_mels, int* s_start, int* s_count, int* s_off, int* s_wave) {
  constexpr int RPT = kMaxMels / THREADS;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int st[RPT], cnt[RPT], sum = 0;
#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    const int m = RPT * tid + j;
    st[j] = m < n_mels ? min(max(band_start[m], 0), BINS) : 0;
    cnt[j] = m < n_mels ? min(max(band_count[m], 0), 1 << 20) : 0;
    sum += cnt[j];
  }
  int v = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  if (lane == 63) s_wave[wid] = v;
  __syncthreads();
  int off = v - sum;
  for (int i = 0; i < wid; ++i) off += s_wave[i];
#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    const int m = RPT * tid + j;
    s_off[m] = off;
    s_start[m] = st[j];
    s_count[m] = min(cnt[j], BINS - st[j]);
    off += cnt[j];
  }
}

// Mel row m of the two packed frames whose powers are in lds: (10 log10(max(1e-10, energy_a)), the same of b).
__device__ __forceinline__ float2 mel_db_pair(const double2* lds, const float* __restrict__ band_w, int n_w, int s0,
                                              int c, int off) {
  double ea = 0.0, eb = 0.0;
  for (int j = 0; j < c; ++j) {
    const double wj = off + j < n_w ? (double)band_w[off + j] : 0.0;
    const double2 p = lds[lds_idx(s0 + j)];
    ea = fma(wj, p.x, ea);
    eb = fma(wj, p.y, eb);
  }
  return make_float2(10.0f * log10f(fmaxf(1e-10f, (float)ea)), 10.0f * log10f(fmaxf(1e-10f, (float)eb)));
}

// Mel rows t, t + Q, ... (stage_bands' tables) of the two packed frames whose powers are in lds: frame a's to Da[m]
// when va, frame b's to Da[n_mels + m] when vb, and the stored values folded into mx.
template <int N>
__device__ __forceinline__ void mel_rows(const double2* lds, int t, const float* band_w, int n_w,
                                         const int* s_start, const int* s_count, const int* s_off, int n_mels,
                                         bool va, bool vb, float* Da, float& mx) {
  for (int m = t; m < n_mels; m += N / 16) {
    const float2 d = mel_db_pair(lds, band_w, n_w, s_start[m], s_count[m], s_off[m]);
    if (va) {
      Da[m] = d.x;
      mx = fmaxf(mx, d.x);
    }
    if (vb) {
      Da[n_mels + m] = d.y;
      mx = fmaxf(mx, d.y);
    }
  }
}

// The largest mx over a workgroup of WAVES waves (s_max: WAVES floats), valid in thread 0; one barrier.
template <int WAVES>
__device__ __forceinline__ float workgroup_max(float mx, float* s_max) {
  const int tid = threadIdx.x;
  mx = wave_max(mx);
  if ((tid & 63) == 0) s_max[tid >> 6] = mx;
  __syncthreads();
  if (tid == 0) {
    mx = s_max[0];
#pragma unroll
    for (int i = 1; i < WAVES; ++i) mx = fmaxf(mx, s_max[i]);
  }
  return mx;
}

// One pass of the MFCC's loop: frames fa and fa + 1 of the call through the packed transform, then both frames'
// power over the spectrum in place (the thread that owns the pair {k, N-k} writes slot k; no other thread reads k
// or N-k), published by the closing barrier.  Kept out of line on purpose: inlined into the caller's loop over
// passes, this code came out of the compiler wrong on gfx950 for every n_fft whose last FFT stage is not radix-2
// (bin 0 exact, every other bin off by decibels; the same source as a function, or with the loop removed, is
// exact).  The cause in the compiler was not found; tests/test_gpu_stream_features.py covers every size.
// The fetch comes by value, in registers: by reference the caller had to keep it in 48 B of scratch per thread.
template <int N>
__device__ __noinline__ void spectrum_power_pass(const StreamFetch fetch, int fa, int t, double2* lds) {
  constexpr int Q = N / 16, BINS = N / 2 + 1;
  packed_spectrum<N>(fetch, fa, t, lds);
  for (int k = t; k < BINS; k += Q) lds[lds_idx(k)] = packed_power<N>(lds, k);
  __syncthreads();
}

struct MfccTables {
  const int *start, *count;
  const float* w;
  int n_w;
  const float* dct;
  int n_mels, n_mfcc;
  float top_db;
};

// The LDS the streamed MFCC keeps beside the transforms' lds_all.
struct MfccLds {
  float* sD;  // [kStreamMaxFrames * kMaxMels]: the call's D
  int *s_start, *s_count, *s_off;  // [kMaxMels] each
  int* s_wave;   // [waves of the workgroup]
  float* s_max;  // [waves of the workgroup]
  float* s_floor;
};

// The streamed MFCC of one item's call by one workgroup of kPoints<N>/16 threads (features.hip's stream_mfcc_kernel;
// stream_analysis_mfcc.hip's MFCC workgroup): it loops over the call's frame pairs (kPoints/N transforms per pass) as
// mel_db_kernel does, keeping D[frames, n_mels] in LDS; folds the call's largest D with the item's carried maximum
// *runmax (taken as absent when `carried` is false, whatever the stored bits) and stores the result; clamps D at
// that maximum - top_db; and applies the DCT out of LDS as mfcc_dct_kernel does (kDctFrames frames per round, the
// table staged kDctChunk columns at a time in the transforms' LDS, m ascending, fp64 accumulator) into
// out[frames, n_mfcc].  A second run before the advance folds the same call into a maximum that already holds it:
// the same bits.  Every thread of the workgroup calls this.
template <int N>
__device__ __forceinline__ void stream_mfcc_body(const StreamFetch& fetch, bool carried, double2* lds_all,
                                                 const MfccLds& s, const MfccTables& m,
                                                 float* runmax, float* __restrict__ out) {
  constexpr int Q = N / 16, THREADS = kPoints<N> / 16, TPW = kPoints<N> / N, BINS = N / 2 + 1;
  constexpr int WAVES = THREADS / 64, FR = kDctFrames, MC = kDctChunk;
  constexpr int TASKS = FR * kMaxMels / THREADS;  // DCT outputs per thread and round
  static_assert(sizeof(double2) * TPW * (N + N / 16) >= sizeof(float) * kMaxMels * (MC + 1), "the DCT table's LDS");
  float* sT = reinterpret_cast<float*>(lds_all);
  float* sD = s.sD;
  const int frames = fetch.frames, n_mels = m.n_mels, n_mfcc = m.n_mfcc;
  const int tid = threadIdx.x;
  stage_bands<THREADS, BINS>(m.start, m.count, n_mels, s.s_start, s.s_count, s.s_off, s.s_wave);
  const int tr = threadIdx.x / Q, t = threadIdx.x - tr * Q;  // thread t of the workgroup's transform tr
  double2* lds = lds_all + tr * (N + N / 16);
  float mx = -INFINITY;
  for (int f0 = 0; f0 < frames; f0 += 2 * TPW) {
    const int fa = f0 + 2 * tr;
    spectrum_power_pass<N>(fetch, fa, t, lds);  // (its barriers publish s_*)
    const bool va = fa < frames, vb = fa + 1 < frames;
    mel_rows<N>(lds, t, m.w, m.n_w, s.s_start, s.s_count, s.s_off, n_mels, va, vb, sD + (va ? fa : 0) * n_mels, mx);
    __syncthreads();  // the powers consumed before the next pass (or the DCT table) overwrites them
  }
  float r = workgroup_max<WAVES>(mx, s.s_max);
  if (tid == 0) {
    if (carried) r = fmaxf(r, *runmax);
    *runmax = r;
    *s.s_floor = r - m.top_db;
  }
  __syncthreads();
  const float floor_db = *s.s_floor;
  for (int i = tid; i < frames * n_mels; i += THREADS) sD[i] = fmaxf(sD[i], floor_db);
  for (int f0 = 0; f0 < frames; f0 += FR) {
    const int nf = min(FR, frames - f0);
    const int tasks = nf * n_mfcc;  // task o = f * n_mfcc + i, <= THREADS * TASKS
    double acc[TASKS];
#pragma unroll
    for (int j = 0; j < TASKS; ++j) acc[j] = 0.0;
    for (int m0 = 0; m0 < n_mels; m0 += MC) {
      const int mc = min(MC, n_mels - m0);
      __syncthreads();  // the clamp complete (first pass); the previous chunk consumed (later ones)
      for (int idx = tid; idx < n_mfcc * MC; idx += THREADS) {
        const int i = idx / MC, mm = idx - i * MC;
        sT[i * (MC + 1) + mm] = mm < mc ? m.dct[(int64_t)i * n_mels + m0 + mm] : 0.0f;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < TASKS; ++j) {
        const int o = tid + THREADS * j;
        if (o < tasks) {
          const int f = o / n_mfcc, i = o - f * n_mfcc;
          const float* trow = sT + i * (MC + 1);
          const float* dr = sD + (f0 + f) * n_mels + m0;
          double a = acc[j];
          for (int mm = 0; mm < mc; ++mm) a = fma((double)trow[mm], (double)dr[mm], a);
          acc[j] = a;
        }
      }
    }
    float* ot = out + (int64_t)f0 * n_mfcc;
#pragma unroll
    for (int j = 0; j < TASKS; ++j) {
      const int o = tid + THREADS * j;
      if (o < tasks) ot[o] = (float)acc[j];
    }
  }
}

// The MFCC parameters that are invalid whatever the envelope (include/ddsp_hip.h), checked before any HIP call.
inline bool mfcc_params_invalid(int64_t n_band_weights, int64_t n_mels, int64_t n_mfcc, float top_db) {
  return n_band_weights < 0 || n_band_weights > INT32_MAX || !(top_db >= 0.0f) || n_mels < 1 || n_mfcc < 1 ||
         n_mfcc > n_mels;
}

// The streamed MFCC's parameters where nothing is checked between the invalid ones and the n_mels cap
// (ddsp_hip_stream_analysis_mfcc); the streaming envelope is the caller's.
inline int check_stream_mfcc_params(int64_t n_band_weights, int64_t n_mels, int64_t n_mfcc, float top_db) {
  if (mfcc_params_invalid(n_band_weights, n_mels, n_mfcc, top_db)) return DDSP_HIP_EINVAL;
  return n_mels > kMaxMels ? DDSP_HIP_ERANGE : DDSP_HIP_OK;
}

}  // namespace
}  // namespace ddsp
