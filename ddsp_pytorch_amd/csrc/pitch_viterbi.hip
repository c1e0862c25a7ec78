// Viterbi-decoded pitch: a salience per frame over log-spaced lag bins from YIN's d' (one launch), then a min-plus
// decode over time (one launch).  include/ddsp_hip.h ("pitch_viterbi") holds the definition; tests/viterbi_ref.py
// restates it in numpy.
//
// Salience: pitch_kernel's grid and workgroup around salience_role (analysis_bodies.h): the frame's d' by yin_dprime
// (the first part of yin_frame), then the transform's Q threads take bins t, t + Q, ..., each scanning its few lags of
// d' in LDS and finishing the parabola.  With the raw outputs asked for, yin_pick runs on the same d': ddsp_hip_pitch's
// bits.
//
// Decode: one workgroup per item, one thread per bin.  delta lives in LDS as two fp64 rows with R entries of +inf
// on each side (viterbi_rows; no bounds branch in the neighbour loop), written in turn: one barrier per frame;
// the rows' set-up (viterbi_rows) is analysis_bodies.h's, shared with stream_pitch_viterbi.hip.  The next frame's
// cost is loaded before the barrier, off the dependent chain.  Back-offsets i - j go to the workspace as int8; the
// backtrack stages them into LDS in chunks of viterbi_chunk_frames(n_bins) frames (coalesced), one thread walks the
// chunk in LDS, and all threads gather and store the chunk's path, f0 and confidence.  Fixed orders, no atomics.
// The decode is latency-bound by design (F barriers per item): a preprocessing step, not a training loop.
#include <hip/hip_runtime.h>

#include "analysis_bodies.h"

namespace ddsp {
namespace {

constexpr int kViterbiChunkBytes = 32 * 1024;  // back-offsets staged per backtrack chunk
constexpr int kViterbiMaxChunk = 512;          // frames per chunk at most (the chunk's path in LDS)

// frames per backtrack chunk at n_bins in [1, kMaxBins]
__host__ __device__ inline int viterbi_chunk_frames(int n_bins) {
  const int g = kViterbiChunkBytes / n_bins;
  return g < kViterbiMaxChunk ? g : kViterbiMaxChunk;
}

// grid (ceil(frames / (kPoints/N)), B), kPoints/16 threads; cost / f0c / lag [B, frames, n_bins], f0 / conf /
// period [B, frames] (f0 == nullptr: the pick is not run)
template <int N>
__global__ void __launch_bounds__(kPoints<N> / 16) pitch_salience_kernel(
    const float* __restrict__ x, int64_t T, int hop, int frames, PitchParams p, const int32_t* __restrict__ lo,
    const int32_t* __restrict__ hi, int n_bins, float* __restrict__ cost, float* __restrict__ f0c,
    int32_t* __restrict__ lag, float* __restrict__ f0, float* __restrict__ conf, int32_t* __restrict__ period) {
  constexpr int TPW = kPoints<N> / N;
  __shared__ double2 lds_all[TPW * (N + N / 16)];
  __shared__ double wsum[4];
  __shared__ int rint[8];
  const int b = blockIdx.y;
  salience_role<N>(ReflectFetch<N>{x + (int64_t)b * T, T, hop, frames}, blockIdx.x, lds_all, wsum, rint, p, b, lo, hi,
                   n_bins, cost, f0c, lag, f0, conf, period);
}

// grid B, n_bins rounded up to whole waves; ws [B, frames, n_bins] int8
__global__ void __launch_bounds__(kMaxBins) pitch_viterbi_kernel(
    const float* __restrict__ cost, const float* __restrict__ f0c, float* __restrict__ f0, float* __restrict__ conf,
    int32_t* __restrict__ path, int8_t* ws, int frames, int NB, int R, float transition) {
  __shared__ double rows[2 * kViterbiStride];
  __shared__ int8_t chunk[kViterbiChunkBytes];
  __shared__ int32_t cpath[kViterbiMaxChunk];
  __shared__ double rbest[kMaxBins / 64];
  __shared__ int rbesti[kMaxBins / 64];
  const int j = threadIdx.x, nt = blockDim.x;
  const bool active = j < NB;
  const int64_t base = (int64_t)blockIdx.x * frames;  // the item's first frame
  const float* cb = cost + base * NB;
  int8_t* wb = ws + base * NB;
  const double lam = (double)transition;

  double* prev = viterbi_rows(rows, j, nt, R);
  double* cur = prev + kViterbiStride;
  float c = 0.0f;
  if (active) {
    prev[j] = (double)cb[j];
    wb[j] = 0;
    if (frames > 1) c = cb[NB + j];
  }
  __syncthreads();
  for (int t = 1; t < frames; ++t) {
    float cn = 0.0f;
    if (active && t + 1 < frames) cn = cb[(int64_t)(t + 1) * NB + j];  // off the chain: used after the barrier
    if (active) {
      double best = INFINITY;
      int bk = 0;
      for (int k = -R; k <= R; ++k) {  // i = j + k ascending: the smallest i among equals
        const double v = prev[j + k] + lam * (double)abs(k);
        if (v < best) {
          best = v;
          bk = k;
        }
      }
      cur[j] = best + (double)c;
      wb[(int64_t)t * NB + j] = (int8_t)bk;
    }
    __syncthreads();
    double* sw = prev;
    prev = cur;
    cur = sw;
    c = cn;
  }

  // path(F-1): the smallest argmin of the last row, a fixed-order reduction.  wave_argmin<64>'s loop and the fold of
  // the waves' pairs, written out: through the functions this one-off code came out one instruction longer, the
  // backtrack's loops below moved by four bytes, and the decode measured 0.4 % slower on gfx950 (per frame, so the
  // walk); written out, the kernel's code is what it was before the pieces were shared.
  double best = active ? prev[j] : INFINITY;
  int besti = active ? j : INT_MAX;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_down(best, o, 64);
    const int oi = __shfl_down(besti, o, 64);
    take_min(best, besti, ov, oi);
  }
  if ((j & 63) == 0) {
    rbest[j >> 6] = best;
    rbesti[j >> 6] = besti;
  }
  __syncthreads();  // (also: every back-offset of the item is written)
  int s = 0;
  if (j == 0) {
    for (int i = 1; i < (nt >> 6); ++i) take_min(best, besti, rbest[i], rbesti[i]);
    s = min(max(besti, 0), NB - 1);
  }

  // the backtrack, chunk by chunk from the end
  const int G = viterbi_chunk_frames(NB);
  for (int t0 = ((frames - 1) / G) * G; t0 >= 0; t0 -= G) {
    const int n = min(G, frames - t0);
    const int8_t* src = wb + (int64_t)t0 * NB;
    for (int i = j; i < n * NB; i += nt) chunk[i] = src[i];
    __syncthreads();
    if (j == 0) {
      for (int u = n - 1; u >= 0; --u) {
        cpath[u] = s;
        if (t0 + u > 0) s = min(max(s + (int)chunk[u * NB + s], 0), NB - 1);  // bp_t(path(t)) = path(t - 1)
      }
    }
    __syncthreads();
    for (int u = j; u < n; u += nt) {
      const int64_t o = base + t0 + u;
      const int st = cpath[u];
      path[o] = st;
      f0[o] = f0c[o * NB + st];
      if (conf) conf[o] = 1.0f - cost[o * NB + st];
    }
    __syncthreads();  // the chunk and its path are consumed before the next one takes their place
  }
}

int launch_salience(const float* x, int64_t B, int64_t T, int64_t L, int hop, int frames, const PitchParams& p,
                    const int32_t* lo, const int32_t* hi, int n_bins, float* cost, float* f0c, int32_t* lag,
                    float* f0, float* conf, int32_t* period, void* stream) {
  return for_frame_length<kPitchMinFrame>(L, [&](auto size) {
    constexpr int N = decltype(size)::value;
    hipLaunchKernelGGL(pitch_salience_kernel<N>, dim3(pitch_blocks(N, frames), (unsigned)B), dim3(kPoints<N> / 16), 0,
                       S(stream), x, T, hop, frames, p, lo, hi, n_bins, cost, f0c, lag, f0, conf, period);
    return launch_status();
  });
}

// The decode's sizes (include/ddsp_hip.h), checked before any HIP call.
inline int check_viterbi_sizes(int64_t batch, int64_t frames, int64_t n_bins) {
  if (batch < 0 || frames < 0 || n_bins < 1) return DDSP_HIP_EINVAL;
  if (n_bins > kMaxBins || batch > INT32_MAX || frames > INT32_MAX) return DDSP_HIP_ERANGE;
  return DDSP_HIP_OK;
}

}  // namespace
}  // namespace ddsp

using namespace ddsp;

extern "C" {

int ddsp_hip_pitch_salience(const float* x, const int32_t* lo, const int32_t* hi, float* cost, float* f0c,
                            int32_t* lag, float* f0, float* confidence, int32_t* period, int64_t batch,
                            int64_t n_samples, int64_t frame_length, int64_t hop, int64_t tau_min, int64_t tau_max,
                            int64_t n_bins, float sample_rate, float threshold, void* stream) {
  if (batch < 0 || n_samples < 1 || hop < 1 || frame_length < 1 || n_bins < 1) return DDSP_HIP_EINVAL;
  const int st = check_pitch_params(frame_length, tau_min, tau_max, sample_rate);
  if (st) return st;
  if (frame_length / 2 >= n_samples) return DDSP_HIP_EINVAL;  // reflect padding, as ddsp_hip_pitch
  if (!f0 && (confidence || period)) return DDSP_HIP_EINVAL;
  if (n_bins > kMaxBins || batch > 65535 || n_samples / hop + 1 > INT32_MAX) return DDSP_HIP_ERANGE;
  if (batch == 0) return DDSP_HIP_OK;
  if (!x || !lo || !hi || !cost || !f0c) return DDSP_HIP_EINVAL;
  const int frames = (int)(n_samples / hop);
  if (frames == 0) return DDSP_HIP_OK;
  return launch_salience(x, batch, n_samples, frame_length, (int)hop, frames,
                         pitch_params(tau_min, tau_max, sample_rate, threshold), lo, hi, (int)n_bins, cost, f0c, lag,
                         f0, confidence, period, stream);
}

size_t ddsp_hip_pitch_viterbi_workspace_bytes(int64_t batch, int64_t frames, int64_t n_bins) {
  if (check_viterbi_sizes(batch, frames, n_bins)) return 0;
  return (size_t)batch * (size_t)frames * (size_t)n_bins;
}

int64_t ddsp_hip_pitch_viterbi_chunk_frames(int64_t n_bins) {
  if (n_bins < 1 || n_bins > kMaxBins) return 0;
  return viterbi_chunk_frames((int)n_bins);
}

int ddsp_hip_pitch_viterbi(const float* cost, const float* f0c, float* f0, float* confidence, int32_t* path,
                           void* workspace, size_t workspace_bytes, int64_t batch, int64_t frames, int64_t n_bins,
                           int64_t max_jump, float transition, void* stream) {
  const int st = check_viterbi_sizes(batch, frames, n_bins);
  if (st) return st;
  if (max_jump < 0 || !(transition >= 0.0f) || std::isinf(transition)) return DDSP_HIP_EINVAL;
  if (max_jump > kMaxJump) return DDSP_HIP_ERANGE;
  if (batch == 0 || frames == 0) return DDSP_HIP_OK;
  if (!cost || !f0c || !f0 || !path || !workspace) return DDSP_HIP_EINVAL;
  if (workspace_bytes < ddsp_hip_pitch_viterbi_workspace_bytes(batch, frames, n_bins)) return DDSP_HIP_EWORKSPACE;
  const unsigned threads = (unsigned)((n_bins + 63) / 64 * 64);
  hipLaunchKernelGGL(pitch_viterbi_kernel, dim3((unsigned)batch), dim3(threads), 0, S(stream), cost, f0c, f0,
                     confidence, path, reinterpret_cast<int8_t*>(workspace), (int)frames, (int)n_bins, (int)max_jump,
                     transition);
  return launch_status();
}

}  // extern "C"
