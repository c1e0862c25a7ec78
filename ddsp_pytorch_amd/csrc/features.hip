// On-device audio analysis: the two features the models consume, from raw audio x[B, T].
//
//   loudness  ddsp/core.py:81-97 extract_loudness: mean over the bins of ln(|X| + 1e-7) + A-weighting,
//             frames 0 .. T/hop - 1 (the reference computes 1 + T/hop and drops the last);
//   mfcc      ddsp/preprocess.py:30-32 librosa.feature.mfcc: mel power spectrogram -> 10 log10(max(1e-10, .))
//             -> clamp at (item maximum - top_db) -> orthonormal DCT-II, all 1 + T/hop frames.
//
// Both use librosa.stft's frames (center=True, pad_mode='reflect', periodic Hann(n_fft), an UNNORMALISED
// FFT): stft_frames.h's reflect indexing, two real frames per LDS-resident complex FFT, split by
// Z[k] +- conj(Z[N-k]) as in stft.hip — with the transform in fp64 (analysis_frames.h says why: the log of a
// single bin near a spectral zero multiplies the transform's absolute error by 1/|X|).  No spectrogram
// reaches HBM: the loudness kernel reduces a frame's bins in its epilogue; the MFCC's first launch overwrites
// the spectrum in LDS with both frames' power (P_a[k], P_b[k]) and takes the mel rows' short dot products out
// of it (one LDS read serves both frames), writing only D[B, frames, n_mels] (dB) and one maximum per
// workgroup.  top_db needs the maximum over the whole item, hence a second launch: it folds the item's
// workgroup maxima, clamps and applies the DCT.  Every reduction has a fixed order and there are no atomics:
// results are bit-reproducible and an item's values do not depend on the batch around it.
//
// The same two features call by call for a realtime stream (ddsp_hip_stream_loudness / ddsp_hip_stream_mfcc, further
// down): the samples a window needs from before the call are carried in a ring per item, the frames are the
// stream's own (zeros before its start, no reflect padding), the MFCC's clamp is causal, one launch per feature.
//
// A workgroup transforms kPoints<N> points: 2048 (128 threads, 34 KB of LDS, 2048/N transforms) or, for
// N = 4096, one transform of 4096 (256 threads, 68 KB: gfx950's LDS is 160 KB per CU).
// The kernels are shells around analysis_bodies.h's roles: loudness_kernel and stream_loudness_kernel around
// loudness_role, stream_mfcc_kernel around stream_mfcc_body, mel_db_kernel around the MFCC's pieces (stage_bands,
// mel_rows, workgroup_max); stream_analysis.hip and stream_analysis_mfcc.hip run the same roles.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "analysis_bodies.h"

namespace ddsp {
namespace {

// grid (ceil(frames / (2 * kPoints/N)), B), kPoints/16 threads; out[B, frames]
template <int N>
__global__ void __launch_bounds__(kPoints<N> / 16) loudness_kernel(const float* __restrict__ x, int64_t T, int hop,
                                                                   int frames, const float* __restrict__ w,
                                                                   float* __restrict__ out) {
  constexpr int TPW = kPoints<N> / N;
  __shared__ double2 lds_all[TPW * (N + N / 16)];
  __shared__ double red[8];
  const int b = blockIdx.y;
  loudness_role<N>(ReflectFetch<N>{x + (int64_t)b * T, T, hop, frames}, blockIdx.x, w, lds_all, red, out, b);
}

// MFCC launch (a).  grid (ceil(frames / (2 * kPoints/N)), B), kPoints/16 threads.  Mel row m is the band
// [start[m], start[m] + count[m]) of bins with weights packed row after row in band_w (n_w floats); a band
// that leaves the spectrum or the weight array is cut there, never read past.  D[B, frames, n_mels] =
// 10 log10(max(1e-10, mel energy)); wgmax[b * gridDim.x + blockIdx.x] = the workgroup's largest D.
template <int N>
__global__ void __launch_bounds__(kPoints<N> / 16) mel_db_kernel(const float* __restrict__ x, int64_t T, int hop,
                                                                 int frames, const int* __restrict__ band_start,
                                                                 const int* __restrict__ band_count,
                                                                 const float* __restrict__ band_w, int n_w,
                                                                 int n_mels, float* __restrict__ D,
                                                                 float* __restrict__ wgmax) {
  constexpr int Q = N / 16, THREADS = kPoints<N> / 16, TPW = kPoints<N> / N, BINS = N / 2 + 1;
  constexpr int WAVES = THREADS / 64;
  __shared__ double2 lds_all[TPW * (N + N / 16)];
  __shared__ int s_start[kMaxMels], s_count[kMaxMels], s_off[kMaxMels];
  __shared__ int s_wave[WAVES];
  __shared__ float s_max[WAVES];
  stage_bands<THREADS, BINS>(band_start, band_count, n_mels, s_start, s_count, s_off, s_wave);
  const int tr = threadIdx.x / Q, t = threadIdx.x - tr * Q;
  double2* lds = lds_all + tr * (N + N / 16);
  const int b = blockIdx.y;
  const int fa = 2 * (blockIdx.x * TPW + tr);
  // (its barriers publish s_*)
  packed_spectrum<N>(ReflectFetch<N>{x + (int64_t)b * T, T, hop, frames}, fa, t, lds);
  // power of both frames over the spectrum, in place: the thread that owns the pair {k, N-k} writes slot k
  // (no other thread reads k or N-k)
  for (int k = t; k < BINS; k += Q) lds[lds_idx(k)] = packed_power<N>(lds, k);
  __syncthreads();
  const bool va = fa < frames, vb = fa + 1 < frames;
  float mx = -INFINITY;
  mel_rows<N>(lds, t, band_w, n_w, s_start, s_count, s_off, n_mels, va, vb,
              D + ((int64_t)b * frames + (va ? fa : 0)) * n_mels, mx);
  mx = workgroup_max<WAVES>(mx, s_max);
  if (threadIdx.x == 0) wgmax[(int64_t)b * gridDim.x + blockIdx.x] = mx;
}

// MFCC launch (b).  grid (ceil(frames / kDctFrames), B), 256 threads.  The item's maximum from its nblk
// workgroup maxima, D <- max(D, Dmax - top_db), out[b, f, i] = sum_m dct[i, m] D[b, f, m] (m ascending, fp64
// accumulator).  The DCT table passes through LDS kDctChunk mel columns at a time, rows padded to an odd
// stride: lanes that differ in i read different banks, lanes of one frame share D's address (a broadcast).
__global__ void __launch_bounds__(256) mfcc_dct_kernel(const float* __restrict__ D, const float* __restrict__ wgmax,
                                                       int nblk, int frames, int n_mels, int n_mfcc,
                                                       const float* __restrict__ dct, float top_db,
                                                       float* __restrict__ out) {
  constexpr int FR = kDctFrames, MC = kDctChunk;
  __shared__ float sD[FR * kMaxMels];
  __shared__ float sT[kMaxMels * (MC + 1)];
  __shared__ float s_max[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b = blockIdx.y;
  const int f0 = blockIdx.x * FR;
  const int nf = min(FR, frames - f0);
  float mx = -INFINITY;
  for (int i = tid; i < nblk; i += 256) mx = fmaxf(mx, wgmax[(int64_t)b * nblk + i]);
  mx = wave_max(mx);
  if (lane == 0) s_max[wid] = mx;
  __syncthreads();
  const float floor_db = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3])) - top_db;
  const float* Dt = D + ((int64_t)b * frames + f0) * n_mels;
  for (int i = tid; i < nf * n_mels; i += 256) sD[i] = fmaxf(Dt[i], floor_db);
  const int tasks = nf * n_mfcc;  // task o = f * n_mfcc + i, <= 256 * FR
  double acc[FR];
#pragma unroll
  for (int j = 0; j < FR; ++j) acc[j] = 0.0;
  for (int m0 = 0; m0 < n_mels; m0 += MC) {
    const int mc = min(MC, n_mels - m0);
    __syncthreads();  // sD complete (first pass); the previous chunk consumed (later ones)
    for (int idx = tid; idx < n_mfcc * MC; idx += 256) {
      const int i = idx / MC, mm = idx - i * MC;
      sT[i * (MC + 1) + mm] = mm < mc ? dct[(int64_t)i * n_mels + m0 + mm] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < FR; ++j) {
      const int o = tid + 256 * j;
      if (o < tasks) {
        const int f = o / n_mfcc, i = o - f * n_mfcc;
        const float* tr = sT + i * (MC + 1);
        const float* dr = sD + f * n_mels + m0;
        double a = acc[j];
        for (int mm = 0; mm < mc; ++mm) a = fma((double)tr[mm], (double)dr[mm], a);
        acc[j] = a;
      }
    }
  }
  float* ot = out + ((int64_t)b * frames + f0) * n_mfcc;
#pragma unroll
  for (int j = 0; j < FR; ++j) {
    const int o = tid + 256 * j;
    if (o < tasks) ot[o] = (float)acc[j];
  }
}

// ---------------- streaming analysis: one call of a stream (include/ddsp_hip.h; analysis_frames.h) ----------------
// grid (ceil(ceil(frames / 2) / (kPoints/N)), B), kPoints/16 threads; out[B, frames].  Frames (j, j + 1), j even,
// share a transform.  The item's workgroups share the ring copy.
template <int N>
__global__ void __launch_bounds__(kPoints<N> / 16) stream_loudness_kernel(const float* __restrict__ x,
                                                                          const float* __restrict__ w,
                                                                          float* __restrict__ out,
                                                                          const uint64_t* __restrict__ counter,
                                                                          float* ring, int n, int len, int hs,
                                                                          int hop, int frames) {
  constexpr int TPW = kPoints<N> / N;
  __shared__ double2 lds_all[TPW * (N + N / 16)];
  __shared__ double red[8];
  const int b = blockIdx.y;
  const StreamFetch fetch = open_stream_call(*counter, ring, x, n, len, hs, hop, frames, b,
                                             blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
  loudness_role<N>(fetch, blockIdx.x, w, lds_all, red, out, b);
}

// The MFCC of one call in one launch: grid (B), kPoints/16 threads, one workgroup per item running
// stream_mfcc_body (analysis_bodies.h) with the item's carried maximum runmax[b], taken as absent when the counter
// is 0.
template <int N>
__global__ void __launch_bounds__(kPoints<N> / 16) stream_mfcc_kernel(
    const float* __restrict__ x, const int* __restrict__ band_start, const int* __restrict__ band_count,
    const float* __restrict__ band_w, int n_w, const float* __restrict__ dct, float* __restrict__ out,
    const uint64_t* __restrict__ counter, float* ring, float* runmax, int n, int len, int hs, int hop, int frames,
    int n_mels, int n_mfcc, float top_db) {
  constexpr int THREADS = kPoints<N> / 16, TPW = kPoints<N> / N, WAVES = THREADS / 64;
  __shared__ double2 lds_all[TPW * (N + N / 16)];
  __shared__ float sD[kStreamMaxFrames * kMaxMels];
  __shared__ int s_start[kMaxMels], s_count[kMaxMels], s_off[kMaxMels];
  __shared__ int s_wave[WAVES];
  __shared__ float s_max[WAVES];
  __shared__ float s_floor;
  const int b = blockIdx.x;
  const uint64_t k = *counter;
  const StreamFetch fetch = open_stream_call(k, ring, x, n, len, hs, hop, frames, b, threadIdx.x, THREADS);
  stream_mfcc_body<N>(fetch, k != 0, lds_all, MfccLds{sD, s_start, s_count, s_off, s_wave, s_max, &s_floor},
                      MfccTables{band_start, band_count, band_w, n_w, dct, n_mels, n_mfcc, top_db}, runmax + b,
                      out + (int64_t)b * frames * n_mfcc);
}

// The envelope both features share (include/ddsp_hip.h), checked before any HIP call.
int check_features(int64_t B, int64_t T, int64_t n_fft, int64_t hop) {
  if (B < 0 || T < 1 || hop < 1 || n_fft < 1) return DDSP_HIP_EINVAL;
  if (n_fft < 16 || n_fft > 4096 || (n_fft & (n_fft - 1))) return DDSP_HIP_ERANGE;
  if (n_fft / 2 >= T) return DDSP_HIP_EINVAL;  // reflect padding needs T > n_fft/2 (as librosa / torch.stft)
  if (B > 65535 || T / hop + 1 > INT32_MAX) return DDSP_HIP_ERANGE;
  return DDSP_HIP_OK;
}

int launch_loudness(const float* x, const float* w, float* out, int64_t B, int64_t T, int64_t n_fft, int hop,
                    int frames, void* stream) {
  return for_frame_length<16>(n_fft, [&](auto size) {
    constexpr int N = decltype(size)::value;
    hipLaunchKernelGGL(loudness_kernel<N>, dim3(frame_blocks(N, frames), (unsigned)B), dim3(kPoints<N> / 16), 0,
                       S(stream), x, T, hop, frames, w, out);
    return launch_status();
  });
}

int launch_mel_db(const float* x, const int* bs, const int* bc, const float* bw, int n_w, int n_mels, float* D,
                  float* wgmax, int64_t B, int64_t T, int64_t n_fft, int hop, int frames, void* stream) {
  return for_frame_length<16>(n_fft, [&](auto size) {
    constexpr int N = decltype(size)::value;
    hipLaunchKernelGGL(mel_db_kernel<N>, dim3(frame_blocks(N, frames), (unsigned)B), dim3(kPoints<N> / 16), 0,
                       S(stream), x, T, hop, frames, bs, bc, bw, n_w, n_mels, D, wgmax);
    return launch_status();
  });
}

int launch_stream_loudness(const StreamArgs& a, int64_t n_fft, const float* w, float* out) {
  return for_frame_length<16>(n_fft, [&](auto size) {
    constexpr int N = decltype(size)::value;
    hipLaunchKernelGGL(stream_loudness_kernel<N>, dim3(frame_blocks(N, a.frames), (unsigned)a.B),
                       dim3(kPoints<N> / 16), 0, S(a.stream), a.x, w, out, a.counter, a.ring, a.n, a.len, a.hs, a.hop,
                       a.frames);
    return launch_status();
  });
}

int launch_stream_mfcc(const StreamArgs& a, int64_t n_fft, const MfccTables& m, float* runmax, float* out) {
  return for_frame_length<16>(n_fft, [&](auto size) {
    constexpr int N = decltype(size)::value;
    hipLaunchKernelGGL(stream_mfcc_kernel<N>, dim3((unsigned)a.B), dim3(kPoints<N> / 16), 0, S(a.stream), a.x,
                       m.start, m.count, m.w, m.n_w, m.dct, out, a.counter, a.ring, runmax, a.n, a.len, a.hs, a.hop,
                       a.frames, m.n_mels, m.n_mfcc, m.top_db);
    return launch_status();
  });
}

}  // namespace
}  // namespace ddsp

using namespace ddsp;

extern "C" {

int ddsp_hip_loudness(const float* x, const float* weights, float* out, int64_t batch, int64_t n_samples,
                      int64_t n_fft, int64_t hop, void* stream) {
  const int st = check_features(batch, n_samples, n_fft, hop);
  if (st) return st;
  if (batch == 0) return DDSP_HIP_OK;
  if (!x || !out) return DDSP_HIP_EINVAL;
  const int frames = (int)(n_samples / hop);
  if (frames == 0) return DDSP_HIP_OK;
  return launch_loudness(x, weights, out, batch, n_samples, n_fft, (int)hop, frames, stream);
}

size_t ddsp_hip_mfcc_workspace_size(int64_t batch, int64_t n_samples, int64_t n_fft, int64_t hop, int64_t n_mels) {
  if (batch < 1 || n_mels < 1 || check_features(batch, n_samples, n_fft, hop)) return 0;
  const int64_t frames = n_samples / hop + 1;
  return sizeof(float) * ((size_t)batch * (size_t)frames * (size_t)n_mels +
                          (size_t)batch * (size_t)frame_blocks(n_fft, frames));
}

int ddsp_hip_mfcc(const float* x, const int32_t* band_start, const int32_t* band_count, const float* band_weights,
                  int64_t n_band_weights, const float* dct, float* out, int64_t batch, int64_t n_samples,
                  int64_t n_fft, int64_t hop, int64_t n_mels, int64_t n_mfcc, float top_db, void* workspace,
                  size_t workspace_bytes, void* stream) {
  if (mfcc_params_invalid(n_band_weights, n_mels, n_mfcc, top_db)) return DDSP_HIP_EINVAL;
  int st = check_features(batch, n_samples, n_fft, hop);
  if (st) return st;
  if (n_mels > kMaxMels) return DDSP_HIP_ERANGE;  // after the envelope, as in ddsp_hip_stream_mfcc
  if (batch == 0) return DDSP_HIP_OK;
  if (!x || !band_start || !band_count || !band_weights || !dct || !out) return DDSP_HIP_EINVAL;
  if (!workspace || workspace_bytes < ddsp_hip_mfcc_workspace_size(batch, n_samples, n_fft, hop, n_mels))
    return DDSP_HIP_EWORKSPACE;
  const int frames = (int)(n_samples / hop + 1);
  const unsigned nblk = frame_blocks(n_fft, frames);
  float* D = reinterpret_cast<float*>(workspace);
  float* wgmax = D + (size_t)batch * (size_t)frames * (size_t)n_mels;
  st = launch_mel_db(x, band_start, band_count, band_weights, (int)n_band_weights, (int)n_mels, D, wgmax, batch,
                     n_samples, n_fft, (int)hop, frames, stream);
  if (st) return st;
  const unsigned gx = (unsigned)((frames + kDctFrames - 1) / kDctFrames);
  hipLaunchKernelGGL(mfcc_dct_kernel, dim3(gx, (unsigned)batch), dim3(256), 0, S(stream), D, wgmax, (int)nblk, frames,
                     (int)n_mels, (int)n_mfcc, dct, top_db, out);
  return launch_status();
}

size_t ddsp_hip_stream_features_state_bytes(int64_t batch, int64_t call_samples, int64_t n_fft, int64_t hop) {
  StreamSizes sz;
  if (batch < 1 || check_stream_features(batch, call_samples, n_fft, hop, &sz)) return 0;
  return stream_features_bytes(batch, sz);
}

int ddsp_hip_stream_loudness(const float* x, const float* weights, float* out, const uint64_t* counter, void* state,
                             size_t state_bytes, int64_t batch, int64_t call_samples, int64_t n_fft, int64_t hop,
                             void* stream) {
  StreamSizes sz;
  const int st = check_stream_features(batch, call_samples, n_fft, hop, &sz);
  if (st) return st;
  if (batch == 0) return DDSP_HIP_OK;
  if (!x || !out || !counter || !state) return DDSP_HIP_EINVAL;
  if (state_bytes < stream_features_bytes(batch, sz)) return DDSP_HIP_EWORKSPACE;
  return launch_stream_loudness(stream_args(x, counter, state, batch, call_samples, hop, sz, stream), n_fft, weights,
                                out);
}

int ddsp_hip_stream_mfcc(const float* x, const int32_t* band_start, const int32_t* band_count,
                         const float* band_weights, int64_t n_band_weights, const float* dct, float* out,
                         const uint64_t* counter, void* state, size_t state_bytes, int64_t batch,
                         int64_t call_samples, int64_t n_fft, int64_t hop, int64_t n_mels, int64_t n_mfcc, float top_db,
                         void* stream) {
  if (mfcc_params_invalid(n_band_weights, n_mels, n_mfcc, top_db)) return DDSP_HIP_EINVAL;
  StreamSizes sz;
  const int st = check_stream_features(batch, call_samples, n_fft, hop, &sz);
  if (st) return st;
  // not check_stream_mfcc_params: the n_mels cap is tested after the envelope here, and a call that breaks both
  // reports the envelope's status
  if (n_mels > kMaxMels) return DDSP_HIP_ERANGE;
  if (batch == 0) return DDSP_HIP_OK;
  if (!x || !band_start || !band_count || !band_weights || !dct || !out || !counter || !state) return DDSP_HIP_EINVAL;
  if (state_bytes < stream_features_bytes(batch, sz)) return DDSP_HIP_EWORKSPACE;
  const StreamArgs a = stream_args(x, counter, state, batch, call_samples, hop, sz, stream);
  const MfccTables m{band_start, band_count, band_weights, (int)n_band_weights, dct, (int)n_mels, (int)n_mfcc, top_db};
  return launch_stream_mfcc(a, n_fft, m, a.ring + (size_t)batch * (size_t)sz.len, out);
}

}  // extern "C"
