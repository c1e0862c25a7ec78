// On-device audio analysis: the two features the models consume, from raw audio x[B, T].
//
//   loudness  ddsp/core.py:81-97 extract_loudness: mean over the bins of ln(|X| + 1e-7) + A-weighting,
//             frames 0 .. T/hop - 1 (the reference computes 1 + T/hop and drops the last);
//   mfcc      ddsp/preprocess.py:30-32 librosa.feature.mfcc: mel power spectrogram -> 10 log10(max(1e-10, .))
//             -> clamp at (item maximum - top_db) -> orthonormal DCT-II, all 1 + T/hop frames.
//
// Both use librosa.stft's frames (center=True, pad_mode='reflect', periodic Hann(n_fft), an UNNORMALISED
// FFT): stft_frames.h's reflect indexing, two real frames per LDS-resident complex FFT, split by
// Z[k] +- conj(Z[N-k]) as in stft.hip — with the transform in fp64 (fft_radix_f64.h says why: the log of a
// single bin near a spectral zero multiplies the transform's absolute error by 1/|X|).  No spectrogram
// reaches HBM: the loudness kernel reduces a frame's bins in its epilogue; the MFCC's first launch overwrites
// the spectrum in LDS with both frames' power (P_a[k], P_b[k]) and takes the mel rows' short dot products out
// of it (one LDS read serves both frames), writing only D[B, frames, n_mels] (dB) and one maximum per
// workgroup.  top_db needs the maximum over the whole item, hence a second launch: it folds the item's
// workgroup maxima, clamps and applies the DCT.  Every reduction has a fixed order and there are no atomics:
// results are bit-reproducible and an item's values do not depend on the batch around it.
//
// A workgroup transforms kPoints<N> points: 2048 (128 threads, 34 KB of LDS, 2048/N transforms) or, for
// N = 4096, one transform of 4096 (256 threads, 68 KB: gfx950's LDS is 160 KB per CU).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "common.h"
#include "fft_radix_f64.h"
#include "stft_frames.h"

namespace ddsp {
namespace {

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

constexpr int kMaxMels = 256;  // n_mels cap (the band tables live in LDS)
constexpr int kDctFrames = 8;  // frames per workgroup of the DCT launch
constexpr int kDctChunk = 32;  // mel columns of the DCT table staged per pass

template <int N>
constexpr int kPoints = N == 4096 ? 4096 : 2048;  // points per workgroup; threads = points / 16

// Frames fa and fa + 1 of row xr, windowed (periodic Hann(N) from the fp64 table), through one complex FFT;
// on return this transform's LDS slots hold Z (index k at lds_idx(k)) and the workgroup is synchronised.
template <int N>
__device__ __forceinline__ void packed_spectrum(const float* __restrict__ xr, int64_t T, int hop, int frames, int fa,
                                                int t, double2* lds) {
  constexpr int Q = N / 16, STEP = 4096 / N;
  const int fb = fa + 1;
  double2 v[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = t + Q * r;
    const double w = 0.5 - 0.5 * kTwiddle4096D[2 * ((m * STEP) & 4095)];
    const double a = fa < frames ? (double)reflect_load(xr, T, (int64_t)fa * hop + m - N / 2) * w : 0.0;
    const double b = fb < frames ? (double)reflect_load(xr, T, (int64_t)fb * hop + m - N / 2) * w : 0.0;
    v[r] = make_double2(a, b);
  }
  fft_n_f64<N, false>(v, lds, t);  // lds untouched so far
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) lds[lds_idx(t + Q * r)] = v[r];
  __syncthreads();
}

// |X_a[k]|^2 and |X_b[k]|^2 of the two packed frames:
// X_a = (Z[k] + conj(Z[N-k])) / 2,  X_b = (Z[k] - conj(Z[N-k])) / (2i)
template <int N>
__device__ __forceinline__ double2 packed_power(const double2* lds, int k) {
  const double2 zk = lds[lds_idx(k)], zn = lds[lds_idx((N - k) & (N - 1))];
  const double ar = 0.5 * (zk.x + zn.x), ai = 0.5 * (zk.y - zn.y);
  const double br = 0.5 * (zk.y + zn.y), bi = -0.5 * (zk.x - zn.x);
  return make_double2(fma(ar, ar, ai * ai), fma(br, br, bi * bi));
}

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

// grid (ceil(frames / (2 * kPoints/N)), B), kPoints/16 threads; out[B, frames]
template <int N>
__global__ void __launch_bounds__(kPoints<N> / 16) loudness_kernel(const float* __restrict__ x, int64_t T, int hop,
                                                                   int frames, const float* __restrict__ w,
                                                                   float* __restrict__ out) {
  constexpr int Q = N / 16, TPW = kPoints<N> / N, BINS = N / 2 + 1;
  __shared__ double2 lds_all[TPW * (N + N / 16)];
  __shared__ double red[8];
  const int tr = threadIdx.x / Q, t = threadIdx.x - tr * Q;
  double2* lds = lds_all + tr * (N + N / 16);
  const int b = blockIdx.y;
  const int fa = 2 * (blockIdx.x * TPW + tr);
  packed_spectrum<N>(x + (int64_t)b * T, T, hop, frames, fa, t, lds);
  double sa = 0.0, sb = 0.0;
  for (int k = t; k < BINS; k += Q) {
    const double2 p = packed_power<N>(lds, k);
    const float wk = w ? w[k] : 0.0f;
    sa += (double)(logf((float)sqrt(p.x) + 1e-7f) + wk);
    sb += (double)(logf((float)sqrt(p.y) + 1e-7f) + wk);
  }
  transform_sum2<Q>(sa, sb, red, tr);
  if (t != 0 || fa >= frames) return;
  float* o = out + (int64_t)b * frames + fa;
  o[0] = (float)(sa / (double)BINS);
  if (fa + 1 < frames) o[1] = (float)(sb / (double)BINS);
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o, 64));
  return v;
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
  constexpr int RPT = kMaxMels / THREADS, WAVES = THREADS / 64;  // mel rows per thread in the offset scan
  __shared__ double2 lds_all[TPW * (N + N / 16)];
  __shared__ int s_start[kMaxMels], s_count[kMaxMels], s_off[kMaxMels];
  __shared__ int s_wave[WAVES];
  __shared__ float s_max[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  // the rows' offsets into band_w: exclusive scan of the counts (thread tid holds rows RPT tid ..)
  {
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
  const int tr = tid / Q, t = tid - tr * Q;
  double2* lds = lds_all + tr * (N + N / 16);
  const int b = blockIdx.y;
  const int fa = 2 * (blockIdx.x * TPW + tr);
  packed_spectrum<N>(x + (int64_t)b * T, T, hop, frames, fa, t, lds);  // (its barriers publish s_*)
  // power of both frames over the spectrum, in place: the thread that owns the pair {k, N-k} writes slot k
  // (no other thread reads k or N-k)
  for (int k = t; k < BINS; k += Q) lds[lds_idx(k)] = packed_power<N>(lds, k);
  __syncthreads();
  const bool va = fa < frames, vb = fa + 1 < frames;
  float* Da = D + ((int64_t)b * frames + (va ? fa : 0)) * n_mels;
  float mx = -INFINITY;
  for (int m = t; m < n_mels; m += Q) {
    const int s0 = s_start[m], c = s_count[m], off = s_off[m];
    double ea = 0.0, eb = 0.0;
    for (int j = 0; j < c; ++j) {
      const double wj = off + j < n_w ? (double)band_w[off + j] : 0.0;
      const double2 p = lds[lds_idx(s0 + j)];
      ea = fma(wj, p.x, ea);
      eb = fma(wj, p.y, eb);
    }
    const float da = 10.0f * log10f(fmaxf(1e-10f, (float)ea));
    const float db = 10.0f * log10f(fmaxf(1e-10f, (float)eb));
    if (va) {
      Da[m] = da;
      mx = fmaxf(mx, da);
    }
    if (vb) {
      Da[n_mels + m] = db;
      mx = fmaxf(mx, db);
    }
  }
  mx = wave_max(mx);
  if (lane == 0) s_max[wid] = mx;
  __syncthreads();
  if (tid == 0) {
    float r = s_max[0];
#pragma unroll
    for (int i = 1; i < WAVES; ++i) r = fmaxf(r, s_max[i]);
    wgmax[(int64_t)b * gridDim.x + blockIdx.x] = r;
  }
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

// The envelope both features share (include/ddsp_hip.h), checked before any HIP call.
int check_features(int64_t B, int64_t T, int64_t n_fft, int64_t hop) {
  if (B < 0 || T < 1 || hop < 1 || n_fft < 1) return DDSP_HIP_EINVAL;
  if (n_fft < 16 || n_fft > 4096 || (n_fft & (n_fft - 1))) return DDSP_HIP_ERANGE;
  if (n_fft / 2 >= T) return DDSP_HIP_EINVAL;  // reflect padding needs T > n_fft/2 (as librosa / torch.stft)
  if (B > 65535 || T / hop + 1 > INT32_MAX) return DDSP_HIP_ERANGE;
  return DDSP_HIP_OK;
}

int check_mfcc(int64_t B, int64_t T, int64_t n_fft, int64_t hop, int64_t n_mels, int64_t n_mfcc) {
  if (n_mels < 1 || n_mfcc < 1 || n_mfcc > n_mels) return DDSP_HIP_EINVAL;
  const int st = check_features(B, T, n_fft, hop);
  if (st) return st;
  return n_mels > kMaxMels ? DDSP_HIP_ERANGE : DDSP_HIP_OK;
}

unsigned frame_blocks(int64_t n_fft, int64_t frames) {
  const int64_t per = 2 * ((n_fft == 4096 ? 4096 : 2048) / n_fft);  // two frames per transform, kPoints/N transforms
  return (unsigned)((frames + per - 1) / per);
}

template <int N>
int loudness_launch(const float* x, const float* w, float* out, int64_t B, int64_t T, int hop, int frames,
                    void* stream) {
  hipLaunchKernelGGL(loudness_kernel<N>, dim3(frame_blocks(N, frames), (unsigned)B), dim3(kPoints<N> / 16), 0,
                     S(stream), x, T, hop, frames, w, out);
  return launch_status();
}

template <int N>
int mel_db_launch(const float* x, const int* bs, const int* bc, const float* bw, int n_w, int n_mels, float* D,
                  float* wgmax, int64_t B, int64_t T, int hop, int frames, void* stream) {
  hipLaunchKernelGGL(mel_db_kernel<N>, dim3(frame_blocks(N, frames), (unsigned)B), dim3(kPoints<N> / 16), 0,
                     S(stream), x, T, hop, frames, bs, bc, bw, n_w, n_mels, D, wgmax);
  return launch_status();
}

#define DDSP_FOR_N_FFT(n_fft, CALL)         \
  switch (n_fft) {                          \
    case 16: return CALL(16);               \
    case 32: return CALL(32);               \
    case 64: return CALL(64);               \
    case 128: return CALL(128);             \
    case 256: return CALL(256);             \
    case 512: return CALL(512);             \
    case 1024: return CALL(1024);           \
    case 2048: return CALL(2048);           \
    default: return CALL(4096);             \
  }

int loudness_dispatch(const float* x, const float* w, float* out, int64_t B, int64_t T, int64_t n_fft, int hop,
                      int frames, void* stream) {
#define DDSP_CALL(N) loudness_launch<N>(x, w, out, B, T, hop, frames, stream)
  DDSP_FOR_N_FFT(n_fft, DDSP_CALL)
#undef DDSP_CALL
}

int mel_db_dispatch(const float* x, const int* bs, const int* bc, const float* bw, int n_w, int n_mels, float* D,
                    float* wgmax, int64_t B, int64_t T, int64_t n_fft, int hop, int frames, void* stream) {
#define DDSP_CALL(N) mel_db_launch<N>(x, bs, bc, bw, n_w, n_mels, D, wgmax, B, T, hop, frames, stream)
  DDSP_FOR_N_FFT(n_fft, DDSP_CALL)
#undef DDSP_CALL
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
  return loudness_dispatch(x, weights, out, batch, n_samples, n_fft, (int)hop, frames, stream);
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
  if (n_band_weights < 0 || n_band_weights > INT32_MAX || !(top_db >= 0.0f)) return DDSP_HIP_EINVAL;
  int st = check_mfcc(batch, n_samples, n_fft, hop, n_mels, n_mfcc);
  if (st) return st;
  if (batch == 0) return DDSP_HIP_OK;
  if (!x || !band_start || !band_count || !band_weights || !dct || !out) return DDSP_HIP_EINVAL;
  if (!workspace || workspace_bytes < ddsp_hip_mfcc_workspace_size(batch, n_samples, n_fft, hop, n_mels))
    return DDSP_HIP_EWORKSPACE;
  const int frames = (int)(n_samples / hop + 1);
  const unsigned nblk = frame_blocks(n_fft, frames);
  float* D = reinterpret_cast<float*>(workspace);
  float* wgmax = D + (size_t)batch * (size_t)frames * (size_t)n_mels;
  st = mel_db_dispatch(x, band_start, band_count, band_weights, (int)n_band_weights, (int)n_mels, D, wgmax, batch,
                       n_samples, n_fft, (int)hop, frames, stream);
  if (st) return st;
  const unsigned gx = (unsigned)((frames + kDctFrames - 1) / kDctFrames);
  hipLaunchKernelGGL(mfcc_dct_kernel, dim3(gx, (unsigned)batch), dim3(256), 0, S(stream), D, wgmax, (int)nblk, frames,
                     (int)n_mels, (int)n_mfcc, dct, top_db, out);
  return launch_status();
}

}  // extern "C"
