// The streamed loudness, the streamed MFCC and (on request) the streamed YIN pitch of one call in ONE launch over ONE
// state, on ONE time axis (include/ddsp_hip.h, ddsp_hip_stream_analysis_mfcc): what a z-conditioned model (the
// reference's ddsp/models/encoder.py autoencoder) needs per call of a realtime stream.  stream_analysis.hip's grid with
// one more workgroup per item, which runs the streamed MFCC's per-call code (analysis_bodies.h: features.hip's
// stream_mfcc_kernel is the same body) over the same ring.  A translation unit of its own, so that
// stream_analysis.hip's object stays what it was.
#include <hip/hip_runtime.h>

#include "analysis_bodies.h"

namespace ddsp {
namespace {

// grid (pitch_blocks + frame_blocks + 1, B), kPoints<N>/16 threads.  Per item the pitch and the loudness workgroups are
// stream_analysis_kernel's (pitch_role and loudness_role, so the same bits); the item's last workgroup runs
// stream_mfcc_body<M> over the same ring with each frame's M-sample window centred in the frame's L-sample window
// (the fetch's rel0 moved by (L - M)/2, still inside [-hs, n)), so slot j of all three features is the same stream
// frame.  pblocks == 0: no pitch role.  kPoints<L> == kPoints<M> == 2048: one workgroup shape and one lds_all for
// the three roles; the MFCC's D and band tables come on top of it (nothing is aliased).
template <int N, int M>
__global__ void __launch_bounds__(kPoints<N> / 16) stream_analysis_mfcc_kernel(
    const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ loud,
    const uint64_t* __restrict__ counter, float* ring, float* runmax, int n, int len, int hs, int hop, int frames,
    int pblocks, PitchParams p, float* __restrict__ f0, float* __restrict__ conf, int32_t* __restrict__ period,
    MfccTables m, float* __restrict__ mfcc) {
  constexpr int TPW = kPoints<N> / N, WAVES = kPoints<N> / 1024;
  static_assert(kPoints<N> == 2048 && kPoints<M> == 2048 && (M == N || 2 * M == N), "one workgroup shape");
  __shared__ double2 lds_all[TPW * (N + N / 16)];
  __shared__ double red[8];
  __shared__ int rint[8];
  __shared__ float sD[kStreamMaxFrames * kMaxMels];
  __shared__ int s_start[kMaxMels], s_count[kMaxMels], s_off[kMaxMels];
  __shared__ int s_wave[WAVES];
  __shared__ float s_max[WAVES];
  __shared__ float s_floor;
  const int b = blockIdx.y;
  const uint64_t k = *counter;
  const StreamFetch fetch = open_stream_call(k, ring, x, n, len, hs, hop, frames, b,
                                             blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
  if (blockIdx.x == gridDim.x - 1) {
    StreamFetch centred = fetch;
    centred.rel0 += (N - M) / 2;
    stream_mfcc_body<M>(centred, k != 0, lds_all, MfccLds{sD, s_start, s_count, s_off, s_wave, s_max, &s_floor}, m,
                        runmax + b, mfcc + (int64_t)b * frames * m.n_mfcc);
    return;
  }
  if ((int)blockIdx.x < pblocks) {
    pitch_role<N>(fetch, blockIdx.x, lds_all, red, rint, p, b, f0, conf, period);
    return;
  }
  loudness_role<N>(fetch, blockIdx.x - pblocks, w, lds_all, red, loud, b);
}

struct AnalysisMfccArgs {
  const float* w;
  float* loud;
  PitchParams p;
  float *f0, *conf;
  int32_t* period;
  MfccTables m;
  float *runmax, *mfcc;
};

// half: the MFCC's window is L / 2 samples, else L
int launch_stream_analysis_mfcc(const StreamArgs& a, int64_t L, bool half, const AnalysisMfccArgs& g) {
  return for_frame_length<kPitchMinFrame, 2048>(L, [&](auto size) {
    constexpr int N = decltype(size)::value;
    const auto kernel = half ? stream_analysis_mfcc_kernel<N, N / 2> : stream_analysis_mfcc_kernel<N, N>;
    const unsigned pb = g.f0 ? pitch_blocks(N, a.frames) : 0u;
    hipLaunchKernelGGL(kernel, dim3(pb + frame_blocks(N, a.frames) + 1, (unsigned)a.B), dim3(kPoints<N> / 16), 0,
                       S(a.stream), a.x, g.w, g.loud, a.counter, a.ring, g.runmax, a.n, a.len, a.hs, a.hop, a.frames,
                       (int)pb, g.p, g.f0, g.conf, g.period, g.m, g.mfcc);
    return launch_status();
  });
}

}  // namespace
}  // namespace ddsp

using namespace ddsp;

extern "C" {

int ddsp_hip_stream_analysis_mfcc(const float* x, const float* weights, float* loudness_out, const int32_t* band_start,
                                  const int32_t* band_count, const float* band_weights, int64_t n_band_weights,
                                  const float* dct, float* mfcc_out, float* f0, float* confidence, int32_t* period,
                                  const uint64_t* counter, void* state, size_t state_bytes, int64_t batch,
                                  int64_t call_samples, int64_t frame_length, int64_t mfcc_n_fft, int64_t hop,
                                  int64_t n_mels, int64_t n_mfcc, float top_db, int64_t tau_min, int64_t tau_max,
                                  float sample_rate, float threshold, void* stream) {
  StreamSizes sz;
  int st = check_stream_features(batch, call_samples, frame_length, hop, &sz);
  if (st) return st;
  if (frame_length < kPitchMinFrame || frame_length > 2048) return DDSP_HIP_ERANGE;
  if (f0) {
    st = check_pitch_params(frame_length, tau_min, tau_max, sample_rate);
    if (st) return st;
  } else if (confidence || period) {
    return DDSP_HIP_EINVAL;
  }
  if (mfcc_n_fft != frame_length && 2 * mfcc_n_fft != frame_length) return DDSP_HIP_ERANGE;
  st = check_stream_mfcc_params(n_band_weights, n_mels, n_mfcc, top_db);
  if (st) return st;
  if (batch == 0) return DDSP_HIP_OK;
  if (!x || !loudness_out || !band_start || !band_count || !band_weights || !dct || !mfcc_out || !counter || !state)
    return DDSP_HIP_EINVAL;
  if (state_bytes < stream_features_bytes(batch, sz)) return DDSP_HIP_EWORKSPACE;
  const StreamArgs a = stream_args(x, counter, state, batch, call_samples, hop, sz, stream);
  const AnalysisMfccArgs g{weights,
                           loudness_out,
                           pitch_params(tau_min, tau_max, sample_rate, threshold),
                           f0,
                           confidence,
                           period,
                           MfccTables{band_start, band_count, band_weights, (int)n_band_weights, dct, (int)n_mels,
                                      (int)n_mfcc, top_db},
                           a.ring + (size_t)batch * (size_t)sz.len,
                           mfcc_out};
  return launch_stream_analysis_mfcc(a, frame_length, mfcc_n_fft != frame_length, g);
}

}  // extern "C"
