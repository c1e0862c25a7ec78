// The streamed loudness and the streamed YIN pitch of one call in ONE launch over ONE state (include/ddsp_hip.h,
// ddsp_hip_stream_analysis): what a realtime instrument that is driven by audio alone needs per call.  Both features
// read the same hs + n samples when n_fft == frame_length == L, and each is a dependent chain (loads, the fp64
// transform's LDS exchanges, reductions), so the two chains run side by side in different workgroups of one grid over
// one shared ring, instead of two launches each with a ring and a copy of the call of its own.
//
// grid (pitch_blocks + frame_blocks, B), kPoints<L>/16 threads.  The first pitch_blocks(L, R) workgroups of an item
// run pitch_role<L> (one frame per transform: the longer chain, dispatched first), the remaining
// frame_blocks(L, R) run loudness_role<L> (two frames per transform).  The roles are the ones pitch.hip's and
// features.hip's kernels shell (analysis_bodies.h), so the bits are the separate launches'.  The role branch
// is uniform per workgroup and there is no loop over passes.  Every workgroup copies its strided share of the call
// into the ring; no workgroup reads what another writes (analysis_frames.h), whatever its role.  One lds_all serves
// both roles.  (stream_analysis_mfcc.hip adds the streamed MFCC of the same frames as a third role.)
#include <hip/hip_runtime.h>

#include "analysis_bodies.h"

namespace ddsp {
namespace {

template <int N>
__global__ void __launch_bounds__(kPoints<N> / 16) stream_analysis_kernel(
    const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ loud,
    const uint64_t* __restrict__ counter, float* ring, int n, int len, int hs, int hop, int frames, int pblocks,
    PitchParams p, float* __restrict__ f0, float* __restrict__ conf, int32_t* __restrict__ period) {
  constexpr int TPW = kPoints<N> / N;
  __shared__ double2 lds_all[TPW * (N + N / 16)];
  __shared__ double red[8];  // the loudness's wave sums; the pitch's wsum (its first four)
  __shared__ int rint[8];
  const int b = blockIdx.y;
  const StreamFetch fetch = open_stream_call(*counter, ring, x, n, len, hs, hop, frames, b,
                                             blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
  if ((int)blockIdx.x < pblocks) {
    pitch_role<N>(fetch, blockIdx.x, lds_all, red, rint, p, b, f0, conf, period);
    return;
  }
  loudness_role<N>(fetch, blockIdx.x - pblocks, w, lds_all, red, loud, b);
}

int launch_stream_analysis(const StreamArgs& a, int64_t L, const float* w, float* loud, const PitchParams& p,
                           float* f0, float* conf, int32_t* period) {
  return for_frame_length<kPitchMinFrame>(L, [&](auto size) {
    constexpr int N = decltype(size)::value;
    const unsigned pb = pitch_blocks(N, a.frames);
    hipLaunchKernelGGL(stream_analysis_kernel<N>, dim3(pb + frame_blocks(N, a.frames), (unsigned)a.B),
                       dim3(kPoints<N> / 16), 0, S(a.stream), a.x, w, loud, a.counter, a.ring, a.n, a.len, a.hs,
                       a.hop, a.frames, (int)pb, p, f0, conf, period);
    return launch_status();
  });
}

}  // namespace
}  // namespace ddsp

using namespace ddsp;

extern "C" {

int ddsp_hip_stream_analysis(const float* x, const float* weights, float* loudness_out, float* f0, float* confidence,
                             int32_t* period, const uint64_t* counter, void* state, size_t state_bytes, int64_t batch,
                             int64_t call_samples, int64_t frame_length, int64_t hop, int64_t tau_min, int64_t tau_max,
                             float sample_rate, float threshold, void* stream) {
  StreamSizes sz;
  int st = check_stream_features(batch, call_samples, frame_length, hop, &sz);
  if (st) return st;
  st = check_pitch_params(frame_length, tau_min, tau_max, sample_rate);
  if (st) return st;
  if (batch == 0) return DDSP_HIP_OK;
  if (!x || !loudness_out || !f0 || !counter || !state) return DDSP_HIP_EINVAL;
  if (state_bytes < stream_features_bytes(batch, sz)) return DDSP_HIP_EWORKSPACE;
  const StreamArgs a = stream_args(x, counter, state, batch, call_samples, hop, sz, stream);
  return launch_stream_analysis(a, frame_length, weights, loudness_out,
                                pitch_params(tau_min, tau_max, sample_rate, threshold), f0, confidence, period);
}

}  // extern "C"
