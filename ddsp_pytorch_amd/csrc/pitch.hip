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
// Both kernels are shells around pitch_role (analysis_bodies.h: yin_frame and its helpers), which stream_analysis.hip
// and stream_analysis_mfcc.hip run too.
#include <hip/hip_runtime.h>

#include "analysis_bodies.h"

namespace ddsp {
namespace {

// grid (ceil(frames / (kPoints/N)), B), kPoints/16 threads; f0 / conf / period [B, frames]
template <int N>
__global__ void __launch_bounds__(kPoints<N> / 16) pitch_kernel(const float* __restrict__ x, int64_t T, int hop,
                                                                int frames, PitchParams p, float* __restrict__ f0,
                                                                float* __restrict__ conf,
                                                                int32_t* __restrict__ period) {
  constexpr int TPW = kPoints<N> / N;
  __shared__ double2 lds_all[TPW * (N + N / 16)];
  __shared__ double wsum[4];
  __shared__ int rint[8];
  const int b = blockIdx.y;
  pitch_role<N>(ReflectFetch<N>{x + (int64_t)b * T, T, hop, frames}, blockIdx.x, lds_all, wsum, rint, p, b, f0, conf,
                period);
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
  constexpr int TPW = kPoints<N> / N;
  __shared__ double2 lds_all[TPW * (N + N / 16)];
  __shared__ double wsum[4];
  __shared__ int rint[8];
  const int b = blockIdx.y;
  const StreamFetch fetch = open_stream_call(*counter, ring, x, n, len, hs, hop, frames, b,
                                             blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
  pitch_role<N>(fetch, blockIdx.x, lds_all, wsum, rint, p, b, f0, conf, period);
}

int launch_pitch(const float* x, int64_t B, int64_t T, int64_t L, int hop, int frames, const PitchParams& p,
                 float* f0, float* conf, int32_t* period, void* stream) {
  return for_frame_length<kPitchMinFrame>(L, [&](auto size) {
    constexpr int N = decltype(size)::value;
    hipLaunchKernelGGL(pitch_kernel<N>, dim3(pitch_blocks(N, frames), (unsigned)B), dim3(kPoints<N> / 16), 0,
                       S(stream), x, T, hop, frames, p, f0, conf, period);
    return launch_status();
  });
}

int launch_stream_pitch(const StreamArgs& a, int64_t L, const PitchParams& p, float* f0, float* conf,
                        int32_t* period) {
  return for_frame_length<kPitchMinFrame>(L, [&](auto size) {
    constexpr int N = decltype(size)::value;
    hipLaunchKernelGGL(stream_pitch_kernel<N>, dim3(pitch_blocks(N, a.frames), (unsigned)a.B), dim3(kPoints<N> / 16),
                       0, S(a.stream), a.x, a.counter, a.ring, a.n, a.len, a.hs, a.hop, a.frames, p, f0, conf, period);
    return launch_status();
  });
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
  return launch_pitch(x, batch, n_samples, frame_length, (int)hop, frames,
                      pitch_params(tau_min, tau_max, sample_rate, threshold), f0, confidence, period, stream);
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
  const StreamArgs a = stream_args(x, counter, state, batch, call_samples, hop, sz, stream);
  return launch_stream_pitch(a, frame_length, pitch_params(tau_min, tau_max, sample_rate, threshold), f0, confidence,
                             period);
}

}  // extern "C"
