// Reverb.build_impulse (ddsp/models/modules.py:21-26) and its backward, written once for every kernel
// that forms a tap or its gradient (reverb.hip: build_impulse_kernel, impulse_backward_kernel and its
// finish; upols.hip: upols_impulse_spectrum_kernel, the IR cache's ir_window,
// upols_corr_finish_impulse_kernel):
//   imp[i] = noise[i] env[i] w (i >= 1), env = exp(-softplus(-decay) t 500), w = sigmoid(wet),
//   t = fl32(i / sr) as torch.arange(L) / sr; imp[0] = 1 carries no gradient.
// The library is compiled with -ffp-contract=off, so the grouping written here is the result: the
// callers agree bit for bit because they call these, not because they were copied in step.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ddsp {

struct ImpulseParams {
  float d;    // -decay, the softplus argument
  float neg;  // -softplus(-decay)
  float w;    // sigmoid(wet)
};

__device__ __forceinline__ float impulse_arg(float decay) { return -decay; }
__device__ __forceinline__ float impulse_wet(float wet) { return 1.0f / (1.0f + expf(-wet)); }

__device__ __forceinline__ ImpulseParams impulse_params(float decay, float wet) {
  const float d = impulse_arg(decay);
  const float sp = d > 20.0f ? d : log1pf(expf(d));  // softplus(-decay), torch's threshold 20
  return {d, -sp, impulse_wet(wet)};
}

__device__ __forceinline__ float impulse_time(int64_t i, float sr) { return (float)i / sr; }

__device__ __forceinline__ float impulse_env(const ImpulseParams& p, float t) { return expf((p.neg * t) * 500.0f); }
__device__ __forceinline__ float impulse_env(const ImpulseParams& p, int64_t i, float sr) {
  return impulse_env(p, impulse_time(i, sr));
}

// tap i from its envelope and its noise value (the value, not the array: the IR cache holds its taps in
// registers); tap 0 uses neither
__device__ __forceinline__ float impulse_tap(const ImpulseParams& p, int64_t i, float env, float noise) {
  return i == 0 ? 1.0f : (noise * env) * p.w;
}

// Backward of one tap: gi = the tap's upstream gradient (0 at tap 0 and at taps cropped away by a shorter
// input).  Returns d_noise and adds the tap's terms of sum dimp*noise*env and sum dimp*noise*env*t to the
// fp64 sums.
__device__ __forceinline__ float impulse_tap_grad(const ImpulseParams& p, float gi, float noise, float env, float t,
                                                  double& aw, double& ad) {
  const float d_noise = gi * env * p.w;
  const float gne = gi * noise * env;
  aw += (double)gne;
  ad += (double)gne * (double)t;
  return d_noise;
}

// softplus'(d), the decay's share of d_decay
__device__ __forceinline__ float impulse_slope(float d) { return d > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-d)); }

// d_wet and d_decay from the two sums reduced over every tap, w = sigmoid(wet) and spg = impulse_slope(-decay)
__device__ __forceinline__ void impulse_close(float w, float spg, double sw, double sd, float* d_decay, float* d_wet) {
  d_wet[0] = (float)(sw * (double)w * (1.0 - (double)w));
  d_decay[0] = (float)(sd * (double)w * 500.0 * (double)spg);
}

}  // namespace ddsp
