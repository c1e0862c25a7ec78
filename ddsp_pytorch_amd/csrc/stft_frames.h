// Centred, reflect-padded, Hann-windowed frames for the LDS-resident FFTs of stft.hip (the
// multiscale STFT and the spectral loss) and features.hip (loudness, MFCC): frame f of x[T] is
// centred at f * hop (torch.stft / librosa.stft with center=True, pad_mode='reflect'), and two
// real frames ride in one complex transform as z = frame_a + i frame_b.
#pragma once

#include <hip/hip_runtime.h>

#include "fft_radix.h"

namespace ddsp {
namespace {

// reflect-padded sample of row xr at padded position p (center=True pads N/2 on both sides)
__device__ __forceinline__ float reflect_load(const float* xr, int64_t T, int64_t i) {
  if (i < 0) i = -i;
  if (i >= T) i = 2 * (T - 1) - i;
  return xr[i];
}

template <int N>
__device__ __forceinline__ void load_frames(const float* __restrict__ xr, int64_t T, int hop, int frames, int fa,
                                            int t, float2 (&v)[16]) {
  constexpr int Q = N / 16, STEP = 4096 / N;
  const int fb = fa + 1;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = t + Q * r;
    const float w = 0.5f - 0.5f * kTwiddle4096[2 * ((m * STEP) & 4095)];  // periodic Hann(N)
    const float a = fa < frames ? reflect_load(xr, T, (int64_t)fa * hop + m - N / 2) * w : 0.0f;
    const float b = fb < frames ? reflect_load(xr, T, (int64_t)fb * hop + m - N / 2) * w : 0.0f;
    v[r] = make_float2(a, b);
  }
}

}  // namespace
}  // namespace ddsp
