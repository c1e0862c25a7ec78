// The harmonic frame: what the two per-frame gradient kernels of the harmonic synthesis share, written once —
// harmonic_vjp_kernel (backward.hip, the gradient of the amplitudes: sines) and frame_pitch_grad_kernel
// (pitch_grad.hip, the gradient of f0: cosines).  Both run one workgroup per (item, frame) over the same table of
// (omega_t, g_t) pairs with the same thread grid; the phase convention, the padding rule and the segment shape
// live here alone:
//   omega_{f,j} = S0_f + (j+1) inc_f for sample j < bs of frame f, inc_f = phase_inc(f0_f, sr),
//   S0_f = bs sum_{f'<f} inc_{f'} in fp64;
//   item (kq, s) of the ceil(H/kKPT) x NS grid works on the harmonics k = kKPT kq .. kKPT kq + 3 over segment s of
//   the frame's samples; the NS segments are SL samples each (even, NS * SL >= bs), and (omega, g) = 0 past bs
//   adds exact zeros, so every thread's hardware-sine / -cosine loop has the same scalar trip count: no per-lane
//   exit masks (4 VALU per 8 sines before; 152 -> 146.5-147.7 us for the VJP at config 2, same box,
//   tools/ab_prof.sh bwd).
// The kernels' inner loops are not here: they differ in every line that matters, and their placement is pinned.
#pragma once

#include <algorithm>

#include "common.h"

namespace ddsp {

constexpr int kKPT = 4;  // harmonics per thread
// ceil(H/kKPT) x NS fills about this many threads (small workgroups: several per CU hide each one's
// latency-bound phases); measured best for the VJP at config 2 (64..512 swept)
constexpr int kHarmonicThreads = 128;
// core.FRAME_PREFIX_MIN_FRAMES: past it the pitch gradient reads S0 from a ddsp_hip_frame_phase_prefix launch
constexpr int kPrefixMinFrames = 512;

// workgroup threads nt and sample segments ns
inline void harmonic_backward_shape(int H, int bs, int& nt, int& ns) {
  const int kq = (H + kKPT - 1) / kKPT;
  ns = std::max(1, std::min(std::min(kHarmonicThreads / kq, bs), 64));
  nt = std::min(512, ((kq * ns + 63) / 64) * 64);
}

// samples per segment
__host__ __device__ inline int harmonic_segment_len(int bs, int ns) { return ((bs + ns - 1) / ns + 1) & ~1; }

// dynamic LDS floats of a kernel built on harmonic_frame_setup (its layout, on the host)
inline size_t harmonic_frame_lds_floats(int H, int bs, int ns, size_t own_floats) {
  return (size_t)2 * ns * harmonic_segment_len(bs, ns) + own_floats + H;
}

struct HarmonicFrame {
  float2* wg;  // [NS * SL] (omega_t, g_t) per sample, zero past bs
  float* own;  // [own_floats] the kernel's per-segment partial sums
  float* uk;   // [H] the normalised distribution u_k
  int SL;
  double S0, dinc;  // the frame's phase offset and increment
  float pitch0, half_sr;
  float norm;  // PARAMS: D = sum_k v_k
  float a;     // the frame's amplitude
  const float* prow;  // PARAMS: the frame's row of param
  int64_t frame;      // b * F + f
};

// Phases 1 and 2 of both kernels: the loads, the fp64 sum of the earlier frames' phase increments (strided over
// the workgroup; read from prefix[frame] instead where prefix is given), the table and the frame's controls —
// PARAMS: from the raw projection param[B,F,H+1] (controls_value, scale_fn, u_k = v_k / D), else the frame
// controls amp[B,F], dist[B,F,H].  own_floats: what the kernel keeps between wg and uk.  red: >= 32 doubles.
// The caller's barrier publishes wg and uk.
template <bool PARAMS>
__device__ __forceinline__ HarmonicFrame harmonic_frame_setup(
    float* smem, double* red, int own_floats, const float* __restrict__ f0, const float* __restrict__ grad,
    const float* __restrict__ param, const float* __restrict__ amp, const float* __restrict__ dist,
    const double* __restrict__ prefix, int F, int H, int bs, float sr, int NS) {
  HarmonicFrame fr;
  fr.SL = harmonic_segment_len(bs, NS);
  const int WGN = NS * fr.SL;
  fr.wg = reinterpret_cast<float2*>(smem);
  fr.own = smem + 2 * WGN;
  fr.uk = fr.own + own_floats;
  float2* wg = fr.wg;
  float* uk = fr.uk;
  const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, NT = blockDim.x;
  fr.frame = (int64_t)b * F + f;
  const float* gf = grad + fr.frame * bs;

  // ---- phase 1: loads ----
  double part_s = 0.0, part_d = 0.0;
  fr.half_sr = sr * 0.5f;
  fr.prow = PARAMS ? param + fr.frame * (H + 1) : nullptr;
  const float* f0b = f0 + (int64_t)b * F;
  fr.pitch0 = f0b[f];
  if (!prefix)
    for (int q = tid; q < f; q += NT) part_s += (double)bs * (double)phase_inc(f0b[q], sr);
  for (int k = tid; k < H; k += NT) {
    if (PARAMS) {
      const float v = controls_value(fr.prow[1 + k], fr.pitch0, k, fr.half_sr);
      uk[k] = v;
      part_d += (double)v;
    } else {
      uk[k] = dist[fr.frame * H + k];
    }
  }
  for (int j = tid; j < WGN; j += NT) wg[j].y = j < bs ? gf[j] : 0.0f;
  block_sum_double2(part_s, part_d, red);

  // ---- phase 2: phases, normalised distribution ----
  fr.S0 = prefix ? prefix[fr.frame] : part_s;
  fr.norm = (float)part_d;
  fr.dinc = (double)phase_inc(fr.pitch0, sr);
  for (int j = tid; j < WGN; j += NT) wg[j].x = j < bs ? (float)(fr.S0 + (double)(j + 1) * fr.dinc) : 0.0f;
  fr.a = PARAMS ? scale_fn(fr.prow[0]) : amp[fr.frame];
  if (PARAMS)
    for (int k = tid; k < H; k += NT) uk[k] = uk[k] / fr.norm;  // (each thread its own phase-1 elements)
  return fr;
}

}  // namespace ddsp
