// fft_radix.h's forward Stockham transform in fp64, for features.hip: the analysis features take the LOG of
// single bins, so a bin near a spectral zero (reflect padding makes frame 0 exactly even, its spectrum real and
// such bins common) multiplies the transform's absolute error by 1/|X|.  An fp32 transform of this structure
// measured 2-3x the absolute error of a real-input fp32 FFT on the CPU (packing two frames adds each frame's
// rounding to the other), which those bins turn into the whole error of a frame; in fp64 the transform's error
// vanishes beside the fp32 input's.  MI355X issues fp64 FMAs at the rate of unpacked fp32 ones, so the cost is
// LDS traffic (16-byte elements) and registers, not arithmetic.  Same layout and contract as fft_n: thread t of
// the N/16 of a transform holds v[i] = in[t + (N/16) i] on entry, out[t + (N/16) i] on exit; lds holds
// N + N/16 double2 slots per transform; every thread of the workgroup calls it.
// Twiddles: W_4096^m in fp64 (tools/gen_twiddles.py 4096 f64), each read from the table.
#pragma once

#include <hip/hip_runtime.h>

#include "fft_radix.h"
#include "twiddle4096_f64.inc"

namespace ddsp {
namespace {

__device__ __forceinline__ double2 cmul_d(double2 a, double2 b) {
  return make_double2(fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x));
}

__device__ __forceinline__ double2 twiddle_d(int m) { return reinterpret_cast<const double2*>(kTwiddle4096D)[m]; }

__device__ __forceinline__ void dft2_d(double2& a, double2& b) {
  const double2 s = make_double2(a.x + b.x, a.y + b.y), d = make_double2(a.x - b.x, a.y - b.y);
  a = s;
  b = d;
}

__device__ __forceinline__ void dft4_d(double2& a0, double2& a1, double2& a2, double2& a3) {
  const double2 s02 = make_double2(a0.x + a2.x, a0.y + a2.y);
  const double2 d02 = make_double2(a0.x - a2.x, a0.y - a2.y);
  const double2 s13 = make_double2(a1.x + a3.x, a1.y + a3.y);
  const double2 d13 = make_double2(a1.x - a3.x, a1.y - a3.y);
  const double2 rot = make_double2(d13.y, -d13.x);  // W4 = -i
  a0 = make_double2(s02.x + s13.x, s02.y + s13.y);
  a2 = make_double2(s02.x - s13.x, s02.y - s13.y);
  a1 = make_double2(d02.x + rot.x, d02.y + rot.y);
  a3 = make_double2(d02.x - rot.x, d02.y - rot.y);
}

__device__ __forceinline__ void dft8_d(double2& a0, double2& a1, double2& a2, double2& a3, double2& a4, double2& a5,
                                       double2& a6, double2& a7) {
  dft4_d(a0, a2, a4, a6);
  dft4_d(a1, a3, a5, a7);
  const double h = 0.70710678118654752440;
  const double2 o1 = make_double2((a3.x + a3.y) * h, (a3.y - a3.x) * h);
  const double2 o2 = make_double2(a5.y, -a5.x);
  const double2 o3 = make_double2((a7.y - a7.x) * h, -(a7.x + a7.y) * h);
  const double2 e0 = a0, e1 = a2, e2 = a4, e3 = a6, o0 = a1;
  a0 = make_double2(e0.x + o0.x, e0.y + o0.y);
  a4 = make_double2(e0.x - o0.x, e0.y - o0.y);
  a1 = make_double2(e1.x + o1.x, e1.y + o1.y);
  a5 = make_double2(e1.x - o1.x, e1.y - o1.y);
  a2 = make_double2(e2.x + o2.x, e2.y + o2.y);
  a6 = make_double2(e2.x - o2.x, e2.y - o2.y);
  a3 = make_double2(e3.x + o3.x, e3.y + o3.y);
  a7 = make_double2(e3.x - o3.x, e3.y - o3.y);
}

// 16-point DFT in registers: r = 4 r1 + r0, k = k0 + 4 k1 (as dft16)
__device__ __forceinline__ void dft16_d(double2 (&v)[16]) {
#pragma unroll
  for (int r0 = 0; r0 < 4; ++r0) dft4_d(v[r0], v[4 + r0], v[8 + r0], v[12 + r0]);
#pragma unroll
  for (int r0 = 1; r0 < 4; ++r0)
#pragma unroll
    for (int k0 = 1; k0 < 4; ++k0) v[4 * k0 + r0] = cmul_d(v[4 * k0 + r0], twiddle_d(256 * r0 * k0));
  double2 t[16];
#pragma unroll
  for (int k0 = 0; k0 < 4; ++k0) {
    double2 a0 = v[4 * k0 + 0], a1 = v[4 * k0 + 1], a2 = v[4 * k0 + 2], a3 = v[4 * k0 + 3];
    dft4_d(a0, a1, a2, a3);
    t[k0 + 0] = a0; t[k0 + 4] = a1; t[k0 + 8] = a2; t[k0 + 12] = a3;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = t[i];
}

template <int N, bool SYNC_ENTRY = true>
__device__ __forceinline__ void fft_n_f64(double2 (&v)[16], double2* lds, int t) {
  static_assert(N >= 16 && N <= 4096 && (N & (N - 1)) == 0, "power-of-two N in [16, 4096]");
  constexpr int Q = N / 16;
  constexpr int R = (N == 16 || N == 256 || N == 4096) ? 1 : (N == 32 || N == 512) ? 2 : (N == 64 || N == 1024) ? 4 : 8;
  constexpr int A = (N == 16 || N == 32 || N == 64 || N == 128) ? 1 : (N <= 2048 ? 2 : 3);
  int Ns = 1;
#pragma unroll
  for (int pass = 0; pass < A; ++pass) {
    if (pass > 0) {
      const int step = (t % (1 << (4 * pass))) * (256 >> (4 * pass));
#pragma unroll
      for (int r = 1; r < 16; ++r) v[r] = cmul_d(v[r], twiddle_d(step * r));
    }
    dft16_d(v);
    if (pass == A - 1 && R == 1) return;
    if (pass > 0 || SYNC_ENTRY) __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) lds[lds_idx(out_index(t, Ns, r))] = v[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = lds[lds_idx(t + Q * r)];
    Ns *= 16;
  }
  constexpr int M = 16 / R, STEP = 4096 / N;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int b = t + Q * m;
#pragma unroll
    for (int i = 1; i < R; ++i) v[m + M * i] = cmul_d(v[m + M * i], twiddle_d((b * i * STEP) & 4095));
    if (R == 2) dft2_d(v[m], v[m + M]);
    if (R == 4) dft4_d(v[m], v[m + M], v[m + 2 * M], v[m + 3 * M]);
    if (R == 8)
      dft8_d(v[m], v[m + M], v[m + 2 * M], v[m + 3 * M], v[m + 4 * M], v[m + 5 * M], v[m + 6 * M], v[m + 7 * M]);
  }
}

}  // namespace
}  // namespace ddsp
