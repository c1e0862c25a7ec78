// The radix-16 Stockham transform for LDS-resident power-of-two FFTs on gfx950, written once for both precisions:
// fft_n on float2 serves the streamed reverb (stream_reverb.hip) and the multiscale STFT (stft.hip), fft_n on double2
// the analysis kernels (analysis_frames.h says why those run in fp64); the partitioned reverb's fft4096 (upols.hip)
// is built from the same pieces.
// Twiddles come from one 4096-entry table per precision (W_4096^m, fp64-evaluated; the fp32 table rounded once):
// every transform size used here divides 4096.  The launchers' dispatch from a runtime transform size to the
// template argument (for_frame_length) closes the file.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "twiddle4096.inc"

namespace ddsp {
namespace {

__device__ __forceinline__ int lds_idx(int i) { return i + (i >> 4); }

// W_4096^m in C's precision.  The fp64 table is specialised where the fp64 users meet (analysis_frames.h), so a
// unit that transforms in fp32 alone never sees it.
template <class C>
struct TwiddleTable;
template <>
struct TwiddleTable<float2> {
  static __device__ __forceinline__ const float2* data() { return reinterpret_cast<const float2*>(kTwiddle4096); }
};

template <class C>
__device__ __forceinline__ C twiddle(int m, bool inv) {
  const C w = TwiddleTable<C>::data()[m];
  return inv ? C{w.x, -w.y} : w;
}

template <class C>
__device__ __forceinline__ C cmul(C a, C b) {
  return C{fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x)};
}

template <class C>
__device__ __forceinline__ void dft2(C& a, C& b) {
  const C s{a.x + b.x, a.y + b.y}, d{a.x - b.x, a.y - b.y};
  a = s;
  b = d;
}

template <bool INV, class C>
__device__ __forceinline__ void dft4(C& a0, C& a1, C& a2, C& a3) {
  const C s02{a0.x + a2.x, a0.y + a2.y};
  const C d02{a0.x - a2.x, a0.y - a2.y};
  const C s13{a1.x + a3.x, a1.y + a3.y};
  const C d13{a1.x - a3.x, a1.y - a3.y};
  // forward: W4 = -i ; inverse: +i.  (-i)*(x+iy) = y - ix
  const C rot = INV ? C{-d13.y, d13.x} : C{d13.y, -d13.x};
  a0 = C{s02.x + s13.x, s02.y + s13.y};
  a2 = C{s02.x - s13.x, s02.y - s13.y};
  a1 = C{d02.x + rot.x, d02.y + rot.y};
  a3 = C{d02.x - rot.x, d02.y - rot.y};
}

template <bool INV, class C>
__device__ __forceinline__ void dft8(C& a0, C& a1, C& a2, C& a3, C& a4, C& a5, C& a6, C& a7) {
  // radix-2 over two 4-point DFTs of the even / odd inputs
  dft4<INV>(a0, a2, a4, a6);
  dft4<INV>(a1, a3, a5, a7);
  const typename C::value_type h = 0.70710678118654752440;
  // odd outputs times W8^k: k=1: (1 -+ i)/sqrt2, k=2: -+i, k=3: (-1 -+ i)/sqrt2
  const C o1 = INV ? C{(a3.x - a3.y) * h, (a3.x + a3.y) * h} : C{(a3.x + a3.y) * h, (a3.y - a3.x) * h};
  const C o2 = INV ? C{-a5.y, a5.x} : C{a5.y, -a5.x};
  const C o3 = INV ? C{-(a7.x + a7.y) * h, (a7.x - a7.y) * h} : C{(a7.y - a7.x) * h, -(a7.x + a7.y) * h};
  const C e0 = a0, e1 = a2, e2 = a4, e3 = a6, o0 = a1;
  a0 = C{e0.x + o0.x, e0.y + o0.y};
  a4 = C{e0.x - o0.x, e0.y - o0.y};
  a1 = C{e1.x + o1.x, e1.y + o1.y};
  a5 = C{e1.x - o1.x, e1.y - o1.y};
  a2 = C{e2.x + o2.x, e2.y + o2.y};
  a6 = C{e2.x - o2.x, e2.y - o2.y};
  a3 = C{e3.x + o3.x, e3.y + o3.y};
  a7 = C{e3.x - o3.x, e3.y - o3.y};
}

// 16-point DFT in registers: r = 4 r1 + r0, k = k0 + 4 k1.
template <bool INV, class C>
__device__ __forceinline__ void dft16(C (&v)[16]) {
#pragma unroll
  for (int r0 = 0; r0 < 4; ++r0) dft4<INV>(v[r0], v[4 + r0], v[8 + r0], v[12 + r0]);
  // v[4*k0 + r0] now holds u[r0][k0]; internal twiddles W16^{r0*k0} = W4096^{256*r0*k0}
#pragma unroll
  for (int r0 = 1; r0 < 4; ++r0)
#pragma unroll
    for (int k0 = 1; k0 < 4; ++k0) v[4 * k0 + r0] = cmul(v[4 * k0 + r0], twiddle<C>(256 * r0 * k0, INV));
  C t[16];
#pragma unroll
  for (int k0 = 0; k0 < 4; ++k0) {
    C a0 = v[4 * k0 + 0], a1 = v[4 * k0 + 1], a2 = v[4 * k0 + 2], a3 = v[4 * k0 + 3];
    dft4<INV>(a0, a1, a2, a3);
    t[k0 + 0] = a0; t[k0 + 4] = a1; t[k0 + 8] = a2; t[k0 + 12] = a3;  // X[k0 + 4 k1]
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = t[i];
}

// fp32: the twiddles w^r, r = 1..15, of one Stockham pass from four table loads (w, w^2, w^4, w^8): every other
// power is a product of at most three table values (error <= ~3 ulp), so a pass costs 4 global loads instead of 15
// and they can be issued before the LDS phases.  (fp64 reads each of the 15 from its table: no product's rounding.)
struct Tw4 {
  float2 t1, t2, t4, t8;
};

template <bool INV>
__device__ __forceinline__ Tw4 load_tw(int step) {
  Tw4 t;
  t.t1 = twiddle<float2>(step, INV);
  t.t2 = twiddle<float2>(2 * step, INV);
  t.t4 = twiddle<float2>(4 * step, INV);
  t.t8 = twiddle<float2>(8 * step, INV);
  return t;
}

__device__ __forceinline__ void apply_tw(float2 (&v)[16], const Tw4& t) {
  const float2 w3 = cmul(t.t1, t.t2), w5 = cmul(t.t4, t.t1), w6 = cmul(t.t4, t.t2);
  const float2 w7 = cmul(t.t4, w3);
  v[1] = cmul(v[1], t.t1);
  v[2] = cmul(v[2], t.t2);
  v[3] = cmul(v[3], w3);
  v[4] = cmul(v[4], t.t4);
  v[5] = cmul(v[5], w5);
  v[6] = cmul(v[6], w6);
  v[7] = cmul(v[7], w7);
  v[8] = cmul(v[8], t.t8);
  v[9] = cmul(v[9], cmul(t.t8, t.t1));
  v[10] = cmul(v[10], cmul(t.t8, t.t2));
  v[11] = cmul(v[11], cmul(t.t8, w3));
  v[12] = cmul(v[12], cmul(t.t8, t.t4));
  v[13] = cmul(v[13], cmul(t.t8, w5));
  v[14] = cmul(v[14], cmul(t.t8, w6));
  v[15] = cmul(v[15], cmul(t.t8, w7));
}

__device__ __forceinline__ int out_index(int j, int Ns, int r) {
  return (j / Ns) * Ns * 16 + (j & (Ns - 1)) + r * Ns;
}

// Generic Stockham FFT of N = 16^a * r points (r in {1, 2, 4, 8}, N | 4096, N >= 16) on C = float2 or double2, one
// transform per N/16 threads: thread t (< N/16) holds v[i] = in[t + (N/16) i] on entry and out[t + (N/16) i] on
// exit.  lds: this transform's N + N/16 slots of C.  Every thread of the workgroup must call it (it synchronises
// the workgroup between passes).
template <int N, bool INV, bool SYNC_ENTRY = true, class C>
__device__ __forceinline__ void fft_n(C (&v)[16], C* lds, int t) {
  static_assert(N >= 16 && N <= 4096 && (N & (N - 1)) == 0, "power-of-two N in [16, 4096]");
  constexpr bool F32 = std::is_same_v<C, float2>;
  constexpr int Q = N / 16;  // threads per transform
  constexpr int R = (N == 16 || N == 256 || N == 4096) ? 1 : (N == 32 || N == 512) ? 2 : (N == 64 || N == 1024) ? 4 : 8;
  constexpr int A = (N == 16 || N == 32 || N == 64 || N == 128) ? 1 : (N <= 2048 ? 2 : 3);  // radix-16 passes
  // fp32: the twiddles of passes 1.. are loaded up front, so their latency hides behind pass 0
  [[maybe_unused]] Tw4 tw[A > 1 ? A - 1 : 1];
  if constexpr (F32) {
#pragma unroll
    for (int pass = 1; pass < A; ++pass) {
      const int ns = 1 << (4 * pass);
      tw[pass - 1] = load_tw<INV>((t % ns) * (256 / ns));
    }
  }
  int Ns = 1;
#pragma unroll
  for (int pass = 0; pass < A; ++pass) {
    if (pass > 0) {
      if constexpr (F32) {
        apply_tw(v, tw[pass - 1]);
      } else {
        const int step = (t % (1 << (4 * pass))) * (256 >> (4 * pass));
#pragma unroll
        for (int r = 1; r < 16; ++r) v[r] = cmul(v[r], twiddle<C>(step * r, INV));
      }
    }
    dft16<INV>(v);
    if (pass == A - 1 && R == 1) return;  // last pass with Ns = N/16: natural order in registers
    // (SYNC_ENTRY = false: the caller guarantees no thread still reads lds on entry)
    if (pass > 0 || SYNC_ENTRY) __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) lds[lds_idx(out_index(t, Ns, r))] = v[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = lds[lds_idx(t + Q * r)];
    Ns *= 16;
  }
  // final radix-R pass (Ns = N/R): butterfly b = t + Q m reads v[m + (16/R) i], twiddle W_N^{b i}
  constexpr int M = 16 / R, STEP = 4096 / N;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int b = t + Q * m;
#pragma unroll
    for (int i = 1; i < R; ++i) v[m + M * i] = cmul(v[m + M * i], twiddle<C>((b * i * STEP) & 4095, INV));
    if (R == 2) dft2(v[m], v[m + M]);
    if (R == 4) dft4<INV>(v[m], v[m + M], v[m + 2 * M], v[m + 3 * M]);
    if (R == 8)
      dft8<INV>(v[m], v[m + M], v[m + 2 * M], v[m + 3 * M], v[m + 4 * M], v[m + 5 * M], v[m + 6 * M],
                v[m + 7 * M]);
  }
}

// The launchers' one dispatch on the transform size (host): f(std::integral_constant<int, L>{}) for a power of two
// L in [N, MAX), f(<MAX>) for anything else (the entry points have checked L against their envelopes).
template <int N, int MAX = 4096, class F>
inline int for_frame_length(int64_t L, const F& f) {
  if constexpr (N < MAX) {
    return L == N ? f(std::integral_constant<int, N>{}) : for_frame_length<2 * N, MAX>(L, f);
  } else {
    return f(std::integral_constant<int, MAX>{});
  }
}

}  // namespace
}  // namespace ddsp
