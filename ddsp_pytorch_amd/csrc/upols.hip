// Uniformly partitioned FFT convolution (UPOLS) for gfx950.
//
// Replaces the reference's one-shot 2T-point FFT convolution (ddsp/core.py:169-176, used by
// Reverb.forward, ddsp/models/modules.py:28-35) for long signals and kernels.  Only the first
// T outputs of the causal linear convolution are kept, so any exact method is a faithful
// restatement; this one is laid out for the MI355X memory system:
//
//   partition size P = 2048, FFT size N = 4096 (= 16^3: three radix-16 Stockham passes, one
//   workgroup of 256 threads per transform, 16 points per thread, 34 KB of LDS);
//   two real rows sharing one kernel are packed as z = x_a + i*x_b: the kernel is real, so
//   z (*) h = (x_a (*) h) + i (x_b (*) h) — one complex FFT serves two rows with no
//   Hermitian post-processing;
//   the overlap sits on the KERNEL side: the input blocks are zero-padded, the kernel windows
//   overlap by half (q = 0..Q, Q = ceil(L/P), h_{-1} = h_Q = 0):
//   kernel:   G_q = FFT_N([h_{q-1}, h_q]) / N                   (computed once per IR)
//   forward:  Z_b = FFT_N([x_b, 0])                             (upols_forward_kernel)
//   MAC:      Y_b = sum_{q=0..Q} Z_{b-q} G_q   per frequency bin (upols_mac_ring_kernel)
//   inverse:  y[bP, (b+1)P) = last P points of IFFT_N(Y_b)      (upols_inverse_kernel)
//   (circular convolution of [x_{b-q}, 0] with [h_{q-1}, h_q]: its second half holds exactly the
//   terms h[tau] x[bP + n - tau] with tau in ((q-1)P + n, qP + n], so the Q+1 terms cover every
//   tau once.)  Against the input-overlap form (X_b = FFT([x_{b-1}, x_b]) = Z_{b-1} + (-1)^f Z_b,
//   Q kernel spectra) each input sample is read once instead of twice, for one more MAC term.
//
// HBM traffic per real output sample: x read (4 B), Z write/read (16 B), Y write/read (16 B),
// y write (4 B).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "impulse.h"
#include "upols.h"
#include "fft_radix.h"

namespace ddsp {
namespace {

constexpr int kNT = 256;            // threads per transform
constexpr int kPad = kN + kN / 16;  // LDS float2 slots: one pad slot per 16 (bank spreading)

// Full 4096-point transform (three radix-16 Stockham passes, Ns = 1, 16, 256):
// v holds in[j + 256 r] on entry and out[j + 256 r] on exit.
// fft_n<4096, INV, false> but for one barrier: the second sits after the read-back, not before the next store.  Kept:
// with fft_n the uncached-IR step measured 185.3 / 185.6 us against 183.9 / 183.9 (profiles/fft_once_ab.txt).
template <bool INV>
__device__ __forceinline__ void fft4096(float2 (&v)[16], float2* lds, int j = threadIdx.x) {
  // pass twiddle steps: k * N/(Ns*16) with k = j mod Ns
  const Tw4 tw2 = load_tw<INV>((j & 15) * 16);
  const Tw4 tw3 = load_tw<INV>(j);
  dft16<INV>(v);
#pragma unroll
  for (int r = 0; r < 16; ++r) lds[lds_idx(out_index(j, 1, r))] = v[r];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = lds[lds_idx(j + 256 * r)];
  __syncthreads();
  apply_tw(v, tw2);
  dft16<INV>(v);
#pragma unroll
  for (int r = 0; r < 16; ++r) lds[lds_idx(out_index(j, 16, r))] = v[r];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = lds[lds_idx(j + 256 * r)];
  apply_tw(v, tw3);
  dft16<INV>(v);  // Ns = 256: output index == j + 256 r (coalesced)
}

// A transform's registers against one spectrum row: thread j holds elements j + 256 r
__device__ __forceinline__ void row_load16(float2 (&v)[16], const float2* row, int j) {
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = row[j + 256 * r];
}
__device__ __forceinline__ void row_store16(float2* row, const float2 (&v)[16], int j) {
#pragma unroll
  for (int r = 0; r < 16; ++r) row[j + 256 * r] = v[r];
}

// v = G_q = FFT(h[(q-1)P, (q+1)P) (zero outside [0, klen))) / N of one kernel window, h[s] = tap(s, r)
// for the thread's r-th element: the one place a kernel spectrum is built (load, scale, transform).
// The three callers store v with their own loop over out[j + 256 r], not row_store16: through the
// helper the compiler splits that address another way and their register counts move.
template <class Tap>
__device__ __forceinline__ void window_spectrum(float2 (&v)[16], int q, int64_t klen, Tap tap, float2* lds) {
  const int j = threadIdx.x;
  const float inv_n = 1.0f / (float)kN;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t s = (int64_t)(q - 1) * kP + j + 256 * r;
    float h = 0.0f;
    if (s >= 0 && s < klen) h = tap(s, r);
    v[r] = make_float2(h * inv_n, 0.0f);
  }
  fft4096<false>(v, lds);
}

// Complex multiply-accumulate as two packed FMAs (v_pk_fma_f32: two fp32 FMAs per lane per
// instruction): acc += a * b = a.x * (b.x, b.y) + a.y * (-b.y, b.x), with b and its rotation
// formed once per partition and shared by every accumulator.
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void cmac(v2f& acc, float2 a, v2f b, v2f b_rot) {
  acc = __builtin_elementwise_fma((v2f){a.x, a.x}, b, acc);
  acc = __builtin_elementwise_fma((v2f){a.y, a.y}, b_rot, acc);
}

// MAC shape: the register-ring kernel, 25 output blocks per thread, operands prefetched 3 steps
// ahead, a G ring of 3 (25.7-26.7 us at config 2 against 29.3 us for the shifting
// window it replaced)
constexpr int kRingBlk = 25;
constexpr int kRingPF = 3;
constexpr int kRingGR = 3;

// rows of the packed signal: pair -> (row_a, row_b or -1)
__device__ __forceinline__ void pair_rows(int pair, int rows, int pairing, int& ra, int& rb) {
  if (pairing) {
    ra = 2 * pair;
    rb = 2 * pair + 1 < rows ? 2 * pair + 1 : -1;
  } else {
    ra = pair;
    rb = -1;
  }
}

// X[pair][b][:] = FFT(z[(b+off)P, (b+off+2)P)) with one half zeroed; grid (nb, npairs).
//   off = 0, zero_half = 2: Z_b = FFT([z_b, 0]), the zero-padded input blocks (forward);
//   off = -1, zero_half = 1: FFT([0, z_b]), the adjoint of the inverse transform's "keep the
//   second half" (backward).  reverse: z read time-reversed (z'[s] = z[T-1-s], the transposed
//   convolution of the input gradient).
__device__ __forceinline__ void forward_block(const float* __restrict__ x, int64_t ld, int64_t T, int rows,
                                              int pairing, int nb, int off, int zero_half, int reverse,
                                              float2* __restrict__ X, int b, int pair, float2* lds) {
  const int j = threadIdx.x;
  int ra, rb;
  pair_rows(pair, rows, pairing, ra, rb);
  const float* xa = x + (int64_t)ra * ld;
  const float* xb = rb >= 0 ? x + (int64_t)rb * ld : nullptr;
  const int64_t s0 = (int64_t)(b + off) * kP;
  float2 v[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t s = s0 + j + 256 * r;
    const bool ok = s >= 0 && s < T && !(zero_half == 1 && r < 8) && !(zero_half == 2 && r >= 8);
    const int64_t si = reverse ? T - 1 - s : s;
    v[r] = make_float2(ok ? xa[si] : 0.0f, (ok && xb) ? xb[si] : 0.0f);
  }
  fft4096<false>(v, lds);
  row_store16(X + ((int64_t)pair * nb + b) * kN, v, j);
}

__global__ void __launch_bounds__(kNT) upols_forward_kernel(const float* __restrict__ x, int64_t ld,
                                                            int64_t T, int rows, int pairing, int nb,
                                                            int off, int zero_half, int reverse,
                                                            float2* __restrict__ X) {
  __shared__ float2 lds[kPad];
  forward_block(x, ld, T, rows, pairing, nb, off, zero_half, reverse, X, blockIdx.x, blockIdx.y, lds);
}

// The reverb's IR spectrum cached on the device and validated there on every call (Reverb.forward,
// modules.py:21-35, rebuilds it every call; a host-side cache keyed on parameter versions misses
// writes through .data).  Per kernel window q the cache keeps the spectrum G_q and a snapshot of the
// exact inputs it was built from — the noise taps of the window [(q-1)P, (q+1)P) ∩ [0, klen) bit for
// bit, decay, wet, the sample rate and klen + 1 (0 in a zero-filled cache: nothing valid yet).  The
// window's workgroup compares them with the current parameters and rebuilds G_q (as
// upols_impulse_spectrum_kernel does, bit for bit) only when one differs or `force` is set.  Each
// window's snapshot is its own (windows overlap by P taps), so no two workgroups write one word.
constexpr int kSnapWords = 2 * kP + 4;

__device__ __forceinline__ void ir_window(const float* __restrict__ noise, const float* __restrict__ decay,
                                          const float* __restrict__ wet, int64_t klen, float sr, int force, int q,
                                          float2* __restrict__ Hs, uint32_t* __restrict__ snap, float2* lds) {
  const int j = threadIdx.x;
  uint32_t* sq = snap + (int64_t)q * kSnapWords;
  float nv[16];
  bool diff = false;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t s = (int64_t)(q - 1) * kP + j + 256 * r;
    const bool in = s >= 0 && s < klen;
    nv[r] = in ? noise[s] : 0.0f;
    diff |= in && __float_as_uint(nv[r]) != sq[j + 256 * r];
  }
  const float dec = decay[0], wt = wet[0];
  if (j == 0)
    diff |= sq[2 * kP] != __float_as_uint(dec) || sq[2 * kP + 1] != __float_as_uint(wt) ||
            sq[2 * kP + 2] != __float_as_uint(sr) || sq[2 * kP + 3] != (uint32_t)(klen + 1);
  if (!__syncthreads_or(diff || force)) return;  // the cached G_q is this window's spectrum
  const ImpulseParams ip = impulse_params(dec, wt);
  float2 v[16];
  window_spectrum(v, q, klen, [&](int64_t s, int r) { return impulse_tap(ip, s, impulse_env(ip, s, sr), nv[r]); }, lds);
  float2* out = Hs + (int64_t)q * kN;
#pragma unroll
  for (int r = 0; r < 16; ++r) out[j + 256 * r] = v[r];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t s = (int64_t)(q - 1) * kP + j + 256 * r;
    if (s >= 0 && s < klen) sq[j + 256 * r] = __float_as_uint(nv[r]);
  }
  if (j == 0) {
    sq[2 * kP] = __float_as_uint(dec);
    sq[2 * kP + 1] = __float_as_uint(wt);
    sq[2 * kP + 2] = __float_as_uint(sr);
    sq[2 * kP + 3] = (uint32_t)(klen + 1);
  }
}

// The reverb's forward transform (Z_b = FFT([x_b, 0]), grid rows y >= 1: pair y - 1) with the IR cache's
// validation in the same launch (row y = 0, x = window — dispatched first, so the usually trivial
// validation workgroups do not trail the transforms): the MAC that follows reads a spectrum that is
// current, and no launch is added to the step.  npairs == 0: the validation alone.
__global__ void __launch_bounds__(kNT) upols_forward_ir_kernel(
    const float* __restrict__ x, int64_t T, int rows, int nb, float2* __restrict__ X, const float* __restrict__ noise,
    const float* __restrict__ decay, const float* __restrict__ wet, int64_t klen, float sr, int force, int QG,
    float2* __restrict__ Hs, uint32_t* __restrict__ snap) {
  __shared__ float2 lds[kPad];
  if (blockIdx.y == 0) {
    if ((int)blockIdx.x < QG) ir_window(noise, decay, wet, klen, sr, force, blockIdx.x, Hs, snap, lds);
  } else if ((int)blockIdx.x < nb) {
    forward_block(x, T, T, rows, 1, nb, 0, 2, 0, X, blockIdx.x, blockIdx.y - 1, lds);
  }
}

// 8-byte load at byte offset voff of one spectrum row through a raw buffer descriptor (stride 0,
// `bytes` records; offsets at or past `bytes` read as zero).  The row pointer and size are
// wave-uniform, so the descriptor lives in SGPRs.
typedef int i32x2 __attribute__((ext_vector_type(2)));
constexpr int kBufferWord3 = 0x00020000;  // gfx9 raw-buffer DATA_FORMAT word
template <int AUX = 0>  // cache-policy bits of the load (gfx950: 1 sc0, 2 nt, 16 sc1)
__device__ __forceinline__ float2 row_load(const float2* row, int bytes, int voff) {
  const __amdgpu_buffer_rsrc_t r =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float2*>(row), (short)0, bytes, kBufferWord3);
  const i32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, 0, AUX);
  return make_float2(__int_as_float(v.x), __int_as_float(v.y));
}

// G[row][q][:] = FFT(h[row][(q-1)P, (q+1)P) (zero outside [0, klen))) / N, q = 0..Q;
// grid (Q + 1, krows)
__global__ void __launch_bounds__(kNT) upols_kernel_spectrum_kernel(const float* __restrict__ h,
                                                                    int64_t ld, int64_t klen, int QG,
                                                                    float2* __restrict__ Hs) {
  __shared__ float2 lds[kPad];
  const int q = blockIdx.x, row = blockIdx.y, j = threadIdx.x;
  const float* hr = h + (int64_t)row * ld;
  float2 v[16];
  window_spectrum(v, q, klen, [&](int64_t s, int) { return hr[s]; }, lds);
  float2* out = Hs + ((int64_t)row * QG + q) * kN;
#pragma unroll
  for (int r = 0; r < 16; ++r) out[j + 256 * r] = v[r];
}

// Reverb.build_impulse (modules.py:21-26) fused into the IR's partition spectra (modules.py:30-35):
// G[q][:] = FFT(imp[(q-1)P, (q+1)P)) / N with imp[i] = noise[i] exp(-softplus(-decay) t 500) sigmoid(wet),
// t = fl32(i / sr), imp[0] = 1, zero at or past klen — impulse.h's tap, the one reverb.hip's
// build_impulse_kernel stores, so the spectra are those of upols_spectrum(build_impulse(...)) bit for bit.
// One launch instead of two (the impulse never goes to HBM); grid (Q + 1)
__global__ void __launch_bounds__(kNT) upols_impulse_spectrum_kernel(const float* __restrict__ noise,
                                                                     const float* __restrict__ decay,
                                                                     const float* __restrict__ wet, int64_t klen,
                                                                     float sr, int QG, float2* __restrict__ Hs) {
  __shared__ float2 lds[kPad];
  const int q = blockIdx.x, j = threadIdx.x;
  const ImpulseParams ip = impulse_params(decay[0], wet[0]);
  float2 v[16];
  window_spectrum(v, q, klen, [&](int64_t s, int) { return impulse_tap(ip, s, impulse_env(ip, s, sr), noise[s]); }, lds);
  float2* out = Hs + (int64_t)q * kN;
#pragma unroll
  for (int r = 0; r < 16; ++r) out[j + 256 * r] = v[r];
}

// Cache policy of the forward MAC's input-spectra (Z) and kernel-spectra (G) loads: non-temporal (nt; G
// also sc0).  With the default policy the fused synthesis kernel that follows the reverb in the next
// step runs at ~2.2 instead of ~2.38 GHz: the G loads' nt bit removes that, the Z
// loads' adds a little (config-2 step 223.8-226.3 -> 208.3 us, tools/exp_timing.py, same box).
// A/B builds override them (-DDDSP_MAC_ZAUX=0 -DDDSP_MAC_GAUX=0: the round-2 policy).
#ifndef DDSP_MAC_ZAUX
#define DDSP_MAC_ZAUX 2
#endif
#ifndef DDSP_MAC_GAUX
#define DDSP_MAC_GAUX 3
#endif

// The two directions of the MAC, everything in which they differ:
//   forward  Y_b = sum_q Z_{b-q} G_q                     (the lag-q operand of block b is block b - q)
//   adjoint  V_k = (-1)^f sum_q conj(G_q) GZ_{k+q}       (block k + q; (-1)^f dZ_k, the form the
//            forward's inverse kernel takes, see the backward below; one kernel for every pair)
// The ring kernel's chunks of BLK output blocks are laid from the far end of the signal, so the
// partial chunk sits at the end the operands run out at, and only blocks past that one end can lie
// outside the signal: those are the descriptors with no records (zeros) and the outputs not stored.
struct MacForward {
  static constexpr int kStep = -1;  // block index of the operand per lag
  static constexpr int kZAux = DDSP_MAC_ZAUX, kGAux = DDSP_MAC_GAUX;
  // chunks end at the signal's end: the first one may start before block 0
  static __device__ __forceinline__ int chunk_base(int nb, int blk) {
    return nb - (int)(gridDim.y - blockIdx.y) * blk;
  }
  static __device__ __forceinline__ bool in_signal(int m, int) { return m >= 0; }
  static __device__ __forceinline__ int clamped(int m, int) { return max(m, 0); }
  static __device__ __forceinline__ int lags(int base, int, int blk) { return base + blk; }  // that reach block 0
  static __device__ __forceinline__ void operand(float2 h, v2f& hb, v2f& hr) {
    hb = (v2f){h.x, h.y};
    hr = (v2f){-h.y, h.x};
  }
  static __device__ __forceinline__ const float2* kernel_rows(const float2* Hs, int pair, int64_t pair_stride) {
    return Hs + (int64_t)pair * pair_stride;
  }
  static __device__ __forceinline__ float2 output(v2f acc, int) { return make_float2(acc.x, acc.y); }
};
struct MacAdjoint {
  static constexpr int kStep = 1;
  // default cache policy: the forward MAC's non-temporal bits slowed the train step here
  // (0.556 -> 0.565-0.571 ms)
  static constexpr int kZAux = 0, kGAux = 0;
  static __device__ __forceinline__ int chunk_base(int, int blk) { return blockIdx.y * blk; }
  static __device__ __forceinline__ bool in_signal(int m, int nb) { return m < nb; }
  static __device__ __forceinline__ int clamped(int m, int nb) { return min(m, nb - 1); }
  static __device__ __forceinline__ int lags(int base, int nb, int) { return nb - base; }  // that stay below nb
  static __device__ __forceinline__ void operand(float2 h, v2f& hb, v2f& hr) {  // conj(h) and its rotation
    hb = (v2f){h.x, -h.y};
    hr = (v2f){h.y, h.x};
  }
  static __device__ __forceinline__ const float2* kernel_rows(const float2* Hs, int, int64_t) { return Hs; }
  static __device__ __forceinline__ float2 output(v2f acc, int f) {
    const float sgn = (f & 1) ? -1.0f : 1.0f;
    return make_float2(sgn * acc.x, sgn * acc.y);
  }
};

// The same sums with the operand window as a register ring indexed statically.  A thread owns the
// BLK output blocks b0 + d; at lag p it needs the blocks b0 + d + kStep p, a window that slides one
// block per lag (backward in the forward MAC, forward in the adjoint).  The p loop is unrolled by
// the ring size R = BLK + PF - 1, so the slot (m - b0) mod R of block m is a compile-time register
// at every unrolled step and the window never shifts (no v_mov).  After step p's products, the
// block the window reaches PF steps later is loaded into the slot step p freed, and G_{p+PF} into a
// G ring of GR >= PF slots (GR | R): every operand is loaded PF steps before its first use.  The
// unrolled rounds carry no per-step guards (guards made the compiler enter the round through a
// jump table, whose joins forced a wait on every load at every step): steps past the last useful
// one read the zero spectra of out-of-range descriptors (G_q, q >= Q; blocks outside the signal)
// and add exact zeros.  grid (N/256, ceil(nb/BLK), npairs)
template <class Dir, int BLK, int PF, int GR>
__global__ void __launch_bounds__(kNT) upols_mac_ring_kernel(const float2* __restrict__ X,
                                                             const float2* __restrict__ Hs,
                                                             int64_t h_pair_stride, int nb, int Q,
                                                             float2* __restrict__ Y) {
  constexpr int R = BLK + PF - 1;
  static_assert(PF >= 1 && R % GR == 0 && GR >= PF, "ring shapes");
  constexpr int kRow = kN * (int)sizeof(float2);
  constexpr int kStep = Dir::kStep;
  constexpr int kLead = kStep > 0 ? BLK - 1 : 0;  // the window's leading block at lag 0, from b0
  constexpr auto slot = [](int e) { return (e % R + R) % R; };
  const int f = blockIdx.x * kNT + threadIdx.x;
  const int b0 = Dir::chunk_base(nb, BLK);
  const int pair = blockIdx.z;
  // Every spectrum row is read through a buffer descriptor built in SGPRs for that row (base =
  // the row, lane offset = 8 f): no per-lane address arithmetic, and rows outside the signal or
  // the kernel are descriptors with no records, whose loads return 0 without a select.
  const float2* Xrow = X + (int64_t)pair * nb * kN;
  const float2* Hrow = Dir::kernel_rows(Hs, pair, h_pair_stride);
  const int voff = f * (int)sizeof(float2);
  float2 ring[R], g[GR];
  v2f acc[BLK];
  auto zload = [&](int m, float2& dst) {
    dst = row_load<Dir::kZAux>(Xrow + (int64_t)Dir::clamped(m, nb) * kN, Dir::in_signal(m, nb) ? kRow : 0, voff);
  };
  auto gload = [&](int q, float2& dst) {
    dst = row_load<Dir::kGAux>(Hrow + (int64_t)min(q, Q - 1) * kN, q < Q ? kRow : 0, voff);
  };
#pragma unroll
  for (int d = 0; d < BLK; ++d) {
    acc[d] = (v2f){0.f, 0.f};
    zload(b0 + d, ring[d]);
  }
#pragma unroll
  for (int j = 1; j < PF; ++j) zload(b0 + kLead + kStep * j, ring[slot(kLead + kStep * j)]);
#pragma unroll
  for (int j = 0; j < PF; ++j) gload(j, g[j]);
  const int pmax = min(Q, Dir::lags(b0, nb, BLK));
  for (int pb = 0; pb < pmax; pb += R) {
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int p = pb + u;
      v2f hb, hr;
      Dir::operand(g[u % GR], hb, hr);
#pragma unroll
      for (int d = 0; d < BLK; ++d) cmac(acc[d], ring[slot(d + kStep * u)], hb, hr);
      gload(p + PF, g[(u + PF) % GR]);
      zload(b0 + kStep * p + (kStep * PF + kLead), ring[slot(kLead + kStep * (u + PF))]);
      // keep the scheduler from sinking the loads toward their uses (it did, to cut register
      // live ranges, which turned the prefetch into a wait on every load)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  float2* Yp = Y + (int64_t)pair * nb * kN + f;
#pragma unroll
  for (int d = 0; d < BLK; ++d)
    if (Dir::in_signal(b0 + d, nb)) Yp[(int64_t)(b0 + d) * kN] = Dir::output(acc[d], f);
}

// 16-byte access at byte offset voff of a descriptor over two consecutive spectrum rows (`bytes`
// records: 2, 1 or 0 rows; what lies past them reads as zero and is not stored)
typedef int i32x4 __attribute__((ext_vector_type(4)));
template <int AUX>
__device__ __forceinline__ i32x4 row_pair_load(const float2* row, int bytes, int voff) {
  const __amdgpu_buffer_rsrc_t r =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float2*>(row), (short)0, bytes, kBufferWord3);
  return __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, AUX);
}
__device__ __forceinline__ void row_pair_store(float2* row, int bytes, int voff, i32x4 v) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(row, (short)0, bytes, kBufferWord3);
  __builtin_amdgcn_raw_buffer_store_b128(v, r, voff, 0, 0);
}
// v_permlane32_swap_b32: lanes 32-63 of a change places with lanes 0-31 of b
__device__ __forceinline__ void half_swap(int& a, int& b) {
  const auto r = __builtin_amdgcn_permlane32_swap((unsigned)a, (unsigned)b, false, false);
  a = (int)r[0];
  b = (int)r[1];
}
// Two rows (m0, m0 + 1) of two adjacent bins between their memory image and their owners.  In memory
// order (v of a 16-byte access) lanes 0-31 hold bins f0 + 2l, f0 + 2l + 1 of row m0 and lanes 32-63 the
// same bins of row m0 + 1; owned, lane l holds bin f0 + 2l of both rows and lane l + 32 bin f0 + 2l + 1.
// The exchange is its own inverse.
__device__ __forceinline__ void rows_to_bins(i32x4 v, float2& a, float2& b) {
  int ax = v.x, ay = v.y, bx = v.z, by = v.w;
  half_swap(ax, bx);
  half_swap(ay, by);
  a = make_float2(__int_as_float(ax), __int_as_float(ay));
  b = make_float2(__int_as_float(bx), __int_as_float(by));
}
__device__ __forceinline__ i32x4 bins_to_rows(float2 a, float2 b) {
  int ax = __float_as_int(a.x), ay = __float_as_int(a.y), bx = __float_as_int(b.x), by = __float_as_int(b.y);
  half_swap(ax, bx);
  half_swap(ay, by);
  return (i32x4){ax, ay, bx, by};
}

// The same sums for a whole pair row in one thread (nb == NBK, Q <= NQ): every operand block and G_q of
// the bin is loaded once and stays in registers (the ring kernel's two 25-block chunks re-read ~1.5x of
// them: 122 vs 104 MB of Z at config 2), and the outputs stream from the end the window starts at (the
// forward from block 0 up, the adjoint from block NBK - 1 down): a step forms its output block from the
// blocks and kernel windows already in registers and stores it while the loads of later steps are in
// flight, so loads, products and stores overlap inside every wave (grid N/256 x npairs).  Same-box A/Bs
// at config 2 of the 8-byte form of this kernel (one bin per lane in lane order, one block per step,
// profiles/r05_ab_mac_vjp.log), forward: 24.5-24.8 us against 32.1-32.4 us for the ring kernel on boxes
// where the ring runs 32 us (step -3.8 / -6.4 us), equal (25.0 vs 24.9-25.0 us) where the ring runs 25 us;
// adjoint: 23.1-23.2 us against 29.8-29.9 (tools/ab_prof.sh reverb_bwd).  The ring kernel serves the
// other shapes.
//
// The spectra move 16 bytes per lane: 38 buffer_load_dwordx4 + 25 buffer_store_dwordx4 per thread.  As
// 75 + 50 dwordx2 the same sums in the same order ran 24.4-24.9 us in the bench step against 21.6-22.0,
// forward, and 20.9-22.6 against 19.3-19.7, adjoint (the same bytes in half the memory
// instructions; profiles/mac_wide_*.log).  A wave owns 64 consecutive bins f0 .. f0 + 63 of its
// pair; lane l < 32 owns bin f0 + 2l and lane l + 32 bin f0 + 2l + 1 (a bin's sums depend on nothing but
// the bin, so which lane owns it is free).  Rows go two at a time, (m0, m0 + 1) with m0 even, in one
// access whose descriptor spans both: lanes 0-31 move bins f0 + 2l, f0 + 2l + 1 of row m0, lanes 32-63
// the same bins of row m0 + 1 (their offset is one row further), and two v_permlane32_swap per access
// trade the low lanes' second bin for the high lanes' first.  So the steps go in pairs of output blocks,
// the forward's rows (2t, 2t + 1) ascending, the adjoint's (NBK - 2 - 2t, NBK - 1 - 2t) descending; step
// pair t issues the loads of pair t + PF (two Z rows, G_{2(t+PF)} and G_{2(t+PF)+1}) and swaps its own
// pair's rows where it first uses them (swapped where they are loaded, the wait sits behind the load and
// the prefetch is gone).  Each output block's sum is the 8-byte form's, term for term (q ascending, even
// q into acc, odd q into acc2, one final add), so Y is the same bits.  G pairs at or past Q have
// descriptors over the rows that exist (1 or 0): the rest reads as zero without a select, and no cache
// row past Q is read.  224-226 VGPRs: two waves per SIMD, which config 2's grid (2048 waves) fills in
// one round.  The time does not move with PF (1, 2, 3: 20.6-21.9 us in tools/kernel_probe.py; 4:
// 22.0-22.4 us).
template <class Dir, int NBK, int NQ, int PF>
__global__ void __launch_bounds__(kNT) upols_mac_stream_kernel(const float2* __restrict__ X,
                                                               const float2* __restrict__ Hs,
                                                               int64_t h_pair_stride, int nb, int Q,
                                                               float2* __restrict__ Y) {
  static_assert(NBK % 2 == 0, "rows go in pairs");
  constexpr int kRow = kN * (int)sizeof(float2);
  constexpr int kStep = Dir::kStep;
  constexpr int NP = NBK / 2, NG = (NQ + 1) / 2;
  constexpr auto block = [](int s) { return kStep < 0 ? s : NBK - 1 - s; };  // output block of step s
  constexpr auto even_row = [](int t) { return kStep < 0 ? 2 * t : NBK - 2 - 2 * t; };  // of step pair t
  const int lane = threadIdx.x & 63, hi = lane >> 5;
  const int f0 = blockIdx.x * kNT + (threadIdx.x & ~63);
  const int f = f0 + 2 * (lane & 31) + hi;  // the bin this lane owns
  const int voff = (f0 + 2 * (lane & 31)) * (int)sizeof(float2) + hi * kRow;
  const int pair = blockIdx.y;
  const float2* Xrow = X + (int64_t)pair * nb * kN;
  const float2* Hrow = Dir::kernel_rows(Hs, pair, h_pair_stride);
  float2* Yrow = Y + (int64_t)pair * nb * kN;
  i32x4 zp[NP], gp[NG];
  float2 z[NBK], g[2 * NG];
  auto zload = [&](int t) { zp[t] = row_pair_load<Dir::kZAux>(Xrow + (int64_t)even_row(t) * kN, 2 * kRow, voff); };
  auto gload = [&](int u) {
    gp[u] = row_pair_load<Dir::kGAux>(Hrow + (int64_t)min(2 * u, Q - 1) * kN, min(max(Q - 2 * u, 0), 2) * kRow, voff);
  };
#pragma unroll
  for (int t = 0; t < PF; ++t) {
    if (t < NG) gload(t);
    zload(t);
  }
#pragma unroll
  for (int t = 0; t < NP; ++t) {
    const int m0 = even_row(t);
    if (t + PF < NG) gload(t + PF);
    if (t + PF < NP) zload(t + PF);
    __builtin_amdgcn_sched_barrier(0);
    rows_to_bins(zp[t], z[m0], z[m0 + 1]);
    if (t < NG) rows_to_bins(gp[t], g[2 * t], g[2 * t + 1]);
    float2 out[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int s = 2 * t + e, b = block(s);
      v2f acc = {0.f, 0.f}, acc2 = {0.f, 0.f};
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        if (q <= s) {
          v2f hb, hr;
          Dir::operand(g[q], hb, hr);
          if (q & 1) cmac(acc2, z[b + kStep * q], hb, hr);
          else cmac(acc, z[b + kStep * q], hb, hr);
        }
      }
      out[b - m0] = Dir::output((v2f){acc.x + acc2.x, acc.y + acc2.y}, f);
    }
    row_pair_store(Yrow + (int64_t)m0 * kN, 2 * kRow, voff, bins_to_rows(out[0], out[1]));
    __builtin_amdgcn_sched_barrier(0);
  }
}

// The whole-row MAC form (upols_mac_stream_kernel, both directions) for the row length it
// is built for: 50 blocks (config 2's 102400 samples), up to 25 kernel windows (a 1 s IR at 48 kHz);
// loads issued 2 step pairs (4 blocks) ahead
constexpr int kStreamNB = 50, kStreamNQ = 25, kStreamPF = 2;

// y[row][bP + n] = IFFT(Y_b)[P + n]; grid (nb, npairs)
__global__ void __launch_bounds__(kNT) upols_inverse_kernel(const float2* __restrict__ Y, int nb,
                                                            int64_t T, int rows, int pairing, int reverse,
                                                            float* __restrict__ y, int64_t ld) {
  __shared__ float2 lds[kPad];
  const int b = blockIdx.x, pair = blockIdx.y, j = threadIdx.x;
  const float2* in = Y + ((int64_t)pair * nb + b) * kN;
  float2 v[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = in[j + 256 * r];  // not row_load16: it moves this hot kernel's schedule
  fft4096<true>(v, lds);
  int ra, rb;
  pair_rows(pair, rows, pairing, ra, rb);
  float* ya = y + (int64_t)ra * ld;
  float* yb = rb >= 0 ? y + (int64_t)rb * ld : nullptr;
#pragma unroll
  for (int r = 8; r < 16; ++r) {
    const int64_t s = (int64_t)b * kP + j + 256 * r - kP;
    if (s < T) {
      const int64_t so = reverse ? T - 1 - s : s;
      // non-temporal: the reverb's output is not read again by the step (16.6 vs 17.6 us at config 2,
      // the next synthesis launch unchanged, same-box A/B)
      __builtin_nontemporal_store(v[r].x, ya + so);
      if (yb) __builtin_nontemporal_store(v[r].y, yb + so);
    }
  }
}

// Backward of the partitioned convolution (Reverb.forward, modules.py:28-35), the adjoint of
// each forward step (F = unnormalised FFT, its adjoint the unnormalised inverse):
//   y_b = second half of F^-1(Y_b)           ->  dY_b = GZ_b = F([0, g_b])
//   Y_b = sum_q Z_{b-q} G_q                   ->  dZ_k = sum_q conj(G_q) GZ_{k+q}   (the MAC kernels, MacAdjoint)
//                                                 dG_q = sum_b conj(Z_{b-q}) GZ_b  (upols_corr_kernel)
//   Z_b = F([x_b, 0])                         ->  dx_b = first half of F^-1(dZ_b) = second half of
//                                                 F^-1((-1)^f dZ_b), so the forward's inverse kernel applies
//   G_q = F([h_{q-1}, h_q]) / N               ->  dh_p = Re(first half of F^-1(dG_{p+1}) + second half of
//                                                 F^-1(dG_p)) / N = Re(second half of F^-1(dG_p + (-1)^f dG_{p+1})) / N
// For a packed pair (z = x_a + i x_b, g likewise) the real part of F^-1(conj(Z) GZ) is corr_a + corr_b:
// the packed spectra are used as they are.  GZ is shared by both gradients, and Z is the forward's.

// dG_q[f] = sum_{pair in group} sum_j conj(Z[pair][j][f]) * G[pair][j+q][f]: PC consecutive
// lags per thread with a sliding register window of conj(Z).  A workgroup is 64 bins x
// kCorrSlices waves; the waves take interleaved pairs of the group (pair = grp * S + s, stepping
// by groups * S) and are summed through LDS, so the grid has (N/64) * ceil(Q/PC) * groups
// workgroups and only `groups` partial spectra per lag reach HBM.
constexpr int kCorrSlices = 4;
template <int PC>
__global__ void __launch_bounds__(64 * kCorrSlices) upols_corr_kernel(const float2* __restrict__ Xz,
                                                                     const float2* __restrict__ Gw, int nb,
                                                                     int Q, int npairs, int groups,
                                                                     float2* __restrict__ part) {
  __shared__ float2 red[kCorrSlices][PC][64];
  const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
  const int f = blockIdx.x * 64 + lane;
  const int p0 = blockIdx.y * PC;
  const int grp = blockIdx.z;
  const float2 zero = make_float2(0.f, 0.f);
  v2f acc[PC];
#pragma unroll
  for (int d = 0; d < PC; ++d) acc[d] = (v2f){0.f, 0.f};
  for (int pair = grp * kCorrSlices + s; pair < npairs; pair += groups * kCorrSlices) {
    const float2* Xp = Xz + (int64_t)pair * nb * kN + f;
    const float2* Gp = Gw + (int64_t)pair * nb * kN + f;
    float2 win[PC];
#pragma unroll
    for (int d = 0; d < PC; ++d) win[d] = zero;
#pragma unroll 4
    for (int k = p0; k < nb; ++k) {
#pragma unroll
      for (int d = PC - 1; d > 0; --d) win[d] = win[d - 1];
      const float2 xv = Xp[(int64_t)(k - p0) * kN];
      win[0] = make_float2(xv.x, -xv.y);
      const float2 g = Gp[(int64_t)k * kN];
      const v2f gb = {g.x, g.y}, gr = {-g.y, g.x};
#pragma unroll
      for (int d = 0; d < PC; ++d) cmac(acc[d], win[d], gb, gr);
    }
  }
#pragma unroll
  for (int d = 0; d < PC; ++d) red[s][d][lane] = make_float2(acc[d].x, acc[d].y);
  __syncthreads();
  // wave s reduces partitions d = s, s + S, ... over the slices (fixed order: deterministic)
  for (int d = s; d < PC; d += kCorrSlices) {
    float2 t = red[0][d][lane];
#pragma unroll
    for (int q = 1; q < kCorrSlices; ++q) {
      t.x += red[q][d][lane].x;
      t.y += red[q][d][lane].y;
    }
    if (p0 + d < Q) part[((int64_t)grp * Q + p0 + d) * kN + f] = t;
  }
}

// dimp[pP + n] = Re(IFFT(sum_groups part[grp][p] + (-1)^f part[grp][p+1])) [P + n] / N for n < P,
// pP + n < klen (part holds Q + 1 lags; lag Q + 1 is zero), in two kernels:
// sum[p][f] = sum_groups part[grp][p][f] + (-1)^f part[grp][p+1][f] (lag Q + 1 is zero): the group
// reduction spread over the chip (grid (N/256, Qp)) so that the per-lag transform below reads one
// spectrum (with the sum inside the 24 one-lag workgroups, each read 8 groups' spectra alone:
// 14.5 us, per-CU bandwidth)
__global__ void __launch_bounds__(kNT) upols_corr_sum_kernel(const float2* __restrict__ part, int groups, int QG,
                                                             float2* __restrict__ sum, unsigned* __restrict__ arrivals) {
  const int f = blockIdx.x * kNT + threadIdx.x, p = blockIdx.y;
  if (arrivals && f == 0 && p == 0) *arrivals = 0u;  // upols_corr_finish_impulse_kernel's counter
  const bool next = p + 1 < QG;
  const float sg = (f & 1) ? -1.0f : 1.0f;
  float2 v = make_float2(0.f, 0.f);
  for (int g = 0; g < groups; ++g) {
    const float2* in = part + ((int64_t)g * QG + p) * kN + f;
    const float2 w = in[0];
    const float2 w1 = next ? in[kN] : make_float2(0.f, 0.f);
    v.x += w.x + sg * w1.x;
    v.y += w.y + sg * w1.y;
  }
  sum[(int64_t)p * kN + f] = v;
}

// dimp[pP + n] = Re(IFFT(sum[p]))[P + n] / N for n < P, pP + n < klen; grid (Qp)
__global__ void __launch_bounds__(kNT) upols_corr_finish_kernel(const float2* __restrict__ sum, int64_t klen,
                                                                float* __restrict__ dimp) {
  __shared__ float2 lds[kPad];
  const int p = blockIdx.x, j = threadIdx.x;
  float2 v[16];
  row_load16(v, sum + (int64_t)p * kN, j);
  fft4096<true>(v, lds);
  const float inv_n = 1.0f / (float)kN;
#pragma unroll
  for (int r = 8; r < 16; ++r) {
    const int64_t s = (int64_t)p * kP + j + 256 * r - kP;
    if (s < klen) dimp[s] = v[r].x * inv_n;
  }
}

// upols_corr_finish_kernel fused with Reverb.build_impulse's backward (modules.py:21-26; reverb.hip
// impulse_backward_kernel calls the same impulse.h per tap, so d_noise is bit-identical): workgroup p turns its
// 2048 taps of dimp straight into d_noise and fp64 partial sums of sum dimp*noise*env and sum
// dimp*noise*env*t; the last workgroup to arrive (counter zeroed by upols_corr_sum_kernel) reduces the
// partials in index order (deterministic) into d_wet and d_decay and leaves the counter at 0.  Two launches
// fewer in the train step than dimp -> impulse_backward_kernel -> impulse_backward_finish_kernel.
__global__ void __launch_bounds__(kNT) upols_corr_finish_impulse_kernel(
    const float2* __restrict__ sum, int64_t kc, ImpulseGrad ig, double* __restrict__ partials,
    unsigned* __restrict__ arrivals, float* __restrict__ dimp) {
  __shared__ float2 lds[kPad];
  __shared__ double red[32];
  __shared__ bool last;
  const int p = blockIdx.x, j = threadIdx.x, Qp = gridDim.x;
  float2 v[16];
  row_load16(v, sum + (int64_t)p * kN, j);
  // the taps' envelope and noise ahead of the transform (independent of dimp; their latency hides under it)
  const ImpulseParams ip = impulse_params(ig.decay[0], ig.wet[0]);
  float tt[8], env[8], nz[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int64_t i = (int64_t)p * kP + j + 256 * r;
    tt[r] = impulse_time(i, ig.sr);
    env[r] = impulse_env(ip, tt[r]);
    nz[r] = i < ig.L ? ig.noise[i] : 0.0f;
  }
  fft4096<true>(v, lds);
  const float inv_n = 1.0f / (float)kN;
  double aw = 0.0, ad = 0.0;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int64_t i = (int64_t)p * kP + j + 256 * r;
    const float di = v[r + 8].x * inv_n;
    if (dimp && i < kc) dimp[i] = di;
    if (i < ig.L) {
      const float gi = (i >= 1 && i < kc) ? di : 0.0f;
      ig.d_noise[i] = impulse_tap_grad(ip, gi, nz[r], env[r], tt[r], aw, ad);
    }
  }
  // taps past the partitions (an IR longer than the signal): no gradient
  for (int64_t i = (int64_t)Qp * kP + (int64_t)p * kNT + j; i < ig.L; i += (int64_t)Qp * kNT) ig.d_noise[i] = 0.0f;
  block_sum_double2(aw, ad, red);
  if (j == 0) {
    partials[2 * p] = aw;
    partials[2 * p + 1] = ad;
    __threadfence();
    last = atomicAdd(arrivals, 1u) == (unsigned)(Qp - 1);
  }
  __syncthreads();
  if (!last || j >= 64) return;
  __threadfence();
  double sw = 0.0, sd = 0.0;
  for (int i = j; i < Qp; i += 64) {
    sw += __hip_atomic_load(partials + 2 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sd += __hip_atomic_load(partials + 2 * i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sw += __shfl_down(sw, o, 64);
    sd += __shfl_down(sd, o, 64);
  }
  if (j != 0) return;
  impulse_close(ip.w, impulse_slope(ip.d), sw, sd, ig.d_decay, ig.d_wet);
  *arrivals = 0u;
}

}  // namespace

// IR-gradient partial sums: one per group of kCorrSlices pairs, at most 8
static int64_t corr_groups(int64_t npairs) {
  return std::min<int64_t>((npairs + kCorrSlices - 1) / kCorrSlices, 8);
}

int64_t upols_partitions(int64_t klen) { return (std::max<int64_t>(klen, 1) + kP - 1) / kP; }
int64_t upols_blocks(int64_t n) { return (n + kP - 1) / kP; }

// kernel spectra per row: G_0 .. G_Q
static int64_t upols_kernel_windows(int64_t klen) { return upols_partitions(klen) + 1; }

size_t upols_spectrum_floats(int64_t krows, int64_t klen) {
  return (size_t)krows * (size_t)upols_kernel_windows(klen) * kN * 2;
}

size_t upols_workspace_bytes(int64_t rows, int64_t n, bool pairing) {
  const int64_t npairs = pairing ? (rows + 1) / 2 : rows;
  return 2 * (size_t)npairs * (size_t)upols_blocks(n) * kN * sizeof(float2);
}

// The grid limits of every launch here: nb signal blocks (x of the transforms; chunks of kRingBlk on
// the ring MAC's y), rows pairs or kernel rows (y or z), wins kernel windows or lags (x or y: held to
// the y limit wherever they sit).
static int64_t ring_chunks(int64_t nb) { return (nb + kRingBlk - 1) / kRingBlk; }
static bool grid_fits(int64_t nb, int64_t rows, int64_t wins) {
  return nb <= INT32_MAX && ring_chunks(nb) <= 65535 && rows <= 65535 && wins <= 65535;
}

int upols_spectrum(const float* h, int64_t ld, int64_t klen, int64_t krows, float* spectrum,
                   void* stream) {
  const int64_t QG = upols_kernel_windows(klen);
  if (!grid_fits(0, krows, QG)) return DDSP_HIP_EINVAL;
  hipLaunchKernelGGL(upols_kernel_spectrum_kernel, dim3((unsigned)QG, (unsigned)krows), dim3(kNT), 0,
                     S(stream), h, ld, klen, (int)QG, reinterpret_cast<float2*>(spectrum));
  return launch_status();
}

int upols_impulse_spectrum(const float* noise, const float* decay, const float* wet, int64_t klen, float sr,
                           float* spectrum, void* stream) {
  const int64_t QG = upols_kernel_windows(klen);
  if (!grid_fits(0, 0, QG)) return DDSP_HIP_EINVAL;
  hipLaunchKernelGGL(upols_impulse_spectrum_kernel, dim3((unsigned)QG), dim3(kNT), 0, S(stream), noise, decay, wet,
                     klen, sr, (int)QG, reinterpret_cast<float2*>(spectrum));
  return launch_status();
}

// Z[pair][b] = FFT of block b of the packed rows with one half zeroed (zh: 2 = [x_b, 0], 1 = [0, x_b]).
// (Measured slower: a persistent, software-pipelined variant that loads the next block under the
// current transform, 20.5 us vs 18.7 at config 2 with 2 blocks per workgroup, 26 us with 6: each
// transform is a ~4 us latency-bound chain of LDS passes, and fewer resident workgroups expose it.)
static int launch_forward(const float* x, int64_t n, int64_t rows, int pairing, int64_t nb, int64_t npairs, int off,
                          int zh, int reverse, float2* Z, void* stream) {
  hipLaunchKernelGGL(upols_forward_kernel, dim3((unsigned)nb, (unsigned)npairs), dim3(kNT), 0, S(stream), x, n, n,
                     (int)rows, pairing, (int)nb, off, zh, reverse, Z);
  return launch_status();
}

// The MAC of one direction over the block spectra `in`: the whole-row form for the shape it is built
// for, else the ring with kRingBlk (25) output blocks per thread: each operand row is re-read
// (Q+BLK-1)/BLK times through L2 (A/B at config 2, forward: 25 blocks 26.6 us vs 16 blocks 28.3 us, 8
// and 32 no better; measured slower: an LDS-tiled variant that reads Z once, 25%: lower occupancy,
// exposed loads; every operand loaded up front from registers, 40%: 202 VGPRs, 2 waves/SIMD; one thread
// per (pair, bin) streaming all blocks with a register ring, 8%)
template <class Dir>
static int launch_mac(const float2* in, const float* spectrum, int64_t h_stride, int64_t nb, int64_t Q,
                      int64_t npairs, float2* out, void* stream) {
  const float2* Hs = reinterpret_cast<const float2*>(spectrum);
  if (nb == kStreamNB && Q <= kStreamNQ)
    hipLaunchKernelGGL((upols_mac_stream_kernel<Dir, kStreamNB, kStreamNQ, kStreamPF>),
                       dim3(kN / kNT, (unsigned)npairs), dim3(kNT), 0, S(stream), in, Hs, h_stride, (int)nb, (int)Q,
                       out);
  else
    hipLaunchKernelGGL((upols_mac_ring_kernel<Dir, kRingBlk, kRingPF, kRingGR>),
                       dim3(kN / kNT, (unsigned)ring_chunks(nb), (unsigned)npairs), dim3(kNT), 0, S(stream), in, Hs,
                       h_stride, (int)nb, (int)Q, out);
  return launch_status();
}

int upols_apply_spectra(const float2* Z, int64_t rows, int64_t n, const float* spectrum, int64_t klen,
                        bool per_row_kernel, float* y, float2* Y, void* stream, bool reverse) {
  const bool pairing = !per_row_kernel;
  const int64_t npairs = pairing ? (rows + 1) / 2 : rows;
  const int64_t nb = upols_blocks(n);
  const int64_t Q = upols_kernel_windows(std::min(klen, n));
  const int64_t h_stride = per_row_kernel ? upols_kernel_windows(klen) * kN : 0;
  if (!grid_fits(nb, npairs, 0)) return DDSP_HIP_EINVAL;
  int st = launch_mac<MacForward>(Z, spectrum, h_stride, nb, Q, npairs, Y, stream);
  if (st) return st;
  hipLaunchKernelGGL(upols_inverse_kernel, dim3((unsigned)nb, (unsigned)npairs), dim3(kNT), 0, S(stream),
                     Y, (int)nb, n, (int)rows, (int)pairing, (int)reverse, y, n);
  return launch_status();
}

int upols_apply(const float* x, int64_t rows, int64_t n, const float* spectrum, int64_t klen,
                bool per_row_kernel, float* y, void* ws, size_t ws_bytes, void* stream, bool reverse) {
  const bool pairing = !per_row_kernel;
  const int64_t npairs = pairing ? (rows + 1) / 2 : rows;
  const int64_t nb = upols_blocks(n);
  if (!ws || ws_bytes < upols_workspace_bytes(rows, n, pairing)) return DDSP_HIP_EWORKSPACE;
  if (!grid_fits(nb, npairs, 0)) return DDSP_HIP_EINVAL;
  float2* X = reinterpret_cast<float2*>(ws);
  float2* Y = X + (size_t)npairs * nb * kN;
  // Z_b = FFT([x_b, 0])
  int st = launch_forward(x, n, rows, (int)pairing, nb, npairs, 0, 2, (int)reverse, X, stream);
  if (st) return st;
  return upols_apply_spectra(X, rows, n, spectrum, klen, per_row_kernel, y, Y, stream, reverse);
}

size_t upols_ir_cache_bytes(int64_t klen) {
  const int64_t QG = upols_kernel_windows(klen);
  return (size_t)QG * kN * sizeof(float2) + (size_t)QG * kSnapWords * sizeof(uint32_t);
}

int upols_reverb_cached(const float* x, int64_t rows, int64_t n, const float* noise, const float* decay,
                        const float* wet, int64_t klen, float sr, int force, void* cache, float* y, void* ws,
                        size_t ws_bytes, void* stream) {
  const int64_t QG = upols_kernel_windows(klen);
  const int64_t npairs = (rows + 1) / 2;
  const int64_t nb = rows > 0 ? upols_blocks(n) : 0;
  // one launch with blocks and windows on x (both held to the window limit) and a row more than the pairs
  if (!grid_fits(nb, npairs + 1, std::max(nb, QG))) return DDSP_HIP_EINVAL;
  if (rows > 0 && (!ws || ws_bytes < upols_workspace_bytes(rows, n, true))) return DDSP_HIP_EWORKSPACE;
  float2* Hs = reinterpret_cast<float2*>(cache);
  uint32_t* snap = reinterpret_cast<uint32_t*>(Hs + (size_t)QG * kN);
  float2* X = reinterpret_cast<float2*>(ws);
  hipLaunchKernelGGL(upols_forward_ir_kernel, dim3((unsigned)std::max(nb, QG), (unsigned)(npairs + 1)), dim3(kNT), 0,
                     S(stream), x, n, (int)rows, (int)nb, X, noise, decay, wet, klen, sr, force, (int)QG, Hs, snap);
  int st = launch_status();
  if (st || rows == 0) return st;
  return upols_apply_spectra(X, rows, n, reinterpret_cast<const float*>(Hs), klen, false, y,
                             X + (size_t)npairs * nb * kN, stream, false);
}

size_t upols_spectra_bytes(int64_t rows, int64_t n) {
  const int64_t npairs = (rows + 1) / 2;
  return (size_t)npairs * upols_blocks(n) * kN * sizeof(float2);
}

static size_t impulse_scratch_bytes(int64_t Q) { return 256 + (((size_t)Q * 2 * sizeof(double) + 255) & ~(size_t)255); }

size_t upols_backward_workspace_bytes(int64_t rows, int64_t n, int64_t klen, bool have_x) {
  const int64_t Q = upols_kernel_windows(std::min(klen, n));
  const int64_t groups = corr_groups((rows + 1) / 2);
  // + the fused impulse gradient's partial sums and arrival counter (upols_corr_finish_impulse_kernel)
  return (have_x ? 2 : 3) * upols_spectra_bytes(rows, n) + (size_t)(groups + 1) * Q * kN * sizeof(float2) +
         impulse_scratch_bytes(Q);
}

int upols_backward(const float* x, const float* x_spectra, const float* spectrum, const float* g, int64_t rows,
                   int64_t n, int64_t klen, float* dx, float* dimp, void* ws, size_t ws_bytes, void* stream,
                   const ImpulseGrad* ig) {
  const int64_t npairs = (rows + 1) / 2;
  const int64_t nb = upols_blocks(n);
  const int64_t kc = std::min(klen, n);
  const int64_t Qp = upols_partitions(kc), Q = Qp + 1;  // output partitions of dimp; kernel windows
  const int64_t groups = corr_groups(npairs);
  const bool need_x = (dimp || ig) && !x_spectra;
  if (!ws || ws_bytes < upols_backward_workspace_bytes(rows, n, klen, !need_x)) return DDSP_HIP_EWORKSPACE;
  if (!grid_fits(nb, npairs, Q)) return DDSP_HIP_EINVAL;
  const size_t sb = upols_spectra_bytes(rows, n);
  char* w = reinterpret_cast<char*>(ws);
  float2* GZ = reinterpret_cast<float2*>(w);
  float2* V = reinterpret_cast<float2*>(w + sb);
  float2* part = reinterpret_cast<float2*>(w + 2 * sb);
  const bool want_imp = dimp || ig;
  char* scratch = w + 2 * sb + (size_t)(groups + 1) * Q * kN * sizeof(float2);
  unsigned* arrivals = reinterpret_cast<unsigned*>(scratch);
  double* partials = reinterpret_cast<double*>(scratch + 256);
  float2* Xs = need_x ? reinterpret_cast<float2*>(scratch + impulse_scratch_bytes(Q))
                      : const_cast<float2*>(reinterpret_cast<const float2*>(x_spectra));
  // GZ_b = F([0, g_b])
  int st = launch_forward(g, n, rows, 1, nb, npairs, -1, 1, 0, GZ, stream);
  if (st) return st;
  if (dx) {
    if ((st = launch_mac<MacAdjoint>(GZ, spectrum, 0, nb, Q, npairs, V, stream))) return st;
    hipLaunchKernelGGL(upols_inverse_kernel, dim3((unsigned)nb, (unsigned)npairs), dim3(kNT), 0, S(stream), V,
                       (int)nb, n, (int)rows, 1, 0, dx, n);
    if ((st = launch_status())) return st;
  }
  if (want_imp) {
    if (need_x) {
      if (!x) return DDSP_HIP_EINVAL;
      if ((st = launch_forward(x, n, rows, 1, nb, npairs, 0, 2, 0, Xs, stream))) return st;
    }
    // Every pass over the spectra covers PC lags, so the fewest passes win: PC = 13 up to 13 kernel
    // windows, else 25 (Q = 25 at config 2: 8 lags per pass, 37.1 us -> 13, 26.8 -> 25, 24.7-25.0 us;
    // 25 lags with 2 waves per workgroup and 16 groups 26.3, 1 wave and 32 groups 28.2)
    if (Q <= 13)
      hipLaunchKernelGGL(upols_corr_kernel<13>, dim3(kN / 64, 1, (unsigned)groups), dim3(64 * kCorrSlices), 0,
                         S(stream), Xs, GZ, (int)nb, (int)Q, (int)npairs, (int)groups, part);
    else
      hipLaunchKernelGGL(upols_corr_kernel<25>, dim3(kN / 64, (unsigned)((Q + 24) / 25), (unsigned)groups),
                         dim3(64 * kCorrSlices), 0, S(stream), Xs, GZ, (int)nb, (int)Q, (int)npairs, (int)groups,
                         part);
    if ((st = launch_status())) return st;
    float2* psum = part + (size_t)groups * Q * kN;
    hipLaunchKernelGGL(upols_corr_sum_kernel, dim3(kN / kNT, (unsigned)Qp), dim3(kNT), 0, S(stream), part,
                       (int)groups, (int)Q, psum, ig ? arrivals : nullptr);
    if ((st = launch_status())) return st;
    if (ig)
      hipLaunchKernelGGL(upols_corr_finish_impulse_kernel, dim3((unsigned)Qp), dim3(kNT), 0, S(stream), psum, kc, *ig,
                         partials, arrivals, dimp);
    else
      hipLaunchKernelGGL(upols_corr_finish_kernel, dim3((unsigned)Qp), dim3(kNT), 0, S(stream), psum, kc, dimp);
    if ((st = launch_status())) return st;
  }
  return DDSP_HIP_OK;
}

}  // namespace ddsp
