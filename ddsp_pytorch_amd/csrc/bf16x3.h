// The exact three-term bf16 split ("bf16x3") of fp32 operands for the bf16 matrix cores, and the product of two
// splits: csrc/dense.hip's MLP blocks, Linear, projections and weight gradient, csrc/gru.hip's persistent
// recurrence and BPTT.
//
// v = hi + mid + lo with hi = v with its low 16 bits cleared, mid the same of v - hi, lo = v - hi - mid — each
// subtraction exact, each term 8 significant bits, together all 24 of the fp32 significand; summed as the six
// products hi.hi, hi.mid, mid.hi, hi.lo, lo.hi, mid.mid (each exact in fp32; the dropped ones are below 2^-24 of
// the product) a product of two splits is fp32-accurate.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ddsp {

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x2v_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

// the high halves (the bf16 terms) of two fp32 words as one fragment word, the lower element first
__device__ __forceinline__ uint32_t pack_bf16_pair(uint32_t e0, uint32_t e1) {
  return __builtin_amdgcn_perm(e1, e0, 0x07060302u);
}

// 8 floats -> their exact three-term bf16 split, packed as MFMA fragments (element e = value e).  Two forms
// with the same bits: this one subtracts element by element, from two float4 as loaded (the x W^T kernels, the
// recurrence); split_bf16x3_pk below forms the residuals two at a time for the weight gradient, which splits
// both operands of every chunk.  Each kernel keeps the form it was measured with.
__device__ __forceinline__ void split_bf16x3(const float4& a, const float4& b, u32x4_t& hi, u32x4_t& mid,
                                             u32x4_t& lo) {
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t h[8], m[8], l[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const uint32_t u = __float_as_uint(v[e]);
    h[e] = u & 0xffff0000u;
    const float r1 = v[e] - __uint_as_float(h[e]);  // exact
    m[e] = __float_as_uint(r1) & 0xffff0000u;
    l[e] = __float_as_uint(r1 - __uint_as_float(m[e]));  // exact, <= 8 significant bits
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    hi[e] = pack_bf16_pair(h[2 * e], h[2 * e + 1]);
    mid[e] = pack_bf16_pair(m[2 * e], m[2 * e + 1]);
    lo[e] = pack_bf16_pair(l[2 * e], l[2 * e + 1]);
  }
}

// The packed-subtraction form: the two exact residual subtractions on fp32 pairs (v_pk_add_f32), 8 floats from
// an array.
__device__ __forceinline__ void split_bf16x3_pk(const float* v, u32x4_t& hi, u32x4_t& mid, u32x4_t& lo) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t u0 = __float_as_uint(v[2 * e]), u1 = __float_as_uint(v[2 * e + 1]);
    const f32x2v_t x = {v[2 * e], v[2 * e + 1]};
    const f32x2v_t h = {__uint_as_float(u0 & 0xffff0000u), __uint_as_float(u1 & 0xffff0000u)};
    const f32x2v_t r = x - h;  // exact
    const uint32_t m0 = __float_as_uint(r.x) & 0xffff0000u, m1 = __float_as_uint(r.y) & 0xffff0000u;
    const f32x2v_t l = r - (f32x2v_t){__uint_as_float(m0), __uint_as_float(m1)};  // exact
    hi[e] = pack_bf16_pair(u0, u1);
    mid[e] = pack_bf16_pair(m0, m1);
    lo[e] = pack_bf16_pair(__float_as_uint(l.x), __float_as_uint(l.y));
  }
}

__device__ __forceinline__ bf16x8_t as_bf16x8(const u32x4_t& v) { return __builtin_bit_cast(bf16x8_t, v); }

// c + a b for 16 x 16 x 32 tiles of two splits (v_mfma_f32_16x16x32_bf16): the six products, small terms first —
// mid.mid, lo.hi, hi.lo, mid.hi, hi.mid, hi.hi.  The order fixes the result's bits; every bf16x3 kernel sums in
// this one.
__device__ __forceinline__ f32x4_t mfma_bf3(const u32x4_t& ah, const u32x4_t& am, const u32x4_t& al,
                                            const u32x4_t& bh, const u32x4_t& bm, const u32x4_t& bl, f32x4_t c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(am), as_bf16x8(bm), c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(al), as_bf16x8(bh), c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(ah), as_bf16x8(bl), c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(am), as_bf16x8(bh), c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(ah), as_bf16x8(bm), c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(ah), as_bf16x8(bh), c, 0, 0, 0);
}

}  // namespace ddsp
