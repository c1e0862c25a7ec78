// The realtime stream's device state (ddsp_hip_stream_*): one caller-allocated buffer, zero-filled for a fresh
// stream, shared by the streamed synthesis (synth_frame.hip) and the streamed reverb (stream_reverb.hip):
//   [0, 8 B)           double carry[B]                the running phase prefix per item
//   hist  (16-aligned)  float  hist[B][N]              the reverb's previous input block per item
//   ring  (16-aligned)  float2 ring[B][P][N + 1]       the reverb's frequency-domain delay line: the spectra
//                                                      (bins 0..N of the 2N-point transform) of the last
//                                                      P = ceil(L / N) input windows; call k writes slot k mod P
// A stream without a reverb (ir_length 0) holds the carry alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace ddsp {

struct StreamLayout {
  size_t hist, ring, bytes;
  int64_t P;
};

// call sizes the streamed reverb takes: the 2N-point transform must divide the 4096-entry twiddle table
inline bool stream_block_ok(int64_t n) { return n >= 64 && n <= 2048 && (n & (n - 1)) == 0; }

inline StreamLayout stream_layout(int64_t B, int64_t N, int64_t L) {
  StreamLayout s;
  const size_t carry = (size_t)B * sizeof(double);
  s.P = L > 0 ? (L + N - 1) / N : 0;
  s.hist = (carry + 15) & ~(size_t)15;
  if (L <= 0) {
    s.ring = s.hist;
    s.bytes = carry;
    return s;
  }
  s.ring = (s.hist + (size_t)B * N * sizeof(float) + 15) & ~(size_t)15;
  s.bytes = s.ring + (size_t)B * s.P * (size_t)(N + 1) * sizeof(float2);
  return s;
}

// x modulo 2 pi in fp64 (2 pi as a two-term constant, each product inside an fma): the stream's carry stays
// below 2 pi for ever, and sin(k (x - 2 pi n)) = sin(k x) for the integer harmonic numbers k
__device__ __forceinline__ double wrap_2pi(double x) {
  constexpr double kHi = 6.283185307179586, kLo = 2.4492935982947064e-16;
  const double n = floor(x * (1.0 / kHi));
  return fma(-n, kLo, fma(-n, kHi, x));
}

}  // namespace ddsp
