// The pitch (f0) gradient of the frame-rate synthesis (modules.py:69-80 through core.py:136-141): what the
// reference's autograd sends into f0 through torch.cumsum and torch.sin.  remove_above_nyquist is a comparison
// (zero gradient), and the frame's harmonic amplitudes A_k are constants of the frame with respect to f0.
//
// With the phase of the frame kernels, omega_{f,j} = S0_f + (j+1) inc_f for sample j < bs of frame f,
// inc_f = phase_inc(f0_f, sr) = c f0_f (c = 2 pi / sr) and S0_f = bs sum_{f'<f} inc_{f'}:
//   q_{f,j} = g_{f,j} sum_k k A_{f,k} cos(fl32(omega_{f,j} k))      dL/d omega at that sample
//   Q_f = sum_j q_{f,j},   R_f = sum_j (j+1) q_{f,j}
//   dL/d f0_f = c (R_f + bs sum_{f'>f} Q_{f'})
// The sums over (j, k) are swapped, C_k = sum_j g_j cos(.), C'_k = sum_j (j+1) g_j cos(.), so that
// Q = sum_k k A_k C_k and R = sum_k k A_k C'_k: the loop shape of harmonic_vjp_kernel's sines (backward.hip), one
// (omega, g) pair from LDS feeding several harmonic chains.  The frame's set-up (phase convention, table, segment
// shape, controls) is the one of that kernel: harmonic_frame.h.
//
// Two launches: frame_pitch_grad_kernel writes (Q_f, R_f) as two doubles per frame, pitch_grad_scan_kernel makes
// the exclusive reverse scan of Q over each item's frames and writes the gradient.  Past kPrefixMinFrames frames
// per item a ddsp_hip_frame_phase_prefix launch ahead of them precomputes S0 (as the fused forward does).
//
// The per-sample op (core.py:136-141 at f0 [B,T,1]) has no such frames: its f0 gradient would be a scan over T,
// a different kernel, and the host layer keeps refusing it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "common.h"
#include "harmonic_frame.h"

namespace ddsp {
namespace {

constexpr int kScanChunk = 256;  // frames per step of the reverse scan (= its workgroup's threads)

// cos(2 pi y) on the hardware cosine (v_cos_f32 takes revolutions, as v_sin_f32)
__device__ __forceinline__ float cos_rev(float y) { return __builtin_amdgcn_cosf(y); }

// arguments beyond kFastArgLimit: the fp64 cosine of the exact fp32 value, rounded (mirrors sin_slow)
__device__ __noinline__ float cos_slow(float x) { return (float)cos((double)x); }

// One workgroup per (item, frame), on harmonic_frame.h's set-up (phases 1 and 2): item (kq, s) of the ceil(H/4) x
// NS grid sums g_t cos(w_t k) and (t+1) g_t cos(w_t k) for the 4 harmonics k = 4kq+1..4kq+4 over segment s of the
// frame's samples.  PARAMS: A_k from the raw projection param[B,F,H+1], else from the frame controls amp[B,F],
// normalised dist[B,F,H].  prefix (nullable): S0 per frame.
template <bool PARAMS>
__global__ void __launch_bounds__(512) frame_pitch_grad_kernel(
    const float* __restrict__ f0, const float* __restrict__ grad, const float* __restrict__ param,
    const float* __restrict__ amp, const float* __restrict__ dist, const double* __restrict__ prefix,
    double* __restrict__ qr, int F, int H, int bs, float sr, int NS) {
  extern __shared__ float smem[];
  __shared__ double red[32];
  __shared__ int fast_s;
  const int tid = threadIdx.x, NT = blockDim.x;
  const HarmonicFrame fr =
      harmonic_frame_setup<PARAMS>(smem, red, 2 * NS * H, f0, grad, param, amp, dist, prefix, F, H, bs, sr, NS);
  const float2* wg = fr.wg;
  float* partc = fr.own;          // [NS * H] C_k per segment
  float* partd = partc + NS * H;  // [NS * H] C'_k per segment
  const float* uk = fr.uk;
  const int SL = fr.SL;
  if (tid == 0) {
    const float w0 = (float)(fr.S0 + fr.dinc), w1 = (float)(fr.S0 + (double)bs * fr.dinc);
    fast_s = fmaxf(fabsf(w0), fabsf(w1)) * (float)H < kFastArgLimit;
  }
  __syncthreads();

  // ---- phase 3: C_k = sum_t g_t cos(w_t k), C'_k = sum_t (t+1) g_t cos(w_t k) ----
  const int KQ = (H + kKPT - 1) / kKPT;
  for (int item = tid; item < KQ * NS; item += NT) {
    const int s = item / KQ, kq = item - s * KQ;
    const int j0 = s * SL, j1 = min(j0 + SL, bs);
    float kf[kKPT], c0[kKPT], d0[kKPT];
#pragma unroll
    for (int c = 0; c < kKPT; ++c) {
      kf[c] = (float)(kKPT * kq + c + 1);
      c0[c] = 0.0f;
      d0[c] = 0.0f;
    }
    if (fast_s) {
      float c1[kKPT], d1[kKPT];
#pragma unroll
      for (int c = 0; c < kKPT; ++c) {
        c1[c] = 0.0f;
        d1[c] = 0.0f;
      }
      asm volatile(".p2align 3");
      const float2* wq = wg + j0;
      float t1 = (float)(j0 + 1);  // the sample's weight j + 1 (exact: <= 8192 + 64)
      for (int i = 0; i < SL; i += 2) {  // two samples per iteration: 8 independent cosine chains
        const float2 p = wq[i], p1 = wq[i + 1];
        const float gt = p.y * t1, gt1 = p1.y * (t1 + 1.0f);
        t1 += 2.0f;
        float y[2 * kKPT];
#pragma unroll
        for (int c = 0; c < kKPT; ++c) {
          y[c] = cos_rev(reduce_rev(p.x * kf[c]));
          y[kKPT + c] = cos_rev(reduce_rev(p1.x * kf[c]));
        }
#pragma unroll
        for (int c = 0; c < kKPT; ++c) {
          c0[c] = fmaf(p.y, y[c], c0[c]);
          d0[c] = fmaf(gt, y[c], d0[c]);
          c1[c] = fmaf(p1.y, y[kKPT + c], c1[c]);
          d1[c] = fmaf(gt1, y[kKPT + c], d1[c]);
        }
      }
#pragma unroll
      for (int c = 0; c < kKPT; ++c) {
        c0[c] += c1[c];
        d0[c] += d1[c];
      }
    } else {
      for (int j = j0; j < j1; ++j) {
        const float2 p = wg[j];
        const float gt = p.y * (float)(j + 1);
#pragma unroll
        for (int c = 0; c < kKPT; ++c) {
          const float x = p.x * kf[c];
          const float v = fabsf(x) < kFastArgLimit ? cos_rev(reduce_rev(x)) : cos_slow(x);
          c0[c] = fmaf(p.y, v, c0[c]);
          d0[c] = fmaf(gt, v, d0[c]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < kKPT; ++c)
      if (kKPT * kq + c < H) {
        partc[s * H + kKPT * kq + c] = c0[c];
        partd[s * H + kKPT * kq + c] = d0[c];
      }
  }
  __syncthreads();

  // ---- phase 4: Q = sum_k k A_k C_k, R = sum_k k A_k C'_k over segments and harmonics in fp64 ----
  double q = 0.0, r = 0.0;
  for (int k = tid; k < H; k += NT) {
    double ck = 0.0, dk = 0.0;
    for (int s = 0; s < NS; ++s) {
      ck += (double)partc[s * H + k];
      dk += (double)partd[s * H + k];
    }
    const double w = (double)(k + 1) * ((double)fr.a * (double)uk[k]);
    q += w * ck;
    r += w * dk;
  }
  block_sum_double2(q, r, red);
  if (tid == 0) {
    qr[2 * fr.frame] = q;
    qr[2 * fr.frame + 1] = r;
  }
}

// d_f0[b,f] = (float)(c (R_f + bs sum_{f'>f} Q_{f'})), one workgroup per item: an exclusive reverse scan of Q in
// fp64 over chunks of kScanChunk frames, walked from the last chunk to the first with a running suffix (any F).
__global__ void __launch_bounds__(kScanChunk) pitch_grad_scan_kernel(const double* __restrict__ qr,
                                                                     float* __restrict__ d_f0, int F, int bs,
                                                                     float sr) {
  __shared__ double sc[kScanChunk];
  const int b = blockIdx.x, tid = threadIdx.x;
  const double* qb = qr + 2 * (int64_t)b * F;
  float* out = d_f0 + (int64_t)b * F;
  const double c = 6.283185307179586476925 / (double)sr;
  double carry = 0.0;  // sum of Q over the frames after the chunk
  for (int base = ((F - 1) / kScanChunk) * kScanChunk; base >= 0; base -= kScanChunk) {
    const int f = base + tid;
    const double own = f < F ? qb[2 * f] : 0.0;
    sc[tid] = own;
    __syncthreads();
    double v = own;  // inclusive suffix sum within the chunk (Hillis-Steele)
    for (int o = 1; o < kScanChunk; o <<= 1) {
      const double add = tid + o < kScanChunk ? sc[tid + o] : 0.0;
      __syncthreads();
      v += add;
      sc[tid] = v;
      __syncthreads();
    }
    if (f < F) out[f] = (float)(c * (qb[2 * f + 1] + (double)bs * (carry + (v - own))));
    carry += sc[0];
    __syncthreads();  // sc[0] read before the next chunk overwrites it
  }
}

size_t pitch_grad_ws_bytes(int64_t batch, int64_t frames) {
  if (batch <= 0 || frames <= 0) return 0;
  const size_t rows = (size_t)batch * (size_t)frames;
  return sizeof(double) * rows * (frames > kPrefixMinFrames ? 3 : 2);
}

// params != nullptr: the raw-projection form, else the frame-control form
int pitch_grad_launch(const float* f0, const float* param, const float* amp, const float* dist, const float* grad,
                      float* grad_f0, int64_t batch, int64_t frames, int64_t H, int64_t bs, float sr,
                      void* workspace, size_t workspace_bytes, void* stream) {
  if (batch < 0 || frames < 0 || bs < 1 || H < 1 || !(sr > 0)) return DDSP_HIP_EINVAL;
  if (batch == 0 || frames == 0) return DDSP_HIP_OK;
  if (!f0 || !grad || !grad_f0 || !(param || (amp && dist))) return DDSP_HIP_EINVAL;
  if (batch > 65535 || frames > INT32_MAX / 4 || H > 4096 || bs > 8192) return DDSP_HIP_ERANGE;
  if (!workspace || ((uintptr_t)workspace & 7)) return DDSP_HIP_EINVAL;
  if (workspace_bytes < pitch_grad_ws_bytes(batch, frames)) return DDSP_HIP_EWORKSPACE;
  int nt, ns;
  harmonic_backward_shape((int)H, (int)bs, nt, ns);
  const size_t shm = sizeof(float) * harmonic_frame_lds_floats((int)H, (int)bs, ns, (size_t)2 * ns * H);
  if (shm > 150 * 1024) return DDSP_HIP_ERANGE;
  double* qr = static_cast<double*>(workspace);
  double* prefix = nullptr;
  if (frames > kPrefixMinFrames) {
    prefix = qr + 2 * batch * frames;
    const int st = ddsp_hip_frame_phase_prefix(f0, batch, frames, bs, sr, prefix, stream);
    if (st) return st;
  }
  const dim3 grid((unsigned)frames, (unsigned)batch);
  if (param)
    hipLaunchKernelGGL((frame_pitch_grad_kernel<true>), grid, dim3(nt), shm, S(stream), f0, grad, param, amp, dist,
                       prefix, qr, (int)frames, (int)H, (int)bs, sr, ns);
  else
    hipLaunchKernelGGL((frame_pitch_grad_kernel<false>), grid, dim3(nt), shm, S(stream), f0, grad, param, amp, dist,
                       prefix, qr, (int)frames, (int)H, (int)bs, sr, ns);
  int st = launch_status();
  if (st) return st;
  hipLaunchKernelGGL(pitch_grad_scan_kernel, dim3((unsigned)batch), dim3(kScanChunk), 0, S(stream), qr, grad_f0,
                     (int)frames, (int)bs, sr);
  return launch_status();
}

}  // namespace
}  // namespace ddsp

using namespace ddsp;

extern "C" {

size_t ddsp_hip_frame_pitch_grad_workspace_size(int64_t batch, int64_t frames) {
  return pitch_grad_ws_bytes(batch, frames);
}

int64_t ddsp_hip_frame_pitch_grad_scan_chunk(void) { return kScanChunk; }

int ddsp_hip_harmonic_synth_frames_pitch_grad(const float* f0, const float* amplitudes, const float* distribution,
                                              const float* grad, float* grad_f0, int64_t batch, int64_t frames,
                                              int64_t n_harmonic, int64_t block_size, float sample_rate,
                                              void* workspace, size_t workspace_bytes, void* stream) {
  if (batch > 0 && frames > 0 && (!amplitudes || !distribution)) return DDSP_HIP_EINVAL;
  return pitch_grad_launch(f0, nullptr, amplitudes, distribution, grad, grad_f0, batch, frames, n_harmonic,
                           block_size, sample_rate, workspace, workspace_bytes, stream);
}

int ddsp_hip_harmonic_synth_params_pitch_grad(const float* f0, const float* param, const float* grad, float* grad_f0,
                                              int64_t batch, int64_t frames, int64_t n_harmonic, int64_t block_size,
                                              float sample_rate, void* workspace, size_t workspace_bytes,
                                              void* stream) {
  if (batch > 0 && frames > 0 && !param) return DDSP_HIP_EINVAL;
  return pitch_grad_launch(f0, param, nullptr, nullptr, grad, grad_f0, batch, frames, n_harmonic, block_size,
                           sample_rate, workspace, workspace_bytes, stream);
}

}  // extern "C"
