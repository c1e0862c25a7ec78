// Viterbi-decoded pitch per call of a stream: the salience of the call's frames (one launch), then the carried decode
// with a fixed-lag decision (one launch).  include/ddsp_hip.h ("pitch_viterbi_stream") holds the definition;
// tests/stream_viterbi_ref.py restates it in numpy.
//
// Salience: stream_pitch_kernel's grid, workgroup and ring copy around salience_role (analysis_bodies.h, the role
// pitch_viterbi.hip's kernel shells) over the call's StreamFetch.  With the raw outputs asked for, yin_pick runs on
// the same d': ddsp_hip_stream_pitch's bits.
//
// Decode: one workgroup per item, one thread per bin, pitch_viterbi_kernel's recursion out of the same pieces
// (viterbi_rows and wave_argmin shared; the neighbour loop and the fold written out as there): delta in LDS as two padded
// fp64 rows written in turn, one barrier per frame, the next frame's cost loaded ahead of it.  The row comes from
// the state's delta[k & 1] and goes to delta[(k + 1) & 1]; the call's cost and f0c go into the ring before the
// recursion starts (independent loads and stores), so the frame loop stores back-offsets alone.  Each frame's argmin
// costs no barrier of its own: a thread reduces the value it has just computed inside its wave (take_min, a fixed
// order), lane 0 leaves the wave's pair in LDS, and the frame's barrier publishes it with the row; after the last
// frame, thread jj < R folds frame jj's at most 16 pairs in wave order and walks its min(D, n) back-offsets, the R
// walks side by side.
// The ring of back-offsets is walked in global memory, not staged: a walk reads min(D, n) bytes, one per frame,
// out of a ring of (D + R) n_bins bytes (96 KB at the caps, past the 64 KB a workgroup may declare, and a coalesced
// staging pass would move all of it to use D R bytes); the lines are in L2, written by this workgroup this call or
// the calls just before.  The workgroup reads what it wrote to the state only after the last frame's barrier.
// Fixed orders, no atomics.
#include <hip/hip_runtime.h>

#include "analysis_bodies.h"

namespace ddsp {
namespace {

constexpr int kViterbiMaxLag = 64;  // D cap: the ring holds D + R frames

// grid (ceil(frames / (kPoints/N)), B), kPoints/16 threads; cost / f0c / lag [B, frames, n_bins], f0 / conf /
// period [B, frames] (f0 == nullptr: the pick is not run).  The item's workgroups share the ring copy
// (analysis_frames.h: no workgroup reads what another writes).
template <int N>
__global__ void __launch_bounds__(kPoints<N> / 16) stream_pitch_salience_kernel(
    const float* __restrict__ x, const uint64_t* __restrict__ counter, float* ring, int n, int len, int hs, int hop,
    int frames, PitchParams p, const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, int n_bins,
    float* __restrict__ cost, float* __restrict__ f0c, int32_t* __restrict__ lag, float* __restrict__ f0,
    float* __restrict__ conf, int32_t* __restrict__ period) {
  constexpr int TPW = kPoints<N> / N;
  __shared__ double2 lds_all[TPW * (N + N / 16)];
  __shared__ double wsum[4];
  __shared__ int rint[8];
  const int b = blockIdx.y;
  const StreamFetch fetch = open_stream_call(*counter, ring, x, n, len, hs, hop, frames, b,
                                             blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
  salience_role<N>(fetch, blockIdx.x, lds_all, wsum, rint, p, b, lo, hi, n_bins, cost, f0c, lag, f0, conf, period);
}

// The decode's state, per item: double delta[2][NB], then the ring of P = D + R frames as float f0c[P][NB],
// float cost[P][NB], int8 bp[P][NB] (slot n mod P), rounded up to 8 bytes so that the next item's doubles align.
struct ViterbiStateLayout {
  size_t item_bytes;
  int P;
};

inline ViterbiStateLayout viterbi_state_layout(int64_t R, int64_t NB, int64_t D) {
  const size_t P = (size_t)(D + R);
  return {(16 * (size_t)NB + 9 * P * (size_t)NB + 7) / 8 * 8, (int)P};
}

// grid B, n_bins rounded up to whole waves; cost / f0c [B, R, NB]; f0 / conf / path [B, R]
__global__ void __launch_bounds__(kMaxBins) stream_pitch_viterbi_kernel(
    const float* __restrict__ cost, const float* __restrict__ f0c, const uint64_t* __restrict__ counter,
    unsigned char* state, size_t item_bytes, float* __restrict__ f0, float* __restrict__ conf,
    int32_t* __restrict__ path, int R, int NB, int J, int D, float transition) {
  constexpr int WAVES = kMaxBins / 64;
  __shared__ double rows[2 * kViterbiStride];
  __shared__ double rbest[kStreamMaxFrames * WAVES];
  __shared__ int rbesti[kStreamMaxFrames * WAVES];
  const int j = threadIdx.x, nt = blockDim.x;
  const bool active = j < NB;
  const int P = D + R;
  const uint64_t k = *counter;
  const bool fresh = k == 0;  // (not the stored bits: whatever the state holds, call 0 starts the stream)
  unsigned char* sb = state + (size_t)blockIdx.x * item_bytes;
  double* delta = reinterpret_cast<double*>(sb);
  float* rf0c = reinterpret_cast<float*>(sb + 16 * (size_t)NB);
  float* rcost = rf0c + (size_t)P * NB;
  int8_t* rbp = reinterpret_cast<int8_t*>(rcost + (size_t)P * NB);
  const double* din = delta + (size_t)(k & 1) * NB;
  double* dout = delta + (size_t)((k + 1) & 1) * NB;
  const int s0 = (int)(((k % (uint64_t)P) * (uint64_t)R) % (uint64_t)P);  // the slot of frame n = k R
  const float* cb = cost + (int64_t)blockIdx.x * R * NB;
  const float* fb = f0c + (int64_t)blockIdx.x * R * NB;
  const double lam = (double)transition;

  // the call's cost and f0c into the ring first: independent loads and stores, off the recursion's chain
  if (active) {
    for (int jj = 0; jj < R; ++jj) {
      const int o = ((s0 + jj) % P) * NB + j;
      rcost[o] = cb[jj * NB + j];
      rf0c[o] = fb[jj * NB + j];
    }
  }
  double* prev = viterbi_rows(rows, j, nt, J);
  double* cur = prev + kViterbiStride;
  float c = 0.0f;
  if (active) {
    c = cb[j];
    if (!fresh) prev[j] = din[j];
  }
  __syncthreads();
  for (int jj = 0; jj < R; ++jj) {
    float cn = 0.0f;
    if (active && jj + 1 < R) cn = cb[(jj + 1) * NB + j];  // off the chain: used after the barrier
    double v = INFINITY;
    int vi = INT_MAX;
    if (active) {
      int bk = 0;
      if (fresh && jj == 0) {
        v = (double)c;  // delta_0 = cost(0)
      } else {
        double best = INFINITY;
        for (int q = -J; q <= J; ++q) {  // i = j + q ascending: the smallest i among equals
          const double w = prev[j + q] + lam * (double)abs(q);
          if (w < best) {
            best = w;
            bk = q;
          }
        }
        v = best + (double)c;
      }
      vi = j;
      cur[j] = v;
      rbp[((s0 + jj) % P) * NB + j] = (int8_t)bk;
    }
    // the frame's smallest argmin, this wave's share: a fixed-order reduction of the values just computed
    wave_argmin<64>(v, vi);
    if ((j & 63) == 0) {
      rbest[jj * WAVES + (j >> 6)] = v;
      rbesti[jj * WAVES + (j >> 6)] = vi;
    }
    __syncthreads();
    double* sw = prev;
    prev = cur;
    cur = sw;
    c = cn;
  }
  // (the last barrier: the row, every frame's wave pairs and everything written to the ring are published)
  if (active) dout[j] = prev[j];
  if (j < R) {
    double best = rbest[j * WAVES];
    int besti = rbesti[j * WAVES];
    for (int i = 1; i < (nt >> 6); ++i) take_min(best, besti, rbest[j * WAVES + i], rbesti[j * WAVES + i]);
    int st = min(max(besti, 0), NB - 1);
    // min(D, n) steps back from s_n, n = k R + j: bp_n, bp_{n-1}, ..., bp_{m+1}
    const int steps = (k > (uint64_t)kViterbiMaxLag || k * (uint64_t)R + (uint64_t)j >= (uint64_t)D)
                          ? D
                          : (int)(k * (uint64_t)R) + j;
    int slot = (s0 + j) % P;
    for (int u = 0; u < steps; ++u) {
      st = min(max(st + (int)rbp[slot * NB + st], 0), NB - 1);
      slot = slot == 0 ? P - 1 : slot - 1;
    }
    const int64_t o = (int64_t)blockIdx.x * R + j;
    path[o] = st;
    f0[o] = rf0c[slot * NB + st];
    if (conf) conf[o] = 1.0f - rcost[slot * NB + st];
  }
}

int launch_stream_salience(const StreamArgs& a, int64_t L, const PitchParams& p, const int32_t* lo,
                           const int32_t* hi, int n_bins, float* cost, float* f0c, int32_t* lag, float* f0,
                           float* conf, int32_t* period) {
  return for_frame_length<kPitchMinFrame>(L, [&](auto size) {
    constexpr int N = decltype(size)::value;
    hipLaunchKernelGGL(stream_pitch_salience_kernel<N>, dim3(pitch_blocks(N, a.frames), (unsigned)a.B),
                       dim3(kPoints<N> / 16), 0, S(a.stream), a.x, a.counter, a.ring, a.n, a.len, a.hs, a.hop,
                       a.frames, p, lo, hi, n_bins, cost, f0c, lag, f0, conf, period);
    return launch_status();
  });
}

// The carried decode's sizes (include/ddsp_hip.h), checked before any HIP call.
inline int check_stream_viterbi_sizes(int64_t batch, int64_t R, int64_t NB, int64_t J, int64_t D) {
  if (batch < 0 || R < 1 || NB < 1 || J < 0 || D < 0) return DDSP_HIP_EINVAL;
  if (R > kStreamMaxFrames || NB > kMaxBins || J > kMaxJump || D > kViterbiMaxLag || batch > INT32_MAX)
    return DDSP_HIP_ERANGE;
  return DDSP_HIP_OK;
}

}  // namespace
}  // namespace ddsp

using namespace ddsp;

extern "C" {

int ddsp_hip_stream_pitch_salience(const float* x, const int32_t* lo, const int32_t* hi, float* cost, float* f0c,
                                   int32_t* lag, float* f0, float* confidence, int32_t* period,
                                   const uint64_t* counter, void* state, size_t state_bytes, int64_t batch,
                                   int64_t call_samples, int64_t frame_length, int64_t hop, int64_t tau_min,
                                   int64_t tau_max, int64_t n_bins, float sample_rate, float threshold,
                                   void* stream) {
  StreamSizes sz;
  int st = check_stream_features(batch, call_samples, frame_length, hop, &sz);
  if (st) return st;
  st = check_pitch_params(frame_length, tau_min, tau_max, sample_rate);
  if (st) return st;
  if (n_bins < 1) return DDSP_HIP_EINVAL;
  if (n_bins > kMaxBins) return DDSP_HIP_ERANGE;
  if (!f0 && (confidence || period)) return DDSP_HIP_EINVAL;
  if (batch == 0) return DDSP_HIP_OK;
  if (!x || !lo || !hi || !cost || !f0c || !counter || !state) return DDSP_HIP_EINVAL;
  if (state_bytes < stream_features_bytes(batch, sz)) return DDSP_HIP_EWORKSPACE;
  const StreamArgs a = stream_args(x, counter, state, batch, call_samples, hop, sz, stream);
  return launch_stream_salience(a, frame_length, pitch_params(tau_min, tau_max, sample_rate, threshold), lo, hi,
                                (int)n_bins, cost, f0c, lag, f0, confidence, period);
}

size_t ddsp_hip_stream_viterbi_state_bytes(int64_t batch, int64_t frames_per_call, int64_t n_bins, int64_t lag) {
  if (batch < 1 || check_stream_viterbi_sizes(batch, frames_per_call, n_bins, 0, lag)) return 0;
  return ((size_t)batch * viterbi_state_layout(frames_per_call, n_bins, lag).item_bytes + 15) / 16 * 16;
}

int ddsp_hip_stream_pitch_viterbi(const float* cost, const float* f0c, float* f0, float* confidence, int32_t* path,
                                  const uint64_t* counter, void* state, size_t state_bytes, int64_t batch,
                                  int64_t frames_per_call, int64_t n_bins, int64_t max_jump, int64_t lag,
                                  float transition, void* stream) {
  if (batch < 0 || frames_per_call < 1 || n_bins < 1 || max_jump < 0 || lag < 0) return DDSP_HIP_EINVAL;
  if (!(transition >= 0.0f) || std::isinf(transition)) return DDSP_HIP_EINVAL;
  const int st = check_stream_viterbi_sizes(batch, frames_per_call, n_bins, max_jump, lag);
  if (st) return st;
  if (batch == 0) return DDSP_HIP_OK;
  if (!cost || !f0c || !f0 || !path || !counter || !state) return DDSP_HIP_EINVAL;
  if (state_bytes < ddsp_hip_stream_viterbi_state_bytes(batch, frames_per_call, n_bins, lag))
    return DDSP_HIP_EWORKSPACE;
  const ViterbiStateLayout lay = viterbi_state_layout(frames_per_call, n_bins, lag);
  const unsigned threads = (unsigned)((n_bins + 63) / 64 * 64);
  hipLaunchKernelGGL(stream_pitch_viterbi_kernel, dim3((unsigned)batch), dim3(threads), 0, S(stream), cost, f0c,
                     counter, reinterpret_cast<unsigned char*>(state), lay.item_bytes, f0, confidence, path,
                     (int)frames_per_call, (int)n_bins, (int)max_jump, (int)lag, transition);
  return launch_status();
}

}  // extern "C"
