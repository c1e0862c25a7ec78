/*
 * ddsp_hip.h — C-ABI of the MI355X (gfx950) DDSP harmonic-plus-noise synthesis path.
 *
 * The reference (hugofloresgarcia/ddsp_pytorch) has no native ABI: its hot path is
 * six module-global Python functions in ddsp/core.py, looked up late-bound through
 * the `ddsp` package by the synth modules in ddsp/models/modules.py.  Each entry
 * point below replaces one of those functions (or one module forward) and names
 * the reference interface it stands in for (file:line under /root/reference).
 *
 * Conventions (all entry points):
 *   - plain device pointers and sizes; fp32 data, contiguous unless a stride is given;
 *     tensors are channels-last [batch, time, channel] as in the reference;
 *   - every launch is enqueued on `stream` (a hipStream_t, NULL = default stream);
 *     nothing synchronises the host;
 *   - outputs and workspaces are caller-allocated; the library never allocates
 *     device memory;
 *   - return DDSP_HIP_OK (0) or a DDSP_HIP_E* code; ddsp_hip_status_string() maps it
 *     to text.  Invalid shapes are rejected before any launch;
 *   - thread-safe and stateless: callable from any host thread, e.g. the realtime
 *     host's worker thread (ddsp_tilde.cpp:88-92).
 */
#ifndef DDSP_HIP_H
#define DDSP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  DDSP_HIP_OK = 0,
  DDSP_HIP_EINVAL = 1,      /* invalid argument / shape */
  DDSP_HIP_ELAUNCH = 2,     /* HIP launch or runtime error */
  DDSP_HIP_EFFT = 3,        /* FFT convolution error */
  DDSP_HIP_EWORKSPACE = 4,  /* workspace too small */
  DDSP_HIP_ERANGE = 5       /* input outside the exactness domain */
};

const char* ddsp_hip_status_string(int status);
int ddsp_hip_version(void);

/* ---------------- function level: ddsp/core.py ---------------- */

/* ddsp/core.py:77-78  scale_function(x) = 2*sigmoid(x)**ln(10) + 1e-7, elementwise over n values.
 * `bias` is added to x first (FilteredNoise.get_controls, modules.py:111-114 passes -5). */
int ddsp_hip_scale_function(const float* x, float* y, int64_t n, float bias, void* stream);

/* ddsp/core.py:70-74  remove_above_nyquist(amplitudes[rows,H], f0[rows,1], sr):
 * out = amps * (fl32(f0*k) < sr/2 ? 1.0001f : 1e-4f), k = 1..H. */
int ddsp_hip_remove_above_nyquist(const float* amplitudes, const float* f0, float* out,
                                  int64_t rows, int64_t n_harmonic, float sample_rate,
                                  void* stream);

/* ddsp/core.py:64-67  upsample(signal[B,F,C], factor) -> [B,F*factor,C] (nearest). */
int ddsp_hip_upsample(const float* x, float* y, int64_t batch, int64_t frames, int64_t channels,
                      int64_t factor, void* stream);

/* ddsp/core.py:136-141  harmonic_synth(f0[B,T,1], amplitudes[B,T,H], sr) -> [B,T,1].
 * Per-sample pitch and amplitudes (the op boundary).  Workspace: see *_workspace_size. */
size_t ddsp_hip_harmonic_synth_workspace_size(int64_t batch, int64_t n_samples);
int ddsp_hip_harmonic_synth(const float* f0, const float* amplitudes, float* out, int64_t batch,
                            int64_t n_samples, int64_t n_harmonic, float sample_rate,
                            void* workspace, size_t workspace_bytes, void* stream);

/* The fp32 phase omega[B,T] = cumsum(2*pi*f0/sr, time) of ddsp/core.py:138, exposed for
 * bit-exact testing of the phase accumulator (same code path as harmonic_synth). */
int ddsp_hip_phase(const float* f0, float* omega, int64_t batch, int64_t n_samples,
                   float sample_rate, void* workspace, size_t workspace_bytes, void* stream);

/* ddsp/core.py:144-166  amp_to_impulse_response(amp[rows,NB], target) -> [rows,target]. */
int ddsp_hip_amp_to_impulse_response(const float* amp, float* impulse, int64_t rows,
                                     int64_t n_bands, int64_t target_size, void* stream);

/* ddsp/core.py:169-176  fft_convolve(signal[rows,N], kernel[kernel_rows,N]) -> [rows,N]:
 * causal linear convolution truncated to N.  kernel_rows is rows or 1 (broadcast).
 * Small N runs a direct LDS convolution; large N a partitioned overlap-save FFT convolution. */
size_t ddsp_hip_fft_convolve_workspace_size(int64_t rows, int64_t kernel_rows, int64_t n);
int ddsp_hip_fft_convolve(const float* signal, const float* kernel, float* out, int64_t rows,
                          int64_t kernel_rows, int64_t n, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---------------- module level: ddsp/models/modules.py ---------------- */

/* modules.py:44-67  HarmonicSynth.get_controls: amplitudes = scale(amp_raw),
 * dist = remove_above_nyquist(scale(dist_raw), f0, sr) / sum.  Inputs may be strided views
 * (param[..., :1] and param[..., 1:]): row r of amp_raw is amp_raw[r*amp_stride],
 * of dist_raw is dist_raw[r*dist_stride + k]. */
int ddsp_hip_harmonic_controls(const float* amp_raw, int64_t amp_stride, const float* dist_raw,
                               int64_t dist_stride, const float* f0, float* amplitudes,
                               float* distribution, int64_t rows, int64_t n_harmonic,
                               float sample_rate, void* stream);

/* modules.py:69-80  HarmonicSynth.forward fused: dist*amps (written back to `distribution`
 * in place when write_back != 0, reproducing modules.py:73), frame->sample upsampling of
 * pitch and amplitudes in registers, and harmonic_synth; [B,F,H] never leaves LDS. */
int ddsp_hip_harmonic_synth_frames(const float* f0, const float* amplitudes, float* distribution,
                                   int write_back, float* out, int64_t batch, int64_t frames,
                                   int64_t n_harmonic, int64_t block_size, float sample_rate,
                                   void* stream);

/* decoder.py:106-113 + modules.py:44-80: HarmonicSynth.get_controls and forward in one launch,
 * straight from the harmonic projection param[B,F,H+1] (amplitude column 0, distribution
 * columns 1..H, decoder.py:107-108).  The controls never reach HBM. */
int ddsp_hip_harmonic_synth_params(const float* f0, const float* param, float* out, int64_t batch,
                                   int64_t frames, int64_t n_harmonic, int64_t block_size,
                                   float sample_rate, void* stream);

/* modules.py:116-128  FilteredNoise.forward fused: per-frame zero-phase FIR from the
 * magnitudes (amp_to_impulse_response) applied to block_size noise samples by truncated
 * linear convolution (fft_convolve).  noise == NULL draws U[-1,1) on device
 * (Philox4x32-10 keyed by seed, counter offset), else noise[B,F,block_size] is used
 * (parity mode: the reference's torch.rand stream).  `add` (nullable, [B,F*bs]) is added
 * to the result (fuses decoder.py:121 `harmonic + noise`); `noise_out` (nullable)
 * receives the filtered noise alone. */
int ddsp_hip_filtered_noise(const float* magnitudes, const float* noise, uint64_t seed,
                            uint64_t offset, const float* add, float* out, float* noise_out,
                            int64_t batch, int64_t frames, int64_t n_bands, int64_t block_size,
                            void* stream);

/* modules.py:111-128  FilteredNoise.get_controls + forward in one launch: raw_magnitudes is the
 * noise projection [B,F,NB] (decoder.py:115); the kernel applies scale_function(x + bias)
 * (bias = initial_bias, -5 by default) before designing the filters.  Other arguments as
 * ddsp_hip_filtered_noise. */
int ddsp_hip_filtered_noise_params(const float* raw_magnitudes, float bias, const float* noise,
                                   uint64_t seed, uint64_t offset, const float* add, float* out,
                                   float* noise_out, int64_t batch, int64_t frames, int64_t n_bands,
                                   int64_t block_size, void* stream);

/* decoder.py:106-121 in one launch: HarmonicSynth.get_controls + forward from the harmonic
 * projection param[B,F,H+1], FilteredNoise.get_controls + forward from the raw noise projection
 * raw_magnitudes[B,F,NB] (scale_function(x + bias)), and signal = harmonic + noise -> out[B,F*bs].
 * noise / seed / offset as ddsp_hip_filtered_noise; harmonic_out and noise_out (nullable)
 * receive the two parts.  Outside the fused kernel's envelope (ddsp_hip_synth_frames_supported)
 * DDSP_HIP_ERANGE is returned and callers use the separate kernels. */
int ddsp_hip_synth_frames(const float* f0, const float* param, const float* raw_magnitudes, float bias,
                          const float* noise, uint64_t seed, uint64_t offset, float* out,
                          float* harmonic_out, float* noise_out, int64_t batch, int64_t frames,
                          int64_t n_harmonic, int64_t n_bands, int64_t block_size, float sample_rate,
                          void* stream);

/* The fused frame kernel's shape envelope, the one shared by ddsp_hip_synth_frames, _controls_prefix,
 * _counter and ddsp_hip_stream_synth_frames: 1 when they take (batch, n_harmonic, n_bands, block_size) for
 * some frames >= 1, 0 when they answer DDSP_HIP_ERANGE or DDSP_HIP_EINVAL.  Today: block_size % 4 == 0 and
 * <= 1024, n_harmonic <= 1024, n_bands <= 1025, batch <= 65535 (a frame's LDS, which also bounds it, cannot
 * bind under these caps).  Host only: no device is needed or touched. */
int ddsp_hip_synth_frames_supported(int64_t batch, int64_t n_harmonic, int64_t n_bands, int64_t block_size);

/* Which form of the fused frame kernel a launch of ddsp_hip_synth_frames, _controls_prefix (with_prefix != 0 when
 * it is given a frame_prefix) or _counter takes, from the same plan the launch follows: *route receives
 *   DDSP_HIP_SYNTH_ROUTE_SPLIT  few frames (batch * frames < 512, no prefix): a frame's harmonics over several
 *                               thread groups, any shape;
 *   DDSP_HIP_SYNTH_ROUTE_FIXED  n_bands == 65 and block_size == 512, not split: the kernel compiled for that shape
 *                               alone (any n_harmonic and leading dimensions; same bits as the other forms);
 *   DDSP_HIP_SYNTH_ROUTE_ANY    every other shape of the envelope, four samples per thread.
 * DDSP_HIP_EINVAL for sizes no frame entry point takes or a null route, DDSP_HIP_ERANGE outside the envelope
 * (*route untouched).  Host only: no device is needed or touched. */
enum ddsp_hip_synth_route { DDSP_HIP_SYNTH_ROUTE_ANY = 0, DDSP_HIP_SYNTH_ROUTE_SPLIT = 1, DDSP_HIP_SYNTH_ROUTE_FIXED = 2 };
int ddsp_hip_synth_frames_route(int64_t batch, int64_t frames, int64_t n_harmonic, int64_t n_bands,
                                int64_t block_size, int with_prefix, int* route);

/* ddsp_hip_synth_frames that also writes the controls DDSPDecoder.forward returns
 * (decoder.py:127-135: output['harmonic_ctrls'], output['noise_ctrls']) into controls_out (nullable),
 * laid out as [amplitudes B*F | harmonic_distribution B*F*H | magnitudes B*F*NB]: amplitudes =
 * scale_function(param[...,0]), harmonic_distribution = the normalised distribution after
 * HarmonicSynth.forward's in-place `*= amplitudes` (modules.py:61,73), magnitudes =
 * scale_function(raw_magnitudes + bias) (modules.py:111-114).  param_ld / magnitudes_ld: elements between
 * consecutive frames' rows (>= H + 1 / >= NB), so both may be column slices of one projection output
 * (decoder.py:106-117 computed as a single GEMM).
 * frame_prefix (nullable): the exact fp64 phase prefix of every frame,
 * frame_prefix[b * frames + f] = sum_{g < f} block_size * fl32(fl32(fl32(2 pi) f0[b, g]) / sr) (the
 * reference's cumsum, core.py:138, at each frame's start), as ddsp_hip_frame_phase_prefix writes it.
 * Without it every frame's workgroup sums its earlier frames itself: O(frames) per frame, O(frames^2)
 * per item — the right choice for a few hundred frames, not for a minute of audio (5,625 frames at
 * block 512).  Both routes give the same bits wherever every partial sum is exact in fp64, i.e. while the
 * increments' significant bits together with log2(frames * block_size) span <= 53 bits (f0 of audio pitch,
 * tests/test_gpu_long_render.py); near-zero f0 (unvoiced frames, increments with ulps far below the running
 * sum's) rounds the sums and the two summation orders may differ in the phase's last bits — inside the
 * sine's 1e-6 tolerance, and checked at that tolerance. */
int ddsp_hip_synth_frames_controls_prefix(const float* f0, const float* param, int64_t param_ld,
                                          const float* raw_magnitudes, int64_t magnitudes_ld, float bias,
                                          const float* noise, uint64_t seed, uint64_t offset, float* out,
                                          float* harmonic_out, float* noise_out, float* controls_out,
                                          const double* frame_prefix, int64_t batch, int64_t frames,
                                          int64_t n_harmonic, int64_t n_bands, int64_t block_size, float sample_rate,
                                          void* stream);
int ddsp_hip_frame_phase_prefix(const float* f0, int64_t batch, int64_t frames, int64_t block_size, float sample_rate,
                                double* frame_prefix, void* stream);

/* ddsp_hip_synth_frames for a stream of calls replayed from a captured HIP graph (the ddsp~
 * realtime host, realtime/ddsp_tilde/ddsp_model.cpp:32-52, calling the exported model once per
 * 1024-sample buffer): the Philox offset of the on-device noise is read from the device word
 * *counter, which a second launch on the same stream then increments, so every replay draws
 * fresh noise (a graph freezes by-value arguments).  Call k draws the noise of
 * ddsp_hip_synth_frames(..., seed, offset = k, ...). */
int ddsp_hip_synth_frames_counter(const float* f0, const float* param, const float* raw_magnitudes, float bias,
                                  uint64_t seed, uint64_t* counter, float* out, int64_t batch, int64_t frames,
                                  int64_t n_harmonic, int64_t n_bands, int64_t block_size, float sample_rate,
                                  void* stream);

/* modules.py:21-26  Reverb.build_impulse: noise[L]*exp(-softplus(-decay)*t*500)*sigmoid(wet),
 * impulse[0] = 1.  decay and wet are device scalars. */
int ddsp_hip_reverb_build_impulse(const float* noise, const float* decay, const float* wet,
                                  float* impulse, int64_t length, float sample_rate,
                                  void* stream);

/* modules.py:28-35  Reverb.forward: IR padded/cropped to n_samples, then fft_convolve.
 * Split in two so the IR spectrum is computed once and cached by the caller:
 *   ddsp_hip_reverb_spectrum: impulse[L] -> spectrum (ddsp_hip_reverb_spectrum_floats floats:
 *     partitioned-convolution spectra of the IR cropped to min(L, n_samples));
 *   ddsp_hip_reverb_apply:   x[B,T] (*) IR -> out[B,T] using that spectrum. */
size_t ddsp_hip_reverb_spectrum_floats(int64_t n_samples, int64_t ir_length);
size_t ddsp_hip_reverb_workspace_size(int64_t batch, int64_t n_samples, int64_t ir_length);
/* modules.py:21-35: Reverb.build_impulse and the IR's partition spectra (as ddsp_hip_reverb_spectrum of
 * the built impulse, bit for bit) in ONE launch — the impulse is never written.  For a reverb whose
 * parameters change every call (training: the reference rebuilds the IR in every Reverb.forward). */
int ddsp_hip_reverb_impulse_spectrum(const float* noise, const float* decay, const float* wet, int64_t ir_length,
                                     float sample_rate, int64_t n_samples, float* spectrum, void* stream);
int ddsp_hip_reverb_spectrum(const float* impulse, int64_t ir_length, int64_t n_samples,
                             float* spectrum, void* stream);
int ddsp_hip_reverb_apply(const float* x, const float* spectrum, float* out, int64_t batch,
                          int64_t n_samples, int64_t ir_length, void* workspace,
                          size_t workspace_bytes, void* stream);
/* modules.py:21-35 Reverb.forward (build_impulse, crop/pad to n_samples, fft_convolve) with the IR's partition
 * spectra cached on the device and VALIDATED there on every call: `cache` (caller-owned device memory of
 * ddsp_hip_reverb_cache_bytes bytes, zero-filled once: a zeroed cache holds nothing) keeps, per IR window,
 * the spectrum and a bit-exact copy of the inputs it was built from (the window's noise taps, decay, wet,
 * sample_rate).  The input transform's launch compares them with the current parameters and rebuilds the
 * windows that differ, so any write to the parameters (optimizer steps, writes through aliases such as
 * `.data`) is seen by the next call, and unchanged parameters cost no rebuild.  force != 0 rebuilds every
 * window (the reference's every-call rebuild).  batch == 0 validates the cache only.  The cache's first
 * ddsp_hip_reverb_spectrum_floats(n_samples, ir_length) floats are then the current spectrum (as
 * ddsp_hip_reverb_impulse_spectrum writes it, bit for bit; used by ddsp_hip_reverb_backward).  Workspace:
 * ddsp_hip_reverb_workspace_size; it then holds x's input spectra as after ddsp_hip_reverb_apply. */
size_t ddsp_hip_reverb_cache_bytes(int64_t n_samples, int64_t ir_length);
int ddsp_hip_reverb_forward(const float* x, const float* noise, const float* decay, const float* wet,
                            int64_t ir_length, float sample_rate, int force, void* cache, size_t cache_bytes,
                            float* out, int64_t batch, int64_t n_samples, void* workspace, size_t workspace_bytes,
                            void* stream);

/* ---------------- the decoder network for a few frames: core.py:122-129, decoder.py:43-68 ----------------
 * One Linear for rows <= 8 frames (the realtime stream's 1024-sample calls, ddsp_model.cpp:32-52)
 * with the previous MLP block's LayerNorm + LeakyReLU folded into its input:
 *   a[r, :] = concat over inputs s of act_s(x_s[r, :])
 *   y[r, n] = sum_k weight[n, k] a[r, k] + bias[n]          weight [out_features, K] (nn.Linear)
 * act_s: x' = x * scale + shift (the exported model's loudness normalisation, export.py:35;
 * 1 and 0 otherwise); with w1/b1 (a K=1 nn.Linear of width `width`, the first layer of
 * core.py:122's mlp(1, ...)) x is one value per row and x'' = w1[c] * x' + b1[c]; with
 * gamma/beta: leaky_relu(layer_norm(x'') * gamma + beta, 0.01), eps 1e-5 (core.py:126), or with
 * plain_norm != 0 the LayerNorm alone (the MFCC encoder's `norm`, encoder.py; a zero-filled struct
 * keeps the LeakyReLU).  x_copy (nullable, w1 inputs only) receives x' per row.  Up to
 * DDSP_HIP_DENSE_MAX_PROBLEMS independent Linears share one launch (the f0, loudness and z MLPs).
 * rows <= 8, K <= 1536 (else DDSP_HIP_ERANGE): K <= 1088 runs the kernel with 17 register chunks of
 * 64 columns per W row, a wider K (the z-conditioned GRU input's 3 x 512) the one with 24. */
#define DDSP_HIP_DENSE_MAX_INPUTS 3
#define DDSP_HIP_DENSE_MAX_PROBLEMS 3
typedef struct ddsp_hip_dense_input {
  const float* x;      /* [rows, ld] (w1 inputs: x[r * ld] is the row's value) */
  int64_t ld;
  int64_t width;       /* columns contributed to K */
  float scale, shift;
  const float* w1;     /* nullable [width] */
  const float* b1;     /* [width] when w1 */
  const float* gamma;  /* nullable [width]: LayerNorm + LeakyReLU */
  const float* beta;
  float* x_copy;       /* nullable [rows] */
  int plain_norm;      /* with gamma: 0 = LayerNorm + LeakyReLU(0.01), non-zero = the LayerNorm alone */
} ddsp_hip_dense_input;
typedef struct ddsp_hip_dense_problem {
  ddsp_hip_dense_input inputs[DDSP_HIP_DENSE_MAX_INPUTS];
  int n_inputs;
  const float* weight; /* [out_features, K] */
  const float* bias;   /* nullable [out_features] */
  float* y;            /* [rows, ldy] */
  int64_t ldy;
  int64_t out_features;
} ddsp_hip_dense_problem;
int ddsp_hip_dense_rows(const ddsp_hip_dense_problem* problems, int n_problems, int64_t rows, void* stream);

/* ddsp/core.py:122-129: one whole MLP block, y = LeakyReLU(LayerNorm(x W^T + b)), W [out, w_ld] the
 * nn.Linear weight, for out_features = 512 (else DDSP_HIP_ERANGE): the Linear on the matrix cores,
 * LayerNorm + LeakyReLU in its epilogue.  e0/e1 (nullable, per-row scalars at stride e_ld) add
 * e0[r] W[:, in] + e1[r] W[:, in + 1] — the decoder's out_mlp input [gru_out, f0, loudness]
 * (decoder.py:68) without the concatenation.  y [rows, y_ld] may be a column slice.
 * The Linear's arithmetic: at in_features 512 with 16-byte aligned rows (the decoder's blocks) both operands
 * split exactly into three bf16 terms and summed as six bf16 products per term pair on the bf16 matrix
 * cores — fp32-accurate (the dropped terms are ~2^-24 of each product), not the same bits as an fp32 fma
 * chain; flags = DDSP_HIP_MLP_EXACT_F32 (or any other shape) takes the f32-input MFMA (one kernel for every
 * K, x and W staged through LDS), whose sums are exactly k-ordered fp32 fma chains. */
enum { DDSP_HIP_MLP_EXACT_F32 = 1 };
int ddsp_hip_mlp_block(const float* x, int64_t x_ld, int64_t in_features, const float* w, int64_t w_ld,
                       const float* bias, const float* e0, const float* e1, int64_t e_ld, const float* gamma,
                       const float* beta, float eps, float slope, float* y, int64_t y_ld, int64_t rows,
                       int64_t out_features, int flags, void* stream);
/* ddsp/core.py:122-129 (one MLP block after its Linear, decoder.py:25-42): y = LeakyReLU(LayerNorm(h))
 * per row of cols features, h = x [rows, x_ld] or, with w1/b1 (a Linear with ONE input feature),
 * h = x[r] * w1 + b1 formed on the fly.  gamma/beta: the LayerNorm's affine; eps and the negative
 * slope as in torch (1e-5, 0.01).  y [rows, y_ld] may be a column slice of a wider buffer.  One pass
 * instead of torch's two; cols 512 or 1024 with 16-byte aligned rows, else DDSP_HIP_ERANGE. */
int ddsp_hip_layer_norm_leaky_relu(const float* x, int64_t x_ld, const float* w1, const float* b1, const float* gamma,
                                   const float* beta, float eps, float slope, float* y, int64_t y_ld, int64_t rows,
                                   int64_t cols, void* stream);

/* Weight gradient of a Linear under autograd, grad_w[m][n] = sum_r grad_y[r][m] x[r][n] (grad_w [out_features,
 * dw_ld], nn.Linear's weight layout; torch: grad_y^T @ x), on the bf16 matrix cores with the fp32-accurate
 * three-term split: the decoder MLPs' Linears and projections (core.py:122-129, decoder.py:106-117) and the GRU's
 * W_ih / W_hh (decoder.py:33-68).  Any widths (tiles past an edge are padding of the partials); split over row
 * ranges whose partials are summed in a fixed order (deterministic).  ws:
 * ddsp_hip_linear_weight_grad_workspace_size(rows, out_features, in_features) bytes.  DDSP_HIP_ERANGE when a row
 * range's byte offsets pass 2^31 (dy_ld / x_ld beyond ~2^24 floats) or a width passes 2^24: callers keep their
 * library GEMM. */
size_t ddsp_hip_linear_weight_grad_workspace_size(int64_t rows, int64_t out_features, int64_t in_features);
int ddsp_hip_linear_weight_grad(const float* grad_y, int64_t dy_ld, const float* x, int64_t x_ld, float* grad_w,
                                int64_t dw_ld, int64_t rows, int64_t out_features, int64_t in_features, void* ws,
                                size_t ws_bytes, void* stream);

/* Backward of ddsp_hip_layer_norm_leaky_relu without w1 (training: the MLP blocks' LayerNorm + LeakyReLU,
 * core.py:122-129, replacing torch's leaky_relu_backward + native_layer_norm_backward): from the pre-activation x
 * [rows, x_ld] and grad_y, grad_x [rows, dx_ld] and (each nullable) grad_gamma / grad_beta [cols], the column sums
 * over all rows (deterministic order).  The LeakyReLU's branch is taken on z = LayerNorm(x) formed as the forward
 * forms it.  ws: ddsp_hip_layer_norm_leaky_relu_backward_workspace_size(cols) bytes when a parameter gradient is
 * requested.  cols 512 or 1024 with 16-byte aligned rows, else DDSP_HIP_ERANGE. */
size_t ddsp_hip_layer_norm_leaky_relu_backward_workspace_size(int64_t cols);
int ddsp_hip_layer_norm_leaky_relu_backward(const float* x, int64_t x_ld, const float* gamma, const float* beta, float eps,
                                            float slope, const float* grad_y, int64_t dy_ld, float* grad_x, int64_t dx_ld,
                                            float* grad_gamma, float* grad_beta, int64_t rows, int64_t cols, void* ws,
                                            size_t ws_bytes, void* stream);

/* A Linear y = x W^T + b (W [out_features, w_ld], the nn.Linear / nn.GRU weight layout) on the bf16 matrix cores
 * with the fp32-accurate three-term split of ddsp_hip_mlp_block: the decoder's GRU input projection for every
 * step at once (decoder.py:41, torch.nn.GRU's x W_ih^T + b_ih; 12,800 x 1024 -> 1536 at config 2).
 * Under autograd also the input gradient of the MLP blocks' Linears (dx = dy W, W^T as the weight) and of the
 * GRU's input projection (in_features 1536 = 3 gates x 512).  in_features 512, 1024 or 1536, out_features a
 * multiple of 512, x and W 16-byte aligned with ld % 4 == 0; else DDSP_HIP_ERANGE (callers keep their library
 * GEMM). */
int ddsp_hip_linear(const float* x, int64_t x_ld, int64_t in_features, const float* w, int64_t w_ld,
                    const float* bias, float* y, int64_t y_ld, int64_t rows, int64_t out_features, void* stream);

/* decoder.py:106-117 (param = harmonic_proj(hidden), magnitudes = noise_proj(hidden)) in ONE launch on the bf16
 * matrix cores with the fp32-accurate three-term split of ddsp_hip_linear, reading both layers' parameters where
 * they lie (nn.Linear layout, W1 [n1, w1_ld], W2 [n2, w2_ld]): y[r][c] = x[r] W1[c]^T + b1[c] for c < n1 and
 * x[r] W2[c - n1]^T + b2[c - n1] for n1 <= c < n1 + n2; columns of y past n1 + n2 are not written.  Replaces
 * the two nn.Linear calls of decoder.py:106-117 (stack_rows + one library GEMM before).  in_features 512, x, W1,
 * W2 16-byte aligned with ld % 4 == 0; else DDSP_HIP_ERANGE (callers keep their library GEMM). */
int ddsp_hip_projections(const float* x, int64_t x_ld, int64_t in_features, const float* w1, int64_t w1_ld,
                         const float* b1, int64_t n1, const float* w2, int64_t w2_ld, const float* b2, int64_t n2,
                         float* y, int64_t y_ld, int64_t rows, void* stream);

/* decoder.py:106-117 (param = harmonic_proj(hidden), magnitudes = noise_proj(hidden)): the two projections'
 * parameters stacked into one zero-padded matrix w [n_pad, in_features] and
 * bias b [n_pad] (caller buffers; rows n1 + n2 .. n_pad - 1 zero), for one library GEMM over both at a
 * width it is fast at.  One launch; the parameters are read as they are at the call. */
int ddsp_hip_stack_rows(const float* w1, int64_t w1_ld, const float* b1, int64_t n1, const float* w2, int64_t w2_ld,
                        const float* b2, int64_t n2, int64_t in_features, float* w, float* b, int64_t n_pad,
                        void* stream);

/* ---------------- the decoder network's recurrence: decoder.py:33-68 (torch.nn.GRU) ----------------
 * out[B,T,H] = GRU(h0) over xp[B,T,3H] = x W_ih^T + b_ih (the input projection for every step,
 * computed by the caller's GEMM), W_hh[3H,H], b_hh[3H] in torch's (r, z, n) order; h0 [B,H]
 * (NULL = zeros); h_last [B,H] (nullable) receives h_T; gates (nullable, training) [4][B,T,H]
 * receives r, z, n and W_hn h + b_hn of every step for the backward.  One launch per time
 * step; hidden % 64 == 0 (else DDSP_HIP_ERANGE).
 * Backward (BPTT): from grad_out[B,T,H] (nullable) and grad_h_last[B,H] (nullable) ->
 * grad_xp[B,T,3H] (gradient of the input projection: dW_ih, db_ih, dx are GEMMs of it),
 * grad_gn[B,T,H] (with grad_xp's r and z planes, the gradient of W_hh h + b_hh: dW_hh and db_hh
 * are GEMMs of it against h_{t-1}), grad_h0[B,H] (nullable).  Workspace: *_workspace_size. */
int ddsp_hip_gru_forward(const float* xp, const float* w_hh, const float* b_hh, const float* h0, float* out,
                         float* h_last, float* gates, int64_t batch, int64_t steps, int64_t hidden, void* stream);
/* The same forward as ONE persistent launch (hidden 512, batch <= 64, out < 2 GiB, >= 256 CUs, a stream
 * whose kernels may use every CU, h_last != h0; else DDSP_HIP_ERANGE and the caller uses
 * ddsp_hip_gru_forward, which allows h_T over h0 in place): 8 groups
 * of 32 workgroups, group g owning items g, g + 8, ...; each workgroup keeps its 48 rows of W_hh in
 * registers for the whole sequence and the group's slots hand h_t to each other through the output
 * sequence (a per-group counter).  It needs all 256 workgroups resident together; when they are not (another
 * long-running kernel beside it, GPU sharing) every wait ends within 200 ms, the launch aborts, and a rescue
 * kernel that the call always enqueues behind it recomputes out, h_last and gates exactly as
 * ddsp_hip_gru_forward does (bit for bit) — the outputs are right either way, and the abort is reported in
 * the workspace's status word (below).  Workspace: ddsp_hip_gru_persistent_workspace_size() bytes (zeroed by
 * the call, on the stream, by a kernel of its own: the call stays capturable into a HIP graph); after the
 * stream has passed the call, the uint32 at byte offset ddsp_hip_gru_persistent_status_offset() holds
 * DDSP_HIP_GRU_STATUS_LOCAL (the hand-off stayed inside each XCD's L2), 0 (the placement-independent
 * write-through hand-off) or DDSP_HIP_GRU_STATUS_RESCUED (aborted, the outputs come from the rescue kernel).
 * flags: 0, or test hooks — DDSP_HIP_GRU_SPREAD (use the placement-independent hand-off whatever the
 * census finds), DDSP_HIP_GRU_NO_MASK_CHECK (launch on a CU-masked stream anyway: the abort path under a
 * real residency failure), DDSP_HIP_GRU_FORCE_ABORT (abort at the census). */
enum {
  DDSP_HIP_GRU_SPREAD = 1,
  DDSP_HIP_GRU_NO_MASK_CHECK = 2,
  DDSP_HIP_GRU_FORCE_ABORT = 4,
  DDSP_HIP_GRU_STATUS_LOCAL = 1,
  DDSP_HIP_GRU_STATUS_RESCUED = 2
};
size_t ddsp_hip_gru_persistent_workspace_size(void);
size_t ddsp_hip_gru_persistent_status_offset(void);
int ddsp_hip_gru_forward_persistent(const float* xp, const float* w_hh, const float* b_hh, const float* h0, float* out,
                                    float* h_last, float* gates, int64_t batch, int64_t steps, int64_t hidden,
                                    int flags, void* workspace, size_t workspace_bytes, void* stream);
/* The BPTT as ONE persistent launch (the training mirror of ddsp_hip_gru_forward_persistent: same envelope —
 * hidden 512, batch <= 64, grad_xp < 2 GiB, >= 256 CUs, a stream that may use every CU; else DDSP_HIP_ERANGE and
 * the caller uses ddsp_hip_gru_backward —, same groups, census, hand-off, flags, abort, rescue and status word):
 * each workgroup keeps its 16 units' W_hh columns in registers and the slots hand each step's gate gradients
 * (the grad_xp / grad_gn rows themselves) to each other; W_hh^T dG on the bf16 matrix cores with the
 * fp32-accurate three-term split.  Outputs as ddsp_hip_gru_backward (fp32-accurate, not the same bits).
 * Workspace: ddsp_hip_gru_persistent_workspace_size() bytes. */
int ddsp_hip_gru_backward_persistent(const float* w_hh, const float* gates, const float* out, const float* h0,
                                     const float* grad_out, const float* grad_h_last, float* grad_xp, float* grad_gn,
                                     float* grad_h0, int64_t batch, int64_t steps, int64_t hidden, int flags,
                                     void* workspace, size_t workspace_bytes, void* stream);
size_t ddsp_hip_gru_backward_workspace_size(int64_t batch, int64_t hidden);
int ddsp_hip_gru_backward(const float* w_hh, const float* gates, const float* out, const float* h0,
                          const float* grad_out, const float* grad_h_last, float* grad_xp, float* grad_gn,
                          float* grad_h0, int64_t batch, int64_t steps, int64_t hidden, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---------------- training loss: ddsp/core.py:27-41 multiscale_fft ----------------
 * One scale of multiscale_fft: |torch.stft(x, n_fft, hop, n_fft, hann(n_fft), center=True
 * (reflect), normalized=True)| for x[batch, n_samples] (n_fft a power of two in [16, 4096],
 * n_samples > n_fft/2).  magnitudes are written frame-major [batch, frames, n_fft/2+1]
 * (frames = ddsp_hip_stft_frames(n_samples, hop) = n_samples/hop + 1); the reference's
 * [batch, n_fft/2+1, frames] is its transpose.  The backward maps grad_magnitudes (same layout)
 * to grad_x[batch, n_samples] (|Z| has zero gradient where Z = 0, as torch's abs). */
int64_t ddsp_hip_stft_frames(int64_t n_samples, int64_t hop);
int ddsp_hip_stft_magnitude(const float* x, float* magnitudes, int64_t batch, int64_t n_samples, int64_t n_fft,
                            int64_t hop, void* stream);
size_t ddsp_hip_stft_backward_workspace_size(int64_t batch, int64_t n_samples, int64_t n_fft, int64_t hop);
int ddsp_hip_stft_magnitude_backward(const float* x, const float* grad_magnitudes, float* grad_x, int64_t batch,
                                     int64_t n_samples, int64_t n_fft, int64_t hop, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* train.py:70-76 + 91-104: the multiscale spectral loss of a reconstruction against a target
 * (both [batch, n_samples]), sum over scales of mean|Mx - My| + mean|log(Mx+1e-7) - log(My+1e-7)|,
 * fused per scale (no spectrogram reaches memory) -> loss (device scalar) and, when grad_recon is
 * not NULL, dloss/drecon [batch, n_samples].  n_ffts/hops: host arrays of n_scales entries
 * (hop = int(n_fft * (1 - overlap))).  Deterministic (fixed-order fp64 reductions). */
size_t ddsp_hip_spectral_loss_workspace_size(int64_t batch, int64_t n_samples, const int64_t* n_ffts,
                                             const int64_t* hops, int n_scales);
int ddsp_hip_spectral_loss(const float* target, const float* recon, int64_t batch, int64_t n_samples,
                           const int64_t* n_ffts, const int64_t* hops, int n_scales, float* loss, float* grad_recon,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---------------- audio analysis: the features the models consume, from raw audio ----------------
 * Both take x[batch, n_samples] and librosa.stft's frames: centred (reflect padding by n_fft/2, frame f
 * centred at f * hop), periodic Hann(n_fft), an UNNORMALISED FFT (ddsp_hip_stft_magnitude scales by
 * n_fft^-1/2; these do not), computed in fp64 from the fp32 input (the features take logs of single bins; inputs,
 * tables, logs and outputs are fp32).  No spectrogram is written; every reduction has a fixed order (no atomics), so
 * the results are bit-reproducible and independent of the batch around an item.
 * Envelope, checked before any HIP call: n_fft a power of two in [16, 4096] (else DDSP_HIP_ERANGE),
 * n_samples > n_fft/2 (else DDSP_HIP_EINVAL), hop >= 1 (any value: not a power of two, n_samples % hop != 0),
 * batch <= 65535 (else DDSP_HIP_ERANGE), and for the MFCC 1 <= n_mfcc <= n_mels (else DDSP_HIP_EINVAL),
 * n_mels <= 256 (else DDSP_HIP_ERANGE), top_db >= 0.  Null pointers and negative sizes: DDSP_HIP_EINVAL;
 * batch == 0: a no-op success; a short workspace: DDSP_HIP_EWORKSPACE. */

/* ddsp/core.py:81-97  extract_loudness(signal, sample_rate, block_size = hop, n_fft):
 * out[b, f] = mean over k = 0..n_fft/2 of (ln(|X[b,f,k]| + 1e-7) + weights[k]), f = 0 .. n_samples/hop - 1
 * (core.py:95 drops the last of librosa's 1 + n_samples/hop frames; it is not computed).  weights: the
 * caller's additive table of n_fft/2+1 floats (core.py:90-93: librosa.A_weighting of the bin frequencies, in
 * dB, added to the NATURAL log as the reference does); NULL = zeros.  out [batch, n_samples/hop]. */
int ddsp_hip_loudness(const float* x, const float* weights, float* out, int64_t batch, int64_t n_samples,
                      int64_t n_fft, int64_t hop, void* stream);

/* ddsp/preprocess.py:30-32  librosa.feature.mfcc(x, sr, n_mfcc, n_fft, hop_length, fmin, fmax, n_mels).T:
 * per frame the power |X_k|^2, the mel energies M[m] = sum_k fb[m,k] |X_k|^2, D[m] = 10 log10(max(1e-10, M[m]));
 * per item D <- max(D, max(D) - top_db) (librosa.power_to_db, ref = 1); then the DCT
 * out[b, f, i] = sum_m dct[i, m] D[b, f, m], i < n_mfcc — out [batch, frames, n_mfcc] with all
 * frames = n_samples/hop + 1 (ddsp/data.py:25 drops the last one later).
 * The filterbank comes as one band of bins per mel row: row m weighs bins band_start[m] ..
 * band_start[m] + band_count[m] - 1 with band_weights[o_m ..], o_m = band_count[0] + .. + band_count[m-1]
 * (n_band_weights floats in all; a band that would leave the spectrum or the array is cut there).  dct: the
 * caller's table [n_mfcc, n_mels] (librosa: orthonormal DCT-II).  Two launches (the clamp needs the item's
 * maximum).  Workspace: ddsp_hip_mfcc_workspace_size bytes (0 for sizes outside the envelope); after the call
 * its first batch * frames * n_mels floats hold D before the clamp, [batch, frames, n_mels]. */
size_t ddsp_hip_mfcc_workspace_size(int64_t batch, int64_t n_samples, int64_t n_fft, int64_t hop, int64_t n_mels);
int ddsp_hip_mfcc(const float* x, const int32_t* band_start, const int32_t* band_count, const float* band_weights,
                  int64_t n_band_weights, const float* dct, float* out, int64_t batch, int64_t n_samples,
                  int64_t n_fft, int64_t hop, int64_t n_mels, int64_t n_mfcc, float top_db, void* workspace,
                  size_t workspace_bytes, void* stream);

/* ---------------- backward (training): train.py:84-130 back-propagates through the path ----------------
 * Vector-Jacobian products of the entry points above.  `grad*` inputs are the upstream
 * gradients (same shapes as the forward outputs), `grad_*` outputs are caller-allocated and
 * overwritten.  Pitch (f0) is an input feature in the reference's training loop and gets no
 * gradient. */

/* core.py:77-78 scale_function backward: dx = grad * scale'(x + bias). */
int ddsp_hip_scale_function_backward(const float* x, const float* grad, float* dx, int64_t n, float bias,
                                     void* stream);

/* core.py:64-67 upsample backward: dx[B,F,C] = sum over each block of grad[B,F*factor,C]. */
int ddsp_hip_upsample_backward(const float* grad, float* dx, int64_t batch, int64_t frames, int64_t channels,
                               int64_t factor, void* stream);

/* core.py:136-141 harmonic_synth backward w.r.t. amplitudes at the op boundary:
 * grad_amplitudes[B,T,H] = grad[B,T] * sin(fl32(omega[B,T] * k)); omega from ddsp_hip_phase. */
int ddsp_hip_harmonic_synth_backward(const float* omega, const float* grad, float* grad_amplitudes,
                                     int64_t batch, int64_t n_samples, int64_t n_harmonic, void* stream);

/* core.py:144-166 amp_to_impulse_response backward: grad_impulse[rows,target] -> grad_amp[rows,NB]. */
int ddsp_hip_amp_to_impulse_response_backward(const float* grad_impulse, float* grad_amp, int64_t rows,
                                              int64_t n_bands, int64_t target_size, void* stream);

/* modules.py:44-67 HarmonicSynth.get_controls backward: (grad_amplitudes[rows], grad_distribution
 * [rows,H]) -> gradients of the raw inputs (strided as in ddsp_hip_harmonic_controls). */
int ddsp_hip_harmonic_controls_backward(const float* amplitudes_raw, int64_t amp_stride,
                                        const float* distribution_raw, int64_t dist_stride, const float* f0,
                                        const float* grad_amplitudes, const float* grad_distribution,
                                        float* grad_amplitudes_raw, float* grad_distribution_raw,
                                        int64_t rows, int64_t n_harmonic, float sample_rate, void* stream);

/* modules.py:69-80 HarmonicSynth.forward backward (ddsp_hip_harmonic_synth_frames): the sine products
 * summed over each block, dA[b,f,k] = sum_t grad[t] sin(w_t k), then grad_distribution = dA * amp and
 * grad_amplitudes = sum_k dA * distribution.  `distribution` is the normalised distribution
 * BEFORE the in-place multiplication by the amplitudes. */
int ddsp_hip_harmonic_synth_frames_backward(const float* f0, const float* amplitudes, const float* distribution,
                                            const float* grad, float* grad_amplitudes,
                                            float* grad_distribution, int64_t batch, int64_t frames,
                                            int64_t n_harmonic, int64_t block_size, float sample_rate,
                                            void* stream);

/* decoder.py:106-113 + modules.py:44-80 backward (ddsp_hip_harmonic_synth_params, and the harmonic
 * half of ddsp_hip_synth_frames): grad[B,F*bs] -> grad_param[B,F,H+1]. */
int ddsp_hip_harmonic_synth_params_backward(const float* f0, const float* param, const float* grad,
                                            float* grad_param, int64_t batch, int64_t frames,
                                            int64_t n_harmonic, int64_t block_size, float sample_rate,
                                            void* stream);

/* The pitch (f0) gradient of the frame-rate harmonic synthesis, what the reference's autograd sends into f0
 * through torch.cumsum and torch.sin (core.py:136-141; remove_above_nyquist, a comparison, contributes nothing):
 *   grad_f0[b,f] = c (R_f + bs sum_{f'>f} Q_{f'}),  c = 2 pi / sample_rate,
 *   Q_f = sum_j q_j, R_f = sum_j (j+1) q_j,  q_j = grad[f,j] sum_k k A_k cos(fl32(omega_{f,j} k)),
 * with the frame kernels' phase omega_{f,j} and the frame's harmonic amplitudes A_k, formed either from the frame
 * controls (ddsp_hip_harmonic_synth_frames_pitch_grad: amplitudes[B,F] and the normalised distribution[B,F,H]
 * BEFORE the in-place multiplication, as ddsp_hip_harmonic_synth_frames_backward takes them) or from the raw
 * projection (ddsp_hip_harmonic_synth_params_pitch_grad: param[B,F,H+1], also the harmonic half of
 * ddsp_hip_synth_frames).  grad[B,F*bs] -> grad_f0[B,F].  Two launches (the per-frame sums as doubles in the
 * workspace, then a reverse scan over each item's frames; past 512 frames per item a ddsp_hip_frame_phase_prefix
 * launch ahead of them).  workspace: 8-byte aligned, ddsp_hip_frame_pitch_grad_workspace_size(batch, frames)
 * bytes.  ddsp_hip_frame_pitch_grad_scan_chunk: the frames per step of the reverse scan (any frame count is
 * valid; tests place frame counts around its multiples).
 * Checked before any launch: negative batch / frames, block_size < 1, n_harmonic < 1, sample_rate not > 0, null
 * buffers or workspace: DDSP_HIP_EINVAL; batch > 65535, n_harmonic > 4096, block_size > 8192: DDSP_HIP_ERANGE; a
 * short workspace: DDSP_HIP_EWORKSPACE; batch == 0 or frames == 0: a no-op success.  The per-sample op
 * (ddsp_hip_harmonic_synth, f0[B,T]) has no f0 gradient here: that is a scan over T, another kernel. */
size_t ddsp_hip_frame_pitch_grad_workspace_size(int64_t batch, int64_t frames);
int64_t ddsp_hip_frame_pitch_grad_scan_chunk(void);
int ddsp_hip_harmonic_synth_frames_pitch_grad(const float* f0, const float* amplitudes, const float* distribution,
                                              const float* grad, float* grad_f0, int64_t batch, int64_t frames,
                                              int64_t n_harmonic, int64_t block_size, float sample_rate,
                                              void* workspace, size_t workspace_bytes, void* stream);
int ddsp_hip_harmonic_synth_params_pitch_grad(const float* f0, const float* param, const float* grad, float* grad_f0,
                                              int64_t batch, int64_t frames, int64_t n_harmonic, int64_t block_size,
                                              float sample_rate, void* workspace, size_t workspace_bytes,
                                              void* stream);

/* decoder.py:106-121 backward (ddsp_hip_synth_frames): grad_param[B,F,H+1] and grad_magnitudes[B,F,NB]
 * (raw projections) from the upstream gradient of the signal, as two launches (harmonic, noise); the noise
 * is `noise` or the forward's Philox (seed, offset).  grad_noise (nullable) is a separate upstream
 * gradient for the noise half (when the parts are used separately); NULL = grad_harmonic. */
int ddsp_hip_synth_frames_backward(const float* f0, const float* param, const float* raw_magnitudes, float bias,
                                   const float* noise, uint64_t seed, uint64_t offset, const float* grad_harmonic,
                                   const float* grad_noise, float* grad_param, float* grad_magnitudes,
                                   int64_t batch, int64_t frames, int64_t n_harmonic, int64_t n_bands,
                                   int64_t block_size, float sample_rate, void* stream);

/* modules.py:111-128 FilteredNoise backward (ddsp_hip_filtered_noise[_params], the noise half of
 * ddsp_hip_synth_frames): grad[B,F*bs] -> grad_magnitudes[B,F,NB].  The noise is `noise` as given
 * to the forward, or (noise == NULL) regenerated from the forward's (seed, offset).  raw != 0:
 * `magnitudes` are the raw projections and scale_function(x + bias) is differentiated too. */
int ddsp_hip_filtered_noise_backward(const float* magnitudes, const float* noise, uint64_t seed, uint64_t offset,
                                     int raw, float bias, const float* grad, float* grad_magnitudes,
                                     int64_t batch, int64_t frames, int64_t n_bands, int64_t block_size,
                                     void* stream);

/* modules.py:28-35 Reverb.forward backward.
 *   ddsp_hip_reverb_apply_transposed: grad_x[b,t] = sum_tau grad[b,t+tau] IR[tau] (same spectrum and
 *     workspace as ddsp_hip_reverb_apply);
 *   ddsp_hip_reverb_backward: grad_x (nullable) as above and grad_impulse[tau] (nullable) =
 *     sum_b sum_t grad[b,t+tau] x[b,t] for tau < L (zero for taps cropped away when L > n_samples),
 *     sharing one transform of grad.  input_spectra (nullable): the first
 *     ddsp_hip_reverb_input_spectra_bytes bytes of the workspace ddsp_hip_reverb_apply used for this
 *     x, which hold x's partition spectra on return — kept by the caller, they spare a transform of x;
 *   ddsp_hip_reverb_impulse_backward (modules.py:21-26): grad_impulse -> grad_noise[L], and the
 *     device scalars grad_decay, grad_wet (taps >= grad_length carry no gradient). */
int ddsp_hip_reverb_apply_transposed(const float* grad, const float* spectrum, float* grad_x, int64_t batch,
                                     int64_t n_samples, int64_t ir_length, void* workspace,
                                     size_t workspace_bytes, void* stream);
size_t ddsp_hip_reverb_input_spectra_bytes(int64_t batch, int64_t n_samples);
size_t ddsp_hip_reverb_backward_workspace_size(int64_t batch, int64_t n_samples, int64_t ir_length,
                                               int have_input_spectra);
int ddsp_hip_reverb_backward(const float* x, const float* input_spectra, const float* spectrum, const float* grad,
                             float* grad_x, float* grad_impulse, int64_t batch, int64_t n_samples,
                             int64_t ir_length, void* workspace, size_t workspace_bytes, void* stream);
/* modules.py:21-35 Reverb.forward backward with respect to the signal AND the reverb's parameters in one call:
 * ddsp_hip_reverb_backward's grad_x (nullable) and ddsp_hip_reverb_impulse_backward's grad_noise[ir_length],
 * grad_decay, grad_wet (device scalars) from grad_impulse without materialising it — the partition
 * transforms of the impulse gradient also apply build_impulse's backward and reduce the decay / wet sums
 * (in a fixed order: deterministic).  Workspace: ddsp_hip_reverb_backward_workspace_size. */
int ddsp_hip_reverb_backward_params(const float* x, const float* input_spectra, const float* spectrum, const float* grad,
                                    const float* noise, const float* decay, const float* wet, float sample_rate,
                                    float* grad_x, float* grad_noise, float* grad_decay, float* grad_wet, int64_t batch,
                                    int64_t n_samples, int64_t ir_length, void* workspace, size_t workspace_bytes,
                                    void* stream);
size_t ddsp_hip_reverb_impulse_backward_workspace_size(int64_t length);
int ddsp_hip_reverb_impulse_backward(const float* noise, const float* decay, const float* wet,
                                     const float* grad_impulse, int64_t length, int64_t grad_length,
                                     float sample_rate, float* grad_noise, float* grad_decay, float* grad_wet,
                                     void* workspace, size_t workspace_bytes, void* stream);

/* ---------------- seamless realtime streaming ----------------
 * K calls of N samples that render what one call of K N samples renders (no reference counterpart: the
 * reference's realtime model restarts every oscillator at phase zero on each call and has no reverb,
 * decoder.py:138-158, export.py:37-40).  The stream's state is ONE caller-allocated device buffer of
 * ddsp_hip_stream_state_bytes(batch, call_samples, ir_length) bytes, 16-byte aligned, zero-filled for a fresh
 * stream: double carry[batch] (the running phase prefix per item) at offset 0, then, with ir_length > 0, the
 * reverb's previous input block and its ring of P = ceil(ir_length / call_samples) block spectra per item
 * (ir_length 0: the carry alone, any call_samples).  The call counter is a device word of the caller's
 * (zero for a fresh stream): it is the Philox offset of the on-device noise and, modulo P, the reverb's ring
 * slot, so a captured HIP graph replays with no by-value state.  One call of the stream is
 *   ddsp_hip_stream_synth_frames -> [ddsp_hip_stream_reverb] -> ddsp_hip_stream_advance
 * on one HIP stream: the first two only read the counter and the carry, the advance moves both. */
size_t ddsp_hip_stream_state_bytes(int64_t batch, int64_t call_samples, int64_t ir_length);
/* floats of the stream reverb's IR partition spectra (P x (call_samples + 1) complex bins); 0 outside the
 * reverb's range (call_samples a power of two in [64, 2048], ir_length >= 1) */
size_t ddsp_hip_stream_spectrum_floats(int64_t call_samples, int64_t ir_length);
/* The IR partition spectra of impulse[ir_length] (Reverb.build_impulse at full length, modules.py:21-26) for
 * calls of call_samples: shared by all items, built once per IR.  DDSP_HIP_ERANGE outside the range above,
 * DDSP_HIP_EWORKSPACE when spectrum_floats is short. */
int ddsp_hip_stream_spectrum(const float* impulse, int64_t ir_length, int64_t call_samples, float* spectrum,
                             size_t spectrum_floats, void* stream);
/* ddsp_hip_synth_frames for one call of a stream: frame f uses the phase prefix carry[b] + sum_{g<f} bs inc_g in
 * fp64 (wrap != 0: the carry reduced modulo 2 pi first).  noise [B,F,bs] injected, or NULL: on-device Philox
 * with (seed, offset = *counter).  Envelope and DDSP_HIP_ERANGE as ddsp_hip_synth_frames; DDSP_HIP_EWORKSPACE
 * when state_bytes is short.  Reads state and counter only. */
int ddsp_hip_stream_synth_frames(const float* f0, const float* param, const float* raw_magnitudes, float bias,
                                 const float* noise, uint64_t seed, const uint64_t* counter, const void* state,
                                 size_t state_bytes, int wrap, float* out, float* harmonic_out, float* noise_out,
                                 int64_t batch, int64_t frames, int64_t n_harmonic, int64_t n_bands,
                                 int64_t block_size, float sample_rate, void* stream);
/* One call of the stream's reverb: y[B, N] such that the calls' outputs laid end to end are the causal
 * convolution (x_all * impulse)[0 : K N] with the impulse at its full length (modules.py:28-35 without the
 * crop to the input's length).  One launch, one workgroup per item; y may be x.  call_samples a power of two
 * in [64, 2048] (else DDSP_HIP_ERANGE); DDSP_HIP_EWORKSPACE when state_bytes or spectrum_floats is short.
 * Writes the item's history and ring slot *counter mod P; reads the counter. */
int ddsp_hip_stream_reverb(const float* x, const float* spectrum, size_t spectrum_floats, const uint64_t* counter,
                           void* state, size_t state_bytes, float* y, int64_t batch, int64_t call_samples,
                           int64_t ir_length, void* stream);
/* The end of a call, one one-workgroup launch: carry[b] += sum_g bs inc_g over the call's frames f0[B, F]
 * (wrap != 0: then reduced modulo 2 pi in fp64 — sin(k omega) is unchanged for the integer harmonic numbers k
 * and omega keeps its fp32 resolution for ever) and *counter += 1.  batch or frames 0: the counter alone. */
int ddsp_hip_stream_advance(const float* f0, uint64_t* counter, void* state, size_t state_bytes, int wrap,
                            int64_t batch, int64_t frames, int64_t block_size, float sample_rate, void* stream);

/* ---------------- streaming analysis: the features of a stream, call by call ----------------
 * The input side of a realtime stream: each call hands over the next N = call_samples samples x[batch, N] of the
 * stream x_all and receives the R = N / hop feature frames whose windows those samples complete, computed with the
 * arithmetic of ddsp_hip_loudness / ddsp_hip_mfcc (periodic Hann(n_fft), unnormalised fp64 transform, fp32 logs,
 * fixed-order reductions, no atomics: bit-reproducible and independent of the batch around an item).
 *
 * Frames.  Frame f is the n_fft samples x_all[f * hop - n_fft/2 + i], i = 0 .. n_fft-1, with 0 where the index is
 * negative: samples before the stream's start are zero.  A stream has no "before", so the offline entry points'
 * reflect padding does not apply (away from the first n_fft/2 samples the frames are the offline ones).  With
 * d = ceil((n_fft/2) / hop), call k (the device counter; 0 for a fresh stream) receives samples [k N, (k+1) N) and
 * emits
 *     f = k R - d + 1 + j,   j = 0 .. R-1,
 * the frames that have just become complete (the newest sample needed, (k+1) N - d hop + n_fft/2 - 1, is at most
 * (k+1) N - 1).  Frames with f < 0 lie before the stream and are computed like any other, from zeros.  The
 * features therefore lag the reference's decimated alignment (frame f at sample f * hop) by d - 1 frames: 768
 * samples at n_fft 2048 and hop 256.  The call's frames ride two per complex transform as (j, j + 1), j even (R
 * odd: the last alone), so the bits are not those of the offline entry points, whose pairs are (f, f + 1), f even.
 *
 * State: one caller-allocated device buffer of ddsp_hip_stream_features_state_bytes(batch, call_samples, n_fft,
 * hop) bytes per feature, 16-byte aligned, zero-filled for a fresh stream: per item a ring of Hs + N floats
 * (Hs = (d-1) hop + n_fft/2 carried samples; sample s of the stream at position s mod (Hs + N)), then one float
 * per item, the MFCC's running maximum; the size rounded up to 16 bytes.  Call k reads [k N - Hs, k N) from the
 * ring and [k N, (k+1) N) from x, and copies x over the ring's region for [k N, (k+1) N): with that length the
 * region written is disjoint from everything the call reads, so the copy needs no ordering, and running call k
 * twice before the advance gives the same bits.  The counter is the stream's (see above): these entry points read
 * it, ddsp_hip_stream_advance ends the call — one advance for synthesis and analysis alike when they share it.
 *
 * Envelope, checked before any HIP call: n_fft a power of two in [16, 4096] (else DDSP_HIP_ERANGE), hop >= 1 and
 * call_samples a positive multiple of hop (else DDSP_HIP_EINVAL), R <= 32, batch <= 65535 and call_samples <=
 * 2^24 (else DDSP_HIP_ERANGE); for the MFCC 1 <= n_mfcc <= n_mels and top_db >= 0 (else DDSP_HIP_EINVAL), n_mels
 * <= 256 (else DDSP_HIP_ERANGE).  Null pointers and negative sizes: DDSP_HIP_EINVAL; batch == 0: a no-op success;
 * a short state: DDSP_HIP_EWORKSPACE.  ddsp_hip_stream_features_state_bytes is 0 outside the envelope and for
 * batch < 1. */
size_t ddsp_hip_stream_features_state_bytes(int64_t batch, int64_t call_samples, int64_t n_fft, int64_t hop);

/* ddsp/core.py:81-97 extract_loudness over a stream: out[b, j] = mean over k' = 0..n_fft/2 of
 * (ln(|X[b, f, k']| + 1e-7) + weights[k']) for the call's frames f = k R - d + 1 + j; weights as
 * ddsp_hip_loudness (NULL = zeros).  out [batch, R].  One launch. */
int ddsp_hip_stream_loudness(const float* x, const float* weights, float* out, const uint64_t* counter, void* state,
                             size_t state_bytes, int64_t batch, int64_t call_samples, int64_t n_fft, int64_t hop,
                             void* stream);

/* ddsp/preprocess.py:30-32 librosa.feature.mfcc over a stream: D[b, j, m] = 10 log10(max(1e-10, mel energy)) of the
 * call's frames f = k R - d + 1 + j (tables as ddsp_hip_mfcc), the clamp, then out[b, j, i] = sum_m dct[i, m]
 * D[b, j, m] — out [batch, R, n_mfcc].  The clamp is causal: D <- max(D, runmax - top_db) with runmax the item's
 * maximum over every D the stream has emitted up to and including this call, carried in the state ("no maximum
 * yet" is taken from counter == 0, not from the stored bits).  It equals the offline clamp (the item's global
 * maximum) once the item's loudest frame has passed; before that it differs from it by construction.  One launch,
 * one workgroup per item, no workspace. */
int ddsp_hip_stream_mfcc(const float* x, const int32_t* band_start, const int32_t* band_count,
                         const float* band_weights, int64_t n_band_weights, const float* dct, float* out,
                         const uint64_t* counter, void* state, size_t state_bytes, int64_t batch,
                         int64_t call_samples, int64_t n_fft, int64_t hop, int64_t n_mels, int64_t n_mfcc, float top_db,
                         void* stream);

/* ---------------- pitch: YIN f0 from raw audio, offline and per call of a stream ----------------
 * The reference's extract_pitch (ddsp/core.py:100-119) is the CREPE network; this is not it but the classical YIN
 * estimator (de Cheveigne & Kawahara, JASA 2002), so that the third input of the models can come from audio too.
 *
 * Parameters.  frame_length L, a power of two in [64, 4096]; W = L/2; hop; sample_rate sr; threshold (0.1 is usual);
 * the lag range tau_min .. tau_max in samples, which the caller derives from its frequency range once, in double
 * precision: tau_min = max(floor(sr / fmax), 1), tau_max = min(ceil(sr / fmin), L - W - 1).  The entry points take
 * the integers, so that caller and kernel cannot disagree about a rounding; 1 <= tau_min <= tau_max <= W - 1.
 *
 * Frames, no window applied.  Offline, frame f is y[i] = x[reflect(f * hop - L/2 + i)], i < L, for
 * f = 0 .. n_samples/hop - 1: ddsp_hip_loudness's frames.  Streamed, the frames of "streaming analysis" above with
 * n_fft := L: frame f starts at f * hop - L/2, samples before the stream are zero, call k emits f = k R - d + 1 + j.
 *
 * Per frame, for tau = 0 .. tau_max + 1, in fp64 on the fp32 samples:
 *   1. E(tau) = sum_{j<W} y[j + tau]^2
 *   2. r(tau) = sum_{j<W} y[j] y[j + tau]
 *   3. d(tau) = E(0) + E(tau) - 2 r(tau)
 *   4. d(tau) := 0 wherever d(tau) < 2^-40 (E(0) + E(tau)): silent, onset and exactly periodic frames come out the
 *      same whether r is a direct sum (exactly 0 or exactly cancelling there) or taken through a transform
 *      (~1e-16 E); 2^-40 is far below what an fp32 input with audible content produces and far above the fp64
 *      transform's error.  (r(tau) is exactly 0 where y[0..W) or y[tau..tau+W) is all zeros; the kernels return
 *      exactly that.)
 *   5. d'(0) = 1; with S(tau) = sum_{k=1..tau} d(k), d'(tau) = d(tau) tau / S(tau) if S(tau) > 0, else 1
 *   6. candidates: tau in [tau_min, tau_max] with d'(tau) < d'(tau-1) and d'(tau) <= d'(tau+1).  tau* = the smallest
 *      candidate with d' < threshold; if there is none, the smallest tau in [tau_min, tau_max] attaining the minimum
 *      of d' over that range
 *   7. with a = d'(tau*-1), b = d'(tau*), c = d'(tau*+1): if b <= a, b <= c and a - 2b + c > 0 the shift is
 *      s = (a - c) / (2 (a - 2b + c)), otherwise s = 0
 *   8. f0 = sr / (tau* + s), confidence = 1 - min(1, b - (a - c) s / 4), period = tau*.
 * An all-zero frame therefore gives period tau_min, f0 = sr / tau_min and confidence 0, never a NaN.  The threshold
 * is the fp32 value passed, widened.  Outputs: f0 and confidence fp32, period int32, each [batch, frames]; confidence
 * and period may be NULL.  r goes through the fp64 transform of features (d cancels to zero at the pitch), E and S
 * through fp64 scans, tau* through fixed-order reductions: no atomics, bit-reproducible, independent of the batch
 * around an item.  One launch.
 * Checked before any HIP call: null x / f0 (streamed: counter, state too), sizes < 1, tau bounds, sr <= 0 (NaN
 * included), frame_length/2 >= n_samples (reflect padding, as ddsp_hip_loudness): DDSP_HIP_EINVAL; frame_length not
 * a power of two in [64, 4096], batch > 65535 and the streaming envelope's caps: DDSP_HIP_ERANGE; a short state:
 * DDSP_HIP_EWORKSPACE; batch == 0: a no-op success. */
int ddsp_hip_pitch(const float* x, float* f0, float* confidence, int32_t* period, int64_t batch, int64_t n_samples,
                   int64_t frame_length, int64_t hop, int64_t tau_min, int64_t tau_max, float sample_rate,
                   float threshold, void* stream);

/* The same per call of a stream: x [batch, call_samples], outputs [batch, R].  State: a buffer of
 * ddsp_hip_stream_features_state_bytes(batch, call_samples, frame_length, hop) bytes of its own, zero-filled for a
 * fresh stream (the trailing float per item is unused); the counter is read and never written, and may be shared
 * with the other features and with a synthesis stream.  The call copies x into the ring under the argument given
 * above, so a call run twice before the advance gives the same bits. */
int ddsp_hip_stream_pitch(const float* x, float* f0, float* confidence, int32_t* period, const uint64_t* counter,
                          void* state, size_t state_bytes, int64_t batch, int64_t call_samples, int64_t frame_length,
                          int64_t hop, int64_t tau_min, int64_t tau_max, float sample_rate, float threshold,
                          void* stream);

/* ---------------- pitch_viterbi: a Viterbi-decoded f0 over YIN's d' as the salience, offline ----------------
 * The reference's extract_pitch is crepe.predict(..., viterbi=True): a salience per frame, then a Viterbi decode over
 * time.  The decode does not care which estimator made the salience; here the salience is 1 - d' of "pitch" above, so
 * that a frame whose smallest dip sits an octave off is overruled by its neighbours.  Two launches, offline only (the
 * decode needs the future; "pitch_viterbi_stream" below is its fixed-lag form for a stream).
 *
 * Frames and d'.  Exactly ddsp_hip_pitch's: offline reflect-indexed frames, L a power of two in [64, 4096], W = L/2,
 * hop, d'(tau) for tau = 0 .. tau_max + 1 by steps 1-5 of "pitch" in fp64, the 2^-40 floor and the zero-energy rule
 * included; tau_min and tau_max as there.
 *
 * Bins: host integers, built once in double precision.  With beta = bins per octave (48 is usual: 25 cents),
 *   bin(tau) = rint(beta log2(tau_max / tau)) for tau in [tau_min, tau_max] (rint: halves to even), so bin(tau_max) = 0;
 *   n_bins NB = bin(tau_min) + 1, at most 1024 (else DDSP_HIP_ERANGE);
 *   lo_i / hi_i = the smallest / the largest tau with bin(tau) = i; where no lag falls in bin i (high frequencies),
 *   lo_i = hi_i = clip(rint(tau_max 2^(-i / beta)), tau_min, tau_max).
 * The entry point takes lo[NB] and hi[NB] as int32 device arrays and clamps them into tau_min <= lo_i <= hi_i <=
 * tau_max, so that no table can make it read outside d'.
 *
 * Salience, per frame f and bin i:
 *   tau^ = the smallest tau in [lo_i, hi_i] attaining the minimum of d' over that range;
 *   cost(f, i) = (float)min(1, d'(tau^));
 *   f0c(f, i)  = (float)(sr / (tau^ + s)), s by step 7 of "pitch" over d'(tau^ - 1 .. tau^ + 1);
 *   lag(f, i)  = tau^.
 * A silent frame gives cost 1 in every bin and f0c = sr / lo_i: finite, never a NaN.
 *
 * Decode, per item over its frames t = 0 .. F - 1, all in fp64; lambda = transition (the fp32 value passed, widened),
 * R = max_jump in bins, 0 <= R <= 127; pen(k) = lambda k (exact):
 *   delta_0(j) = cost(0, j);
 *   delta_t(j) = min over i in [max(0, j - R), min(NB - 1, j + R)] of (delta_{t-1}(i) + pen(|i - j|)),
 *                then + cost(t, j);  bp_t(j) = the smallest i attaining that minimum;
 *   path(F - 1) = the smallest argmin of delta_{F-1};  path(t - 1) = bp_t(path(t));
 *   f0(t) = f0c(t, path(t)), confidence(t) = 1 - cost(t, path(t)), path(t) int32: each [batch, F].
 * Every operation is one fp64 addition or a comparison, so a restatement reproduces the path bit for bit from the
 * same costs.  With lambda > 0 and all costs equal the path is all zeros.  Fixed orders, no atomics: two runs give the
 * same bits and an item's bits do not depend on the batch around it.
 *
 * ddsp_hip_pitch_salience: x [batch, n_samples] -> cost, f0c [batch, F, NB] fp32, lag [batch, F, NB] int32 (may be
 * NULL), F = n_samples / hop; pitch_kernel's grid.  With f0 given ([batch, F]; confidence and period [batch, F] may
 * then be given too) the same launch also writes ddsp_hip_pitch's outputs for the threshold, bit for bit.
 * Checked before any HIP call, as ddsp_hip_pitch, and: n_bins < 1, confidence or period without f0: DDSP_HIP_EINVAL;
 * n_bins > 1024: DDSP_HIP_ERANGE; batch == 0: a no-op success; null x / lo / hi / cost / f0c: DDSP_HIP_EINVAL. */
int ddsp_hip_pitch_salience(const float* x, const int32_t* lo, const int32_t* hi, float* cost, float* f0c,
                            int32_t* lag, float* f0, float* confidence, int32_t* period, int64_t batch,
                            int64_t n_samples, int64_t frame_length, int64_t hop, int64_t tau_min, int64_t tau_max,
                            int64_t n_bins, float sample_rate, float threshold, void* stream);

/* The decode: cost, f0c [batch, frames, n_bins] -> f0, confidence (may be NULL), path [batch, frames].  One workgroup
 * per item, one thread per bin, one barrier per frame: latency-bound by design (a preprocessing step).  The workspace
 * holds the back-offsets bp_t(j) - j as int8: ddsp_hip_pitch_viterbi_workspace_bytes = batch frames n_bins bytes (0
 * for sizes the entry point refuses); nothing in it needs zeroing.  The backtrack stages them through LDS
 * ddsp_hip_pitch_viterbi_chunk_frames(n_bins) = min(32768 / n_bins, 512) frames at a time (0 outside [1, 1024]).
 * Checked before any HIP call: negative batch / frames / max_jump, n_bins < 1, transition negative, infinite or NaN:
 * DDSP_HIP_EINVAL; n_bins > 1024, max_jump > 127: DDSP_HIP_ERANGE; batch == 0 or frames == 0: a no-op success; null
 * cost / f0c / f0 / path / workspace: DDSP_HIP_EINVAL; a short workspace: DDSP_HIP_EWORKSPACE. */
size_t ddsp_hip_pitch_viterbi_workspace_bytes(int64_t batch, int64_t frames, int64_t n_bins);
int64_t ddsp_hip_pitch_viterbi_chunk_frames(int64_t n_bins);
int ddsp_hip_pitch_viterbi(const float* cost, const float* f0c, float* f0, float* confidence, int32_t* path,
                           void* workspace, size_t workspace_bytes, int64_t batch, int64_t frames, int64_t n_bins,
                           int64_t max_jump, float transition, void* stream);

/* ---------------- pitch_viterbi_stream: the same decode per call of a stream, at a fixed lag ----------------
 * Only the final backtrack of "pitch_viterbi" needs the future; the forward recursion is causal.  Carried from call
 * to call in a device state, it gives at frame n the best endpoint s_n = argmin delta_n, and walking its
 * back-pointers D frames gives a decision for frame n - D that has seen D frames of its future.  Two launches per
 * call, salience then decode (not one: the decode needs every frame's costs, and no workgroup here waits for
 * another).  No reference counterpart: crepe.predict(..., viterbi=True) decodes a whole file.
 *
 * Salience.  ddsp_hip_stream_pitch_salience is ddsp_hip_pitch_salience over the stream's own frames, as
 * ddsp_hip_stream_pitch is to ddsp_hip_pitch: call k emits f = k R - d + 1 + j, zeros before the stream, L, hop,
 * tau_min, tau_max, lo, hi and the per-frame definition exactly as in "pitch_viterbi".  x [batch, call_samples] ->
 * cost, f0c [batch, R, NB] fp32, lag [batch, R, NB] int32 (may be NULL); with f0 given ([batch, R]; confidence and
 * period may then be given too) the same launch also writes ddsp_hip_stream_pitch's outputs for the threshold, bit
 * for bit.  One launch, ddsp_hip_stream_pitch's grid.  State: a ring buffer of ddsp_hip_stream_features_state_bytes(
 * batch, call_samples, frame_length, hop) bytes of its own, zero-filled for a fresh stream; the call copies x into
 * the ring under the argument of "streaming analysis", so a call run twice before the advance gives the same bits.
 * Checked before any HIP call, in this order: the streaming envelope; the pitch parameters (as
 * ddsp_hip_stream_pitch); n_bins < 1: DDSP_HIP_EINVAL, n_bins > 1024: DDSP_HIP_ERANGE; confidence or period without
 * f0: DDSP_HIP_EINVAL; batch == 0: a no-op success; null x / lo / hi / cost / f0c / counter / state:
 * DDSP_HIP_EINVAL; a short state: DDSP_HIP_EWORKSPACE. */
int ddsp_hip_stream_pitch_salience(const float* x, const int32_t* lo, const int32_t* hi, float* cost, float* f0c,
                                   int32_t* lag, float* f0, float* confidence, int32_t* period,
                                   const uint64_t* counter, void* state, size_t state_bytes, int64_t batch,
                                   int64_t call_samples, int64_t frame_length, int64_t hop, int64_t tau_min,
                                   int64_t tau_max, int64_t n_bins, float sample_rate, float threshold,
                                   void* stream);

/* The carried decode.  R = frames_per_call in [1, 32]; NB = n_bins <= 1024; J = max_jump <= 127; lambda = transition
 * (the fp32 value passed, widened); D = lag in frames, 0 <= D <= 64.  Call k = *counter takes cost, f0c [batch, R, NB]
 * of the stream's emitted frames n = k R + j, j < R, and, per item, all in fp64:
 *   delta_0(j) = cost(0, j) — "fresh" is taken from counter == 0, not from the stored bits;
 *   delta_n, bp_n  exactly the recursion of "pitch_viterbi" (one addition or comparison per operation, the smallest
 *                  i among equals), continued across calls;
 *   s_n        = the smallest argmin of delta_n;
 *   m          = n - min(D, n);
 *   path(n)    = bp_{m+1}( ... bp_n(s_n)): min(D, n) steps back from s_n (none for D = 0: path(n) = s_n);
 *   f0(n)      = f0c(m, path(n)), confidence(n) = 1 - cost(m, path(n)).
 * Outputs f0, confidence (may be NULL) fp32 and path int32, each [batch, R]: slot j of call k describes emitted frame
 * m = k R + j - D once n >= D (before that, frame 0 repeatedly: the stream has no earlier decision to give).
 * By construction path(n) is element m of ddsp_hip_pitch_viterbi's path over frames 0 .. n, so the offline
 * restatement is the yardstick, and a restatement reproduces the stream bit for bit from the same costs.
 * delta is never renormalised: a frame adds at most 1 + lambda J (1.24 at the defaults), so after 2^32 frames (265
 * days at 187.5 frames a second) delta is below 2^33 and its fp64 spacing at most 2^-20, 1/20000 of lambda = 0.02;
 * every rounding is the restatement's too, and the result does not depend on how the stream is cut into calls.
 *
 * State: ddsp_hip_stream_viterbi_state_bytes(batch, R, NB, D) bytes, 16-byte aligned, zero-filled for a fresh stream:
 * per item double delta[2][NB], then a ring of P = D + R frames (frame n in slot n mod P) as float f0c[P][NB], float
 * cost[P][NB] and int8 bp[P][NB] (the back-offsets bp_n(j) - j; f0c and cost because frame m may belong to an earlier
 * call), the item rounded up to 8 bytes: batch * roundup8(16 NB + 9 P NB), rounded up to 16; 0 outside the envelope
 * and for batch < 1.  Call k reads row k & 1 and writes row (k + 1) & 1; it writes slots k R .. k R + R - 1 and
 * reads back no further than frame k R - D, whose slot is that of frame k R + R: with depth D + R nothing the call
 * reads is overwritten by it, so a call run twice before the advance gives the same bits.  The counter is read and
 * never written (ddsp_hip_stream_advance ends the call) and may be shared with the salience's ring and any other
 * stream state.
 * One launch: one workgroup per item, one thread per bin, one barrier per frame; the R backtracks run side by side on
 * R threads over the ring in global memory.  Fixed orders, no atomics: two runs give the same bits and an item's bits
 * do not depend on the batch around it.
 * Checked before any HIP call: negative batch / max_jump / lag, frames_per_call < 1, n_bins < 1, transition negative,
 * infinite or NaN: DDSP_HIP_EINVAL; frames_per_call > 32, n_bins > 1024, max_jump > 127, lag > 64: DDSP_HIP_ERANGE;
 * batch == 0: a no-op success; null cost / f0c / f0 / path / counter / state: DDSP_HIP_EINVAL; a short state:
 * DDSP_HIP_EWORKSPACE. */
size_t ddsp_hip_stream_viterbi_state_bytes(int64_t batch, int64_t frames_per_call, int64_t n_bins, int64_t lag);
int ddsp_hip_stream_pitch_viterbi(const float* cost, const float* f0c, float* f0, float* confidence, int32_t* path,
                                  const uint64_t* counter, void* state, size_t state_bytes, int64_t batch,
                                  int64_t frames_per_call, int64_t n_bins, int64_t max_jump, int64_t lag,
                                  float transition, void* stream);

/* ddsp_hip_stream_loudness and ddsp_hip_stream_pitch of one call in ONE launch over ONE state, for a stream whose
 * loudness and pitch use the same frame length L (n_fft == frame_length == L: the same frames of the same samples).
 * loudness_out [batch, R] holds ddsp_hip_stream_loudness(n_fft = L)'s bits and f0 / confidence / period [batch, R]
 * hold ddsp_hip_stream_pitch(frame_length = L)'s bits: the per-frame code is the same and every reduction order is
 * fixed, so only the grid differs — the first workgroups of an item take the pitch frames (one per transform), the
 * rest the loudness frames (two per transform), side by side.  weights as ddsp_hip_loudness (NULL = zeros);
 * confidence and period may be NULL.  State: one buffer of ddsp_hip_stream_features_state_bytes(batch, call_samples,
 * L, hop) bytes, zero-filled for a fresh stream, with the ring layout of "streaming analysis" above — a state either
 * separate entry point has filled can be continued by this one and back.  The counter is read and never written; the
 * call copies x into the ring under the argument given there (no workgroup reads what another writes, whatever its
 * role), so a call run twice before the advance gives the same bits.
 * Checked before any HIP call, in this order: the streaming envelope (as ddsp_hip_stream_loudness), the pitch
 * parameters (as ddsp_hip_stream_pitch, so L in [64, 4096]), batch == 0: a no-op success, null x / loudness_out / f0 /
 * counter / state: DDSP_HIP_EINVAL, a short state: DDSP_HIP_EWORKSPACE. */
int ddsp_hip_stream_analysis(const float* x, const float* weights, float* loudness_out, float* f0, float* confidence,
                             int32_t* period, const uint64_t* counter, void* state, size_t state_bytes, int64_t batch,
                             int64_t call_samples, int64_t frame_length, int64_t hop, int64_t tau_min, int64_t tau_max,
                             float sample_rate, float threshold, void* stream);

/* ddsp_hip_stream_analysis plus ddsp_hip_stream_mfcc of the same frames in ONE launch over ONE state, on ONE time
 * axis: what a z-conditioned model (the reference's ddsp/models/encoder.py autoencoder) needs per call of a stream.
 * L = frame_length is the loudness's and the pitch's frame, M = mfcc_n_fft the MFCC's n_fft, M == L or M == L/2.
 * MFCC slot j of the call uses the M-sample window centred in frame j's L-sample window (sample (L - M)/2 + i of
 * frame j, i < M), so slot j of loudness_out, mfcc_out and f0 all describe stream frame k R - d(L) + 1 + j, where
 * ddsp_hip_stream_mfcc alone would emit frame k R - d(M) + 1 + j.  loudness_out / f0 / confidence / period hold
 * ddsp_hip_stream_analysis' bits; mfcc_out [batch, R, n_mfcc] holds the bits of ddsp_hip_stream_mfcc(n_fft = M) fed
 * the same stream delayed by (d(L) - d(M)) hop samples (that many zeros first), causal clamp included.
 * Grid: per item the pitch and the loudness workgroups of ddsp_hip_stream_analysis, then one more workgroup that runs
 * the streamed MFCC's per-call code over the same ring.  f0 == NULL: no pitch workgroups are launched (loudness and
 * MFCC only, for a caller who brings a pitch track); confidence and period must then be NULL too and tau_min /
 * tau_max / sample_rate / threshold are not looked at.
 * State: ddsp_hip_stream_features_state_bytes(batch, call_samples, L, hop) bytes, zero-filled for a fresh stream, the
 * layout of "streaming analysis" above: the rings, then the float per item that carries the MFCC's running maximum.
 * Every workgroup copies its strided share of x into the ring and none reads a position another writes; the counter
 * is read and never written; a call run twice before the advance gives the same bits (the maximum is folded into a
 * value that already holds it).
 * Checked before any HIP call, in this order: the streaming envelope (as ddsp_hip_stream_loudness) and L a power of
 * two in [64, 2048] (else DDSP_HIP_ERANGE); with f0 the pitch parameters (as ddsp_hip_stream_pitch), without it
 * confidence == period == NULL (else DDSP_HIP_EINVAL); the MFCC parameters: M in {L, L/2} (else DDSP_HIP_ERANGE) and
 * n_band_weights, n_mels, n_mfcc, top_db held to ddsp_hip_stream_mfcc's limits; batch == 0: a no-op success; null x /
 * loudness_out / band tables / dct / mfcc_out / counter / state: DDSP_HIP_EINVAL; a short state: DDSP_HIP_EWORKSPACE. */
int ddsp_hip_stream_analysis_mfcc(const float* x, const float* weights, float* loudness_out, const int32_t* band_start,
                                  const int32_t* band_count, const float* band_weights, int64_t n_band_weights,
                                  const float* dct, float* mfcc_out, float* f0, float* confidence, int32_t* period,
                                  const uint64_t* counter, void* state, size_t state_bytes, int64_t batch,
                                  int64_t call_samples, int64_t frame_length, int64_t mfcc_n_fft, int64_t hop,
                                  int64_t n_mels, int64_t n_mfcc, float top_db, int64_t tau_min, int64_t tau_max,
                                  float sample_rate, float threshold, void* stream);

/* Two-stage serving pipeline (ddsp_pytorch_amd.synth.PipelinedSynthPath; no reference counterpart:
 * the reference synthesises one batch at a time, decoder.py:101-136).  A HIP stream restricted to
 * the CUs whose bits are set in cu_mask (mask_words 32-bit words, bit c = CU index c; HIP deals
 * consecutive indices over the XCDs).  DDSP_HIP_ELAUNCH if the runtime refuses the mask.  The
 * caller owns the stream and releases it with ddsp_hip_stream_destroy. */
int ddsp_hip_stream_create_cu_masked(const uint32_t* cu_mask, int mask_words, void** stream);
int ddsp_hip_stream_destroy(void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DDSP_HIP_H */
