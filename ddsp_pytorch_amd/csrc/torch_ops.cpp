// TorchScript-visible operators `torch.ops.ddsp_hip.*` over the C-ABI (include/ddsp_hip.h).
//
// The reference's export path (export.py:23-65) scripts the model and the realtime host
// (realtime/ddsp_tilde/ddsp_model.cpp:13-52) runs it through libtorch.  Python-level drop-ins
// are invisible to TorchScript, so the synthesis functions are registered here as operators
// with the reference's argument meaning; a scripted graph calls them like any aten op.
// Host code only: every op validates shapes, allocates outputs/workspaces with ATen on the
// tensors' device, and enqueues the C-ABI entry point on the current HIP stream.  Errors
// surface as c10::Error (RuntimeError in Python), as the reference's torch ops would.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <optional>
#include <tuple>

#include "ddsp_hip.h"

namespace {

void* stream_of(const at::Tensor& t) {
  return reinterpret_cast<void*>(c10::hip::getCurrentHIPStream(t.device().index()).stream());
}

void check_dev(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), "ddsp_hip: ", name, " must be on a HIP device (no CPU fallback)");
  TORCH_CHECK(t.scalar_type() == at::kFloat, "ddsp_hip: ", name, " must be float32");
}

at::Tensor c16(const at::Tensor& t) {  // contiguous + 16-byte aligned (float4 accesses)
  at::Tensor c = t.contiguous();
  if (reinterpret_cast<uintptr_t>(c.data_ptr()) % 16) c = c.clone();
  return c;
}

void ok(int st, const char* fn) {
  TORCH_CHECK(st == DDSP_HIP_OK, "ddsp_hip_", fn, " failed: ", ddsp_hip_status_string(st));
}

at::Tensor workspace(size_t bytes, const at::Tensor& like) {
  return at::empty({(int64_t)std::max<size_t>(bytes, 1)}, like.options().dtype(at::kByte));
}

// ---------------- ddsp/core.py ----------------
at::Tensor scale_function(const at::Tensor& x) {  // core.py:77-78
  check_dev(x, "x");
  at::Tensor xc = c16(x), y = at::empty_like(xc);
  ok(ddsp_hip_scale_function(xc.data_ptr<float>(), y.data_ptr<float>(), xc.numel(), 0.0f, stream_of(xc)),
     "scale_function");
  return y;
}

at::Tensor remove_above_nyquist(const at::Tensor& amplitudes, const at::Tensor& f0, double sample_rate) {
  check_dev(amplitudes, "amplitudes");  // core.py:70-74
  check_dev(f0, "f0");
  TORCH_CHECK(f0.size(-1) == 1, "remove_above_nyquist: f0 must end in a size-1 dim");
  const int64_t H = amplitudes.size(-1);
  auto lead = at::infer_size(amplitudes.sizes().slice(0, amplitudes.dim() - 1), f0.sizes().slice(0, f0.dim() - 1));
  std::vector<int64_t> sa(lead), sf(lead);
  sa.push_back(H);
  sf.push_back(1);
  at::Tensor a = c16(amplitudes.expand(sa)), f = c16(f0.expand(sf));
  at::Tensor out = at::empty_like(a);
  ok(ddsp_hip_remove_above_nyquist(a.data_ptr<float>(), f.data_ptr<float>(), out.data_ptr<float>(),
                                   a.numel() / std::max<int64_t>(H, 1), H, (float)sample_rate, stream_of(a)),
     "remove_above_nyquist");
  return out;
}

at::Tensor upsample(const at::Tensor& signal, int64_t factor) {  // core.py:64-67
  check_dev(signal, "signal");
  TORCH_CHECK(signal.dim() == 3, "upsample: expected [batch, frames, channels]");
  at::Tensor x = c16(signal);
  const int64_t B = x.size(0), F = x.size(1), C = x.size(2);
  at::Tensor y = at::empty({B, F * factor, C}, x.options());
  ok(ddsp_hip_upsample(x.data_ptr<float>(), y.data_ptr<float>(), B, F, C, factor, stream_of(x)), "upsample");
  return y;
}

at::Tensor harmonic_synth(const at::Tensor& f0, const at::Tensor& amplitudes, double sample_rate) {
  check_dev(f0, "f0");  // core.py:136-141
  check_dev(amplitudes, "amplitudes");
  TORCH_CHECK(amplitudes.dim() == 3 && f0.dim() == 3 && f0.size(2) == 1 && f0.size(0) == amplitudes.size(0) &&
                  f0.size(1) == amplitudes.size(1),
              "harmonic_synth: expected f0 [B,T,1] and amplitudes [B,T,H]");
  at::Tensor f = c16(f0), a = c16(amplitudes);
  const int64_t B = a.size(0), T = a.size(1), H = a.size(2);
  at::Tensor out = at::empty({B, T, 1}, f.options());
  at::Tensor ws = workspace(ddsp_hip_harmonic_synth_workspace_size(B, T), f);
  ok(ddsp_hip_harmonic_synth(f.data_ptr<float>(), a.data_ptr<float>(), out.data_ptr<float>(), B, T, H,
                             (float)sample_rate, ws.data_ptr(), ws.numel(), stream_of(f)),
     "harmonic_synth");
  return out;
}

at::Tensor amp_to_impulse_response(const at::Tensor& amp, int64_t target_size) {  // core.py:144-166
  check_dev(amp, "amp");
  const int64_t NB = amp.size(-1);
  TORCH_CHECK(NB >= 2, "amp_to_impulse_response: need at least 2 bands");
  at::Tensor x = c16(amp);
  std::vector<int64_t> shape(amp.sizes().begin(), amp.sizes().end());
  shape.back() = target_size;
  at::Tensor out = at::empty(shape, x.options());
  ok(ddsp_hip_amp_to_impulse_response(x.data_ptr<float>(), out.data_ptr<float>(), x.numel() / NB, NB,
                                      target_size, stream_of(x)),
     "amp_to_impulse_response");
  return out;
}

at::Tensor fft_convolve(const at::Tensor& signal, const at::Tensor& kernel) {  // core.py:169-176
  check_dev(signal, "signal");
  check_dev(kernel, "kernel");
  const int64_t N = signal.size(-1);
  TORCH_CHECK(kernel.size(-1) == N, "fft_convolve: signal and kernel lengths differ");
  auto lead = at::infer_size(signal.sizes().slice(0, signal.dim() - 1), kernel.sizes().slice(0, kernel.dim() - 1));
  std::vector<int64_t> full(lead);
  full.push_back(N);
  int64_t rows = 1;
  for (auto d : lead) rows *= d;
  at::Tensor s = c16(signal.expand(full));
  at::Tensor k;
  int64_t krows;
  if (kernel.numel() == N) {
    k = c16(kernel.reshape({N}));
    krows = 1;
  } else {
    k = c16(kernel.expand(full));
    krows = rows;
  }
  at::Tensor out = at::empty(full, s.options());
  at::Tensor ws = workspace(ddsp_hip_fft_convolve_workspace_size(rows, krows, N), s);
  ok(ddsp_hip_fft_convolve(s.data_ptr<float>(), k.data_ptr<float>(), out.data_ptr<float>(), rows, krows, N,
                           ws.data_ptr(), ws.numel(), stream_of(s)),
     "fft_convolve");
  return out;
}

// ---------------- ddsp/models/modules.py (fused) ----------------
std::tuple<at::Tensor, at::Tensor> harmonic_controls(const at::Tensor& amplitudes, const at::Tensor& distribution,
                                                     const at::Tensor& f0, double sample_rate) {
  check_dev(amplitudes, "amplitudes");  // modules.py:44-67
  check_dev(distribution, "harmonic_distribution");
  check_dev(f0, "f0");
  TORCH_CHECK(distribution.dim() == 3, "harmonic_controls: distribution must be [B,F,H]");
  const int64_t B = distribution.size(0), F = distribution.size(1), H = distribution.size(2);
  TORCH_CHECK(amplitudes.sizes() == at::IntArrayRef({B, F, 1}) && f0.sizes() == at::IntArrayRef({B, F, 1}),
              "harmonic_controls: amplitudes and f0 must be [B,F,1]");
  auto rows_view = [](const at::Tensor& t) {  // core._frame_rows: overlapping (e.g. broadcast) rows are copied
    const bool rows = t.stride(-1) == 1 && t.stride(1) >= std::max<int64_t>(t.size(2), 1) &&
                      t.stride(0) == t.size(1) * t.stride(1);
    return rows ? t : t.contiguous();
  };
  at::Tensor a = rows_view(amplitudes), d = rows_view(distribution), f = c16(f0);
  at::Tensor amp_out = at::empty({B, F, 1}, f.options()), dist_out = at::empty({B, F, H}, f.options());
  ok(ddsp_hip_harmonic_controls(a.data_ptr<float>(), a.stride(1), d.data_ptr<float>(), d.stride(1),
                                f.data_ptr<float>(), amp_out.data_ptr<float>(), dist_out.data_ptr<float>(), B * F,
                                H, (float)sample_rate, stream_of(f)),
     "harmonic_controls");
  return {amp_out, dist_out};
}

at::Tensor harmonic_synth_frames(const at::Tensor& f0, const at::Tensor& amplitudes, at::Tensor& distribution,
                                 int64_t block_size, double sample_rate, bool write_back) {
  check_dev(f0, "f0");  // modules.py:69-80
  check_dev(amplitudes, "amplitudes");
  check_dev(distribution, "harmonic_distribution");
  const int64_t B = distribution.size(0), F = distribution.size(1), H = distribution.size(2);
  at::Tensor f = c16(f0), a = c16(amplitudes);
  at::Tensor d = distribution;
  if (write_back) {
    TORCH_CHECK(d.is_contiguous() && reinterpret_cast<uintptr_t>(d.data_ptr()) % 16 == 0,
                "harmonic_synth_frames: in-place write-back needs a contiguous distribution");
  } else {
    d = c16(d);
  }
  at::Tensor out = at::empty({B, F * block_size, 1}, f.options());
  ok(ddsp_hip_harmonic_synth_frames(f.data_ptr<float>(), a.data_ptr<float>(), d.data_ptr<float>(),
                                    write_back ? 1 : 0, out.data_ptr<float>(), B, F, H, block_size,
                                    (float)sample_rate, stream_of(f)),
     "harmonic_synth_frames");
  return out;
}

at::Tensor harmonic_synth_params(const at::Tensor& f0, const at::Tensor& param, int64_t block_size,
                                 double sample_rate) {
  check_dev(f0, "f0");  // decoder.py:106-113 + modules.py:44-80
  check_dev(param, "param");
  const int64_t B = param.size(0), F = param.size(1), H1 = param.size(2);
  TORCH_CHECK(f0.sizes() == at::IntArrayRef({B, F, 1}) && H1 >= 2, "harmonic_synth_params: bad shapes");
  at::Tensor f = c16(f0), p = c16(param);
  at::Tensor out = at::empty({B, F * block_size, 1}, f.options());
  ok(ddsp_hip_harmonic_synth_params(f.data_ptr<float>(), p.data_ptr<float>(), out.data_ptr<float>(), B, F, H1 - 1,
                                    block_size, (float)sample_rate, stream_of(f)),
     "harmonic_synth_params");
  return out;
}

at::Tensor filtered_noise(const at::Tensor& magnitudes, int64_t block_size, const std::optional<at::Tensor>& noise,
                          int64_t seed, int64_t offset, const std::optional<at::Tensor>& add,
                          std::optional<double> raw_bias) {
  check_dev(magnitudes, "magnitudes");  // modules.py:111-128
  const int64_t B = magnitudes.size(0), F = magnitudes.size(1), NB = magnitudes.size(2);
  at::Tensor m = c16(magnitudes);
  at::Tensor n, a;
  if (noise.has_value()) {
    check_dev(*noise, "noise");
    TORCH_CHECK(noise->sizes() == at::IntArrayRef({B, F, block_size}), "filtered_noise: noise must be [B,F,bs]");
    n = c16(*noise);
  }
  if (add.has_value()) {
    check_dev(*add, "add");
    TORCH_CHECK(add->numel() == B * F * block_size, "filtered_noise: add must have B*F*bs elements");
    a = c16(*add);
  }
  at::Tensor out = at::empty({B, F * block_size, 1}, m.options());
  const float* np = n.defined() ? n.data_ptr<float>() : nullptr;
  const float* ap = a.defined() ? a.data_ptr<float>() : nullptr;
  int st;
  if (raw_bias.has_value())
    st = ddsp_hip_filtered_noise_params(m.data_ptr<float>(), (float)*raw_bias, np, (uint64_t)seed, (uint64_t)offset,
                                        ap, out.data_ptr<float>(), nullptr, B, F, NB, block_size, stream_of(m));
  else
    st = ddsp_hip_filtered_noise(m.data_ptr<float>(), np, (uint64_t)seed, (uint64_t)offset, ap,
                                 out.data_ptr<float>(), nullptr, B, F, NB, block_size, stream_of(m));
  ok(st, "filtered_noise");
  return out;
}

// The fused synthesis ops' frame arguments, checked and contiguous (`op` names the operator in the messages)
struct FrameArgs {
  at::Tensor f, p, m, n;  // f0 [B,F,1], param [B,F,H+1], mags [B,F,NB], noise [B,F,bs] or undefined
  const float* np;        // the noise's pointer, or null
  int64_t B, F, H, NB;
};
FrameArgs frame_args(const at::Tensor& f0, const at::Tensor& param, const at::Tensor& mags,
                     const std::optional<at::Tensor>& noise, int64_t block_size, const char* op) {
  check_dev(f0, "f0");
  check_dev(param, "param");
  check_dev(mags, "mags");
  TORCH_CHECK(param.dim() == 3 && mags.dim() == 3, op, ": param [B,F,H+1] and mags [B,F,NB] expected");
  const int64_t B = param.size(0), F = param.size(1), H1 = param.size(2), NB = mags.size(2);
  TORCH_CHECK(f0.sizes() == at::IntArrayRef({B, F, 1}) && mags.size(0) == B && mags.size(1) == F && H1 >= 2, op,
              ": f0 [B,F,1], param [B,F,H+1], mags [B,F,NB] expected");
  FrameArgs a{c16(f0), c16(param), c16(mags), at::Tensor(), nullptr, B, F, H1 - 1, NB};
  if (noise.has_value()) {
    check_dev(*noise, "noise");
    TORCH_CHECK(noise->sizes() == at::IntArrayRef({B, F, block_size}), op, ": noise must be [B,F,bs]");
    a.n = c16(*noise);
    a.np = a.n.data_ptr<float>();
  }
  return a;
}

// decoder.py:106-121 in one launch (ddsp_hip_synth_frames): harmonic + filtered noise, their controls and
// the sum; outside the fused kernel's shape envelope the two module kernels (harmonic_synth_params, then
// filtered_noise adding the harmonic).  parts: the harmonic and noise signals as well.
std::tuple<at::Tensor, at::Tensor, at::Tensor> synth_frames_impl(const at::Tensor& f0, const at::Tensor& param,
                                                                 const at::Tensor& mags, int64_t block_size,
                                                                 double sample_rate, double bias,
                                                                 const std::optional<at::Tensor>& noise,
                                                                 int64_t seed, int64_t offset, bool parts) {
  const FrameArgs a = frame_args(f0, param, mags, noise, block_size, "synth_frames");
  const float *f = a.f.data_ptr<float>(), *p = a.p.data_ptr<float>(), *m = a.m.data_ptr<float>();
  at::Tensor out = at::empty({a.B, a.F * block_size, 1}, a.f.options());
  at::Tensor harm = parts ? at::empty_like(out) : at::Tensor();
  at::Tensor nz = parts ? at::empty_like(out) : at::Tensor();
  float* nzp = parts ? nz.data_ptr<float>() : nullptr;
  int st = ddsp_hip_synth_frames(f, p, m, (float)bias, a.np, (uint64_t)seed, (uint64_t)offset, out.data_ptr<float>(),
                                 parts ? harm.data_ptr<float>() : nullptr, nzp, a.B, a.F, a.H, a.NB, block_size,
                                 (float)sample_rate, stream_of(a.f));
  if (st == DDSP_HIP_ERANGE) {  // outside the fused kernel's envelope: the two module kernels
    at::Tensor h = parts ? harm : at::empty_like(out);
    ok(ddsp_hip_harmonic_synth_params(f, p, h.data_ptr<float>(), a.B, a.F, a.H, block_size, (float)sample_rate,
                                      stream_of(a.f)),
       "harmonic_synth_params");
    st = ddsp_hip_filtered_noise_params(m, (float)bias, a.np, (uint64_t)seed, (uint64_t)offset, h.data_ptr<float>(),
                                        out.data_ptr<float>(), nzp, a.B, a.F, a.NB, block_size, stream_of(a.f));
  }
  ok(st, "synth_frames");
  return {out, harm, nz};
}

at::Tensor synth_frames(const at::Tensor& f0, const at::Tensor& param, const at::Tensor& mags, int64_t block_size,
                        double sample_rate, double bias, const std::optional<at::Tensor>& noise, int64_t seed,
                        int64_t offset) {
  return std::get<0>(synth_frames_impl(f0, param, mags, block_size, sample_rate, bias, noise, seed, offset, false));
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> synth_frames_parts(const at::Tensor& f0, const at::Tensor& param,
                                                                  const at::Tensor& mags, int64_t block_size,
                                                                  double sample_rate, double bias,
                                                                  const std::optional<at::Tensor>& noise,
                                                                  int64_t seed, int64_t offset) {
  return synth_frames_impl(f0, param, mags, block_size, sample_rate, bias, noise, seed, offset, true);
}

at::Tensor reverb_build_impulse(const at::Tensor& noise, const at::Tensor& decay, const at::Tensor& wet,
                                double sample_rate) {
  check_dev(noise, "noise");  // modules.py:21-26
  check_dev(decay, "decay");
  check_dev(wet, "wet");
  at::Tensor n = c16(noise), d = decay.contiguous(), w = wet.contiguous();
  const int64_t L = n.size(0);
  at::Tensor imp = at::empty({1, L, 1}, n.options());
  ok(ddsp_hip_reverb_build_impulse(n.data_ptr<float>(), d.data_ptr<float>(), w.data_ptr<float>(),
                                   imp.data_ptr<float>(), L, (float)sample_rate, stream_of(n)),
     "reverb_build_impulse");
  return imp;
}

at::Tensor reverb_spectrum(const at::Tensor& impulse, int64_t n_samples) {
  check_dev(impulse, "impulse");
  at::Tensor h = c16(impulse.reshape({-1}));
  const int64_t L = h.numel();
  at::Tensor spec = at::empty({(int64_t)ddsp_hip_reverb_spectrum_floats(n_samples, L)}, h.options());
  ok(ddsp_hip_reverb_spectrum(h.data_ptr<float>(), L, n_samples, spec.data_ptr<float>(), stream_of(h)),
     "reverb_spectrum");
  return spec;
}

at::Tensor reverb_apply(const at::Tensor& x, const at::Tensor& spectrum, int64_t ir_length) {
  check_dev(x, "x");  // modules.py:28-35
  check_dev(spectrum, "spectrum");
  const int64_t B = x.size(0), T = x.size(1);
  TORCH_CHECK(spectrum.numel() == (int64_t)ddsp_hip_reverb_spectrum_floats(T, ir_length),
              "reverb_apply: spectrum was computed for a different length");
  at::Tensor xc = c16(x);
  at::Tensor out = at::empty({B, T, 1}, xc.options());
  at::Tensor ws = workspace(ddsp_hip_reverb_workspace_size(B, T, ir_length), xc);
  ok(ddsp_hip_reverb_apply(xc.data_ptr<float>(), spectrum.data_ptr<float>(), out.data_ptr<float>(), B, T,
                           ir_length, ws.data_ptr(), ws.numel(), stream_of(xc)),
     "reverb_apply");
  return out;
}

// ---------------- seamless realtime streaming (ddsp_hip_stream_*) ----------------
// state: the stream's uint8 device buffer (ddsp_hip_stream_state_bytes), counter: its int64 call counter
void check_stream(const at::Tensor& counter, const at::Tensor& state, const at::Tensor& like) {
  TORCH_CHECK(state.is_cuda() && state.scalar_type() == at::kByte && state.is_contiguous() &&
                  state.device() == like.device(),
              "ddsp_hip: the stream state must be a contiguous uint8 tensor on the inputs' device");
  TORCH_CHECK(counter.is_cuda() && counter.scalar_type() == at::kLong && counter.numel() >= 1 &&
                  counter.device() == like.device(),
              "ddsp_hip: the stream counter must be an int64 tensor on the inputs' device");
}

// the call counter as the C-ABI takes it
uint64_t* counter_ptr(const at::Tensor& counter) { return reinterpret_cast<uint64_t*>(counter.data_ptr<int64_t>()); }

at::Tensor synth_frames_stream(const at::Tensor& f0, const at::Tensor& param, const at::Tensor& mags,
                               int64_t block_size, double sample_rate, double bias,
                               const std::optional<at::Tensor>& noise, int64_t seed, const at::Tensor& counter,
                               at::Tensor& state, bool wrap) {
  const FrameArgs a = frame_args(f0, param, mags, noise, block_size, "synth_frames_stream");
  check_stream(counter, state, f0);
  at::Tensor out = at::empty({a.B, a.F * block_size, 1}, a.f.options());
  ok(ddsp_hip_stream_synth_frames(a.f.data_ptr<float>(), a.p.data_ptr<float>(), a.m.data_ptr<float>(), (float)bias,
                                  a.np, (uint64_t)seed, counter_ptr(counter), state.data_ptr(), (size_t)state.numel(),
                                  wrap ? 1 : 0, out.data_ptr<float>(), nullptr, nullptr, a.B, a.F, a.H, a.NB,
                                  block_size, (float)sample_rate, stream_of(a.f)),
     "stream_synth_frames");
  return out;
}

at::Tensor stream_spectrum(const at::Tensor& impulse, int64_t call_samples) {
  check_dev(impulse, "impulse");
  at::Tensor h = c16(impulse.reshape({-1}));
  const int64_t L = h.numel();
  const size_t floats = ddsp_hip_stream_spectrum_floats(call_samples, L);
  TORCH_CHECK(floats > 0, "stream_spectrum: call_samples must be a power of two in [64, 2048] and the IR non-empty");
  at::Tensor spec = at::empty({(int64_t)floats}, h.options());
  ok(ddsp_hip_stream_spectrum(h.data_ptr<float>(), L, call_samples, spec.data_ptr<float>(), floats, stream_of(h)),
     "stream_spectrum");
  return spec;
}

at::Tensor reverb_stream(const at::Tensor& x, const at::Tensor& spectrum, int64_t ir_length,
                         const at::Tensor& counter, at::Tensor& state) {
  check_dev(x, "x");
  check_dev(spectrum, "spectrum");
  check_stream(counter, state, x);
  TORCH_CHECK(x.dim() >= 2 && spectrum.is_contiguous(), "reverb_stream: x [B,N] or [B,N,1], a contiguous spectrum");
  const int64_t B = x.size(0), N = x.size(1);
  TORCH_CHECK(x.numel() == B * N, "reverb_stream: x [B,N] or [B,N,1] expected");
  at::Tensor xc = c16(x);
  at::Tensor out = at::empty_like(xc);
  ok(ddsp_hip_stream_reverb(xc.data_ptr<float>(), spectrum.data_ptr<float>(), (size_t)spectrum.numel(),
                            counter_ptr(counter), state.data_ptr(), (size_t)state.numel(), out.data_ptr<float>(), B, N,
                            ir_length, stream_of(xc)),
     "stream_reverb");
  return out;
}

void stream_advance(const at::Tensor& f0, int64_t block_size, double sample_rate, at::Tensor& counter,
                    at::Tensor& state, bool wrap) {
  check_dev(f0, "f0");
  check_stream(counter, state, f0);
  TORCH_CHECK(f0.dim() == 3 && f0.size(2) == 1, "stream_advance: f0 [B,F,1] expected");
  at::Tensor f = f0.contiguous();
  ok(ddsp_hip_stream_advance(f.data_ptr<float>(), counter_ptr(counter), state.data_ptr(), (size_t)state.numel(),
                             wrap ? 1 : 0, f.size(0), f.size(1), block_size, (float)sample_rate, stream_of(f)),
     "stream_advance");
}

// ---------------- audio analysis (ddsp/core.py:81-97, ddsp/preprocess.py:30-32) ----------------
// x [T] or [B, T] -> the rows [B, T] contiguous (an exported host feeds audio as it has it)
at::Tensor audio_rows(const at::Tensor& x, const char* op) {
  check_dev(x, "x");
  TORCH_CHECK(x.dim() == 1 || x.dim() == 2, op, ": x [time] or [batch, time] expected");
  return c16(x.dim() == 1 ? x.unsqueeze(0) : x);
}

// one call of a stream: x [B, N] or [B, N, 1] -> the rows [B, N] contiguous
at::Tensor call_rows(const at::Tensor& x, const char* op) {
  check_dev(x, "x");
  TORCH_CHECK((x.dim() == 2 || x.dim() == 3) && x.numel() == x.size(0) * x.size(1), op,
              ": x [batch, call_samples] or [batch, call_samples, 1] expected");
  return c16(x.reshape({x.size(0), x.size(1)}));
}

// R, the frames one call [B, N] completes
int64_t call_frames(const at::Tensor& xc, int64_t hop, const char* op) {
  TORCH_CHECK(hop >= 1 && xc.size(1) % hop == 0, op, ": call_samples must be a multiple of hop");
  return xc.size(1) / hop;
}

// the optional A-weighting table of n/2+1 values (`n_name`: what the op calls n) -> contiguous, or undefined
at::Tensor weights_table(const std::optional<at::Tensor>& weights, int64_t n, const char* op, const char* n_name) {
  if (!weights.has_value() || !weights->defined()) return at::Tensor();
  check_dev(*weights, "weights");
  TORCH_CHECK(weights->numel() == n / 2 + 1, op, ": weights must hold ", n_name, "/2+1 values");
  return weights->contiguous();
}
const float* ptr_or_null(const at::Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }

// the mel tables of the MFCC, contiguous, n_mfcc and n_mels taken from dct (the caller has checked band_weights' and
// dct's device, and its hop, before)
struct MelTables {
  at::Tensor bs, bc, bw, d;
  int64_t n_mfcc, n_mels;
};
MelTables mel_tables(const at::Tensor& band_start, const at::Tensor& band_count, const at::Tensor& band_weights,
                     const at::Tensor& dct, const char* op) {
  TORCH_CHECK(dct.dim() == 2, op, ": dct [n_mfcc, n_mels] expected");
  for (const at::Tensor* t : {&band_start, &band_count})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kInt && t->numel() == dct.size(1), op,
                ": band_start and band_count must be int32 HIP tensors of n_mels values");
  return {band_start.contiguous(), band_count.contiguous(), band_weights.contiguous(), dct.contiguous(), dct.size(0),
          dct.size(1)};
}

// the decode's bin tables (lo, hi), contiguous
std::pair<at::Tensor, at::Tensor> bin_tables(const at::Tensor& lo, const at::Tensor& hi, const char* op) {
  for (const at::Tensor* t : {&lo, &hi})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kInt && t->dim() == 1 && t->numel() == lo.numel(), op,
                ": lo and hi must be int32 HIP tensors of n_bins values");
  return {lo.contiguous(), hi.contiguous()};
}

using Tensor3 = std::tuple<at::Tensor, at::Tensor, at::Tensor>;
// fp32, fp32 and int32 outputs of one shape: (f0, confidence, period or path) [B, F]; (cost, f0c, lag) [B, F, n_bins]
Tensor3 three_outputs(const at::Tensor& like, at::IntArrayRef shape) {
  at::Tensor a = at::empty(shape, like.options());
  return {a, at::empty_like(a), at::empty(shape, like.options().dtype(at::kInt))};
}

at::Tensor loudness(const at::Tensor& x, const std::optional<at::Tensor>& weights, int64_t n_fft, int64_t hop) {
  at::Tensor xc = audio_rows(x, "loudness");  // core.py:81-97 extract_loudness
  TORCH_CHECK(hop >= 1, "loudness: hop must be positive");
  const int64_t B = xc.size(0), T = xc.size(1);
  at::Tensor w = weights_table(weights, n_fft, "loudness", "n_fft");
  at::Tensor out = at::empty({B, T / hop}, xc.options());
  ok(ddsp_hip_loudness(xc.data_ptr<float>(), ptr_or_null(w), out.data_ptr<float>(), B, T, n_fft, hop, stream_of(xc)),
     "loudness");
  return x.dim() == 1 ? out.select(0, 0) : out;
}

at::Tensor mfcc(const at::Tensor& x, const at::Tensor& band_start, const at::Tensor& band_count,
                const at::Tensor& band_weights, const at::Tensor& dct, int64_t n_fft, int64_t hop, double top_db) {
  at::Tensor xc = audio_rows(x, "mfcc");  // preprocess.py:30-32 librosa.feature.mfcc(...).T
  check_dev(band_weights, "band_weights");
  check_dev(dct, "dct");
  TORCH_CHECK(hop >= 1, "mfcc: hop must be positive");
  const MelTables m = mel_tables(band_start, band_count, band_weights, dct, "mfcc");
  const int64_t B = xc.size(0), T = xc.size(1), frames = T / hop + 1;
  at::Tensor out = at::empty({B, frames, m.n_mfcc}, xc.options());
  at::Tensor ws = workspace(ddsp_hip_mfcc_workspace_size(B, T, n_fft, hop, m.n_mels), xc);
  ok(ddsp_hip_mfcc(xc.data_ptr<float>(), m.bs.data_ptr<int32_t>(), m.bc.data_ptr<int32_t>(), m.bw.data_ptr<float>(),
                   m.bw.numel(), m.d.data_ptr<float>(), out.data_ptr<float>(), B, T, n_fft, hop, m.n_mels, m.n_mfcc,
                   (float)top_db, ws.data_ptr(), (size_t)ws.numel(), stream_of(xc)),
     "mfcc");
  return x.dim() == 1 ? out.select(0, 0) : out;
}

// ---------------- streaming analysis: one call of a stream (ddsp_hip_stream_loudness / _mfcc) ----------------
at::Tensor loudness_stream(const at::Tensor& x, const std::optional<at::Tensor>& weights, int64_t n_fft, int64_t hop,
                           const at::Tensor& counter, at::Tensor& state) {
  at::Tensor xc = call_rows(x, "loudness_stream");
  check_stream(counter, state, xc);
  const int64_t R = call_frames(xc, hop, "loudness_stream"), B = xc.size(0), N = xc.size(1);
  at::Tensor w = weights_table(weights, n_fft, "loudness_stream", "n_fft");
  at::Tensor out = at::empty({B, R}, xc.options());
  ok(ddsp_hip_stream_loudness(xc.data_ptr<float>(), ptr_or_null(w), out.data_ptr<float>(), counter_ptr(counter),
                              state.data_ptr(), (size_t)state.numel(), B, N, n_fft, hop, stream_of(xc)),
     "stream_loudness");
  return out;
}

at::Tensor mfcc_stream(const at::Tensor& x, const at::Tensor& band_start, const at::Tensor& band_count,
                       const at::Tensor& band_weights, const at::Tensor& dct, int64_t n_fft, int64_t hop, double top_db,
                       const at::Tensor& counter, at::Tensor& state) {
  at::Tensor xc = call_rows(x, "mfcc_stream");
  check_stream(counter, state, xc);
  check_dev(band_weights, "band_weights");
  check_dev(dct, "dct");
  const int64_t R = call_frames(xc, hop, "mfcc_stream"), B = xc.size(0), N = xc.size(1);
  const MelTables m = mel_tables(band_start, band_count, band_weights, dct, "mfcc_stream");
  at::Tensor out = at::empty({B, R, m.n_mfcc}, xc.options());
  ok(ddsp_hip_stream_mfcc(xc.data_ptr<float>(), m.bs.data_ptr<int32_t>(), m.bc.data_ptr<int32_t>(),
                          m.bw.data_ptr<float>(), m.bw.numel(), m.d.data_ptr<float>(), out.data_ptr<float>(),
                          counter_ptr(counter), state.data_ptr(), (size_t)state.numel(), B, N, n_fft, hop, m.n_mels,
                          m.n_mfcc, (float)top_db, stream_of(xc)),
     "stream_mfcc");
  return out;
}

// ---------------- pitch: YIN f0 (ddsp_hip_pitch / ddsp_hip_stream_pitch) -> (f0, confidence, period) ----------------
Tensor3 pitch(const at::Tensor& x, int64_t frame_length, int64_t hop, int64_t tau_min, int64_t tau_max,
              double sample_rate, double threshold) {
  at::Tensor xc = audio_rows(x, "pitch");
  TORCH_CHECK(hop >= 1, "pitch: hop must be positive");
  const int64_t B = xc.size(0), T = xc.size(1);
  const Tensor3 out = three_outputs(xc, {B, T / hop});
  const auto& [f0, conf, period] = out;
  ok(ddsp_hip_pitch(xc.data_ptr<float>(), f0.data_ptr<float>(), conf.data_ptr<float>(), period.data_ptr<int32_t>(), B,
                    T, frame_length, hop, tau_min, tau_max, (float)sample_rate, (float)threshold, stream_of(xc)),
     "pitch");
  if (x.dim() == 1) return {f0.select(0, 0), conf.select(0, 0), period.select(0, 0)};
  return out;
}

Tensor3 pitch_stream(const at::Tensor& x, int64_t frame_length, int64_t hop, int64_t tau_min, int64_t tau_max,
                     double sample_rate, double threshold, const at::Tensor& counter, at::Tensor& state) {
  at::Tensor xc = call_rows(x, "pitch_stream");
  check_stream(counter, state, xc);
  const int64_t R = call_frames(xc, hop, "pitch_stream"), B = xc.size(0), N = xc.size(1);
  const Tensor3 out = three_outputs(xc, {B, R});
  const auto& [f0, conf, period] = out;
  ok(ddsp_hip_stream_pitch(xc.data_ptr<float>(), f0.data_ptr<float>(), conf.data_ptr<float>(),
                           period.data_ptr<int32_t>(), counter_ptr(counter), state.data_ptr(), (size_t)state.numel(), B,
                           N, frame_length, hop, tau_min, tau_max, (float)sample_rate, (float)threshold, stream_of(xc)),
     "stream_pitch");
  return out;
}

// ---------------- pitch_viterbi: the salience over lag bins and the decode (ddsp_hip_pitch_salience / _viterbi) ------
// -> (cost, f0c, lag), each [B, F, n_bins] ([F, n_bins] for a 1-D signal)
Tensor3 pitch_salience(const at::Tensor& x, const at::Tensor& lo, const at::Tensor& hi, int64_t frame_length,
                       int64_t hop, int64_t tau_min, int64_t tau_max, double sample_rate) {
  at::Tensor xc = audio_rows(x, "pitch_salience");
  TORCH_CHECK(hop >= 1, "pitch_salience: hop must be positive");
  const auto [l, h] = bin_tables(lo, hi, "pitch_salience");
  const int64_t B = xc.size(0), T = xc.size(1), NB = l.numel();
  const Tensor3 out = three_outputs(xc, {B, T / hop, NB});
  const auto& [cost, f0c, lag] = out;
  ok(ddsp_hip_pitch_salience(xc.data_ptr<float>(), l.data_ptr<int32_t>(), h.data_ptr<int32_t>(),
                             cost.data_ptr<float>(), f0c.data_ptr<float>(), lag.data_ptr<int32_t>(), nullptr, nullptr,
                             nullptr, B, T, frame_length, hop, tau_min, tau_max, NB, (float)sample_rate, 0.0f,
                             stream_of(xc)),
     "pitch_salience");
  if (x.dim() == 1) return {cost.select(0, 0), f0c.select(0, 0), lag.select(0, 0)};
  return out;
}

// cost, f0c [B, F, n_bins] -> (f0, confidence, path), each [B, F]
Tensor3 pitch_viterbi(const at::Tensor& cost, const at::Tensor& f0c, double transition, int64_t max_jump) {
  check_dev(cost, "cost");
  check_dev(f0c, "f0c");
  TORCH_CHECK(cost.dim() == 3 && cost.sizes() == f0c.sizes() && cost.size(2) >= 1,
              "pitch_viterbi: cost and f0c must both be [batch, frames, bins]");
  at::Tensor c = cost.contiguous(), g = f0c.contiguous();
  const int64_t B = c.size(0), F = c.size(1), NB = c.size(2);
  const Tensor3 out = three_outputs(c, {B, F});
  const auto& [f0, conf, path] = out;
  at::Tensor ws = at::empty({B * F * NB}, c.options().dtype(at::kChar));
  ok(ddsp_hip_pitch_viterbi(c.data_ptr<float>(), g.data_ptr<float>(), f0.data_ptr<float>(), conf.data_ptr<float>(),
                            path.data_ptr<int32_t>(), ws.data_ptr(), (size_t)ws.numel(), B, F, NB, max_jump,
                            (float)transition, stream_of(c)),
     "pitch_viterbi");
  return out;
}

// ---------------- pitch_viterbi_stream: the same per call of a stream (ddsp_hip_stream_pitch_salience / _viterbi) ----
// -> (cost, f0c, lag), each [B, R, n_bins]
Tensor3 pitch_salience_stream(const at::Tensor& x, const at::Tensor& lo, const at::Tensor& hi, int64_t frame_length,
                              int64_t hop, int64_t tau_min, int64_t tau_max, double sample_rate,
                              const at::Tensor& counter, at::Tensor& state) {
  at::Tensor xc = call_rows(x, "pitch_salience_stream");
  check_stream(counter, state, xc);
  const int64_t R = call_frames(xc, hop, "pitch_salience_stream");
  const auto [l, h] = bin_tables(lo, hi, "pitch_salience_stream");
  const int64_t B = xc.size(0), N = xc.size(1), NB = l.numel();
  const Tensor3 out = three_outputs(xc, {B, R, NB});
  const auto& [cost, f0c, lag] = out;
  ok(ddsp_hip_stream_pitch_salience(xc.data_ptr<float>(), l.data_ptr<int32_t>(), h.data_ptr<int32_t>(),
                                    cost.data_ptr<float>(), f0c.data_ptr<float>(), lag.data_ptr<int32_t>(), nullptr,
                                    nullptr, nullptr, counter_ptr(counter), state.data_ptr(), (size_t)state.numel(), B,
                                    N, frame_length, hop, tau_min, tau_max, NB, (float)sample_rate, 0.0f,
                                    stream_of(xc)),
     "stream_pitch_salience");
  return out;
}

// cost, f0c [B, R, n_bins] of one call -> (f0, confidence, path), each [B, R], `lag` frames back
Tensor3 pitch_viterbi_stream(const at::Tensor& cost, const at::Tensor& f0c, double transition, int64_t max_jump,
                             int64_t lag, const at::Tensor& counter, at::Tensor& state) {
  check_dev(cost, "cost");
  check_dev(f0c, "f0c");
  check_stream(counter, state, cost);
  TORCH_CHECK(cost.dim() == 3 && cost.sizes() == f0c.sizes() && cost.size(2) >= 1,
              "pitch_viterbi_stream: cost and f0c must both be [batch, frames, bins]");
  at::Tensor c = cost.contiguous(), g = f0c.contiguous();
  const int64_t B = c.size(0), R = c.size(1), NB = c.size(2);
  const Tensor3 out = three_outputs(c, {B, R});
  const auto& [f0, conf, path] = out;
  ok(ddsp_hip_stream_pitch_viterbi(c.data_ptr<float>(), g.data_ptr<float>(), f0.data_ptr<float>(),
                                   conf.data_ptr<float>(), path.data_ptr<int32_t>(), counter_ptr(counter),
                                   state.data_ptr(), (size_t)state.numel(), B, R, NB, max_jump, lag, (float)transition,
                                   stream_of(c)),
     "stream_pitch_viterbi");
  return out;
}

// loudness_stream + pitch_stream in one launch over one state (ddsp_hip_stream_analysis)
// -> (loudness, f0, confidence, period)
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> analysis_stream(
    const at::Tensor& x, const std::optional<at::Tensor>& weights, int64_t frame_length, int64_t hop, int64_t tau_min,
    int64_t tau_max, double sample_rate, double threshold, const at::Tensor& counter, at::Tensor& state) {
  at::Tensor xc = call_rows(x, "analysis_stream");
  check_stream(counter, state, xc);
  const int64_t R = call_frames(xc, hop, "analysis_stream"), B = xc.size(0), N = xc.size(1);
  at::Tensor w = weights_table(weights, frame_length, "analysis_stream", "frame_length");
  at::Tensor loud = at::empty({B, R}, xc.options());
  const auto [f0, conf, period] = three_outputs(xc, {B, R});
  ok(ddsp_hip_stream_analysis(xc.data_ptr<float>(), ptr_or_null(w), loud.data_ptr<float>(), f0.data_ptr<float>(),
                              conf.data_ptr<float>(), period.data_ptr<int32_t>(), counter_ptr(counter),
                              state.data_ptr(), (size_t)state.numel(), B, N, frame_length, hop, tau_min, tau_max,
                              (float)sample_rate, (float)threshold, stream_of(xc)),
     "stream_analysis");
  return {loud, f0, conf, period};
}

// loudness_stream + mfcc_stream (+ pitch_stream) in one launch over one state, on one time axis
// (ddsp_hip_stream_analysis_mfcc) -> (loudness, mfcc, f0, confidence, period); pitch == false: the last three empty
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> analysis_mfcc_stream(
    const at::Tensor& x, const std::optional<at::Tensor>& weights, const at::Tensor& band_start,
    const at::Tensor& band_count, const at::Tensor& band_weights, const at::Tensor& dct, int64_t frame_length,
    int64_t mfcc_n_fft, int64_t hop, double top_db, bool pitch, int64_t tau_min, int64_t tau_max, double sample_rate,
    double threshold, const at::Tensor& counter, at::Tensor& state) {
  at::Tensor xc = call_rows(x, "analysis_mfcc_stream");
  check_stream(counter, state, xc);
  check_dev(band_weights, "band_weights");
  check_dev(dct, "dct");
  const int64_t R = call_frames(xc, hop, "analysis_mfcc_stream"), B = xc.size(0), N = xc.size(1);
  const MelTables m = mel_tables(band_start, band_count, band_weights, dct, "analysis_mfcc_stream");
  at::Tensor w = weights_table(weights, frame_length, "analysis_mfcc_stream", "frame_length");
  at::Tensor loud = at::empty({B, R}, xc.options());
  at::Tensor out = at::empty({B, R, m.n_mfcc}, xc.options());
  const auto [f0, conf, period] = three_outputs(xc, {B, pitch ? R : 0});
  ok(ddsp_hip_stream_analysis_mfcc(
         xc.data_ptr<float>(), ptr_or_null(w), loud.data_ptr<float>(), m.bs.data_ptr<int32_t>(),
         m.bc.data_ptr<int32_t>(), m.bw.data_ptr<float>(), m.bw.numel(), m.d.data_ptr<float>(), out.data_ptr<float>(),
         pitch ? f0.data_ptr<float>() : nullptr, pitch ? conf.data_ptr<float>() : nullptr,
         pitch ? period.data_ptr<int32_t>() : nullptr, counter_ptr(counter), state.data_ptr(), (size_t)state.numel(), B,
         N, frame_length, mfcc_n_fft, hop, m.n_mels, m.n_mfcc, (float)top_db, tau_min, tau_max, (float)sample_rate,
         (float)threshold, stream_of(xc)),
     "stream_analysis_mfcc");
  return {loud, out, f0, conf, period};
}

}  // namespace

// ---------------- decoder.py:33-68: the GRU recurrence ----------------
std::tuple<at::Tensor, at::Tensor> gru(const at::Tensor& x, const at::Tensor& w_ih, const at::Tensor& w_hh,
                                       const at::Tensor& b_ih, const at::Tensor& b_hh,
                                       const std::optional<at::Tensor>& h0) {
  check_dev(x, "x");
  TORCH_CHECK(x.dim() == 3, "gru: x must be [batch, time, features]");
  const int64_t B = x.size(0), T = x.size(1), H = w_hh.size(1);
  TORCH_CHECK(w_hh.size(0) == 3 * H && w_ih.size(0) == 3 * H && w_ih.size(1) == x.size(2), "gru: weight shapes");
  at::Tensor xp = at::addmm(b_ih, x.reshape({B * T, x.size(2)}), w_ih.t()).view({B, T, 3 * H});
  at::Tensor out = at::empty({B, T, H}, x.options());
  at::Tensor h_last = at::empty({1, B, H}, x.options());
  at::Tensor h0c;
  if (h0.has_value() && h0->defined()) {
    check_dev(*h0, "h0");
    TORCH_CHECK(h0->numel() == B * H, "gru: h0 must hold batch x hidden values");
    h0c = c16(h0->reshape({B, H}));
  }
  at::Tensor whh = c16(w_hh), bhh = c16(b_hh);
  ok(ddsp_hip_gru_forward(xp.data_ptr<float>(), whh.data_ptr<float>(), bhh.data_ptr<float>(),
                          h0c.defined() ? h0c.data_ptr<float>() : nullptr, out.data_ptr<float>(),
                          h_last.data_ptr<float>(), nullptr, B, T, H, stream_of(x)),
     "gru_forward");
  return {out, h_last};
}

TORCH_LIBRARY(ddsp_hip, m) {
  m.def("scale_function(Tensor x) -> Tensor");
  m.def("remove_above_nyquist(Tensor amplitudes, Tensor f0, float sample_rate) -> Tensor");
  m.def("upsample(Tensor signal, int factor) -> Tensor");
  m.def("harmonic_synth(Tensor f0, Tensor amplitudes, float sample_rate) -> Tensor");
  m.def("amp_to_impulse_response(Tensor amp, int target_size) -> Tensor");
  m.def("fft_convolve(Tensor signal, Tensor kernel) -> Tensor");
  m.def("harmonic_controls(Tensor amplitudes, Tensor harmonic_distribution, Tensor f0, float sample_rate)"
        " -> (Tensor, Tensor)");
  m.def("harmonic_synth_frames(Tensor f0, Tensor amplitudes, Tensor(a!) harmonic_distribution, int block_size,"
        " float sample_rate, bool write_back=True) -> Tensor");
  m.def("harmonic_synth_params(Tensor f0, Tensor param, int block_size, float sample_rate) -> Tensor");
  m.def("filtered_noise(Tensor magnitudes, int block_size, Tensor? noise=None, int seed=0, int offset=0,"
        " Tensor? add=None, float? raw_bias=None) -> Tensor");
  m.def("synth_frames(Tensor f0, Tensor param, Tensor mags, int block_size, float sample_rate, float bias=-5.0,"
        " Tensor? noise=None, int seed=0, int offset=0) -> Tensor");
  m.def("synth_frames_parts(Tensor f0, Tensor param, Tensor mags, int block_size, float sample_rate,"
        " float bias=-5.0, Tensor? noise=None, int seed=0, int offset=0) -> (Tensor, Tensor, Tensor)");
  m.def("reverb_build_impulse(Tensor noise, Tensor decay, Tensor wet, float sample_rate) -> Tensor");
  m.def("reverb_spectrum(Tensor impulse, int n_samples) -> Tensor");
  m.def("reverb_apply(Tensor x, Tensor spectrum, int ir_length) -> Tensor");
  m.def("synth_frames_stream(Tensor f0, Tensor param, Tensor mags, int block_size, float sample_rate, float bias,"
        " Tensor? noise, int seed, Tensor counter, Tensor(a!) state, bool wrap=True) -> Tensor");
  m.def("stream_spectrum(Tensor impulse, int call_samples) -> Tensor");
  m.def("reverb_stream(Tensor x, Tensor spectrum, int ir_length, Tensor counter, Tensor(a!) state) -> Tensor");
  m.def("stream_advance(Tensor f0, int block_size, float sample_rate, Tensor(a!) counter, Tensor(b!) state,"
        " bool wrap=True) -> ()");
  m.def("gru(Tensor x, Tensor w_ih, Tensor w_hh, Tensor b_ih, Tensor b_hh, Tensor? h0=None) -> (Tensor, Tensor)");
  m.def("loudness(Tensor x, Tensor? weights, int n_fft, int hop) -> Tensor");
  m.def("mfcc(Tensor x, Tensor band_start, Tensor band_count, Tensor band_weights, Tensor dct, int n_fft, int hop,"
        " float top_db) -> Tensor");
  m.def("loudness_stream(Tensor x, Tensor? weights, int n_fft, int hop, Tensor counter, Tensor(a!) state) -> Tensor");
  m.def("mfcc_stream(Tensor x, Tensor band_start, Tensor band_count, Tensor band_weights, Tensor dct, int n_fft,"
        " int hop, float top_db, Tensor counter, Tensor(a!) state) -> Tensor");
  m.def("pitch(Tensor x, int frame_length, int hop, int tau_min, int tau_max, float sample_rate, float threshold)"
        " -> (Tensor, Tensor, Tensor)");
  m.def("pitch_stream(Tensor x, int frame_length, int hop, int tau_min, int tau_max, float sample_rate,"
        " float threshold, Tensor counter, Tensor(a!) state) -> (Tensor, Tensor, Tensor)");
  m.def("pitch_salience(Tensor x, Tensor lo, Tensor hi, int frame_length, int hop, int tau_min, int tau_max,"
        " float sample_rate) -> (Tensor, Tensor, Tensor)");
  m.def("pitch_viterbi(Tensor cost, Tensor f0c, float transition, int max_jump) -> (Tensor, Tensor, Tensor)");
  m.def("pitch_salience_stream(Tensor x, Tensor lo, Tensor hi, int frame_length, int hop, int tau_min, int tau_max,"
        " float sample_rate, Tensor counter, Tensor(a!) state) -> (Tensor, Tensor, Tensor)");
  m.def("pitch_viterbi_stream(Tensor cost, Tensor f0c, float transition, int max_jump, int lag, Tensor counter,"
        " Tensor(a!) state) -> (Tensor, Tensor, Tensor)");
  m.def("analysis_stream(Tensor x, Tensor? weights, int frame_length, int hop, int tau_min, int tau_max,"
        " float sample_rate, float threshold, Tensor counter, Tensor(a!) state) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("analysis_mfcc_stream(Tensor x, Tensor? weights, Tensor band_start, Tensor band_count, Tensor band_weights,"
        " Tensor dct, int frame_length, int mfcc_n_fft, int hop, float top_db, bool pitch, int tau_min, int tau_max,"
        " float sample_rate, float threshold, Tensor counter, Tensor(a!) state)"
        " -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(ddsp_hip, CUDA, m) {  // HIP tensors dispatch under the CUDA key on ROCm
  m.impl("scale_function", &scale_function);
  m.impl("remove_above_nyquist", &remove_above_nyquist);
  m.impl("upsample", &upsample);
  m.impl("harmonic_synth", &harmonic_synth);
  m.impl("amp_to_impulse_response", &amp_to_impulse_response);
  m.impl("fft_convolve", &fft_convolve);
  m.impl("harmonic_controls", &harmonic_controls);
  m.impl("harmonic_synth_frames", &harmonic_synth_frames);
  m.impl("harmonic_synth_params", &harmonic_synth_params);
  m.impl("filtered_noise", &filtered_noise);
  m.impl("synth_frames", &synth_frames);
  m.impl("synth_frames_parts", &synth_frames_parts);
  m.impl("reverb_build_impulse", &reverb_build_impulse);
  m.impl("reverb_spectrum", &reverb_spectrum);
  m.impl("reverb_apply", &reverb_apply);
  m.impl("synth_frames_stream", &synth_frames_stream);
  m.impl("stream_spectrum", &stream_spectrum);
  m.impl("reverb_stream", &reverb_stream);
  m.impl("stream_advance", &stream_advance);
  m.impl("gru", &gru);
  m.impl("loudness", &loudness);
  m.impl("mfcc", &mfcc);
  m.impl("loudness_stream", &loudness_stream);
  m.impl("mfcc_stream", &mfcc_stream);
  m.impl("pitch", &pitch);
  m.impl("pitch_stream", &pitch_stream);
  m.impl("pitch_salience", &pitch_salience);
  m.impl("pitch_viterbi", &pitch_viterbi);
  m.impl("pitch_salience_stream", &pitch_salience_stream);
  m.impl("pitch_viterbi_stream", &pitch_viterbi_stream);
  m.impl("analysis_stream", &analysis_stream);
  m.impl("analysis_mfcc_stream", &analysis_mfcc_stream);
}
