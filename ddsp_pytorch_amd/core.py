"""Function-level drop-ins for ``ddsp/core.py`` — same names, arguments and return shapes.

``ddsp/models/modules.py`` looks these up late-bound through the ``ddsp`` package
(``modules.py:33,53-56,74-78,113,117,125``), so rebinding the package attributes to the
functions below (``ddsp_pytorch_amd.install``) moves the reference's own
``DDSPDecoder.forward`` onto the gfx950 kernels without editing it.

Every function here runs on the HIP device through the C-ABI (include/ddsp_hip.h) and
raises — never falls back to CPU — on tensors it cannot take (CPU tensors, non-fp32).
Shape errors raise ``RuntimeError`` as the reference's torch ops would.

Besides the six reference functions, the fused frame-rate ops used by the module-level
drop-ins (``modules.py``) live here: ``harmonic_controls``, ``harmonic_synth_frames``,
``filtered_noise``, ``reverb_build_impulse``, ``reverb_spectrum``, ``reverb_apply``.
"""
import atexit
import ctypes
import itertools
import math

import numpy as np
import torch

from . import _lib

__all__ = [
    "scale_function", "remove_above_nyquist", "upsample", "harmonic_synth",
    "amp_to_impulse_response", "fft_convolve", "phase", "harmonic_controls",
    "harmonic_synth_frames", "harmonic_synth_params", "synth_frames", "synth_signal", "filtered_noise", "reverb_build_impulse", "reverb_spectrum_floats",
    "reverb_spectrum", "reverb_impulse_spectrum", "reverb_apply", "reverb_forward", "reverb_cache_bytes", "set_noise_seed", "safe_log", "stft_magnitude", "multiscale_fft",
    "extract_loudness", "mfcc", "FeatureStreamState", "stream_loudness", "stream_mfcc", "stream_feature_delay",
    "extract_pitch", "stream_pitch", "pitch_lags", "stream_analysis", "stream_analysis_mfcc",
    "pitch_bins", "pitch_salience", "viterbi_path", "track_pitch",
    "ViterbiStreamState", "stream_pitch_salience", "stream_viterbi_path", "stream_track_pitch",
    "stream_pitch_bin_count",
]


def _dev(*tensors):
    for t in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"ddsp_hip: expected a torch.Tensor, got {type(t).__name__}")
        if t.device.type != "cuda":
            raise RuntimeError("ddsp_hip: tensors must be on a HIP device (no CPU fallback); "
                               f"got a tensor on {t.device}")
        if t.dtype != torch.float32:
            raise TypeError(f"ddsp_hip: kernels compute in float32; got {t.dtype}")
    dev = tensors[0].device
    for t in tensors[1:]:
        if t.device != dev:
            raise RuntimeError(f"ddsp_hip: tensors on different devices {dev} and {t.device}")
    return dev


def _wants_grad(*tensors):
    """autograd must record this call: dispatch to the Function in grad.py (backward kernels)."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _c(t):
    """contiguous and 16-byte aligned (the kernels use float4 accesses)."""
    t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t


def _workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------------------------
# ddsp/core.py functions
# ------------------------------------------------------------------------------------
def scale_function(x):
    """ddsp/core.py:77-78  ``2 * sigmoid(x) ** ln(10) + 1e-7``."""
    return scale_with_bias(x, 0.0)


def scale_with_bias(x, bias):
    """``scale_function(x + bias)`` in one kernel (FilteredNoise.get_controls, modules.py:111-114)."""
    _dev(x)
    if _wants_grad(x):
        return _grad.ScaleFn.apply(x, float(bias))
    x = _c(x)
    y = torch.empty_like(x)
    _lib.call("scale_function", _lib.ptr(x), _lib.ptr(y), x.numel(), float(bias), _lib.stream_of(x))
    return y


def remove_above_nyquist(amplitudes, f0, sample_rate):
    """ddsp/core.py:70-74  amplitudes[..., H] * ((f0 * k < sr/2) + 1e-4), k = 1..H."""
    _dev(amplitudes, f0)
    if _wants_grad(amplitudes, f0):
        return _grad.NyquistFn.apply(amplitudes, f0, sample_rate)
    H = amplitudes.shape[-1]
    lead = amplitudes.shape[:-1]
    if f0.shape[-1] != 1:
        raise RuntimeError(f"remove_above_nyquist: f0 must end in a size-1 dim, got {tuple(f0.shape)}")
    out_lead = torch.broadcast_shapes(lead, f0.shape[:-1])
    amplitudes = _c(amplitudes.expand(*out_lead, H))
    f0 = _c(f0.expand(*out_lead, 1))
    out = torch.empty_like(amplitudes)
    rows = amplitudes.numel() // max(H, 1)
    _lib.call("remove_above_nyquist", _lib.ptr(amplitudes), _lib.ptr(f0), _lib.ptr(out), rows, H,
              float(sample_rate), _lib.stream_of(out))
    return out


def upsample(signal, factor):
    """ddsp/core.py:64-67  nearest upsampling [B, F, C] -> [B, F*factor, C]."""
    _dev(signal)
    if _wants_grad(signal):
        return _grad.UpsampleFn.apply(signal, int(factor))
    if signal.dim() != 3:
        raise RuntimeError(f"upsample: expected [batch, frames, channels], got {tuple(signal.shape)}")
    factor = int(factor)
    B, F, C = signal.shape
    x = _c(signal)
    y = torch.empty(B, F * factor, C, dtype=x.dtype, device=x.device)
    _lib.call("upsample", _lib.ptr(x), _lib.ptr(y), B, F, C, factor, _lib.stream_of(x))
    return y


def harmonic_synth(f0, amplitudes, sample_rate):
    """ddsp/core.py:136-141  f0[B, T, 1], amplitudes[B, T, H] -> [B, T, 1]."""
    _dev(f0, amplitudes)
    if _wants_grad(f0, amplitudes):
        # per-sample f0: its gradient is a reverse scan over T, not built (the frame-rate ops below have one)
        _grad.refuse_f0_grad(f0, "harmonic_synth")
        return _grad.HarmonicSynthFn.apply(f0, amplitudes, sample_rate)
    if amplitudes.dim() != 3 or f0.dim() != 3 or f0.shape[-1] != 1:
        raise RuntimeError("harmonic_synth: expected f0 [B,T,1] and amplitudes [B,T,H], got "
                           f"{tuple(f0.shape)} and {tuple(amplitudes.shape)}")
    B, T, H = amplitudes.shape
    if f0.shape[:2] != (B, T):
        raise RuntimeError(f"harmonic_synth: shape mismatch {tuple(f0.shape)} vs {tuple(amplitudes.shape)}")
    f0 = _c(f0)
    amplitudes = _c(amplitudes)
    out = torch.empty(B, T, 1, dtype=torch.float32, device=f0.device)
    nbytes = _lib.query("harmonic_synth_workspace_size", B, T)
    ws = _workspace(nbytes, f0.device)
    _lib.call("harmonic_synth", _lib.ptr(f0), _lib.ptr(amplitudes), _lib.ptr(out), B, T, H,
              float(sample_rate), _lib.ptr(ws), ws.numel(), _lib.stream_of(out))
    return out


def phase(f0, sample_rate):
    """The fp32 phase ``cumsum(2*pi*f0/sr, 1)`` of ddsp/core.py:138 (exposed for exactness tests)."""
    _dev(f0)
    B, T = f0.shape[0], f0.shape[1]
    f0 = _c(f0)
    out = torch.empty(B, T, 1, dtype=torch.float32, device=f0.device)
    ws = _workspace(_lib.query("harmonic_synth_workspace_size", B, T), f0.device)
    _lib.call("phase", _lib.ptr(f0), _lib.ptr(out), B, T, float(sample_rate), _lib.ptr(ws),
              ws.numel(), _lib.stream_of(out))
    return out


def amp_to_impulse_response(amp, target_size):
    """ddsp/core.py:144-166  zero-phase FIR of length target_size from NB magnitudes."""
    _dev(amp)
    if _wants_grad(amp):
        return _grad.ImpulseResponseFn.apply(amp, int(target_size))
    NB = amp.shape[-1]
    if NB < 2:
        raise RuntimeError("amp_to_impulse_response: need at least 2 frequency bands")
    target = int(target_size)
    x = _c(amp)
    rows = x.numel() // NB
    out = torch.empty(*amp.shape[:-1], target, dtype=torch.float32, device=x.device)
    _lib.call("amp_to_impulse_response", _lib.ptr(x), _lib.ptr(out), rows, NB, target,
              _lib.stream_of(x))
    return out


def fft_convolve(signal, kernel):
    """ddsp/core.py:169-176  causal linear convolution truncated to N (last dim), with broadcasting."""
    _dev(signal, kernel)
    if _wants_grad(signal, kernel):
        return _grad.FFTConvolveFn.apply(signal, kernel)
    N = signal.shape[-1]
    if kernel.shape[-1] != N:
        raise RuntimeError(f"fft_convolve: signal and kernel lengths differ ({N} vs {kernel.shape[-1]})")
    lead = torch.broadcast_shapes(signal.shape[:-1], kernel.shape[:-1])
    rows = math.prod(lead) if len(lead) else 1
    s = _c(signal.expand(*lead, N))
    if kernel.numel() == N:
        k, krows = _c(kernel.reshape(N)), 1
    else:
        k, krows = _c(kernel.expand(*lead, N)), rows
    out = torch.empty(*lead, N, dtype=torch.float32, device=s.device)
    ws = _workspace(_lib.query("fft_convolve_workspace_size", rows, krows, N), s.device)
    _lib.call("fft_convolve", _lib.ptr(s), _lib.ptr(k), _lib.ptr(out), rows, krows, N,
              _lib.ptr(ws), ws.numel(), _lib.stream_of(out))
    return out


# ------------------------------------------------------------------------------------
# fused module-level ops (ddsp/models/modules.py)
# ------------------------------------------------------------------------------------
def _frame_rows(t):
    """(tensor, row stride) for a [B, F, C] tensor read row by row: unit stride on C and one row stride
    over (B, F) — a column slice of a wider projection output qualifies as it is — else a contiguous copy
    (broadcast rows, stride 0, and overlapping rows included).  The kernels read these rows with scalar
    loads only (no 16-byte vector loads), so a view's row base needs no more than 4-byte alignment."""
    if (t.dim() == 3 and t.stride(-1) == 1 and t.stride(1) >= max(t.shape[-1], 1)
            and t.stride(0) == t.shape[1] * t.stride(1)):
        return t, t.stride(1)
    t = t.contiguous()
    return t, t.shape[-1]


def harmonic_controls(amplitudes, harmonic_distribution, f0, sample_rate):
    """modules.py:44-67 HarmonicSynth.get_controls, fused: returns (amplitudes, distribution)."""
    _dev(amplitudes, harmonic_distribution, f0)
    if _wants_grad(amplitudes, harmonic_distribution, f0):
        return _grad.ControlsFn.apply(amplitudes, harmonic_distribution, f0, sample_rate)
    B, F, H = harmonic_distribution.shape
    if amplitudes.shape != (B, F, 1) or f0.shape != (B, F, 1):
        raise RuntimeError("harmonic_controls: expected amplitudes/f0 [B,F,1] matching "
                           f"distribution {tuple(harmonic_distribution.shape)}")
    (a, a_ld), (d, d_ld) = _frame_rows(amplitudes), _frame_rows(harmonic_distribution)
    f0c = _c(f0)
    amp_out = torch.empty(B, F, 1, dtype=torch.float32, device=f0.device)
    dist_out = torch.empty(B, F, H, dtype=torch.float32, device=f0.device)
    _lib.call("harmonic_controls", _lib.ptr(a), a_ld, _lib.ptr(d), d_ld, _lib.ptr(f0c),
              _lib.ptr(amp_out), _lib.ptr(dist_out), B * F, H, float(sample_rate),
              _lib.stream_of(f0c))
    return amp_out, dist_out


def harmonic_synth_frames(f0, amplitudes, harmonic_distribution, block_size, sample_rate,
                          write_back=True):
    """modules.py:69-80 HarmonicSynth.forward, fused at frame rate.

    f0, amplitudes: [B, F, 1]; harmonic_distribution: [B, F, H] (scaled and normalised).
    Returns audio [B, F*block_size, 1].  With ``write_back`` the distribution is multiplied
    by the amplitudes in place, exactly like ``harmonic_distribution *= amplitudes``
    (modules.py:73), which the reference's caller sees through its controls dict.
    Differentiable in the controls and in f0 (grad.SynthFramesHarmonicFn; the pitch gradient, what the
    reference's autograd sends through cumsum and sin, from csrc/pitch_grad.hip).
    """
    _dev(f0, amplitudes, harmonic_distribution)
    if _wants_grad(f0, amplitudes, harmonic_distribution):
        out = _grad.SynthFramesHarmonicFn.apply(f0, amplitudes, harmonic_distribution, block_size, sample_rate)
        if write_back:  # modules.py:73, recorded by autograd like the reference's in-place multiply
            harmonic_distribution.mul_(amplitudes)
        return out
    B, F, H = harmonic_distribution.shape
    f0c, ac = _c(f0), _c(amplitudes)
    dist = harmonic_distribution
    if write_back and not (dist.is_contiguous() and dist.data_ptr() % 16 == 0):
        raise RuntimeError("harmonic_synth_frames: in-place write-back needs a contiguous distribution")
    if not write_back:
        dist = _c(dist)
    bs = int(block_size)
    out = torch.empty(B, F * bs, 1, dtype=torch.float32, device=f0.device)
    _lib.call("harmonic_synth_frames", _lib.ptr(f0c), _lib.ptr(ac), _lib.ptr(dist), int(bool(write_back)),
              _lib.ptr(out), B, F, H, bs, float(sample_rate), _lib.stream_of(out))
    return out


class _NoiseCounter:
    """Philox (seed, offset) for on-device noise: each call consumes a fresh offset."""

    def __init__(self):
        self.seed = 0x5EED_DD5B
        self._offsets = itertools.count()

    def next(self):
        return self.seed, next(self._offsets)


_noise_counter = _NoiseCounter()


def set_noise_seed(seed):
    """Seed the on-device noise generator (throughput mode)."""
    _noise_counter.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    _noise_counter._offsets = itertools.count()


def harmonic_synth_params(f0, param, block_size, sample_rate):
    """decoder.py:106-113 + modules.py:44-80 in one kernel: raw harmonic projection
    param[B, F, H+1] (column 0 amplitude, 1..H distribution) and f0 [B, F, 1] -> audio
    [B, F*block_size, 1].  The controls (scale, Nyquist mask, normalisation) never reach HBM.
    Differentiable in param and in f0 (grad.HarmonicParamsFn; the pitch gradient from csrc/pitch_grad.hip)."""
    _dev(f0, param)
    if _wants_grad(f0, param):
        return _grad.HarmonicParamsFn.apply(f0, param, block_size, sample_rate)
    B, F, H1 = param.shape
    if f0.shape != (B, F, 1) or H1 < 2:
        raise RuntimeError(f"harmonic_synth_params: f0 {tuple(f0.shape)} / param {tuple(param.shape)}")
    f0c, pc = _c(f0), _c(param)
    bs = int(block_size)
    out = torch.empty(B, F * bs, 1, dtype=torch.float32, device=f0.device)
    _lib.call("harmonic_synth_params", _lib.ptr(f0c), _lib.ptr(pc), _lib.ptr(out), B, F, H1 - 1, bs,
              float(sample_rate), _lib.stream_of(out))
    return out


def filtered_noise(magnitudes, block_size, noise=None, add=None, return_noise=False, raw_bias=None):
    """modules.py:116-128 FilteredNoise.forward, fused.

    magnitudes: [B, F, NB] (already scaled by get_controls; with ``raw_bias`` the raw
    projection, scaled in the kernel as scale_function(x + raw_bias)).  ``noise``
    [B, F, block_size] injects the U[-1,1) samples (parity mode, e.g. the reference's
    ``torch.rand`` stream); ``None`` draws them on the device with Philox4x32-10.  ``add``
    [B, F*bs, 1] is added to the result (fuses ``harmonic + noise``); with ``return_noise`` the
    filtered noise alone is returned as a second tensor.
    """
    _dev(magnitudes)
    if _wants_grad(magnitudes, add):
        outs = _grad.FilteredNoiseFn.apply(magnitudes, add, int(block_size), noise, raw_bias,
                                           bool(return_noise))
        if return_noise and not isinstance(outs, tuple):
            return outs, outs
        return outs
    seed, offset = _noise_counter.next() if noise is None else (0, 0)
    out = _filtered_noise_launch(magnitudes, block_size, noise, add, return_noise, raw_bias, seed, offset)
    if return_noise and not isinstance(out, tuple):
        return out, out
    return out


def _filtered_noise_launch(magnitudes, block_size, noise, add, return_noise, raw_bias, seed, offset):
    B, F, NB = magnitudes.shape
    bs = int(block_size)
    m = _c(magnitudes)
    if noise is not None:
        _dev(noise)
        if tuple(noise.shape) != (B, F, bs):
            raise RuntimeError(f"filtered_noise: noise must be [B, F, block_size] = {(B, F, bs)}")
        noise = _c(noise)
    if add is not None:
        _dev(add)
        add = _c(add)
        if add.numel() != B * F * bs:
            raise RuntimeError("filtered_noise: `add` must have B*F*block_size elements")
    out = torch.empty(B, F * bs, 1, dtype=torch.float32, device=m.device)
    nout = torch.empty_like(out) if (return_noise and add is not None) else None
    if raw_bias is None:
        _lib.call("filtered_noise", _lib.ptr(m), _lib.ptr(noise), seed, offset, _lib.ptr(add),
                  _lib.ptr(out), _lib.ptr(nout), B, F, NB, bs, _lib.stream_of(m))
    else:
        _lib.call("filtered_noise_params", _lib.ptr(m), float(raw_bias), _lib.ptr(noise), seed, offset,
                  _lib.ptr(add), _lib.ptr(out), _lib.ptr(nout), B, F, NB, bs, _lib.stream_of(m))
    return (out, nout) if nout is not None else out


EWORKSPACE = 4  # DDSP_HIP_EWORKSPACE
# the fused synthesis kernel's frames sum their phase prefix themselves up to this many frames per item
# (O(F) per frame); past it one ddsp_hip_frame_phase_prefix launch precomputes every frame's prefix
FRAME_PREFIX_MIN_FRAMES = 512
ERANGE = _lib.ERANGE


def synth_frames_in_envelope(n_harmonic, n_bands, block_size, batch=1):
    """The fused kernel's shape envelope, as the library decides it (ddsp_hip_synth_frames_supported)."""
    return bool(_lib.query("synth_frames_supported", int(batch), int(n_harmonic), int(n_bands), int(block_size)))


def _frame_args(f0, param, mags, noise, block_size, name):
    """The frame arguments every fused-synthesis entry takes, checked: f0 [B,F,1], param [B,F,H+1], mags
    [B,F,NB] and, where given, noise [B,F,bs] -> (B, F, H, NB, bs, noise contiguous or None)."""
    _dev(f0, param, mags)
    B, F, H1 = param.shape
    NB = mags.shape[-1]
    bs = int(block_size)
    if f0.shape != (B, F, 1) or mags.shape[:2] != (B, F) or H1 < 2:
        raise RuntimeError(f"{name}: f0 [B,F,1], param [B,F,H+1], mags [B,F,NB] expected")
    if noise is not None:
        _dev(noise)
        if tuple(noise.shape) != (B, F, bs):
            raise RuntimeError(f"{name}: noise must be [B, F, block_size] = {(B, F, bs)}")
        noise = _c(noise)
    return B, F, H1 - 1, NB, bs, noise


def synth_frames(f0, param, mags, block_size, sample_rate, bias=-5.0, noise=None, parts=False, controls=False):
    """decoder.py:106-121 in one kernel: raw harmonic projection param[B,F,H+1], pitch f0[B,F,1]
    and raw noise projection mags[B,F,NB] -> signal = harmonic + noise [B,F*bs,1].

    ``noise`` [B,F,bs] injects the U[-1,1) samples (else on-device Philox).  With ``parts`` the
    harmonic and noise signals are returned too: (signal, harmonic, noise).  With ``controls``
    the controls ``DDSPDecoder.forward`` returns (decoder.py:127-135) are appended as a dict
    ``{"amplitudes" [B,F,1], "harmonic_distribution" [B,F,H], "magnitudes" [B,F,NB]}`` — the
    distribution as the reference's caller sees it after ``modules.py:73``'s in-place
    ``*= amplitudes``; written by the same launch (or, under autograd, by the differentiable
    control ops).  Returns None when the shape is outside the fused kernel's envelope
    (``synth_frames_in_envelope``); ``synth_signal`` runs the two module kernels there."""
    B, F, H, NB, bs, noise = _frame_args(f0, param, mags, noise, block_size, "synth_frames")
    if not synth_frames_in_envelope(H, NB, bs, B):
        return None
    if _wants_grad(f0, param, mags):
        outs = _grad.SynthFramesFn.apply(f0, param, mags, bs, float(sample_rate), float(bias), noise,
                                         bool(parts))
        if not controls:
            return outs
        amps, dist = harmonic_controls(param[..., :1], param[..., 1:], f0, sample_rate)
        ctrl = {"amplitudes": amps, "harmonic_distribution": dist * amps,
                "magnitudes": scale_with_bias(mags, bias)}
        return (*outs, ctrl) if parts else (outs, ctrl)
    seed, offset = _noise_counter.next() if noise is None else (0, 0)
    return _synth_frames_launch(f0, param, mags, bs, sample_rate, bias, noise, parts, seed, offset, controls)


def synth_signal(f0, param, mags, block_size, sample_rate, bias=-5.0, noise=None):
    """The signal of ``synth_frames`` for any shape: on the fused kernel, or outside its envelope on the two
    module kernels (the harmonic signal, then the filtered noise adding it)."""
    signal = synth_frames(f0, param, mags, block_size, sample_rate, bias=bias, noise=noise)
    if signal is None:
        harmonic = harmonic_synth_params(f0, param, block_size, sample_rate)
        signal = filtered_noise(mags, block_size, noise=noise, add=harmonic, raw_bias=bias)
    return signal


def _synth_frames_launch(f0, param, mags, block_size, sample_rate, bias, noise, parts, seed, offset,
                         controls=False):
    B, F, H, NB, bs, noise = _frame_args(f0, param, mags, noise, block_size, "synth_frames")
    f0c = _c(f0)
    (pc, ldp), (mc, ldm) = _frame_rows(param), _frame_rows(mags)
    out = torch.empty(B, F * bs, 1, dtype=torch.float32, device=f0.device)
    harm = torch.empty_like(out) if parts else None
    nz = torch.empty_like(out) if parts else None
    ctrl = torch.empty(B * F * (1 + H + NB), dtype=torch.float32, device=f0.device) if controls else None
    prefix = None
    if F > FRAME_PREFIX_MIN_FRAMES:  # long renders: each frame reads its phase prefix instead of summing
        prefix = torch.empty(B * F, dtype=torch.float64, device=f0.device)
        _lib.call("frame_phase_prefix", _lib.ptr(f0c), B, F, bs, float(sample_rate), _lib.ptr(prefix),
                  _lib.stream_of(out))
    _lib.call("synth_frames_controls_prefix", _lib.ptr(f0c), _lib.ptr(pc), ldp, _lib.ptr(mc), ldm, float(bias),
              _lib.ptr(noise), seed, offset, _lib.ptr(out), _lib.ptr(harm), _lib.ptr(nz), _lib.ptr(ctrl),
              _lib.ptr(prefix), B, F, H, NB, bs, float(sample_rate), _lib.stream_of(out))
    res = (out, harm, nz) if parts else out
    if not controls:
        return res
    BF = B * F
    cd = {"amplitudes": ctrl[:BF].view(B, F, 1), "harmonic_distribution": ctrl[BF:BF * (1 + H)].view(B, F, H),
          "magnitudes": ctrl[BF * (1 + H):].view(B, F, NB)}
    return (*res, cd) if parts else (res, cd)


def synth_frames_counter(f0, param, mags, block_size, sample_rate, counter, seed, bias=-5.0):
    """synth_frames with on-device noise whose Philox offset is the device word counter[0]
    (int64, advanced by one on the stream after the launch): for calls replayed from a captured
    HIP graph, where by-value offsets would freeze.  Call k equals
    synth_frames(..., noise=None) drawn with (seed, offset=k).  Inference only."""
    B, F, H, NB, bs, _ = _frame_args(f0, param, mags, None, block_size, "synth_frames_counter")
    if counter.dtype != torch.int64 or counter.numel() < 1 or counter.device != f0.device:
        raise RuntimeError("synth_frames_counter: counter must be a device int64 tensor")
    if not synth_frames_in_envelope(H, NB, bs, B):
        raise RuntimeError("synth_frames_counter: shape outside the fused kernel's envelope")
    out = torch.empty(B, F * bs, 1, dtype=torch.float32, device=f0.device)
    _lib.call("synth_frames_counter", _lib.ptr(_c(f0)), _lib.ptr(_c(param)), _lib.ptr(_c(mags)), float(bias),
              int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(counter), _lib.ptr(out), B, F, H, NB, bs,
              float(sample_rate), _lib.stream_of(out))
    return out


def reverb_build_impulse(noise, decay, wet, sample_rate):
    """modules.py:21-26 Reverb.build_impulse: noise[L,1] -> impulse [1, L, 1]."""
    _dev(noise, decay, wet)
    if _wants_grad(noise, decay, wet):
        return _grad.BuildImpulseFn.apply(noise, decay, wet, sample_rate)
    L = noise.shape[0]
    n = _c(noise)
    imp = torch.empty(1, L, 1, dtype=torch.float32, device=n.device)
    _lib.call("reverb_build_impulse", _lib.ptr(n), _lib.ptr(_c(decay)), _lib.ptr(_c(wet)),
              _lib.ptr(imp), L, float(sample_rate), _lib.stream_of(n))
    return imp


def reverb_spectrum_floats(n_samples, ir_length):
    return int(_lib.query("reverb_spectrum_floats", int(n_samples), int(ir_length)))


def reverb_spectrum(impulse, n_samples):
    """Partitioned-convolution spectra of the IR cropped/padded to n_samples (for reverb_apply)."""
    _dev(impulse)
    h = _c(impulse.reshape(-1))
    L = h.numel()
    spec = torch.empty(reverb_spectrum_floats(n_samples, L), dtype=torch.float32, device=h.device)
    _lib.call("reverb_spectrum", _lib.ptr(h), L, int(n_samples), _lib.ptr(spec), _lib.stream_of(h))
    return spec


def reverb_impulse_spectrum(noise, decay, wet, sample_rate, n_samples):
    """modules.py:21-35: Reverb.build_impulse and its partition spectra for n_samples in one launch
    (equal to reverb_spectrum(reverb_build_impulse(...), n_samples) bit for bit).  No autograd: the
    module's backward differentiates through noise/decay/wet itself."""
    _dev(noise, decay, wet)
    L = noise.shape[0]
    n = _c(noise)
    spec = torch.empty(reverb_spectrum_floats(n_samples, L), dtype=torch.float32, device=n.device)
    _lib.call("reverb_impulse_spectrum", _lib.ptr(n), _lib.ptr(_c(decay)), _lib.ptr(_c(wet)), L,
              float(sample_rate), int(n_samples), _lib.ptr(spec), _lib.stream_of(n))
    return spec


def reverb_cache_bytes(n_samples, ir_length):
    return int(_lib.query("reverb_cache_bytes", int(n_samples), int(ir_length)))


def reverb_forward(x, noise, decay, wet, ir_length, sample_rate, cache, force=False, n_samples=None):
    """modules.py:21-35 Reverb.forward over a device IR cache that the launch validates against the
    parameters (ddsp_hip_reverb_forward) -> (out [B, T, 1], workspace, spectrum view of the cache).  With
    x None only the cache is validated (for inputs of n_samples).  No autograd (grad.ReverbFn wraps it)."""
    _dev(noise, decay, wet)
    if x is not None:
        _dev(x)
        B, T = x.shape[0], x.shape[1]
        xc = _c(x)
    else:
        B, T, xc = 0, int(n_samples), None
    L = int(ir_length)
    if cache.device != noise.device or cache.numel() < reverb_cache_bytes(T, L):
        raise RuntimeError("reverb_forward: cache on another device or too small")
    out = torch.empty(B, T, 1, dtype=torch.float32, device=noise.device) if B else None
    ws = _workspace(_lib.query("reverb_workspace_size", B, T, L), noise.device) if B else None
    _lib.call("reverb_forward", _lib.ptr(xc), _lib.ptr(_c(noise)), _lib.ptr(_c(decay)), _lib.ptr(_c(wet)), L,
              float(sample_rate), int(bool(force)), _lib.ptr(cache), cache.numel(), _lib.ptr(out), B, T,
              _lib.ptr(ws), ws.numel() if ws is not None else 0, _lib.stream_of(cache))
    spec = cache[:4 * reverb_spectrum_floats(T, L)].view(torch.float32)
    return out, ws, spec


def reverb_apply(x, spectrum, ir_length):
    """modules.py:28-35 Reverb.forward given the cached IR spectrum: x [B, T, 1] -> [B, T, 1]."""
    _dev(x, spectrum)
    if _wants_grad(x, spectrum):
        if spectrum.requires_grad:
            raise NotImplementedError("reverb_apply: the IR spectrum is not differentiable; use "
                                      "modules.Reverb (gradients for noise/decay/wet) instead")
        return _grad.ReverbApplyFn.apply(x, spectrum, int(ir_length))
    return _reverb_apply_launch(x, spectrum, ir_length)[0]


# ------------------------------------------------------------------------------------
# the decoder network's recurrence (decoder.py:33-68)
# ------------------------------------------------------------------------------------
def gru_supported(gru_module):
    """Shapes the step kernel takes: one layer, batch_first, unidirectional, biased, hidden % 64 == 0."""
    g = gru_module
    return (g.num_layers == 1 and g.batch_first and not g.bidirectional and g.bias and
            g.hidden_size % 64 == 0 and g.hidden_size <= 4096)


def gru(x, gru_module, h0=None, persistent_flags=0):
    """torch.nn.GRU(x, h0) forward (1 layer, batch_first) -> (out [B,T,H], h_T [1,B,H]): the input
    projection for all steps as one GEMM, the recurrence on the gfx950 kernels (gru_layer_launch); under
    autograd the backward (BPTT) runs on the step kernels too (grad.GRUFn).  ``persistent_flags``:
    the persistent launch's test hooks (GRU_SPREAD, GRU_NO_MASK_CHECK, GRU_FORCE_ABORT; 0 in use)."""
    _dev(x)
    if not gru_supported(gru_module):
        raise RuntimeError("gru: one layer, batch_first, unidirectional, with bias and hidden % 64 == 0 expected")
    g = gru_module
    params = (g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0)
    if _wants_grad(x, h0, *params):
        return _grad.GRUFn.apply(x, *params, h0)
    out, h_last, h0c = gru_buffers(x, g.hidden_size, h0)
    w_ih, w_hh, b_ih, b_hh = params
    gru_layer_launch(x, w_ih, b_ih, w_hh, b_hh, h0c, out, h_last, None, persistent_flags)
    return out, h_last


def gru_buffers(x, H, h0):
    """One layer call's outputs and initial state as the kernels take them: out [B, T, H], h_T [1, B, H],
    h0 as contiguous [B, H] (or None)."""
    B, T = x.shape[:2]
    out = torch.empty(B, T, H, dtype=torch.float32, device=x.device)
    h_last = torch.empty(1, B, H, dtype=torch.float32, device=x.device)
    return out, h_last, (_c(h0.reshape(B, H)) if h0 is not None else None)


# include/ddsp_hip.h: ddsp_hip_gru_forward_persistent's flags (test hooks) and status bits
GRU_SPREAD, GRU_NO_MASK_CHECK, GRU_FORCE_ABORT = 1, 2, 4
GRU_STATUS_LOCAL, GRU_STATUS_RESCUED = 1, 2
_GRU_LAST = {}  # device index -> (route, persistent workspace or None) of the last GRU launch (_gru_ran)


def _gru_ran(device, route, ws=None):
    """Record the route of the launch just made on ``device`` for gru_last_route; returns it."""
    dev = device.index if device.index is not None else torch.cuda.current_device()
    _GRU_LAST[dev] = (route, ws)
    return route


def gru_layer_launch(x, w_ih, b_ih, w_hh, b_hh, h0c, out, h_last, gates, persistent_flags=0):
    """The layer's forward on the device: the input projection for every step as one GEMM, then the
    recurrence (gru_recurrence; a form with each step's projection inside the step launch measured slower:
    13.3 vs 7.4-7.8 us per step).  Returns the route taken ("persistent" or "steps")."""
    B, T, I = x.shape
    xp = linear(_c(x).reshape(B * T, I), w_ih, b_ih).view(B, T, 3 * w_hh.shape[1])
    return gru_recurrence(xp, w_hh, b_hh, h0c, out, h_last, gates, persistent_flags)


def gru_recurrence(xp, w_hh, b_hh, h0, out, h_last, gates=None, persistent_flags=0, ws=None, persistent=True,
                   h_last_steps=None):
    """The recurrence over the projected inputs xp [B, T, 3H] into out [B, T, H] and h_T: one persistent launch
    (ddsp_hip_gru_forward_persistent: hidden 512, batch <= 64, a stream that may use every CU; W_hh resident
    in registers, h handed between the workgroups of a group), else (ERANGE, or ``persistent=False``: no
    attempt) ddsp_hip_gru_forward's one launch per step.  A persistent launch that cannot get its workgroups
    resident aborts and its outputs are recomputed, on the same stream, with the step kernels' arithmetic
    (gru_rescue_kernel): the values are right on every route; ``gru_last_route`` tells which one ran.
    ``ws``: the persistent launch's workspace where the caller keeps one alive (a captured graph).
    ``h_last_steps``: where the step kernels write h_T if not ``h_last`` — they may write over h0, the
    persistent launch may not (its rescue re-reads h0).  Returns the route taken ("persistent" or "steps")."""
    B, T, H = out.shape
    args = (_lib.ptr(xp), _lib.ptr(_c(w_hh)), _lib.ptr(_c(b_hh)), _lib.ptr(h0), _lib.ptr(out))
    dims = (_lib.ptr(gates), B, T, H)
    if persistent:
        if ws is None:
            ws = _workspace(_lib.query("gru_persistent_workspace_size"), out.device)
        st = _lib.call("gru_forward_persistent", *args, _lib.ptr(h_last), *dims, int(persistent_flags), _lib.ptr(ws),
                       ws.numel(), _lib.stream_of(out), allow=(ERANGE,))
        if st != ERANGE:
            return _gru_ran(out.device, "persistent", ws)
    _lib.call("gru_forward", *args, _lib.ptr(h_last if h_last_steps is None else h_last_steps), *dims,
              _lib.stream_of(out))
    return _gru_ran(out.device, "steps")


def gru_backward_launch(w_hh, gates, out, h0, g_out, g_hlast, dxp, dgn, dh0, persistent_flags=0):
    """The layer's BPTT from the forward's saved gate planes into dxp [B, T, 3H], dgn [B, T, H] and dh0: one
    persistent launch (hidden 512, batch <= 64), else (ERANGE) ddsp_hip_gru_backward's one launch per step.
    ``persistent_flags``: the persistent launch's test hooks.  Returns the route taken."""
    B, T, H = out.shape
    args = (_lib.ptr(_c(w_hh)), _lib.ptr(gates), _lib.ptr(out), _lib.ptr(h0), _lib.ptr(g_out), _lib.ptr(g_hlast),
            _lib.ptr(dxp), _lib.ptr(dgn), _lib.ptr(dh0), B, T, H)
    ws = _workspace(_lib.query("gru_persistent_workspace_size"), out.device)
    st = _lib.call("gru_backward_persistent", *args, int(persistent_flags), _lib.ptr(ws), ws.numel(),
                   _lib.stream_of(dxp), allow=(ERANGE,))
    if st != ERANGE:
        return _gru_ran(out.device, "persistent", ws)
    ws = _workspace(_lib.query("gru_backward_workspace_size", B, H), out.device)
    _lib.call("gru_backward", *args, _lib.ptr(ws), ws.numel(), _lib.stream_of(dxp))
    return _gru_ran(out.device, "steps")


def gru_last_route(device=None):
    """Which recurrence the last gru_layer_launch on ``device`` ran, read after a device synchronize:
    {"route": "persistent" | "steps" | None, "hand_off": "xcd_local" | "write_through" | None,
    "rescued": bool (the persistent launch aborted and the rescue kernel produced the outputs)}."""
    dev = torch.cuda.current_device() if device is None else torch.device(device).index or 0
    route, ws = _GRU_LAST.get(dev, (None, None))
    info = {"route": route, "hand_off": None, "rescued": False}
    if ws is not None:
        torch.cuda.synchronize(dev)
        off = int(_lib.query("gru_persistent_status_offset"))
        word = int(ws[off:off + 4].cpu().view(torch.int32)[0])
        info["rescued"] = bool(word & GRU_STATUS_RESCUED)
        if not info["rescued"]:
            info["hand_off"] = "xcd_local" if word & GRU_STATUS_LOCAL else "write_through"
    return info


def linear(x, weight, bias):
    """x [rows, in] @ weight[out, in]^T + bias -> [rows, out] (no autograd): ddsp_hip_linear — the bf16 matrix
    cores with the fp32-accurate three-term split — where it applies (in 512 / 1024 / 1536, out a multiple of
    512: dense.hip's ddsp_hip_linear), else torch.addmm (hipBLASLt)."""
    _dev(x, weight, bias)
    rows, K = x.shape
    N = weight.shape[0]
    xc, wc, bc = _c(x), _c(weight), _c(bias)
    y = torch.empty(rows, N, dtype=torch.float32, device=x.device)
    st = _lib.call("linear", _lib.ptr(xc), K, K, _lib.ptr(wc), K, _lib.ptr(bc), _lib.ptr(y), N, rows, N,
                   _lib.stream_of(y), allow=(ERANGE,))
    return torch.addmm(bias, x, weight.t()) if st == ERANGE else y


def linear_input_grad(grad_y, weight):
    """grad_y [rows, out] @ weight [out, in] -> [rows, in], a Linear's input gradient (no autograd): ``linear``
    with W^T as its weight and a zero bias."""
    wt = weight.t().contiguous()
    return linear(grad_y, wt, torch.zeros(wt.shape[0], dtype=wt.dtype, device=wt.device))


def linear_weight_grad(grad_y, x):
    """grad_y [rows, out]^T @ x [rows, in] -> [out, in], a Linear's weight gradient (no autograd):
    ddsp_hip_linear_weight_grad — the bf16 matrix cores with the fp32-accurate three-term split, split over
    row ranges summed in a fixed order (any widths; torch.mm only past its 32-bit range offsets)."""
    _dev(grad_y, x)
    rows, M = grad_y.shape
    N = x.shape[1]
    gc, xc = _c(grad_y), _c(x)
    dw = torch.empty(M, N, dtype=torch.float32, device=x.device)
    ws = _workspace(_lib.query("linear_weight_grad_workspace_size", max(rows, 1), M, N), x.device)
    st = _lib.call("linear_weight_grad", _lib.ptr(gc), M, _lib.ptr(xc), N, _lib.ptr(dw), N, rows, M, N,
                   _lib.ptr(ws), ws.numel(), _lib.stream_of(dw), allow=(ERANGE,))
    return grad_y.t().mm(x) if st == ERANGE else dw


MLP_EXACT_F32 = 1  # include/ddsp_hip.h DDSP_HIP_MLP_EXACT_F32


def _row_strided(out, shape):
    """``out`` has ``shape`` [..., cols] with unit stride on cols and one row stride over the leading
    dims (row r at r * out.stride(-2)): a column slice of a wider contiguous buffer qualifies."""
    return (tuple(out.shape) == tuple(shape) and out.stride(-1) == 1 and
            all(out.stride(i) == out.stride(i + 1) * out.shape[i + 1] for i in range(out.dim() - 2)))


def _out_rows(out, lead, cols, device):
    """Where a kernel writes its [*lead, cols] result -> (buffer, row stride): a fresh buffer, or the caller's
    ``out`` if the kernel can address it (_row_strided), else (None, 0)."""
    if out is None:
        out = torch.empty(*lead, cols, dtype=torch.float32, device=device)
    elif not _row_strided(out, tuple(lead) + (cols,)):
        return None, 0
    return out, (out.stride(-2) if out.dim() >= 2 else cols)


# Below one K chunk of the matrix-core kernels (16 wide: k = 16 h + ..., dense.hip's mlp_block_kernel) a block's
# Linear has no work for them: the decoder keeps the K = 1 Linear in the LayerNorm kernel (or torch's, under
# autograd) and runs mlp_block / grad.LinearFn from here up.  A policy of the callers, not an envelope:
# ddsp_hip_mlp_block itself takes any K >= 1.
MLP_MATRIX_MIN_IN = 16


def mlp_block(x, linear, norm, act, out=None, extras=(), flags=0):
    """ddsp/core.py:122-129, one whole block: LeakyReLU(LayerNorm(linear(x))) in one launch
    (ddsp_hip_mlp_block: the Linear on the matrix cores — at 512 inputs fp32-accurate bf16x3 products,
    ``flags=MLP_EXACT_F32`` the f32-input MFMA — LayerNorm + LeakyReLU in its epilogue).
    ``extras``: up to two [..., 1] tensors that are the Linear's LAST input features (the decoder's
    out_mlp input [gru_out, f0, loudness], decoder.py:68, given as x = gru_out, extras = (f0, loudness)).
    Returns None where the kernel does not apply (it is built for 512 output features);
    inference only."""
    _dev(x, linear.weight, linear.bias, norm.weight, norm.bias, *extras)
    n_out, n_in = linear.weight.shape
    K = x.shape[-1]
    if (len(extras) > 2 or K + len(extras) != n_in or n_out != 512 or tuple(norm.normalized_shape) != (n_out,)
            or any(e.shape != x.shape[:-1] + (1,) for e in extras)):
        return None
    xc = _c(x)
    rows = xc.numel() // K if K else 0
    out, y_ld = _out_rows(out, x.shape[:-1], n_out, x.device)
    if out is None:
        return None
    ec = [_c(e) for e in extras]
    st = _lib.call("mlp_block", _lib.ptr(xc), K, K, _lib.ptr(_c(linear.weight)), n_in, _lib.ptr(_c(linear.bias)),
                   _lib.ptr(ec[0] if ec else None), _lib.ptr(ec[1] if len(ec) > 1 else None), 1,
                   _lib.ptr(_c(norm.weight)), _lib.ptr(_c(norm.bias)), float(norm.eps), float(act.negative_slope),
                   _lib.ptr(out), int(y_ld), int(rows), n_out, int(flags), _lib.stream_of(out), allow=(ERANGE,))
    return None if st == ERANGE else out


def projections(x, lin1, lin2, pad_to=64):
    """decoder.py:106-117 in ONE launch: ddsp_hip_projections — both Linears on the bf16 matrix cores with the
    fp32-accurate three-term split, reading each layer's parameters where they lie (at 512 inputs, 16-byte
    aligned rows).  Elsewhere ONE library GEMM: both layers' parameters stacked, fresh every call, into a
    zero-padded [n_pad, K] buffer (ddsp_hip_stack_rows, one launch; n_pad a multiple of ``pad_to``:
    hipBLASLt runs 192 outputs in 28-30 us, the unpadded 166 in 38-39), then F.linear.  Returns the two
    outputs as column slices of one [..., n] result.  Nothing is cached on the modules."""
    _dev(x, lin1.weight, lin1.bias, lin2.weight, lin2.bias)
    n1, n2, K = lin1.out_features, lin2.out_features, x.shape[-1]
    w1, w2 = _c(lin1.weight), _c(lin2.weight)
    y, launched = projections_launch(_c(x), w1, lin1.bias, w2, lin2.bias)
    if launched:
        return y[..., :n1], y[..., n1:n1 + n2]
    n_pad = -(-(n1 + n2) // pad_to) * pad_to
    w = torch.empty(n_pad, K, dtype=torch.float32, device=x.device)
    b = torch.empty(n_pad, dtype=torch.float32, device=x.device)
    _lib.call("stack_rows", _lib.ptr(w1), w1.stride(0), _lib.ptr(_c(lin1.bias)), n1, _lib.ptr(w2), w2.stride(0),
              _lib.ptr(_c(lin2.bias)), n2, K, _lib.ptr(w), _lib.ptr(b), n_pad, _lib.stream_of(w))
    y = torch.nn.functional.linear(x, w, b)  # (this package's matrix-core projection kernel ran 40-44 us)
    return y[..., :n1], y[..., n1:n1 + n2]


def projections_launch(x, w1, b1, w2, b2):
    """ddsp_hip_projections over x [..., K] and the two layers' parameters, all contiguous (_c) -> (y [..., n4],
    launched): both outputs side by side in rows of n4 floats, n1 + n2 rounded up to 4 (16-byte aligned rows).
    ``launched`` False: outside the kernel's shapes (dense.hip's ddsp_hip_projections), y is not written."""
    n1, n2, K = w1.shape[0], w2.shape[0], x.shape[-1]
    n4 = -(-(n1 + n2) // 4) * 4
    y = torch.empty(*x.shape[:-1], n4, dtype=torch.float32, device=x.device)
    st = _lib.call("projections", _lib.ptr(x), K, K, _lib.ptr(w1), K, _lib.ptr(_c(b1)), n1, _lib.ptr(w2), K,
                   _lib.ptr(_c(b2)), n2, _lib.ptr(y), n4, x.numel() // K if K else 0, _lib.stream_of(y),
                   allow=(ERANGE,))
    return y, st != ERANGE


LN_LEAKY_COLS = (512, 1024)  # the widths ddsp_hip_layer_norm_leaky_relu and its backward take (dense.hip)


def layer_norm_leaky_relu(h, norm, act, out=None, w1=None, b1=None):
    """ddsp/core.py:122-129 after one block's Linear: LeakyReLU(LayerNorm(h)) in one pass
    (ddsp_hip_layer_norm_leaky_relu).  h [..., cols] contiguous; or, with w1/b1 (a Linear with one input
    feature), h [..., 1] is that Linear's input and the block's pre-activation is h * w1 + b1.  ``out``
    (optional) may be a column slice of a wider buffer with one row stride.  Returns None where the
    kernel does not apply (the caller runs torch's modules); inference only."""
    _dev(h, norm.weight, norm.bias)
    if len(norm.normalized_shape) != 1:
        return None
    return ln_leaky_launch(h, norm.weight, norm.bias, norm.eps, act.negative_slope, out, w1, b1)


def ln_leaky_launch(h, gamma, beta, eps, slope, out=None, w1=None, b1=None):
    """layer_norm_leaky_relu on the affine parameters themselves (grad.LNLeakyFn has no modules): None where the
    kernel does not apply — shapes that do not fit gamma, an ``out`` it cannot address, ERANGE (widths outside
    LN_LEAKY_COLS, unaligned rows)."""
    cols = gamma.shape[0]
    if h.shape[-1] != (cols if w1 is None else 1):
        return None
    if not h.is_contiguous():
        h = h.contiguous()
    rows = h.numel() // h.shape[-1] if h.shape[-1] else 0
    out, y_ld = _out_rows(out, h.shape[:-1], cols, h.device)
    if out is None:
        return None
    w1c = _c(w1) if w1 is not None else None
    b1c = _c(b1) if b1 is not None else None
    st = _lib.call("layer_norm_leaky_relu", _lib.ptr(h), int(h.shape[-1]), _lib.ptr(w1c), _lib.ptr(b1c),
                   _lib.ptr(_c(gamma)), _lib.ptr(_c(beta)), float(eps), float(slope), _lib.ptr(out), int(y_ld),
                   int(rows), cols, _lib.stream_of(out), allow=(ERANGE,))
    return None if st == ERANGE else out


def dense_input(x, width=None, ld=None, scale=1.0, shift=0.0, first=None, norm=None, x_copy=None, activation=True):
    """One input segment of dense_rows: x [rows, ld] (or, with `first` = a K=1 nn.Linear, one value
    per row at x[r * ld]); `norm` = an nn.LayerNorm applied with LeakyReLU(0.01) after it, or with
    ``activation=False`` alone (the MFCC encoder's ``norm``)."""
    inp = _lib.DenseInput()
    inp.x = x.data_ptr()
    inp.scale, inp.shift = float(scale), float(shift)
    if first is not None:
        inp.w1, inp.b1 = first.weight.data_ptr(), first.bias.data_ptr()
        inp.width = first.out_features
    else:
        inp.width = int(width if width is not None else x.shape[-1])
    inp.ld = int(ld if ld is not None else inp.width)
    if norm is not None:
        if norm.eps != 1e-5 or norm.weight is None:
            raise RuntimeError("dense_input: LayerNorm(eps=1e-5, elementwise_affine) expected")
        inp.gamma, inp.beta = norm.weight.data_ptr(), norm.bias.data_ptr()
        inp.plain_norm = 0 if activation else 1
    elif not activation:
        raise RuntimeError("dense_input: activation=False goes with a norm")
    if x_copy is not None:
        inp.x_copy = x_copy.data_ptr()
    return inp


def dense_rows(problems, rows, device):
    """ddsp_hip_dense_rows: up to three Linears (each `(inputs, linear, y)`, inputs from dense_input,
    y [rows, out_features] contiguous) over `rows` <= 8 rows in one launch (core.py:122-129 blocks
    with the LayerNorm/LeakyReLU of the previous block folded into the input)."""
    if not 1 <= len(problems) <= _lib.DENSE_MAX_PROBLEMS:
        raise RuntimeError(f"dense_rows: 1 to {_lib.DENSE_MAX_PROBLEMS} problems per launch")
    arr = (_lib.DenseProblem * len(problems))()
    for i, (inputs, lin, y) in enumerate(problems):
        P = arr[i]
        for j, inp in enumerate(inputs):
            P.inputs[j] = inp
        P.n_inputs = len(inputs)
        if sum(inp.width for inp in inputs) != lin.in_features:
            raise RuntimeError("dense_rows: inputs do not add up to the Linear's in_features")
        P.weight = lin.weight.data_ptr()
        P.bias = lin.bias.data_ptr() if lin.bias is not None else None
        P.y = y.data_ptr()
        P.ldy = y.shape[-1]
        P.out_features = lin.out_features
    _lib.call("dense_rows", arr, len(problems), int(rows),
              ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))


# ------------------------------------------------------------------------------------
# training loss (ddsp/core.py:10-41; train.py:70-76)
# ------------------------------------------------------------------------------------
def safe_log(x):
    """ddsp/core.py:10-11."""
    return torch.log(x + 1e-7)


def stft_magnitude(signal, n_fft, hop):
    """|torch.stft(signal, n_fft, hop, n_fft, hann_window(n_fft), center=True, normalized=True)|
    for signal [B, T] -> [B, n_fft/2+1, frames] (a transposed view of the kernel's frame-major
    output; the values and shape are the reference's)."""
    _dev(signal)
    if signal.dim() != 2:
        raise RuntimeError(f"stft_magnitude: expected [batch, time], got {tuple(signal.shape)}")
    if _wants_grad(signal):
        return _grad.StftMagFn.apply(signal, int(n_fft), int(hop))
    B, T = signal.shape
    x = _c(signal)
    frames = int(_lib.query("stft_frames", T, int(hop)))
    M = torch.empty(B, frames, int(n_fft) // 2 + 1, dtype=torch.float32, device=x.device)
    _lib.call("stft_magnitude", _lib.ptr(x), _lib.ptr(M), B, T, int(n_fft), int(hop), _lib.stream_of(x))
    return M.transpose(1, 2)


def multiscale_fft(signal, scales, overlap):
    """ddsp/core.py:27-41: one magnitude spectrogram per scale, hop int(s * (1 - overlap))."""
    return [stft_magnitude(signal, s, int(s * (1 - overlap))) for s in scales]


# ------------------------------------------------------------------------------------
# audio analysis: the features the models consume (ddsp/core.py:81-97, ddsp/preprocess.py:28-32)
# ------------------------------------------------------------------------------------
def a_weighting_table(sample_rate, n_fft):
    """core.py:90-91: librosa.A_weighting(librosa.fft_frequencies(sample_rate, n_fft)) in dB, float64
    [n_fft/2+1], clipped below at -80 (so the 0 Hz bin is -80)."""
    f_sq = np.linspace(0.0, float(sample_rate) / 2, 1 + int(n_fft) // 2) ** 2
    c = np.array([12200.0, 20.6, 107.7, 737.9]) ** 2
    with np.errstate(divide="ignore"):
        w = 2.0 + 20.0 * (np.log10(c[0]) + 2 * np.log10(f_sq) - np.log10(f_sq + c[0]) - np.log10(f_sq + c[1])
                          - 0.5 * np.log10(f_sq + c[2]) - 0.5 * np.log10(f_sq + c[3]))
    return np.maximum(w, -80.0)


def _hz_to_mel(f):
    """Slaney's scale (librosa's default, htk=False): linear below 1 kHz, logarithmic above."""
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, math.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, math.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank_table(sample_rate, n_fft, n_mels, fmin, fmax):
    """librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax, htk=False, norm='slaney'), float64
    [n_mels, n_fft/2+1]: triangles between n_mels + 2 mel-spaced edges, each row scaled by 2 / its width."""
    freqs = np.linspace(0.0, float(sample_rate) / 2, 1 + int(n_fft) // 2)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(float(fmin)), _hz_to_mel(float(fmax)), int(n_mels) + 2))
    fdiff = np.diff(edges)
    ramps = edges[:, None] - freqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    fb = np.maximum(0.0, np.minimum(lower, upper))
    return fb * (2.0 / (edges[2:] - edges[:-2]))[:, None]


def mel_bands(filterbank):
    """A dense filterbank [n_mels, bins] as ddsp_hip_mfcc takes it: (first bin, count, packed weights) per
    row — the row's span from its first to its last non-zero bin; an empty row has count 0."""
    starts, counts, weights = [], [], []
    for row in np.asarray(filterbank):
        nz = np.flatnonzero(row)
        s, c = (int(nz[0]), int(nz[-1] - nz[0] + 1)) if nz.size else (0, 0)
        starts.append(s)
        counts.append(c)
        weights.append(row[s:s + c])
    packed = np.concatenate(weights) if weights else np.zeros(0)
    return np.asarray(starts, dtype=np.int32), np.asarray(counts, dtype=np.int32), packed


def dct_table(n_mfcc, n_mels):
    """The first n_mfcc rows of the orthonormal DCT-II of n_mels points (scipy.fftpack.dct(type=2,
    norm='ortho'), librosa.feature.mfcc's), float64 [n_mfcc, n_mels]."""
    i = np.arange(int(n_mfcc))[:, None]
    m = np.arange(int(n_mels))[None, :]
    t = math.sqrt(2.0 / n_mels) * np.cos(math.pi * i * (2 * m + 1) / (2.0 * n_mels))
    t[0] = math.sqrt(1.0 / n_mels)
    return t


_FEATURE_TABLES = {}  # (kind, parameters, device) -> device tensors, built on the host once


def _feature_tables(kind, params, device, make):
    key = (kind, params, device.type, device.index if device.index is not None else torch.cuda.current_device())
    tabs = _FEATURE_TABLES.get(key)
    if tabs is None:
        tabs = tuple(torch.from_numpy(np.ascontiguousarray(a if a.dtype == np.int32 else a.astype(np.float32)))
                     .to(device) for a in make())
        _FEATURE_TABLES[key] = tabs
    return tabs


def _a_weighting(sample_rate, n_fft, device):
    """``a_weighting_table`` on ``device``, cached per (sample_rate, n_fft, device)."""
    return _feature_tables("a_weighting", (float(sample_rate), int(n_fft)), device,
                           lambda: (a_weighting_table(sample_rate, n_fft),))[0]


def _signal_rows(signal, block_size, name):
    """signal [T] or [B, T] on a HIP device -> (contiguous detached [B, T], whether it was 1-D)."""
    _dev(signal)
    if signal.dim() not in (1, 2):
        raise RuntimeError(f"{name}: expected audio [time] or [batch, time], got {tuple(signal.shape)}")
    if int(block_size) < 1:
        raise RuntimeError(f"{name}: block_size must be positive, got {block_size}")
    x = signal.detach()
    return _c(x.unsqueeze(0) if x.dim() == 1 else x), signal.dim() == 1


def extract_loudness(signal, sample_rate, block_size, n_fft=2048):
    """ddsp/core.py:81-97 on the device: signal [T] or [B, T] (HIP, fp32; made contiguous if it is not) ->
    A-weighted log-magnitude loudness [T // block_size] or [B, T // block_size], one launch, no spectrogram
    in memory.  The reference's quirk is kept: the natural log of the magnitude plus a weighting in dB.
    The A-weighting table is built on the host at the first call per (sample_rate, n_fft, device) and cached;
    later calls do not synchronise with the host (capturable in a HIP graph).  No autograd: an input that
    requires grad is analysed detached."""
    x, one_d = _signal_rows(signal, block_size, "extract_loudness")
    n_fft = int(n_fft)
    w = _a_weighting(sample_rate, n_fft, x.device)
    B, T = x.shape
    out = torch.empty(B, T // int(block_size), dtype=torch.float32, device=x.device)
    _lib.call("loudness", _lib.ptr(x), _lib.ptr(w), _lib.ptr(out), B, T, n_fft, int(block_size), _lib.stream_of(x))
    return out[0] if one_d else out


def pitch_lags(sample_rate, fmin, fmax, frame_length):
    """(tau_min, tau_max) of include/ddsp_hip.h ("pitch"): the lag range in samples for a frequency range, in
    double precision, once: max(floor(sr / fmax), 1) and min(ceil(sr / fmin), L - W - 1), W = L / 2."""
    sr, L = float(sample_rate), int(frame_length)
    if not (sr > 0.0 and float(fmin) > 0.0 and float(fmax) > 0.0):
        raise RuntimeError(f"pitch: sample_rate, fmin and fmax must be positive, got {sample_rate}, {fmin}, {fmax}")
    tau_min = max(int(math.floor(sr / float(fmax))), 1)
    tau_max = min(int(math.ceil(sr / float(fmin))), L - L // 2 - 1)
    if tau_min > tau_max:
        raise RuntimeError(f"pitch: no lag lies in [{fmin}, {fmax}] Hz at sample_rate {sample_rate} with "
                           f"frame_length {L} (lags {tau_min} .. {tau_max})")
    return tau_min, tau_max


def _pitch_outputs(B, F, device, return_confidence, return_period):
    f0 = torch.empty(B, F, dtype=torch.float32, device=device)
    conf = torch.empty(B, F, dtype=torch.float32, device=device) if return_confidence else None
    period = torch.empty(B, F, dtype=torch.int32, device=device) if return_period else None
    return f0, conf, period


def _pitch_result(f0, conf, period, one_d):
    out = tuple(t[0] if one_d else t for t in (f0, conf, period) if t is not None)
    return out[0] if len(out) == 1 else out


def extract_pitch(signal, sample_rate, block_size, fmin=50.0, fmax=2000.0, frame_length=2048, threshold=0.1,
                  return_confidence=False, return_period=False):
    """f0 from raw audio on the device: signal [T] or [B, T] (HIP, fp32) -> f0 in Hz, [T // block_size] or
    [B, T // block_size], by the YIN estimator of include/ddsp_hip.h ("pitch": frames of ``frame_length`` samples
    centred at f * block_size with reflect padding, the loudness's frames; the fp64 difference function through
    the FFT, cumulative-mean normalisation, the first dip under ``threshold``, parabolic refinement).  One launch,
    no host synchronisation.  This is NOT the reference's ``extract_pitch`` (ddsp/core.py:100-119: the CREPE
    network on host numpy), whose weights are not part of this package; it stands where that stood so that
    ``features.analyze`` can run from audio alone.  ``return_confidence``: also 1 - d'(tau*) in [0, 1] (what a
    caller thresholds for voicing); ``return_period``: also the integer lag tau* (int32).  No autograd."""
    x, one_d = _signal_rows(signal, block_size, "extract_pitch")
    L = int(frame_length)
    tau_min, tau_max = pitch_lags(sample_rate, fmin, fmax, L)
    B, T = x.shape
    f0, conf, period = _pitch_outputs(B, T // int(block_size), x.device, return_confidence, return_period)
    _lib.call("pitch", _lib.ptr(x), _lib.ptr(f0), _lib.ptr(conf), _lib.ptr(period), B, T, L, int(block_size),
              tau_min, tau_max, float(sample_rate), float(threshold), _lib.stream_of(x))
    return _pitch_result(f0, conf, period, one_d)


def _pitch_bin_arrays(tau_min, tau_max, bins_per_octave):
    """(lo, hi) int32 arrays of include/ddsp_hip.h ("pitch_viterbi", Bins), in double precision."""
    beta = float(bins_per_octave)
    if not beta > 0.0:
        raise RuntimeError(f"pitch_bins: bins_per_octave must be positive, got {bins_per_octave}")
    tau = np.arange(tau_min, tau_max + 1, dtype=np.int64)
    bins = np.rint(beta * np.log2(float(tau_max) / tau.astype(np.float64))).astype(np.int64)  # halves to even
    n_bins = int(bins[0]) + 1
    if n_bins > 1024:
        raise RuntimeError(f"pitch_bins: {n_bins} bins (lags {tau_min} .. {tau_max} at {bins_per_octave} per octave) "
                           "exceed the decode's 1024")
    centre = np.clip(np.rint(float(tau_max) * 2.0 ** (-np.arange(n_bins) / beta)), tau_min, tau_max).astype(np.int64)
    lo, hi = np.full(n_bins, tau_max + 1, dtype=np.int64), np.full(n_bins, -1, dtype=np.int64)
    np.minimum.at(lo, bins, tau)
    np.maximum.at(hi, bins, tau)
    empty = hi < 0
    lo[empty], hi[empty] = centre[empty], centre[empty]
    return lo.astype(np.int32), hi.astype(np.int32)


def pitch_bins(sample_rate, fmin, fmax, frame_length, bins_per_octave=48):
    """(tau_min, tau_max, lo, hi) of include/ddsp_hip.h ("pitch_viterbi"): ``pitch_lags``' lag range and, per
    log-spaced bin i = rint(bins_per_octave * log2(tau_max / tau)), the smallest and the largest lag in it (a bin no
    lag falls in holds its centre's nearest lag); host lists of len n_bins <= 1024, built once in double precision."""
    tau_min, tau_max = pitch_lags(sample_rate, fmin, fmax, frame_length)
    lo, hi = _pitch_bin_arrays(tau_min, tau_max, bins_per_octave)
    return tau_min, tau_max, lo.tolist(), hi.tolist()


def _pitch_bin_tables(sample_rate, fmin, fmax, frame_length, bins_per_octave, device):
    """(tau_min, tau_max, lo, hi) with lo / hi on ``device``, cached per parameters as the other analysis tables."""
    tau_min, tau_max = pitch_lags(sample_rate, fmin, fmax, frame_length)
    lo, hi = _feature_tables("pitch_bins", (tau_min, tau_max, float(bins_per_octave)), device,
                             lambda: _pitch_bin_arrays(tau_min, tau_max, bins_per_octave))
    return tau_min, tau_max, lo, hi


def _salience_outputs(B, F, NB, device, return_lag, return_raw):
    """(cost, f0c, lag, f0, confidence, period) as the salience's launch takes them: None for what is not asked for."""
    cost = torch.empty(B, F, NB, dtype=torch.float32, device=device)
    lag = torch.empty(B, F, NB, dtype=torch.int32, device=device) if return_lag else None
    raw = _pitch_outputs(B, F, device, True, True) if return_raw else (None, None, None)
    return (cost, torch.empty_like(cost), lag) + raw


def pitch_salience(signal, sample_rate, block_size, fmin=50.0, fmax=2000.0, frame_length=2048, bins_per_octave=48,
                   return_lag=False, return_raw=False, threshold=0.1):
    """The salience the Viterbi decode runs over (include/ddsp_hip.h, "pitch_viterbi"): signal [T] or [B, T] (HIP,
    fp32) -> (cost, f0c[, lag]), each [B, T // block_size, n_bins] ([F, n_bins] for a 1-D signal): per frame of
    ``extract_pitch`` and per bin of ``pitch_bins``, min(1, d') at the bin's best lag, the f0 candidate there after
    the parabola, and the lag itself (int32).  ``return_raw``: also ``extract_pitch``'s (f0, confidence, period) for
    ``threshold``, bit for bit, out of the same launch.  One launch; the bin tables are built on the host at the
    first call per parameters and device and cached (no host synchronisation afterwards).  No autograd."""
    x, one_d = _signal_rows(signal, block_size, "pitch_salience")
    L = int(frame_length)
    tau_min, tau_max, lo, hi = _pitch_bin_tables(sample_rate, fmin, fmax, L, bins_per_octave, x.device)
    B, T = x.shape
    NB = lo.numel()
    out = _salience_outputs(B, T // int(block_size), NB, x.device, return_lag, return_raw)
    _lib.call("pitch_salience", _lib.ptr(x), _lib.ptr(lo), _lib.ptr(hi), *map(_lib.ptr, out), B, T, L,
              int(block_size), tau_min, tau_max, NB, float(sample_rate), float(threshold), _lib.stream_of(x))
    return tuple(t[0] if one_d else t for t in out if t is not None)


def viterbi_path(cost, f0c, transition=0.02, max_jump=12):
    """The decode of include/ddsp_hip.h ("pitch_viterbi"): cost, f0c [B, F, n_bins] or [F, n_bins] (HIP, fp32) ->
    (f0, confidence, path), each [B, F] or [F]: the path of least summed cost over the frames when a move of k bins
    (|k| <= ``max_jump`` <= 127) between neighbouring frames costs ``transition`` * k, in fp64 with the smallest index
    winning every tie; f0 = f0c and confidence = 1 - cost along it, path int32.  One launch, one workgroup per item;
    no host synchronisation.  No autograd."""
    _dev(cost, f0c)
    if cost.dim() not in (2, 3) or cost.shape != f0c.shape:
        raise RuntimeError(f"viterbi_path: cost and f0c must both be [frames, bins] or [batch, frames, bins], got "
                           f"{tuple(cost.shape)} and {tuple(f0c.shape)}")
    one = cost.dim() == 2
    c, g = (_c(t.detach().float().unsqueeze(0) if one else t.detach().float()) for t in (cost, f0c))
    B, F, NB = c.shape
    if NB < 1:
        raise RuntimeError("viterbi_path: no bins")
    f0 = torch.empty(B, F, dtype=torch.float32, device=c.device)
    conf = torch.empty_like(f0)
    path = torch.empty(B, F, dtype=torch.int32, device=c.device)
    ws = torch.empty(B * F * NB, dtype=torch.int8, device=c.device)
    _lib.call("pitch_viterbi", _lib.ptr(c), _lib.ptr(g), _lib.ptr(f0), _lib.ptr(conf), _lib.ptr(path), _lib.ptr(ws),
              ws.numel(), B, F, NB, int(max_jump), float(transition), _lib.stream_of(c))
    return (f0[0], conf[0], path[0]) if one else (f0, conf, path)


def track_pitch(signal, sample_rate, block_size, fmin=50.0, fmax=2000.0, frame_length=2048, bins_per_octave=48,
                transition=0.02, max_jump=12, return_confidence=False, return_path=False):
    """f0 from raw audio with a temporal model: ``pitch_salience`` then ``viterbi_path`` — signal [T] or [B, T] (HIP,
    fp32) -> f0 in Hz, [T // block_size] or [B, T // block_size] (and on request the confidence 1 - d' along the path
    and the path's bins, int32).  Where ``extract_pitch`` takes each frame's first dip on its own and jumps an octave
    when a harmonic outweighs the fundamental, the decode pays ``transition`` per bin (1 / ``bins_per_octave``
    octave) moved between frames, which is what ``viterbi=True`` buys the reference's CREPE track.  Offline only (the
    decode needs the whole signal; ``stream_track_pitch`` is its fixed-lag form for a stream); two launches, no host
    synchronisation after the first call.  No autograd."""
    one_d = signal.dim() == 1
    cost, f0c = pitch_salience(signal.unsqueeze(0) if one_d else signal, sample_rate, block_size, fmin=fmin,
                               fmax=fmax, frame_length=frame_length, bins_per_octave=bins_per_octave)
    f0, conf, path = viterbi_path(cost, f0c, transition=transition, max_jump=max_jump)
    return _pitch_result(f0, conf if return_confidence else None, path if return_path else None, one_d)


def mfcc_tables(sample_rate, n_mfcc, n_fft, n_mels, fmin, fmax, device):
    """(band_start, band_count, band_weights, dct) of ``mfcc`` on ``device``, cached per parameters."""
    params = (float(sample_rate), int(n_mfcc), int(n_fft), int(n_mels), float(fmin), float(fmax))

    def make():
        s, c, w = mel_bands(mel_filterbank_table(sample_rate, n_fft, n_mels, fmin, fmax))
        return s, c, w, dct_table(n_mfcc, n_mels)
    return _feature_tables("mfcc", params, torch.device(device), make)


def mfcc(signal, sample_rate, block_size, n_mfcc=30, n_fft=1024, n_mels=128, fmin=20.0, fmax=8000.0, top_db=80.0,
         return_db=False):
    """ddsp/preprocess.py:30-32 on the device: ``librosa.feature.mfcc(x, sr, n_mfcc, n_fft, hop_length=
    block_size, fmin, fmax, n_mels).T`` with librosa's defaults behind it (Slaney mel filterbank, power
    spectrogram, 10 log10 with amin 1e-10 and ref 1, top_db per item, orthonormal DCT-II).  signal [T] or
    [B, T] (HIP, fp32) -> [1 + T // block_size, n_mfcc] or [B, 1 + T // block_size, n_mfcc]; two launches,
    no spectrogram in memory.  ``return_db``: also the mel spectrogram in dB before the clamp,
    [B, frames, n_mels].  Tables: built on the host at the first call per (parameters, device) and cached;
    later calls do not synchronise with the host.  No autograd: an input that requires grad is analysed
    detached."""
    x, one_d = _signal_rows(signal, block_size, "mfcc")
    band_start, band_count, band_weights, dct = mfcc_tables(sample_rate, n_mfcc, n_fft, n_mels, fmin, fmax, x.device)
    B, T = x.shape
    n_fft, hop, n_mels, n_mfcc = int(n_fft), int(block_size), int(n_mels), int(n_mfcc)
    frames = T // hop + 1
    out = torch.empty(B, frames, n_mfcc, dtype=torch.float32, device=x.device)
    ws = _workspace(_lib.query("mfcc_workspace_size", B, T, n_fft, hop, n_mels), x.device)
    _lib.call("mfcc", _lib.ptr(x), _lib.ptr(band_start), _lib.ptr(band_count), _lib.ptr(band_weights),
              band_weights.numel(), _lib.ptr(dct), _lib.ptr(out), B, T, n_fft, hop, n_mels, n_mfcc, float(top_db),
              _lib.ptr(ws), ws.numel(), _lib.stream_of(x))
    db = ws[:4 * B * frames * n_mels].view(torch.float32).view(B, frames, n_mels)  # D before the clamp
    if one_d:
        out, db = out[0], db[0]
    return (out, db) if return_db else out


def _reverb_apply_launch(x, spectrum, ir_length):
    """-> (out, workspace); on return the workspace's first reverb_input_spectra_bytes hold x's
    partition spectra (reused by the backward)."""
    B, T = x.shape[0], x.shape[1]
    if spectrum.numel() != reverb_spectrum_floats(T, ir_length):
        raise RuntimeError("reverb_apply: spectrum was computed for a different length")
    xc = _c(x)
    out = torch.empty(B, T, 1, dtype=torch.float32, device=x.device)
    ws = _workspace(_lib.query("reverb_workspace_size", B, T, int(ir_length)), x.device)
    _lib.call("reverb_apply", _lib.ptr(xc), _lib.ptr(spectrum), _lib.ptr(out), B, T, int(ir_length),
              _lib.ptr(ws), ws.numel(), _lib.stream_of(out))
    return out, ws


# ------------------------------------------------------------------------------------
# seamless realtime streaming (ddsp_hip_stream_*): K calls of N samples render what one call of
# K N samples renders — the oscillator phase carried between calls, a reverb with its full IR
# ------------------------------------------------------------------------------------
class _DeviceState:
    """What the stream states share: ``buf``, zero-filled uint8 on a HIP device, and ``counter``, int64[1] beside it
    (a fresh one, or another state's to share); ``reset()`` zeroes both."""

    @staticmethod
    def _hip_device(device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("ddsp_hip: the stream state lives on a HIP device (no CPU fallback)")
        return device

    def _allocate(self, nbytes, device, counter=None):
        self.buf = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        if counter is None:
            counter = torch.zeros(1, dtype=torch.int64, device=device)
        elif counter.dtype != torch.int64 or counter.numel() != 1 or counter.device != self.buf.device:
            raise RuntimeError(f"{type(self).__name__}: counter must be an int64[1] tensor on the state's device")
        self.counter = counter

    def reset(self):
        self.buf.zero_()
        self.counter.zero_()


class StreamState(_DeviceState):
    """The device state of one realtime stream: ``buf`` (uint8, ddsp_hip_stream_state_bytes: the phase
    carry per item, then — with ``ir_length`` > 0 — the streamed reverb's input history and its ring of
    block spectra) and ``counter`` (int64[1], the call index: Philox offset and ring slot).  Zero-filled
    is a fresh stream."""

    def __init__(self, batch, device, call_samples=0, ir_length=0):
        self.batch, self.call_samples, self.ir_length = int(batch), int(call_samples), int(ir_length)
        if self.batch < 1:
            raise RuntimeError("StreamState: batch must be at least 1")
        nbytes = int(_lib.query("stream_state_bytes", self.batch, self.call_samples, self.ir_length))
        if nbytes == 0:
            raise RuntimeError("StreamState: the streamed reverb takes calls of a power-of-two size in "
                               f"[64, 2048] samples; got {self.call_samples}")
        self._allocate(nbytes, self._hip_device(device))

    @property
    def carry(self):
        """float64 [batch] view of the running phase prefix (writable: a preset phase)."""
        return self.buf[:8 * self.batch].view(torch.float64)


def stream_spectrum(impulse, call_samples):
    """The streamed reverb's IR partition spectra for calls of ``call_samples``: the impulse
    (Reverb.build_impulse, any shape, L values) at its full length, never cropped to the call."""
    _dev(impulse)
    h = _c(impulse.reshape(-1))
    floats = int(_lib.query("stream_spectrum_floats", int(call_samples), h.numel()))
    if floats == 0:
        raise RuntimeError("stream_spectrum: call_samples must be a power of two in [64, 2048] and the "
                           f"impulse non-empty; got {int(call_samples)}, {h.numel()} taps")
    spec = torch.empty(floats, dtype=torch.float32, device=h.device)
    _lib.call("stream_spectrum", _lib.ptr(h), h.numel(), int(call_samples), _lib.ptr(spec), floats,
              _lib.stream_of(h))
    return spec


def stream_synth_frames(f0, param, mags, block_size, sample_rate, state, seed=0, bias=-5.0, noise=None,
                        wrap=True, parts=False):
    """synth_frames for one call of a stream: frame f starts from the phase ``state.carry[b]`` plus its own
    prefix within the call (``wrap``: the carry taken modulo 2 pi).  ``noise`` [B,F,bs] injected, else
    on-device Philox with (seed, offset = state.counter).  Reads the state; ``stream_advance`` ends the
    call.  -> signal [B, F*bs, 1], with ``parts`` (signal, harmonic, noise).  Inference only."""
    B, F, H, NB, bs, noise = _frame_args(f0, param, mags, noise, block_size, "stream_synth_frames")
    if state.batch != B or state.buf.device != f0.device:
        raise RuntimeError("stream_synth_frames: the stream state is for another batch size or device")
    if not synth_frames_in_envelope(H, NB, bs, B):
        raise RuntimeError("stream_synth_frames: shape outside the fused kernel's envelope")
    out = torch.empty(B, F * bs, 1, dtype=torch.float32, device=f0.device)
    harm = torch.empty_like(out) if parts else None
    nz = torch.empty_like(out) if parts else None
    _lib.call("stream_synth_frames", _lib.ptr(_c(f0)), _lib.ptr(_c(param)), _lib.ptr(_c(mags)), float(bias),
              _lib.ptr(noise), int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(state.counter), _lib.ptr(state.buf),
              state.buf.numel(), int(bool(wrap)), _lib.ptr(out), _lib.ptr(harm), _lib.ptr(nz), B, F, H, NB,
              bs, float(sample_rate), _lib.stream_of(out))
    return (out, harm, nz) if parts else out


def stream_reverb(x, spectrum, state, out=None):
    """One call of the streamed reverb: x [B, N] or [B, N, 1] -> the same shape, such that the calls laid end
    to end are the causal convolution of the whole input with the full impulse (``stream_spectrum``).
    Writes the state's history and ring slot; ``stream_advance`` ends the call.  ``out``: a contiguous buffer of
    x's shape to write to; it may be x itself (in place)."""
    _dev(x, spectrum)
    B, N = x.shape[0], x.shape[1]
    if x.numel() != B * N:
        raise RuntimeError("stream_reverb: x [B, N] or [B, N, 1] expected")
    if state.batch != B or state.call_samples != N or state.ir_length < 1 or state.buf.device != x.device:
        raise RuntimeError("stream_reverb: the stream state is for another batch, call size or device, or has "
                           "no reverb section")
    if out is None:
        out = torch.empty_like(x, memory_format=torch.contiguous_format)
    else:
        _dev(out)
        if out.shape != x.shape or not out.is_contiguous() or out.device != x.device:
            raise RuntimeError("stream_reverb: out must be a contiguous tensor of x's shape on its device")
    _lib.call("stream_reverb", _lib.ptr(_c(x)), _lib.ptr(_c(spectrum)), spectrum.numel(), _lib.ptr(state.counter),
              _lib.ptr(state.buf), state.buf.numel(), _lib.ptr(out), B, N, state.ir_length, _lib.stream_of(out))
    return out


def stream_advance(state, f0=None, block_size=1, sample_rate=1.0, wrap=True):
    """The end of a stream call (one launch): the carry moves on by the call's phase, sum_f bs inc(f0[b,f])
    (``wrap``: modulo 2 pi), and the counter by one.  Without ``f0`` (a stream with no synthesis) the
    counter alone."""
    if f0 is None:
        _lib.call("stream_advance", None, _lib.ptr(state.counter), _lib.ptr(state.buf), state.buf.numel(),
                  int(bool(wrap)), 0, 0, 1, 1.0, _lib.stream_of(state.buf))
        return
    _dev(f0)
    B, F = f0.shape[0], f0.shape[1]
    if f0.shape != (B, F, 1) or state.batch != B or state.buf.device != f0.device:
        raise RuntimeError("stream_advance: f0 [B,F,1] on the state's device and of its batch size expected")
    _lib.call("stream_advance", _lib.ptr(f0.contiguous()), _lib.ptr(state.counter), _lib.ptr(state.buf),
              state.buf.numel(), int(bool(wrap)), B, F, int(block_size), float(sample_rate), _lib.stream_of(f0))


# ------------------------------------------------------------------------------------
# streaming analysis (ddsp_hip_stream_loudness / ddsp_hip_stream_mfcc / ddsp_hip_stream_pitch): the features of a
# stream call by call, the history a window needs carried on the device.  With d = ceil((n_fft / 2) / hop), call k
# of N = R hop samples emits the frames f = k R - d + 1 + j, j < R, of the stream (frame f: the n_fft samples from
# f hop - n_fft / 2, zeros before the stream's start — no reflect padding), i.e. the features lag the offline
# alignment by d - 1 frames.  ddsp_hip_stream_analysis: the loudness and the pitch of one frame length in one launch.
# ------------------------------------------------------------------------------------
def stream_feature_delay(n_fft, hop):
    """d - 1, the frames by which a streamed feature lags the offline alignment (frame f at sample f * hop):
    call k's first frame is k R - (d - 1), d = ceil((n_fft / 2) / hop)."""
    return -(-(int(n_fft) // 2) // int(hop)) - 1


class FeatureStreamState(_DeviceState):
    """The device state of one streamed feature (loudness, MFCC or pitch): ``buf`` (uint8,
    ddsp_hip_stream_features_state_bytes: per item a ring of the carried samples plus one call, then the
    MFCC's running maximum per item) and ``counter`` (int64[1], the call index).  Zero-filled is a fresh
    stream.  ``counter``: another state's counter tensor to share (a ``StreamState``'s, so that one
    ``stream_advance`` ends the call for synthesis and analysis alike); ``reset()`` then zeroes it for both."""

    def __init__(self, batch, device, call_samples, n_fft, hop, counter=None):
        self.batch, self.call_samples, self.n_fft, self.hop = int(batch), int(call_samples), int(n_fft), int(hop)
        device = self._hip_device(device)
        if self.batch < 1:
            raise RuntimeError("FeatureStreamState: batch must be at least 1")
        nbytes = int(_lib.query("stream_features_state_bytes", self.batch, self.call_samples, self.n_fft, self.hop))
        if nbytes == 0:
            raise RuntimeError("FeatureStreamState: n_fft must be a power of two in [16, 4096] and call_samples "
                               f"1 to 32 whole hops; got n_fft {self.n_fft}, call_samples {self.call_samples}, "
                               f"hop {self.hop}")
        self.frames = self.call_samples // self.hop
        self.delay_frames = stream_feature_delay(self.n_fft, self.hop)
        self._allocate(nbytes, device, counter)


def _stream_call_rows(x, state, block_size, n_fft, name):
    """x [B, N] or [B, N, 1] of one call -> contiguous detached [B, N], checked against the state."""
    _dev(x)
    if x.dim() not in (2, 3) or x.numel() != x.shape[0] * x.shape[1]:
        raise RuntimeError(f"{name}: expected one call of audio [batch, samples] or [batch, samples, 1], got "
                           f"{tuple(x.shape)}")
    B, N = x.shape[0], x.shape[1]
    if (state.batch, state.call_samples, state.n_fft, state.hop) != (B, N, int(n_fft), int(block_size)) \
            or state.buf.device != x.device:
        raise RuntimeError(f"{name}: the stream state is for another batch, call size, n_fft, hop or device")
    return _c(x.detach().reshape(B, N))


def stream_loudness(x, sample_rate, block_size, state, n_fft=2048):
    """``extract_loudness`` (ddsp/core.py:81-97) for one call of a stream: x [B, N] or [B, N, 1] (HIP, fp32), the
    stream's next N samples -> [B, N // block_size], the frames the call completes (see above: delayed by
    ``state.delay_frames``).  ``state``: a ``FeatureStreamState(B, device, N, n_fft, block_size)``; the call reads
    its counter and writes its ring, ``stream_advance`` ends the call.  One launch; tables cached as
    ``extract_loudness``'s, no host synchronisation after the first call."""
    xc = _stream_call_rows(x, state, block_size, n_fft, "stream_loudness")
    n_fft = int(n_fft)
    w = _a_weighting(sample_rate, n_fft, xc.device)
    B, N = xc.shape
    out = torch.empty(B, state.frames, dtype=torch.float32, device=xc.device)
    _lib.call("stream_loudness", _lib.ptr(xc), _lib.ptr(w), _lib.ptr(out), _lib.ptr(state.counter),
              _lib.ptr(state.buf), state.buf.numel(), B, N, n_fft, int(block_size), _lib.stream_of(xc))
    return out


def stream_mfcc(x, sample_rate, block_size, state, n_mfcc=30, n_fft=1024, n_mels=128, fmin=20.0, fmax=8000.0,
                top_db=80.0):
    """``mfcc`` (ddsp/preprocess.py:30-32) for one call of a stream: x [B, N] or [B, N, 1] -> [B, N // block_size,
    n_mfcc].  The top_db clamp is causal: against the item's maximum over everything the stream has emitted so
    far (carried in ``state``), which is the offline clamp once the item's loudest frame has passed.  ``state``:
    a ``FeatureStreamState(B, device, N, n_fft, block_size)`` of its own (not the loudness's).  One launch."""
    xc = _stream_call_rows(x, state, block_size, n_fft, "stream_mfcc")
    band_start, band_count, band_weights, dct = mfcc_tables(sample_rate, n_mfcc, n_fft, n_mels, fmin, fmax, xc.device)
    B, N = xc.shape
    out = torch.empty(B, state.frames, int(n_mfcc), dtype=torch.float32, device=xc.device)
    _lib.call("stream_mfcc", _lib.ptr(xc), _lib.ptr(band_start), _lib.ptr(band_count), _lib.ptr(band_weights),
              band_weights.numel(), _lib.ptr(dct), _lib.ptr(out), _lib.ptr(state.counter), _lib.ptr(state.buf),
              state.buf.numel(), B, N, int(n_fft), int(block_size), int(n_mels), int(n_mfcc), float(top_db),
              _lib.stream_of(xc))
    return out


def stream_pitch(x, sample_rate, block_size, state, fmin=50.0, fmax=2000.0, frame_length=2048, threshold=0.1,
                 return_confidence=False, return_period=False):
    """``extract_pitch`` for one call of a stream: x [B, N] or [B, N, 1] -> f0 [B, N // block_size] (and the
    confidence, the period) of the frames the call completes, the stream's own frames (zeros before its start;
    delayed by ``state.delay_frames``).  ``state``: a ``FeatureStreamState(B, device, N, frame_length, block_size)``
    of its own; the call reads its counter and writes its ring, ``stream_advance`` ends the call.  One launch."""
    L = int(frame_length)
    xc = _stream_call_rows(x, state, block_size, L, "stream_pitch")
    tau_min, tau_max = pitch_lags(sample_rate, fmin, fmax, L)
    B, N = xc.shape
    f0, conf, period = _pitch_outputs(B, state.frames, xc.device, return_confidence, return_period)
    _lib.call("stream_pitch", _lib.ptr(xc), _lib.ptr(f0), _lib.ptr(conf), _lib.ptr(period), _lib.ptr(state.counter),
              _lib.ptr(state.buf), state.buf.numel(), B, N, L, int(block_size), tau_min, tau_max, float(sample_rate),
              float(threshold), _lib.stream_of(xc))
    return _pitch_result(f0, conf, period, False)


def stream_analysis(x, sample_rate, block_size, state, fmin=50.0, fmax=2000.0, frame_length=2048, threshold=0.1,
                    return_confidence=False, return_period=False):
    """``stream_loudness(n_fft=frame_length)`` and ``stream_pitch(frame_length=frame_length)`` of one call in ONE
    launch over ONE state (ddsp_hip_stream_analysis): x [B, N] or [B, N, 1] -> (loudness [B, R], f0 [B, R]
    [, confidence] [, period]), R = N // block_size, bit for bit what the two separate calls return (the pitch and
    the loudness frames run side by side in different workgroups of one grid over one shared ring).  ``state``: a
    ``FeatureStreamState(B, device, N, frame_length, block_size)``; the call reads its counter and writes its ring,
    ``stream_advance`` ends the call.  Tables cached as ``stream_loudness``'s, lags as ``pitch_lags``; no host
    synchronisation after the first call."""
    L = int(frame_length)
    xc = _stream_call_rows(x, state, block_size, L, "stream_analysis")
    tau_min, tau_max = pitch_lags(sample_rate, fmin, fmax, L)
    w = _a_weighting(sample_rate, L, xc.device)
    B, N = xc.shape
    loud = torch.empty(B, state.frames, dtype=torch.float32, device=xc.device)
    f0, conf, period = _pitch_outputs(B, state.frames, xc.device, return_confidence, return_period)
    _lib.call("stream_analysis", _lib.ptr(xc), _lib.ptr(w), _lib.ptr(loud), _lib.ptr(f0), _lib.ptr(conf),
              _lib.ptr(period), _lib.ptr(state.counter), _lib.ptr(state.buf), state.buf.numel(), B, N, L,
              int(block_size), tau_min, tau_max, float(sample_rate), float(threshold), _lib.stream_of(xc))
    return (loud,) + tuple(t for t in (f0, conf, period) if t is not None)


def stream_analysis_mfcc(x, sample_rate, block_size, state, pitch=True, fmin=50.0, fmax=2000.0, frame_length=2048,
                         threshold=0.1, return_confidence=False, return_period=False, n_mfcc=30, mfcc_n_fft=1024,
                         n_mels=128, mel_fmin=20.0, mel_fmax=8000.0, top_db=80.0):
    """The streamed loudness, MFCC and (``pitch=True``) YIN pitch of one call in ONE launch over ONE state, on ONE
    time axis (ddsp_hip_stream_analysis_mfcc): x [B, N] or [B, N, 1] -> (loudness [B, R], mfcc [B, R, n_mfcc]
    [, f0 [B, R]] [, confidence] [, period]), R = N // block_size.  Loudness and pitch are ``stream_analysis``'s
    bits (frame length ``frame_length`` = L).  MFCC slot j is the ``mfcc_n_fft`` = M-sample window (M = L or L/2)
    centred in frame j's L-sample window, so all three describe stream frame k R - state.delay_frames + j: the
    bits of ``stream_mfcc(n_fft=M)`` fed the same stream delayed by
    (stream_feature_delay(L) - stream_feature_delay(M)) * block_size samples.  ``fmin`` / ``fmax`` / ``threshold``
    are the pitch's, ``mel_fmin`` / ``mel_fmax`` / ``n_mels`` / ``top_db`` the MFCC's (its clamp causal, its running
    maximum in ``state``).  ``state``: a ``FeatureStreamState(B, device, N, frame_length, block_size)``, the same
    as ``stream_analysis``'s; ``stream_advance`` ends the call.  Tables cached as the neighbours'; no host
    synchronisation after the first call."""
    L, M = int(frame_length), int(mfcc_n_fft)
    xc = _stream_call_rows(x, state, block_size, L, "stream_analysis_mfcc")
    if not pitch and (return_confidence or return_period):
        raise RuntimeError("stream_analysis_mfcc: confidence and period come with pitch=True")
    tau_min, tau_max = pitch_lags(sample_rate, fmin, fmax, L) if pitch else (0, 0)
    w = _a_weighting(sample_rate, L, xc.device)
    band_start, band_count, band_weights, dct = mfcc_tables(sample_rate, n_mfcc, M, n_mels, mel_fmin, mel_fmax,
                                                            xc.device)
    B, N = xc.shape
    loud = torch.empty(B, state.frames, dtype=torch.float32, device=xc.device)
    out = torch.empty(B, state.frames, int(n_mfcc), dtype=torch.float32, device=xc.device)
    f0, conf, period = _pitch_outputs(B, state.frames, xc.device, return_confidence, return_period) if pitch \
        else (None, None, None)
    _lib.call("stream_analysis_mfcc", _lib.ptr(xc), _lib.ptr(w), _lib.ptr(loud), _lib.ptr(band_start),
              _lib.ptr(band_count), _lib.ptr(band_weights), band_weights.numel(), _lib.ptr(dct), _lib.ptr(out),
              _lib.ptr(f0), _lib.ptr(conf), _lib.ptr(period), _lib.ptr(state.counter), _lib.ptr(state.buf),
              state.buf.numel(), B, N, L, M, int(block_size), int(n_mels), int(n_mfcc), float(top_db), tau_min,
              tau_max, float(sample_rate), float(threshold), _lib.stream_of(xc))
    return (loud, out) + tuple(t for t in (f0, conf, period) if t is not None)


# ------------------------------------------------------------------------------------
# streamed Viterbi pitch (ddsp_hip_stream_pitch_salience / ddsp_hip_stream_pitch_viterbi): ``track_pitch`` for a
# stream.  The decode's forward recursion is causal; carried from call to call it gives, at every frame n, the offline
# decode of frames 0 .. n, and its element n - lag is a decision at a fixed, small lag (lag 0: none at all).
# ------------------------------------------------------------------------------------
class ViterbiStreamState(_DeviceState):
    """The device state of one streamed Viterbi decode (include/ddsp_hip.h, "pitch_viterbi_stream"): ``buf`` (uint8,
    ddsp_hip_stream_viterbi_state_bytes: per item the two fp64 rows of delta, then a ring of ``lag`` +
    ``frames_per_call`` frames of f0c, cost and back-offsets) and ``counter`` (int64[1], the call index).
    Zero-filled is a fresh stream.  ``counter``: another state's counter tensor to share (the salience's ring's, a
    ``StreamState``'s), so that one ``stream_advance`` ends the call for all of them; ``reset()`` then zeroes it for
    all."""

    def __init__(self, batch, device, frames_per_call, n_bins, lag=0, counter=None):
        self.batch, self.frames, self.n_bins, self.lag = int(batch), int(frames_per_call), int(n_bins), int(lag)
        device = self._hip_device(device)
        if self.batch < 1:
            raise RuntimeError("ViterbiStreamState: batch must be at least 1")
        nbytes = int(_lib.query("stream_viterbi_state_bytes", self.batch, self.frames, self.n_bins, self.lag))
        if nbytes == 0:
            raise RuntimeError("ViterbiStreamState: 1 to 32 frames per call, 1 to 1024 bins and a lag of 0 to 64 "
                               f"frames; got {self.frames} frames, {self.n_bins} bins, lag {self.lag}")
        self._allocate(nbytes, device, counter)


def stream_pitch_salience(x, sample_rate, block_size, state, fmin=50.0, fmax=2000.0, frame_length=2048,
                          bins_per_octave=48, return_lag=False, return_raw=False, threshold=0.1):
    """``pitch_salience`` for one call of a stream: x [B, N] or [B, N, 1] -> (cost, f0c[, lag]), each
    [B, N // block_size, n_bins], of the frames the call completes — the stream's own frames, ``stream_pitch``'s.
    ``return_raw``: also ``stream_pitch``'s (f0, confidence, period) for ``threshold``, bit for bit, out of the same
    launch.  ``state``: a ``FeatureStreamState(B, device, N, frame_length, block_size)`` of its own; the call reads
    its counter and writes its ring, ``stream_advance`` ends the call.  One launch; bin tables cached as
    ``pitch_salience``'s, no host synchronisation after the first call."""
    L = int(frame_length)
    xc = _stream_call_rows(x, state, block_size, L, "stream_pitch_salience")
    tau_min, tau_max, lo, hi = _pitch_bin_tables(sample_rate, fmin, fmax, L, bins_per_octave, xc.device)
    B, N = xc.shape
    NB = lo.numel()
    out = _salience_outputs(B, state.frames, NB, xc.device, return_lag, return_raw)
    _lib.call("stream_pitch_salience", _lib.ptr(xc), _lib.ptr(lo), _lib.ptr(hi), *map(_lib.ptr, out),
              _lib.ptr(state.counter), _lib.ptr(state.buf), state.buf.numel(), B, N, L, int(block_size), tau_min,
              tau_max, NB, float(sample_rate), float(threshold), _lib.stream_of(xc))
    return tuple(t for t in out if t is not None)


def stream_viterbi_path(cost, f0c, state, transition=0.02, max_jump=12):
    """One call of the carried decode (include/ddsp_hip.h, "pitch_viterbi_stream"): cost, f0c [B, R, n_bins] (HIP,
    fp32) of the call's frames -> (f0, confidence, path), each [B, R]: for emitted frame n = k R + j the decision
    ``state.lag`` frames back, which is element n - lag of ``viterbi_path`` over frames 0 .. n (before frame ``lag``:
    element 0).  ``state``: a ``ViterbiStreamState(B, device, R, n_bins, lag)``; the call reads its counter and
    writes its rows and ring, ``stream_advance`` ends the call, and a call run twice before it gives the same bits.
    One launch, one workgroup per item; no host synchronisation.  No autograd."""
    _dev(cost, f0c)
    if cost.dim() != 3 or cost.shape != f0c.shape:
        raise RuntimeError(f"stream_viterbi_path: cost and f0c must both be [batch, frames, bins], got "
                           f"{tuple(cost.shape)} and {tuple(f0c.shape)}")
    B, R, NB = cost.shape
    if (state.batch, state.frames, state.n_bins) != (B, R, NB) or state.buf.device != cost.device:
        raise RuntimeError("stream_viterbi_path: the decode state is for another batch, frames per call, bin count "
                           "or device")
    c, g = _c(cost.detach()), _c(f0c.detach())
    f0 = torch.empty(B, R, dtype=torch.float32, device=c.device)
    conf = torch.empty_like(f0)
    path = torch.empty(B, R, dtype=torch.int32, device=c.device)
    _lib.call("stream_pitch_viterbi", _lib.ptr(c), _lib.ptr(g), _lib.ptr(f0), _lib.ptr(conf), _lib.ptr(path),
              _lib.ptr(state.counter), _lib.ptr(state.buf), state.buf.numel(), B, R, NB, int(max_jump), state.lag,
              float(transition), _lib.stream_of(c))
    return f0, conf, path


def stream_track_pitch(x, sample_rate, block_size, ring_state, viterbi_state, fmin=50.0, fmax=2000.0,
                       frame_length=2048, bins_per_octave=48, transition=0.02, max_jump=12, return_confidence=False,
                       return_path=False):
    """``track_pitch`` for one call of a stream: ``stream_pitch_salience`` over ``ring_state`` then
    ``stream_viterbi_path`` over ``viterbi_state`` — x [B, N] or [B, N, 1] -> f0 [B, N // block_size] (and on
    request the confidence and the path's bins).  Slot j of call k is the decision for stream frame
    k R - ring_state.delay_frames + j - viterbi_state.lag: the streamed features' delay plus the decode's lag (0
    already removes the octave jumps of ``stream_pitch``; a few frames bring the decision to the offline path's).
    The two states share a counter (``ViterbiStreamState(..., counter=ring_state.counter)``) or are advanced
    together; ``stream_advance`` ends the call.  Two launches, no host synchronisation after the first call."""
    cost, f0c = stream_pitch_salience(x, sample_rate, block_size, ring_state, fmin=fmin, fmax=fmax,
                                      frame_length=frame_length, bins_per_octave=bins_per_octave)
    f0, conf, path = stream_viterbi_path(cost, f0c, viterbi_state, transition=transition, max_jump=max_jump)
    return _pitch_result(f0, conf if return_confidence else None, path if return_path else None, False)


def stream_pitch_bin_count(sample_rate, fmin=50.0, fmax=2000.0, frame_length=2048, bins_per_octave=48):
    """n_bins of ``pitch_bins`` for these parameters: what a ``ViterbiStreamState`` is sized by."""
    tau_min, tau_max = pitch_lags(sample_rate, fmin, fmax, frame_length)
    return len(_pitch_bin_arrays(tau_min, tau_max, bins_per_octave)[0])


from . import grad as _grad  # noqa: E402  (autograd Functions over the backward kernels)


_MASKED_STREAMS = {}


@atexit.register
def _release_masked_streams():
    """Destroy the CU-masked streams before the HIP runtime tears down (left to the runtime's own
    teardown they crashed rocprofv3's finalisation)."""
    if not _MASKED_STREAMS:
        return
    try:
        torch.cuda.synchronize()
        lib = _lib.load()
        for s in _MASKED_STREAMS.values():
            lib.ddsp_hip_stream_destroy(s.cuda_stream)
    except Exception:  # teardown path: nothing left to report to
        pass
    _MASKED_STREAMS.clear()


def cu_mask_words(cus, n_cu):
    """The 32-bit mask words of ddsp_hip_stream_create_cu_masked: bit c of word c // 32 set for
    every CU index c in ``cus`` (indices must lie in [0, n_cu))."""
    words = [0] * ((int(n_cu) + 31) // 32)
    for c in cus:
        c = int(c)
        if not 0 <= c < n_cu:
            raise ValueError(f"CU index {c} outside [0, {n_cu})")
        words[c // 32] |= 1 << (c % 32)
    return words


def cu_masked_stream(cus, n_cu=None):
    """A torch stream whose kernels run only on the CUs with the given indices
    (ddsp_hip_stream_create_cu_masked; see synth.PipelinedSynthPath for how indices map to XCDs).
    One stream per (device, mask), kept for the life of the process: the caching allocator may
    still hold blocks tagged with it, so it is never destroyed under them."""
    dev = torch.cuda.current_device()
    cus = tuple(sorted(set(int(c) for c in cus)))
    n_cu = n_cu or torch.cuda.get_device_properties(dev).multi_processor_count
    if not cus or cus[0] < 0 or cus[-1] >= n_cu:
        raise ValueError("CU indices out of range")
    key = (dev, cus)
    if key not in _MASKED_STREAMS:
        words = (ctypes.c_uint32 * ((n_cu + 31) // 32))(*cu_mask_words(cus, n_cu))
        handle = ctypes.c_void_p()
        _lib.call("stream_create_cu_masked", words, len(words), ctypes.byref(handle))
        _MASKED_STREAMS[key] = torch.cuda.ExternalStream(handle.value, device=torch.device("cuda", dev))
    return _MASKED_STREAMS[key]
