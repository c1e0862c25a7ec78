"""The yardstick of the forward synthesis kernels (``csrc/synth_frame.hip``: synth_frame_kernel / frame_synth, and
outside its envelope ``synth.hip``: harmonic_frames_kernel, ``noise.hip``: filtered_noise_kernel): the shape cases
that reach the kernels' branches, fp64 references of every output PER FRAME, the per-frame error metric, a CPU model
of the oscillator bank's summation order, and a Python restatement of the kernels' shape arithmetic.  Test
infrastructure only (numpy, torch on the CPU, no device code); shared by tests/test_synth_ref.py (which ties it to
the goldens and to the fp32 oracle, and proves each case onto its branch) and tests/test_gpu_synth_shapes.py.

The references follow ``oracle/numpy_oracle.py`` step by step and keep the reference's fp32 rounding points, the
values a kernel has to reproduce bit for bit before any smooth arithmetic starts:

* the Nyquist decision ``fl32(f0 * k) < sr / 2`` with the fp32 mask values ``1.0001f`` / ``1e-4f``;
* the fp32 phase ``omega = fl32(sum of the fp32 increments)`` (numpy_oracle.phase) and the product
  ``fl32(omega * k)``;
* the scalar constants ATen casts to fp32 (the exponent ``fl32(ln 10)`` and ``1e-7f`` of scale_function) and the
  fp32 sum ``fl32(magnitudes + bias)`` ahead of it, an exact operation of the inputs that has one result.

Everything after those points (scale function, normalisation, sines, the irfft, window and convolution, every sum)
runs in fp64.

The metric is max_j |got - ref| of a frame against the frame's condition scale from the reference: sum_k |A_k| for
the harmonic part (|sin| <= 1), sum_m |h_m| for the filtered noise (|x| <= 1), their sum for the signal.

Tolerances (the issue behind this file fixes how they are derived; the derivation is asserted in
tests/test_synth_ref.py on every case):

* HARM_FRAME_TOL = 2e-6, one constant for every case: 3.4e-7 (the hardware sine's recorded error of 3.2e-7,
  tools/sin_probe.hip, and the argument reduction's roundings; tests/test_gpu_shared_reduction.py asserts it per
  term, and sum |A_k| eps <= scale eps) + 2 x the sequential fp32 model's largest per-frame error (8.11e-7, at
  H = 1024) = 1.96e-6, rounded up to one digit; its cap is 3e-6.  The factor 2: the kernel rounds once per FMA
  where the model rounds twice, but its partial sums differ in sign pattern.  (Taken literally,
  "2 pi ulp(8.0f)" is 6.0e-6 and would carry the constant past the cap by itself; 3.4e-7 is the figure the model's
  share, (HARM_FRAME_TOL - 3.4e-7) / 2 = 8.3e-7, is worked out with, and the tighter reading.)
  The model sums in the kernels' order, DESCENDING k.  The kernels used to sum in ascending k, and in that order
  the model misses its share on "transition" (H = 1024 at a constant 20 kHz): harmonic 1 alone is audible and is
  0.9 of the scale, and the 1023 masked harmonics (1e-4 each) are added one by one to a sum of that size, each
  addition rounding at its ulp: 3.4e-6 in the worst frame, 1.4e-6 in the median one (3.0e-6 to 3.7e-6 over five
  other draws), and the device measured 3.35e-6.  Small terms first it is 5.4e-7; test_synth_ref.py keeps both
  figures (test_summation_order).
* NOISE_FRAME_TOL = 1.28e-6 = 4 x the fp32 torch oracle's largest per-frame error over the cases (3.0e-7 on the
  host that measured it, taken as 3.2e-7: see NOISE_ORACLE_MAX), cap 1.5e-6: the kernels form taps by a direct cosine sum of up to NB terms and filter by a direct FIR of up to n
  taps, sequential fp32 sums, where the oracle's FFTs grow with log n.  N5b has a bound of its own (NOISE_OWN_ORACLE).
* signal: the two bounds weighted by the two scales, plus one ulp (2^-23) of the sum.
* controls: rtol 1e-6 (amplitudes, magnitudes), rtol 2e-6 + atol 1e-12 (distribution), as
  tests/test_gpu_parity.py::test_synth_frames_controls_output.
"""
import functools
import math
import zlib

import numpy as np
import torch

from oracle import numpy_oracle as no
from oracle import philox
from oracle import torch_ref as tr

f32, f64 = np.float32, np.float64
SR = 48000
BIAS = -5.0
PHILOX_SEED, PHILOX_OFFSET = 77, 2 ** 32 + 5

SINE_TERM = 3.4e-7  # hardware sine + argument reduction, per term against |A_k| (see above)
HARM_MODEL_MAX = 8.11e-7  # the sequential model's largest per-frame error, as measured (Hcap); numpy's fp64 sine
HARM_FRAME_TOL = 2e-6  # SINE_TERM + 2 HARM_MODEL_MAX = 1.96e-6, rounded up to one significant digit
HARM_FRAME_CAP = 3e-6
HARM_MODEL_SHARE = (HARM_FRAME_TOL - SINE_TERM) / 2  # what the sequential fp32 model may use of it: 8.3e-7
# The fp32 torch oracle's largest per-frame error bar NOISE_OWN's cases.  It depends on the host's FFT library:
# 2.99e-7 (transition) on the host these figures were taken on, 2.56e-7 (N7) on another.  The constant is the larger
# with 7% over it for a third library, since a host whose oracle is worse must not fail the CPU test.
NOISE_ORACLE_MAX = 3.2e-7
NOISE_FRAME_TOL = 4 * NOISE_ORACLE_MAX
NOISE_FRAME_CAP = 1.5e-6
# A case whose oracle error alone would carry NOISE_FRAME_TOL past its cap has a bound of its own, 4 x its own
# oracle error: N5b (n = 128 taps cropped to a block of 8, a filter whose L1 norm is 2e-7 to 7e-5 while the
# oracle's 16-point FFTs round against the uncropped magnitudes): oracle 7.3e-7 on one host, 7.1e-7 on another,
# taken with the same margin.
NOISE_OWN_ORACLE = {"N5b": 7.8e-7}


def noise_tol(name):
    base = name.partition("/")[0]
    return 4 * NOISE_OWN_ORACLE[base] if base in NOISE_OWN_ORACLE else NOISE_FRAME_TOL


def noise_oracle_share(name):
    return noise_tol(name) / 4


SUM_ULP = 2.0 ** -23
CTRL_TOL = {"amplitudes": (1e-6, 0.0), "harmonic_distribution": (2e-6, 1e-12), "magnitudes": (1e-6, 0.0)}

# the kernels' constants (csrc/common.h, csrc/synth_frame.hip, ddsp_pytorch_amd/core.py)
FAST_ARG_LIMIT = f32(8.0e6)
SHARED_REV_LIMIT = f32(8.0)
INV_2PI = f32(0.159154936671257019043)
FRAME_PREFIX_MIN_FRAMES = 512
SPLIT_MAX_FRAMES = 512  # frame_plan: B * F < 512 is split

# ------------------------------------------------------------------------------------------ the cases
# name -> (H, NB, bs, B, F, pitch); what each reaches is tabulated in tests/test_gpu_synth_shapes.py
FUSED_CASES = {
    "config": (100, 65, 512, 2, 256, "low"),
    "N2": (64, 65, 256, 8, 64, "low"),
    "N2b": (8, 65, 260, 8, 64, "low"),
    "N3a": (8, 65, 192, 8, 64, "low"),
    "N3b": (8, 65, 188, 8, 64, "low"),
    "N4": (8, 65, 128, 8, 64, "low"),
    "N5a": (8, 65, 64, 8, 64, "low"),
    "N5b": (8, 65, 8, 8, 64, "low"),
    "N6": (17, 18, 64, 8, 64, "low"),
    "N6b": (17, 18, 36, 8, 64, "low"),
    "N7": (1, 2, 4, 8, 64, "low"),
    "N8": (4, 33, 64, 8, 64, "low"),
    "N9": (128, 513, 1024, 8, 64, "low"),
    "N10": (4, 1025, 1024, 8, 64, "low"),
    "Hcap": (1024, 9, 64, 8, 64, "sub"),
    "H12": (12, 9, 64, 8, 64, "low"),
    "persample": (100, 9, 64, 8, 64, "high"),
    "transition": (1024, 9, 64, 1, 512, "20k"),
    "transition_shared": (8, 9, 1024, 1, 512, "21k"),
    "nyquist": (48, 9, 64, 8, 64, "nyquist"),
}
PREFIX_CASES = ("config", "N6", "persample")  # run again as "<name>/prefix": B = 1, F = PREFIX_FRAMES
PREFIX_FRAMES = 520
PHILOX_CASES = ("config", "N5a", "N5b", "N6")  # run again as "<name>/philox": noise = None, pinned seed and offset

# the two module kernels outside the fused envelope: name -> (H, NB, bs); B = 2, F = 5 (4 frames per noise
# workgroup: the last one is partly empty)
FALLBACK_CASES = {
    "F441": (17, 65, 441),
    "F30": (5, 33, 30),
    "F6": (3, 2, 6),
    "F1": (3, 65, 1),
    "F2048": (8, 33, 2048),
    "F255": (8, 33, 255),
    "F256": (8, 65, 256),
    "F36": (4, 9, 36),
    "F35": (4, 18, 35),
    "F128": (9, 9, 128),
    "F129": (9, 9, 129),
    "F130": (9, 9, 130),
    "F1028": (4, 65, 1028),
    "Fslow": (1024, 9, 441),
}
FALLBACK_BF = (2, 5)
# Fslow: one item of 13 frames at a constant 20 kHz: |omega| H4 passes kFastArgLimit in frame 6, so frames 0-5 take
# harmonic_frames_kernel's fast loop, frame 6 both loops and frames 7-12 its general loop with sin_slow
FALLBACK_OWN = {"Fslow": (1, 13, "20k")}


def fallback_shape(name):
    """(B, F, pitch) of a module-kernel case"""
    return FALLBACK_OWN.get(name, FALLBACK_BF + ("low",))

# pitches whose product with some k <= 48 is exactly sr / 2 in fp32 (24000 / k for k = 48, 24, 12, 2, 3, 5, 16, 25)
NYQUIST_EXACT = (500.0, 1000.0, 2000.0, 12000.0, 8000.0, 4800.0, 1500.0, 960.0)
NYQUIST_ALL_MASKED = 30000.0


def all_fused_names():
    return (list(FUSED_CASES) + [f"{n}/prefix" for n in PREFIX_CASES] + [f"{n}/philox" for n in PHILOX_CASES])


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def nyquist_pitches(B, F, gen):
    """frames 0-1 silent from the start (the phase stays 0: exactly zero output), then for every special pitch v
    the fp32 values just below, at and just above it, one silent frame after the phase has moved, random fill"""
    f0 = (50.0 * 20.0 ** torch.rand(B, F, 1, generator=gen)).numpy().astype(f32)
    col = [0.0, 0.0]
    for v in NYQUIST_EXACT + (NYQUIST_ALL_MASKED,):
        v = f32(v)
        col += [np.nextafter(v, f32(0)), v, np.nextafter(v, f32(1e9))]
    col += [0.0]
    assert len(col) <= F
    f0[:, :len(col), 0] = np.asarray(col, dtype=f32)
    return f0


def _pitches(kind, B, F, gen):
    if kind == "low":  # 50 Hz - 1 kHz per frame, as the VJP sweep
        return (50.0 * 20.0 ** torch.rand(B, F, 1, generator=gen)).numpy().astype(f32)
    if kind == "sub":  # 12 - 23 Hz: all of 1024 harmonics below Nyquist
        return (12.0 * (23.0 / 12.0) ** torch.rand(B, F, 1, generator=gen)).numpy().astype(f32)
    if kind == "high":  # log-uniform 3 - 9 kHz
        return (3000.0 * 3.0 ** torch.rand(B, F, 1, generator=gen)).numpy().astype(f32)
    if kind == "20k":
        return np.full((B, F, 1), 20000.0, dtype=f32)
    if kind == "21k":
        return np.full((B, F, 1), 21000.0, dtype=f32)
    if kind == "nyquist":
        return nyquist_pitches(B, F, gen)
    raise KeyError(kind)


def make_inputs(name, H, NB, bs, B, F, pitch):
    """f0 [B,F,1], param [B,F,H+1], mags [B,F,NB] raw randn, noise [B,F,bs] U[-1,1): fp32 numpy, seeded by name"""
    gen = torch.Generator().manual_seed(_seed(name))
    f0 = _pitches(pitch, B, F, gen)
    param = torch.randn(B, F, H + 1, generator=gen).numpy()
    mags = torch.randn(B, F, NB, generator=gen).numpy()
    noise = (torch.rand(B, F, bs, generator=gen) * 2 - 1).numpy()
    return dict(f0=f0, param=param, mags=mags, noise=noise)


def philox_noise(B, F, bs, seed=PHILOX_SEED, offset=PHILOX_OFFSET):
    return np.ascontiguousarray(philox.device_noise(B, F, bs, seed, offset))


# ------------------------------------------------------------------------------------------ the references
def scale64(x):
    """ddsp/core.py:77-78 in fp64 with the scalars as ATen casts them next to an fp32 tensor"""
    sig = 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=f64)))
    return 2.0 * sig ** float(no.LN10_F32) + float(f32(1e-7))


def harmonic_controls64(f0, param, sr=SR):
    """modules.py:44-73 -> (amplitudes [B,F,1], A = distribution * amplitudes [B,F,H]) fp64; the Nyquist decision
    on the fp32 product (numpy_oracle.remove_above_nyquist)"""
    f0 = np.asarray(f0, dtype=f32)
    p = np.asarray(param, dtype=f64)
    H = p.shape[-1] - 1
    amp = scale64(p[..., :1])
    pitches = f0 * np.arange(1, H + 1, dtype=f32)
    assert pitches.dtype == f32
    mask = np.where(pitches < f32(sr / 2), float(f32(1.0) + f32(1e-4)), float(f32(0.0) + f32(1e-4)))
    d = scale64(p[..., 1:]) * mask
    d = d / d.sum(-1, keepdims=True)
    return amp, d * amp


def frame_phase(f0, bs, sr=SR):
    """fp32 omega [B, F, bs] (numpy_oracle.phase of the upsampled pitch)"""
    B, F = f0.shape[:2]
    return no.phase(no.upsample(np.asarray(f0, dtype=f32), bs), sr).reshape(B, F, bs)


def oscillator_ref(f0, A, bs, sr=SR, model=True, descending=True):
    """sum_k A_k sin(fl32(omega k)) per sample for A [B,F,H] fp64 -> (fp64 reference [B,F,bs], sequential model).

    The model accumulates fl32(A_k) * sin(fl32 argument) in fp32, one term after the other, each product and each
    sum rounded, with the correctly rounded fp32 sine: the summation order of the kernels' oscillator loops and
    nothing else.  ``descending`` (the kernels' order: the highest harmonic first) or ascending k."""
    omega = frame_phase(f0, bs, sr)
    A = np.asarray(A, dtype=f64)
    A32 = A.astype(f32)
    ref = np.zeros(omega.shape, dtype=f64)
    seq = np.zeros(omega.shape, dtype=f32) if model else None
    H = A.shape[-1]
    for k in (range(H, 0, -1) if descending else range(1, H + 1)):
        arg = omega * f32(k)
        s = np.sin(arg.astype(f64))
        ref += A[:, :, None, k - 1] * s
        if model:
            seq = seq + A32[:, :, None, k - 1] * s.astype(f32)
    return ref, seq


def impulse_response64(A, target):
    """numpy_oracle.amp_to_impulse_response without its final rounding: fp64 taps [.., target]"""
    imp = np.fft.irfft(np.asarray(A, dtype=f64), axis=-1)
    n = imp.shape[-1]
    imp = np.roll(imp, n // 2, axis=-1) * no.hann_window(n)
    if target >= n:
        imp = np.pad(imp, [(0, 0)] * (imp.ndim - 1) + [(0, target - n)])
    else:
        imp = imp[..., :target]
    return np.roll(imp, -n // 2, axis=-1)


def convolve64(x, h):
    """numpy_oracle.fft_convolve in fp64 without its final rounding: y[j] = sum_{m<=j} h[m] x[j-m]"""
    N = x.shape[-1]
    nfft = 2 * N
    y = np.fft.irfft(np.fft.rfft(np.asarray(x, dtype=f64), nfft, axis=-1) *
                     np.fft.rfft(np.asarray(h, dtype=f64), nfft, axis=-1), nfft, axis=-1)
    return y[..., :N]


def noise_ref(mags, noise, bs, bias=BIAS):
    """-> (filtered noise [B,F,bs], taps h [B,F,bs], magnitudes [B,F,NB]) fp64.  bias None: mags are the scaled
    magnitudes already."""
    if bias is None:
        m = np.asarray(mags, dtype=f64)
    else:
        x = np.asarray(mags, dtype=f32) + f32(bias)
        assert x.dtype == f32
        m = scale64(x)
    h = impulse_response64(m, bs)
    return convolve64(noise, h), h, m


def oracle32_noise(mags, noise, bs, bias=BIAS):
    """the fp32 torch oracle's filtered noise [B,F,bs]"""
    m = torch.from_numpy(np.ascontiguousarray(mags))
    with torch.no_grad():
        m = tr.scale_function(m + bias) if bias is not None else m
        y = tr.noise_forward(m, torch.from_numpy(np.ascontiguousarray(noise)), bs)
    return y.reshape(mags.shape[0], mags.shape[1], bs).numpy()


def _with_refs(c, inp, bs, noise):
    amp, A = harmonic_controls64(inp["f0"], inp["param"])
    harm, seq = oscillator_ref(inp["f0"], A, bs)
    nz, h, m = noise_ref(inp["mags"], noise, bs)
    c.update(inp, noise=noise, harm_ref=harm, harm_model=seq, noise_ref=nz, A=A, h=h, amplitudes=amp, magnitudes=m,
             harm_scale=np.abs(A).sum(-1), noise_scale=np.abs(h).sum(-1))
    return c


@functools.lru_cache(maxsize=None)
def fused_case(name):
    """Inputs (fp32 numpy) and fp64 references of a fused case; computed once, never modified.  "<base>/prefix"
    is the base's shape at B = 1, F = PREFIX_FRAMES with inputs of its own; "<base>/philox" the base's inputs
    with the device's Philox noise."""
    base, _, variant = name.partition("/")
    H, NB, bs, B, F, pitch = FUSED_CASES[base]
    if variant == "prefix":
        B, F = 1, PREFIX_FRAMES
    c = dict(name=name, H=H, NB=NB, bs=bs, B=B, F=F, variant=variant)
    if variant == "philox":
        b = fused_case(base)
        nz, h, m = noise_ref(b["mags"], philox_noise(B, F, bs), bs)
        c.update({k: v for k, v in b.items() if k not in c})
        c.update(noise=philox_noise(B, F, bs), noise_ref=nz, h=h, magnitudes=m, noise_scale=np.abs(h).sum(-1))
        return c
    inp = make_inputs(name, H, NB, bs, B, F, pitch)
    return _with_refs(c, inp, bs, inp["noise"])


@functools.lru_cache(maxsize=None)
def fallback_case(name):
    """Inputs and references of a case of the two module kernels: the harmonic part, and the filtered noise for
    injected and Philox noise, from raw magnitudes (bias -5) and from pre-scaled ones (c["scaled"], fp32)."""
    H, NB, bs = FALLBACK_CASES[name]
    B, F, pitch = fallback_shape(name)
    inp = make_inputs(name, H, NB, bs, B, F, pitch)
    c = _with_refs(dict(name=name, H=H, NB=NB, bs=bs, B=B, F=F), inp, bs, inp["noise"])
    c["scaled"] = c["magnitudes"].astype(f32)
    c["philox"] = philox_noise(B, F, bs)
    c["noise_refs"] = {}
    for kind, x in (("inject", c["noise"]), ("philox", c["philox"])):
        for raw in (True, False):
            nz, h, _ = noise_ref(inp["mags"] if raw else c["scaled"], x, bs, BIAS if raw else None)
            c["noise_refs"][kind, raw] = (nz, np.abs(h).sum(-1))
    return c


# ------------------------------------------------------------------------------------------ the metric
def _np(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=f64)


def frame_err(got, ref, scale):
    """[B, F, bs] (or [B, F*bs, 1]) against ref [B, F, bs] and scale [B, F] -> [B, F] float64:
    max_j |got - ref| / scale of each frame.  A frame whose scale is exactly zero must be exactly zero in ``got``:
    0 there if it is, inf if it is not."""
    ref, scale = _np(ref), _np(scale)
    got = _np(got).reshape(ref.shape)
    assert scale.shape == ref.shape[:2], (scale.shape, ref.shape)
    num = np.abs(got - ref).max(-1)
    num = np.where(np.isnan(num), np.inf, num)
    zero = scale == 0
    out = num / np.where(zero, 1.0, scale)
    return np.where(zero, np.where(num == 0, 0.0, np.inf), out)


def signal_err(got, c):
    """the signal's per-frame error as a fraction of its per-frame bound (<= 1 passes): the two parts' bounds
    weighted by their scales, plus one ulp of the sum"""
    sa, sh = c["harm_scale"], c["noise_scale"]
    e = frame_err(got, c["harm_ref"] + c["noise_ref"], sa + sh)
    bound = (HARM_FRAME_TOL * sa + noise_tol(c["name"]) * sh) / (sa + sh) + SUM_ULP
    return e / bound


def control_err(got, ref, which):
    """largest |got - ref| / (atol + rtol |ref|) over the tensor (<= 1 passes)"""
    rtol, atol = CTRL_TOL[which]
    ref = _np(ref)
    got = _np(got).reshape(ref.shape)
    d = np.abs(got - ref)
    d = np.where(np.isnan(d), np.inf, d)
    return float((d / (atol + rtol * np.abs(ref))).max())


# ------------------------------------------------------------------------------------------ the kernels' shapes
def roundup4(v):
    return (v + 3) & ~3


def frame_shape(NB, bs):
    """synth_frame.hip frame_shape and the two tests frame_synth makes on it"""
    n = 2 * (NB - 1)
    half = n // 2
    lo_end = tail_start = bs
    two_run = bs >= n and bs - half >= roundup4(half)
    if two_run:
        lo_end, tail_start = roundup4(half), bs - half
    dpp_tail = bs - tail_start == 64 and bs - 127 >= lo_end
    return dict(n=n, half=half, lo_end=lo_end, tail_start=tail_start, pad=(lo_end + 4 + 3) & ~3, two_run=two_run,
                dpp_tail=dpp_tail)


def in_envelope(H, NB, bs, B=1):
    return not (bs % 4 or bs > 1024 or H > 1024 or NB > 1025 or B > 65535) and H >= 1 and NB >= 2 and bs >= 4


def frame_plan(B, F, H, NB, bs):
    """synth_frame.hip frame_plan as core._synth_frames_launch drives it -> nt, G (> 1: the SPLIT kernels), NT
    (the threads of the group that builds a frame), prefix (the PREFIX kernels), irfft ("pair" / "general": frame_synth's
    choice between the lane-pair irfft and irfft_tap)"""
    assert in_envelope(H, NB, bs, B)
    prefix = F > FRAME_PREFIX_MIN_FRAMES
    nt = max(64, (bs // 4 + 63) // 64 * 64)
    G = max(1, min(4, 256 // nt)) if (not prefix and B * F < SPLIT_MAX_FRAMES) else 1
    NT = nt * G
    n = 2 * (NB - 1)
    # the lane-pair irfft goes by the launch's width: a block of 256 or less takes it in the SPLIT form only, and
    # irfft_tap with irfft128_tap32 (the lane-pair path's summation tree for tap 32) otherwise
    return dict(nt=nt, G=G, NT=NT, prefix=prefix, irfft="pair" if (n == 128 and NT >= 128) else "general")


def shared_rev_frame(f0, H):
    """[B, F] bool: the frame takes the shared-count loop where its quads are fast (fp32, as the kernel)"""
    H4 = roundup4(H)
    dinc = no.phase_increment(np.asarray(f0, dtype=f32)[..., 0], SR)
    v = f32(0.5) + f32(2.0) * f32(H4) * np.abs(dinc) * INV_2PI
    assert v.dtype == f32
    return v < SHARED_REV_LIMIT


def shared_rev_margin(f0, H):
    """|bound - limit| / limit per frame: how far a frame is from the guard (a frame within an ulp of it could
    take either loop under a fused multiply-add)"""
    H4 = roundup4(H)
    dinc = no.phase_increment(np.asarray(f0, dtype=f32)[..., 0], SR).astype(f64)
    return np.abs(0.5 + 2.0 * H4 * np.abs(dinc) / (2 * math.pi) - 8.0) / 8.0


def fast_quads(f0, H, bs):
    """[B, F, bs/4] bool: all four samples of the quad satisfy |omega| H4 < kFastArgLimit in fp32"""
    H4 = roundup4(H)
    w = frame_phase(f0, bs)
    p = np.abs(w) * f32(H4)
    assert p.dtype == f32
    B, F = w.shape[:2]
    return (p < FAST_ARG_LIMIT).reshape(B, F, bs // 4, 4).all(-1)


def loops(f0, H, bs):
    """per frame, which oscillator loops its quads take: [B, F] arrays "shared", "persample", "general" (bool)"""
    fq = fast_quads(f0, H, bs)
    sh = shared_rev_frame(f0, H)
    any_fast, any_slow = fq.any(-1), (~fq).any(-1)
    return dict(shared=any_fast & sh, persample=any_fast & ~sh, general=any_slow)


def split_slice(name):
    """(items, frames) of the SPLIT launch of a fused case, or None where the shape has none (nt = 256)"""
    base = name.partition("/")[0]
    H, NB, bs, B, F, _ = FUSED_CASES[base]
    if name.endswith("/prefix") or max(64, (bs // 4 + 63) // 64 * 64) > 128:
        return None
    items = (SPLIT_MAX_FRAMES - 1) // F
    if items >= 1:
        return min(items, B), F
    return 1, 128  # one item of 512 frames: its first 128 (a frame's phase depends on the frames before it only)


def harmonic_fallback_plan(bs):
    """synth.hip launch_frames -> (SPT, nt, passes)"""
    if bs >= 256:
        spt, nt = 4, min(256, (bs // 4 + 63) // 64 * 64)
    else:
        spt, nt = 2, max(64, (bs // 2 + 63) // 64 * 64)
    return spt, nt, -(-bs // (nt * spt))


def noise_fallback_plan(NB, bs):
    """noise.hip filtered_noise_launch and the kernel's data-dependent branches"""
    n = 2 * (NB - 1)
    half = n // 2
    bs8 = (bs + 7) & ~7
    if bs >= n:
        lo_end, tail_start = roundup4(half), bs - half
        layout = "two-run"
        if tail_start < lo_end:
            lo_end, tail_start, layout = bs8, bs, "overlap"
    else:
        lo_end, tail_start, layout = bs8, bs, "cropped"
    return dict(n=n, lo_end=lo_end, tail_start=tail_start, layout=layout, vec4_load=(bs & 3) == 0,
                vec4_store=(bs & 7) == 0, table128=n == 128, fir_passes=-(-bs8 // 512))
