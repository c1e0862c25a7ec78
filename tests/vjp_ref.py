"""The yardstick of the synthesis VJP kernels (``csrc/backward.hip``: harmonic_vjp_kernel, noise_vjp_kernel and
noise_vjp_wave_kernel): high-precision references of the gradients, the shape cases that reach the kernels'
branches, and the per-frame error metric.  Test infrastructure only (torch on the CPU, no device code); shared by
tests/test_vjp_ref.py (which ties it to the fp32 oracle's autograd) and tests/test_gpu_vjp_shapes.py.

The references use ``oracle/torch_ref.py``'s operator sequence and keep the reference's fp32 rounding points —
the values the kernels must reproduce bit for bit before any smooth arithmetic starts:

* the Nyquist decision ``fl32(f0 * k) < sr / 2`` with the fp32 mask values ``1.0001f`` / ``1e-4f``
  (ddsp/core.py:70-74);
* the fp32 phase, ``torch.cumsum`` of the fp32 increments on the CPU (ddsp/core.py:138);
* the fp32 product ``omega * k`` (ddsp/core.py:139).

Everything after those points — sine, scale function, normalisation, products, sums — runs in fp64 under autograd.
The noise path has no such points: it is fp64 from the magnitudes on.
"""
import functools
import math

import numpy as np
import torch

from oracle import philox
from oracle import torch_ref as tr

SR = 48000
GRAD_REL = 1e-5  # the project's gradient tolerance (tests/test_gpu_grad.py)
ORACLE_REL = GRAD_REL / 2  # what the fp32 oracle must meet per frame for a case to be usable
PHILOX_SEED, PHILOX_OFFSET = 77, 2 ** 32 + 5

# (B, F, H, bs); what each reaches is listed in tests/test_gpu_vjp_shapes.py
HARMONIC_CASES = {
    1: (1, 3, 1, 64),
    2: (2, 5, 17, 441),
    3: (1, 2, 5, 3),
    4: (1, 4, 3, 1),
    5: (1, 3, 1024, 64),
    6: (1, 2, 2052, 16),
    7: (1, 2, 4096, 8),
    8: (1, 600, 8, 4),
}
SLOW_SINE_CASE = (1, 8, 1024, 512)  # case 9
MASKED_CASE = (2, 6, 8, 64)  # case 10
HIGH_PITCH_CASE = (1, 3, 1, 64)  # case 11: case 1's shape at 2-20 kHz

# (B, F, bs, NB), injected noise
NOISE_CASES = {
    "a": (2, 3, 441, 18),
    "b": (2, 3, 441, 17),
    "c": (1, 3, 64, 65),
    "d": (1, 2, 7, 9),
    "e": (2, 3, 100, 21),
    "f": (2, 5, 64, 33),
    "g": (1, 3, 8, 2),
    "h": (1, 2, 1024, 513),
    "i": (1, 2, 512, 129),
    "j": (1, 5, 512, 65),
    "m": (1, 2, 8, 65),
}
# Philox noise (seed PHILOX_SEED, offset PHILOX_OFFSET): the wave kernel, then the generic kernel
PHILOX_CASES = {
    "k0": (1, 5, 640, 65),
    "k1": (2, 3, 1024, 65),
    "l0": (2, 3, 441, 18),
    "l1": (1, 3, 30, 33),
}
RAW_BIASES = (-5.0, None)


# ------------------------------------------------------------------------------------------ the metric
def _d(t):
    return torch.as_tensor(t).detach().double().cpu()


def relerr(got, ref):
    """whole-tensor relative L2 error ||got - ref|| / ||ref||"""
    got, ref = _d(got), _d(ref)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def per_frame_relerr(got, ref):
    """[B, F, C] -> [B, F] float64: ||got - ref||_2 / ||ref||_2 of each (b, f) row.  A row whose reference is
    exactly zero must be exactly zero in ``got``: 0 there if it is, inf if it is not."""
    got, ref = _d(got), _d(ref)
    assert got.shape == ref.shape and got.dim() == 3, (got.shape, ref.shape)
    num, den = (got - ref).norm(dim=-1), ref.norm(dim=-1)
    zero = den == 0
    out = num / torch.where(zero, torch.ones_like(den), den)
    return torch.where(zero, torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, math.inf)), out)


def max_frame_relerr(got, ref):
    return float(per_frame_relerr(got, ref).max())


def scaled_err(got, ref, scale):
    """[B, F, 1] -> [B, F]: |got - ref| / scale, for a signed sum measured against its condition scale
    sum |terms| (HMODE 1's grad_amplitudes)."""
    got, ref, scale = _d(got), _d(ref), _d(scale)
    return ((got - ref).abs() / scale).reshape(ref.shape[0], ref.shape[1])


# ------------------------------------------------------------------------------------------ harmonic part
def harmonic_fp32_points(f0, H, bs, sr=SR):
    """The reference's fp32 rounding points for f0 [B, F, 1] (fp32, CPU): (mask [B, F, H], omega [B, F*bs, 1],
    arg [B, F, bs, H] = fl32(omega * k)), all fp32."""
    f0 = f0.float()
    B, F = f0.shape[:2]
    k = torch.arange(1, H + 1).to(f0)
    mask = (f0 * k < sr / 2).float() + 1e-4  # ddsp/core.py:70-74
    omega = torch.cumsum(2 * math.pi * tr.upsample(f0, bs) / sr, 1)  # ddsp/core.py:138
    arg = (omega * k).reshape(B, F, bs, H)  # ddsp/core.py:139
    return mask, omega, arg


def _frame_audio(arg, A):
    """sum_k sin(arg) A_k per sample, fp64: arg [B, F, bs, H] fp32, A [B, F, H] fp64 -> [B, F, bs]"""
    return torch.einsum("bfsh,bfh->bfs", torch.sin(arg.double()), A)


def harmonic_params_ref(f0, param, g, bs, sr=SR):
    """HMODE 2: raw param [B, F, H+1] -> grad_param [B, F, H+1] (fp64) for upstream g [B, F*bs, 1]."""
    B, F, H1 = param.shape
    mask, _, arg = harmonic_fp32_points(f0, H1 - 1, bs, sr)
    p = param.detach().double().requires_grad_(True)
    amp = tr.scale_function(p[..., :1])  # modules.py:44-67 in fp64
    dist = tr.scale_function(p[..., 1:]) * mask.double()
    dist = dist / dist.sum(-1, keepdim=True)
    out = _frame_audio(arg, dist * amp)
    (out * g.double().reshape(B, F, bs)).sum().backward()
    return p.grad


def harmonic_frames_ref(f0, amplitudes, distribution, g, bs, sr=SR):
    """HMODE 1: frame controls amplitudes [B, F, 1] and the normalised distribution [B, F, H] before the
    multiply -> (grad_amplitudes [B, F, 1], grad_distribution [B, F, H], scale [B, F, 1]) in fp64, where
    scale = sum_k |dA_k u_k| is the condition scale of the signed sum grad_amplitudes = sum_k dA_k u_k."""
    B, F, H = distribution.shape
    _, _, arg = harmonic_fp32_points(f0, H, bs, sr)
    a = amplitudes.detach().double().requires_grad_(True)
    u = distribution.detach().double().requires_grad_(True)
    out = _frame_audio(arg, u * a)  # modules.py:73
    (out * g.double().reshape(B, F, bs)).sum().backward()
    with torch.no_grad():
        dA = u.grad / a  # dA_k = grad_distribution_k / a
        scale = (dA * u).abs().sum(-1, keepdim=True)
    return a.grad, u.grad, scale


def f0_frames(B, F, gen):
    return 50.0 * 20.0 ** torch.rand(B, F, 1, generator=gen)


@functools.lru_cache(maxsize=None)
def harmonic_case(case):
    """Inputs (fp32, CPU) and fp64 references of harmonic case 1..11; computed once, never modified."""
    gen = torch.Generator().manual_seed(1000 + case)
    if case == 9:
        B, F, H, bs = SLOW_SINE_CASE
        f0 = torch.where(torch.arange(F) % 2 == 0, 21000.0, 23000.0).reshape(1, F, 1).float()
        amp = torch.rand(B, F, 1, generator=gen) + 0.5
        dist = torch.rand(B, F, H, generator=gen)
        dist = dist / dist.sum(-1, keepdim=True)
        param = None
    else:
        B, F, H, bs = {10: MASKED_CASE, 11: HIGH_PITCH_CASE}.get(case) or HARMONIC_CASES[case]
        f0 = f0_frames(B, F, gen)
        if case == 11:
            f0 = 2000.0 * 10.0 ** torch.rand(B, F, 1, generator=gen)
        if case == 10:
            f0[:, [0, 1, 4]] = 0.0
            f0[:, 3] = 30000.0
        param = torch.randn(B, F, H + 1, generator=gen)
        with torch.no_grad():
            amp, dist = tr.harmonic_controls(param[..., :1].clone(), param[..., 1:].clone(), f0, SR)
    g = torch.randn(B, F * bs, 1, generator=gen)
    c = dict(B=B, F=F, H=H, bs=bs, f0=f0, param=param, amp=amp, dist=dist, g=g)
    if param is not None:
        c["grad_param"] = harmonic_params_ref(f0, param, g, bs)
    if case != 10:
        c["grad_amp"], c["grad_dist"], c["amp_scale"] = harmonic_frames_ref(f0, amp, dist, g, bs)
    return c


# ------------------------------------------------------------------------------------------ noise part
def noise_ref(mags, noise, g, bs, raw_bias):
    """grad_magnitudes [B, F, NB] (fp64) of tr.noise_forward(tr.scale_function(mags + raw_bias), noise, bs) —
    or of tr.noise_forward(mags, noise, bs) with raw_bias None — for upstream g [B, F*bs, 1]."""
    m = mags.detach().double().requires_grad_(True)
    A = m if raw_bias is None else tr.scale_function(m + raw_bias)
    out = tr.noise_forward(A, noise.double(), bs)
    (out * g.double()).sum().backward()
    return m.grad


def philox_noise(B, F, bs, seed=PHILOX_SEED, offset=PHILOX_OFFSET):
    return torch.from_numpy(np.ascontiguousarray(philox.device_noise(B, F, bs, seed, offset)))


@functools.lru_cache(maxsize=None)
def noise_case(name):
    """Inputs (fp32, CPU) and fp64 references {raw_bias: grad_magnitudes} of a noise case; computed once."""
    B, F, bs, NB = NOISE_CASES[name] if name in NOISE_CASES else PHILOX_CASES[name]
    gen = torch.Generator().manual_seed(2000 + sum(map(ord, name)))
    mags = torch.randn(B, F, NB, generator=gen)
    if name in PHILOX_CASES:
        noise = philox_noise(B, F, bs)
    else:
        noise = torch.rand(B, F, bs, generator=gen) * 2 - 1
    g = torch.randn(B, F * bs, 1, generator=gen)
    ref = {rb: noise_ref(mags, noise, g, bs, rb) for rb in RAW_BIASES}
    return dict(B=B, F=F, bs=bs, NB=NB, mags=mags, noise=noise, g=g, ref=ref)
