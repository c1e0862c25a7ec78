"""The yardstick of the pitch-gradient kernels (``csrc/pitch_grad.hip``: frame_pitch_grad_kernel and
pitch_grad_scan_kernel): the closed form of the f0 gradient of the frame-rate synthesis in fp64, the shape cases
that reach the kernels' branches, and the per-frame error metric.  Test infrastructure only (torch on the CPU, no
device code); shared by tests/test_f0_grad_ref.py (which ties the closed form to the oracle's autograd) and
tests/test_gpu_f0_grad.py.

The closed form.  With the frame kernels' phase, omega_{f,j} = S0_f + (j+1) inc_f for sample j < bs of frame f,
inc_f = c f0_f (c = 2 pi / sr), S0_f = bs sum_{f'<f} inc_{f'}, the frame's harmonic amplitudes A_{f,k} (constants of
the frame with respect to f0: the Nyquist mask is a comparison) and the upstream gradient g:

    q_{f,j} = g_{f,j} sum_k k A_{f,k} cos(fl32(omega_{f,j} k))       Q_f = sum_j q_{f,j}    R_f = sum_j (j+1) q_{f,j}
    dL/d f0_f = c (R_f + bs sum_{f'>f} Q_{f'})

It is evaluated in fp64 with the reference's fp32 rounding points kept (vjp_ref.harmonic_fp32_points: the mask, the
fp32 omega and fl32(omega k)), and beside the gradient it returns the frame's CONDITION SCALE, the same expression
built from |g_j| sum_k k |A_k|: what the signed sums of the frame could add up to.  The metric is |got - ref| / scale
per frame (vjp_ref.scaled_err; a frame whose scale is exactly zero must be exactly zero) and the whole-tensor
relative L2 error (vjp_ref.relerr).
"""
import functools
import math

import torch

import synth_ref as sr_
import vjp_ref as vr
from oracle import torch_ref as tr

SR = vr.SR
GRAD_REL = vr.GRAD_REL  # whole tensor
FRAME_TOL = sr_.HARM_FRAME_TOL  # 2e-6 per frame against the condition scale: the forward oscillator's bound for the
FRAME_CAP = sr_.HARM_FRAME_CAP  # same kind of sum (H bs hardware-sine terms in fp32 against the sum of their magnitudes)
NB = 9  # noise bands of the synth_frames / synth_signal route (the pitch gradient does not depend on the noise)
SCAN_CHUNK = 256  # pitch_grad.hip kScanChunk (ddsp_hip_frame_pitch_grad_scan_chunk; tests/test_f0_grad_abi.py)

# name -> (H, bs, B, F, pitch kind of synth_ref._pitches); what each reaches is listed in tests/test_gpu_f0_grad.py
CASES = {
    "c8": (100, 512, 2, 8, "low"),
    "m16": (16, 64, 2, 16, "low"),
    "b4": (8, 4, 3, 7, "low"),
    "odd": (5, 12, 2, 9, "low"),
    "h1": (1, 4, 1, 64, "low"),
    "high": (100, 64, 2, 16, "high"),
    "nyq": (48, 64, 1, 64, "nyquist"),
    "sub": (1024, 64, 1, 8, "sub"),
    "f441": (17, 441, 2, 5, "low"),
    "f1": (3, 1, 2, 5, "low"),
    "slow": (1024, 441, 1, 13, "20k"),
    "long": (16, 64, 1, 520, "low"),
    "scan_below": (4, 4, 2, SCAN_CHUNK - 1, "low"),
    "scan_above": (4, 4, 2, SCAN_CHUNK + 1, "low"),
}
ZERO_TAIL = {"b4": 2}  # the upstream gradient of the item's last frames is zero: their scale is exactly zero


# ------------------------------------------------------------------------------------------ the closed form
def fp64_points(f0, H, bs, sr=SR):
    """harmonic_fp32_points with nothing rounded to fp32: (mask, arg [B, F, bs, H]) in fp64 from f0's values."""
    f0 = f0.double()
    B, F = f0.shape[:2]
    k = torch.arange(1, H + 1, dtype=torch.float64)
    mask = (f0 * k < sr / 2).double() + 1e-4
    omega = torch.cumsum(2 * math.pi * tr.upsample(f0, bs) / sr, 1)
    return mask, (omega * k).reshape(B, F, bs, H)


def amplitudes_from_param(param, mask):
    """A [B, F, H] fp64 of modules.py:44-73 from the raw projection and the mask"""
    p = param.double()
    amp = tr.scale_function(p[..., :1])
    dist = tr.scale_function(p[..., 1:]) * mask.double()
    dist = dist / dist.sum(-1, keepdim=True)
    return amp, dist


def closed_form(A, arg, g, bs, sr=SR):
    """-> (gradient [B, F, 1], condition scale [B, F, 1]) fp64 for A [B, F, H] fp64, arg [B, F, bs, H] and the
    upstream gradient g [B, F*bs, 1]"""
    B, F, H = A.shape
    c = 2 * math.pi / sr
    kA = A.double() * torch.arange(1, H + 1, dtype=torch.float64)
    gg = g.double().reshape(B, F, bs)
    j1 = torch.arange(1, bs + 1, dtype=torch.float64)
    q = gg * torch.einsum("bfsh,bfh->bfs", torch.cos(arg.double()), kA)
    qbar = gg.abs() * kA.abs().sum(-1, keepdim=True)

    def finish(q):
        Q, R = q.sum(-1), (q * j1).sum(-1)
        suffix = Q.flip(1).cumsum(1).flip(1) - Q  # sum over the later frames
        return (c * (R + bs * suffix)).unsqueeze(-1)

    return finish(q), finish(qbar)


def params_ref(f0, param, g, bs, sr=SR, points="fp32"):
    """the f0 gradient of harmonic_synth_params / synth_frames: A from the raw projection"""
    H = param.shape[-1] - 1
    if points == "fp32":
        mask, _, arg = vr.harmonic_fp32_points(f0, H, bs, sr)
    else:
        mask, arg = fp64_points(f0, H, bs, sr)
    amp, dist = amplitudes_from_param(param, mask)
    return closed_form(dist * amp, arg, g, bs, sr)


def frames_ref(f0, amp, dist, g, bs, sr=SR):
    """the f0 gradient of harmonic_synth_frames: A = amp * dist from the frame controls as given (fp32 values)"""
    _, _, arg = vr.harmonic_fp32_points(f0, dist.shape[-1], bs, sr)
    return closed_form(dist.double() * amp.double(), arg, g, bs, sr)


# ------------------------------------------------------------------------------------------ the oracle's autograd
def oracle_f0_grad(f0, param, g, bs, dtype, sr=SR):
    """f0.grad of oracle/torch_ref.py's harmonic_controls + harmonic_forward in ``dtype``"""
    f = f0.to(dtype).clone().requires_grad_(True)
    p = param.to(dtype)
    a, d = tr.harmonic_controls(p[..., :1].clone(), p[..., 1:].clone(), f, sr)
    out = tr.harmonic_forward(a, d, f, bs, sr)
    (out * g.to(dtype)).sum().backward()
    return f.grad


# ------------------------------------------------------------------------------------------ the metric
def frame_err(got, ref, scale):
    """[B, F, 1] -> [B, F] float64: |got - ref| / scale per frame.  A frame whose scale is exactly zero must be
    exactly zero in ``got``: 0 there if it is, inf if it is not; a NaN reads inf."""
    got, ref, scale = (torch.as_tensor(t).detach().double().cpu() for t in (got, ref, scale))
    zero = scale == 0
    e = vr.scaled_err(got, ref, torch.where(zero, torch.ones_like(scale), scale))
    e = torch.where(torch.isnan(e), torch.full_like(e, math.inf), e)
    z = zero.reshape(e.shape)
    bad = torch.where(got.reshape(e.shape) == 0, torch.zeros_like(e), torch.full_like(e, math.inf))
    return torch.where(z, bad, e)


# ------------------------------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs (fp32, CPU) and fp64 references of a case; seeded by name, computed once, never modified."""
    H, bs, B, F, pitch = CASES[name]
    gen = torch.Generator().manual_seed(sr_._seed("f0grad/" + name))
    f0 = torch.from_numpy(sr_._pitches(pitch, B, F, gen))
    param = torch.randn(B, F, H + 1, generator=gen)
    mags = torch.randn(B, F, NB, generator=gen)
    noise = torch.rand(B, F, bs, generator=gen) * 2 - 1
    g = torch.randn(B, F * bs, 1, generator=gen)
    if name in ZERO_TAIL:
        g.reshape(B, F, bs)[:, F - ZERO_TAIL[name]:] = 0.0
    mask, _, _ = vr.harmonic_fp32_points(f0, H, bs)
    with torch.no_grad():
        amp64, dist64 = amplitudes_from_param(param, mask)
        amp, dist = amp64.float(), dist64.float()  # the frame route's controls: the fp64 ones rounded to fp32
        grad_params, scale_params = params_ref(f0, param, g, bs)
        grad_frames, scale_frames = frames_ref(f0, amp, dist, g, bs)
    return dict(name=name, H=H, bs=bs, B=B, F=F, f0=f0, param=param, mags=mags, noise=noise, g=g, amp=amp, dist=dist,
                grad_params=grad_params, scale_params=scale_params, grad_frames=grad_frames,
                scale_frames=scale_frames)
