"""tests/vjp_ref.py against the fp32 oracle's autograd (oracle/torch_ref.py, which tests/test_oracle_grad.py pins to
the reference's golden gradients): for every case of tests/test_gpu_vjp_shapes.py the oracle agrees with the
high-precision reference PER FRAME within ORACLE_REL = GRAD_REL / 2 = 5e-6.  That is the condition that keeps the
GPU test honest: its inputs are ones where the reference's own fp32 gradient is that well defined in every frame,
so GRAD_REL leaves the kernels a real margin and a failure is the kernel's.  A case that misses this bound gets
another seed or other inputs, never another bound.  No GPU.

Measured here (max over frames of the per-frame relative L2; the largest whole-tensor figure in brackets):
harmonic cases 1-8, 10, 11, HMODE 2: 1.8e-6 (3.7e-7); cases 1-8, 11, HMODE 1 distribution: 1.8e-6 (3.8e-7), amplitude
against its condition scale 7.2e-7; slow-sine case 9: 5.0e-7 (4.3e-7); the 15 noise shapes, both biases: 1.6e-6 (7.9e-7).
"""
import pytest
import torch

import vjp_ref as vr
from oracle import torch_ref as tr


def oracle_params_grad(c):
    p = c["param"].clone().requires_grad_(True)
    a, d = tr.harmonic_controls(p[..., :1], p[..., 1:], c["f0"], vr.SR)
    (tr.harmonic_forward(a, d, c["f0"], c["bs"], vr.SR) * c["g"]).sum().backward()
    return p.grad


def oracle_frames_grad(c):
    a = c["amp"].clone().requires_grad_(True)
    u = c["dist"].clone().requires_grad_(True)
    # harmonic_forward multiplies its distribution in place (modules.py:73): hand it a copy
    (tr.harmonic_forward(a, u.clone(), c["f0"], c["bs"], vr.SR) * c["g"]).sum().backward()
    return a.grad, u.grad


def oracle_noise_grad(c, raw_bias):
    m = c["mags"].clone().requires_grad_(True)
    A = m if raw_bias is None else tr.scale_function(m + raw_bias)
    (tr.noise_forward(A, c["noise"], c["bs"]) * c["g"]).sum().backward()
    return m.grad


@pytest.mark.parametrize("case", sorted(vr.HARMONIC_CASES) + [10, 11])
def test_oracle_params_grad_per_frame(case):
    c = vr.harmonic_case(case)
    got = oracle_params_grad(c)
    e, w = vr.max_frame_relerr(got, c["grad_param"]), vr.relerr(got, c["grad_param"])
    print(f"harmonic case {case} HMODE 2: per frame {e:.2e}, whole {w:.2e}")
    assert e <= vr.ORACLE_REL and w <= vr.ORACLE_REL


@pytest.mark.parametrize("case", sorted(vr.HARMONIC_CASES) + [9, 11])
def test_oracle_frames_grad_per_frame(case):
    c = vr.harmonic_case(case)
    da, du = oracle_frames_grad(c)
    e, w = vr.max_frame_relerr(du, c["grad_dist"]), vr.relerr(du, c["grad_dist"])
    ea = float(vr.scaled_err(da, c["grad_amp"], c["amp_scale"]).max())
    print(f"harmonic case {case} HMODE 1: distribution per frame {e:.2e}, whole {w:.2e}; amplitude {ea:.2e}")
    assert e <= vr.ORACLE_REL and w <= vr.ORACLE_REL and ea <= vr.ORACLE_REL


def test_slow_sine_case_crosses_the_fast_limit():
    """case 9's arguments: frames 0-4 stay below the kernels' fast-sine limit of 8e6, frames 5-7 exceed it"""
    c = vr.harmonic_case(9)
    _, omega, _ = vr.harmonic_fp32_points(c["f0"], c["H"], c["bs"])
    peak = omega.reshape(c["F"], c["bs"]).abs().max(-1).values * c["H"]
    assert float(peak.max()) > 8e6
    assert [bool(p < 8e6) for p in peak] == [True] * 5 + [False] * 3


def test_masked_case_has_exact_zero_frames():
    """case 10: f0 = 0 from the start keeps the phase at 0, so frames 0-1 have an exactly zero gradient; frame 4
    (f0 = 0 after the phase has moved) and frame 3 (every harmonic above Nyquist) do not"""
    c = vr.harmonic_case(10)
    zero = (c["grad_param"] == 0).all(-1)
    assert zero[:, :2].all() and not zero[:, 2:].any()
    mask, _, _ = vr.harmonic_fp32_points(c["f0"], c["H"], c["bs"])
    assert (mask[:, 3] < 1e-3).all() and (mask[:, [0, 1, 4]] > 1).all()


@pytest.mark.parametrize("raw_bias", vr.RAW_BIASES)
@pytest.mark.parametrize("name", sorted(vr.NOISE_CASES) + sorted(vr.PHILOX_CASES))
def test_oracle_noise_grad_per_frame(name, raw_bias):
    c = vr.noise_case(name)
    got = oracle_noise_grad(c, raw_bias)
    e, w = vr.max_frame_relerr(got, c["ref"][raw_bias]), vr.relerr(got, c["ref"][raw_bias])
    print(f"noise case {name} bias {raw_bias}: per frame {e:.2e}, whole {w:.2e}")
    assert e <= vr.ORACLE_REL and w <= vr.ORACLE_REL


def test_per_frame_metric_sees_one_band():
    """One band of one frame off by 1e-3 of that frame's norm: below GRAD_REL in the whole-tensor L2 over 600 frames,
    reported by the per-frame metric.  The frames' magnitudes spread over two decades, as a gradient's do between
    loud and quiet frames, and the wrong frame is a quiet one (0.05 of the loudest): its error weighs about
    1e-3 * 0.05 / sqrt(sum of the squared frame scales) = 5e-5 / sqrt(600 * 0.109) = 6e-6 in the whole-tensor
    figure (0.109 = the mean of 10^(-4 U))."""
    gen = torch.Generator().manual_seed(0)
    scale = 10.0 ** (-2.0 * torch.rand(1, 600, 1, generator=gen, dtype=torch.float64))
    scale[0, 417] = 0.05
    ref = torch.randn(1, 600, 9, generator=gen, dtype=torch.float64) * scale
    got = ref.clone()
    got[0, 417, 8] += 1e-3 * ref[0, 417].norm()
    assert vr.relerr(got, ref) < vr.GRAD_REL
    pf = vr.per_frame_relerr(got, ref)
    assert pf.shape == (1, 600)
    assert abs(float(pf[0, 417]) - 1e-3) < 1e-9 and int(pf.argmax()) == 417
    assert float(pf.sum()) == float(pf[0, 417])  # every other frame is exact
    assert vr.max_frame_relerr(got, ref) > 50 * vr.GRAD_REL


def test_per_frame_metric_zero_rows():
    ref = torch.ones(1, 3, 4, dtype=torch.float64)
    ref[0, 1] = 0
    got = ref.clone()
    assert vr.per_frame_relerr(got, ref).tolist() == [[0.0, 0.0, 0.0]]
    got[0, 1, 2] = 1e-30
    assert vr.per_frame_relerr(got, ref)[0, 1] == float("inf")
