"""The whole-row MAC with 16-byte accesses (upols_mac_stream_kernel, csrc/upols.hip), at the smallest shapes
that reach it: 50 blocks (T in (100352, 102400]) and at most 25 kernel windows (ceil(L / 2048) + 1).

Row counts 1, 2 and 3 are a lone row in a pair, a full pair and an odd count; T = 100353 leaves one
sample in the last block; L = 300, 2049, 47000, 48000 give 2, 3, 24 and 25 windows (an even and an odd
count at each end: the last pair of kernel-spectra rows is whole, half or absent), and 49152 is the last
length this kernel serves.

Forward: rms error against the fp64 convolution below 1e-6 of the reference's rms
(test_gpu_parity.py::test_reverb_partitioned_shapes' bound), and the largest single-sample error no
larger than PARENT_MAX_ERR, the figure the kernel's 8-byte form before it (the parent commit's) reaches on
the same inputs on an MI355X: the sums run in the same order, so the outputs are meant to be the same
bits and the bound carries no margin.  (The reference is rounded to fp32, so these figures are whole
fp32 steps of the output, 5.7e-6 to 3.1e-5 on outputs of rms 5 to 19; the rms error is 2.3e-7 to
3.0e-7 of the reference's rms in all 30 cases, for both kernels.)

Adjoint: x.grad of Reverb against the fp64 autograd of the reference's convolution, relative L2 error
below 1e-5 (test_gpu_grad.py::test_reverb_grad_oracle's GRAD_REL).
"""
import numpy as np
import pytest
import torch

from conftest import rms
from oracle import numpy_oracle as no
from oracle import torch_ref as tr

pytestmark = pytest.mark.gpu

GRAD_REL = 1e-5
ROWS = (1, 2, 3)
SHAPES = [(T, L) for T in (102400, 100353) for L in (300, 2049, 47000, 48000, 49152)]

# largest |out - ref| of the parent commit's kernel, per (T, L) for 1, 2 and 3 rows
PARENT_MAX_ERR = {
    (102400, 300): (5.7220458984375e-06, 7.62939453125e-06, 7.62939453125e-06),
    (102400, 2049): (1.52587890625e-05, 1.71661376953125e-05, 1.71661376953125e-05),
    (102400, 47000): (2.288818359375e-05, 2.288818359375e-05, 2.6702880859375e-05),
    (102400, 48000): (2.288818359375e-05, 2.6702880859375e-05, 2.6702880859375e-05),
    (102400, 49152): (2.288818359375e-05, 3.0517578125e-05, 3.0517578125e-05),
    (100353, 300): (5.7220458984375e-06, 7.62939453125e-06, 7.62939453125e-06),
    (100353, 2049): (1.52587890625e-05, 1.621246337890625e-05, 1.621246337890625e-05),
    (100353, 47000): (2.288818359375e-05, 2.6702880859375e-05, 2.6702880859375e-05),
    (100353, 48000): (2.288818359375e-05, 3.0517578125e-05, 3.0517578125e-05),
    (100353, 49152): (3.0517578125e-05, 2.6702880859375e-05, 2.6702880859375e-05),
}


@pytest.fixture(scope="module")
def dd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ddsp_pytorch_amd
    ddsp_pytorch_amd._lib.load()
    return ddsp_pytorch_amd


def G(x):
    return torch.as_tensor(np.asarray(x)).float().cuda()


def C(x):
    return x.detach().cpu().numpy()


def signal_and_kernel(T, L, rows=3):
    rng = np.random.default_rng(L + T)
    x = (rng.standard_normal((rows, T, 1)) * 0.3).astype(np.float32)
    h = (rng.standard_normal(L) * np.exp(-np.arange(L) / 8000.0)).astype(np.float32)
    h[0] = 1.0
    return x, h


def forward_errors(dd, T, L):
    """[(rms error, rms of the reference, largest error)] of the first 1, 2 and 3 rows run as batches of
    their own; one fp64 reference serves the three (a row's convolution does not depend on the batch)."""
    x, h = signal_and_kernel(T, L)
    ref = no.reverb(x, h).astype(np.float64)
    res = []
    with torch.no_grad():
        spec = dd.core.reverb_spectrum(G(h), T)
        for rows in ROWS:
            out = C(dd.core.reverb_apply(G(x[:rows]), spec, L))
            r = ref[:rows]
            res.append((rms(out, r), float(np.sqrt(np.mean(r ** 2))), float(np.abs(out - r).max())))
    return res


@pytest.mark.parametrize("T,L", SHAPES)
def test_forward_against_fp64_convolution(dd, T, L):
    res = forward_errors(dd, T, L)
    print(f"mac_wide forward T={T} L={L}: " + " ".join(f"rows={n} rms={e:.4g} scale={s:.4g} max={m!r}"
                                                       for n, (e, s, m) in zip(ROWS, res)))
    for n, (err, scale, worst), bound in zip(ROWS, res, PARENT_MAX_ERR[T, L]):
        assert err < 1e-6 * scale, (n, err, scale)
        assert worst <= bound, (n, worst, bound)


def test_pair_independence(dd):
    """A pair's outputs depend on nothing but the pair: two rows alone, as pair 1 and as pair 2 of six rows."""
    T, L = 102400, 48000
    x, h = signal_and_kernel(T, L, rows=6)
    a, others = x[:2], x[2:]
    with torch.no_grad():
        spec = dd.core.reverb_spectrum(G(h), T)
        alone = C(dd.core.reverb_apply(G(a), spec, L))
        again = C(dd.core.reverb_apply(G(a), spec, L))
        mid = C(dd.core.reverb_apply(G(np.concatenate([others[:2], a, others[2:]])), spec, L))
        last = C(dd.core.reverb_apply(G(np.concatenate([others, a])), spec, L))
    assert np.array_equal(alone, again)
    assert np.array_equal(alone, mid[2:4])
    assert np.array_equal(alone, last[4:6])
    assert np.abs(alone).max() > 0.1 and not np.array_equal(alone, mid[:2])


@pytest.mark.parametrize("L", [2049, 48000])
def test_adjoint_against_fp64_autograd(dd, L):
    B, T = 3, 102383
    g = torch.Generator().manual_seed(B * T + L)
    torch.manual_seed(1)
    rv = dd.modules.Reverb(L, 48000, initial_wet=0.3, initial_decay=4.0)
    ref = tr.Reverb(*(p.detach().double() for p in (rv.noise, rv.decay, rv.wet)), L, 48000)
    x = torch.randn(B, T, 1, generator=g) * 0.3
    w = torch.randn(B, T, 1, generator=g)
    xc = x.double().requires_grad_(True)
    xg = x.cuda().requires_grad_(True)
    (ref(xc) * w.double()).sum().backward()
    rv = rv.cuda()
    (rv(xg) * w.cuda()).sum().backward()
    err = float((xg.grad.double().cpu() - xc.grad).norm() / xc.grad.norm())
    print(f"mac_wide adjoint L={L}: relative L2 error {err:.4g}")
    assert err < GRAD_REL, err
