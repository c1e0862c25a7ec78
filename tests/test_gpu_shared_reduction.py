"""The fused kernel's shared revolution count (synth_frame.hip osc_bank4_shared): the four
samples of an aligned quad subtract the count n = rint(x / 2 pi) of the quad's sample 1 where the frame's
bound on the reduced argument, 0.5 + 2 H4 inc / 2 pi revolutions (H4 = H rounded up to 4), is below 8;
every other frame keeps one count per sample.  Checked on both sides of that guard, in the
4-samples-per-thread form (launches of >= 512 frames) and the one-sample-per-thread SPLIT form (fewer),
which must agree bit for bit.
"""
import numpy as np
import pytest
import torch

from conftest import rms
from oracle import numpy_oracle as no

pytestmark = pytest.mark.gpu

SR = 48000
SHARED_REV_LIMIT = 8.0  # kSharedRevLimit


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


def rev_bound(f0, H):
    """the guard's bound on |y| in revolutions, per frame, as the kernel forms it from the fp32 increment"""
    H4 = (H + 3) & ~3
    inc = no.phase_increment(np.asarray(f0, np.float32), SR).astype(np.float64)
    return 0.5 + 2.0 * H4 * np.abs(inc) / (2.0 * np.pi)


def make_case(case, B, F, H, NB, bs, seed):
    rng = np.random.default_rng(seed)
    f0 = (50.0 * 20.0 ** rng.random((B, F, 1))).astype(np.float32)  # log-uniform 50-1000 Hz
    if case == "high":  # alternate frames of each item at 6-20 kHz
        hi = (6000.0 * (20000.0 / 6000.0) ** rng.random((B, F, 1))).astype(np.float32)
        f0[:, ::2] = hi[:, ::2]
    return {"f0": f0, "param": rng.standard_normal((B, F, H + 1)).astype(np.float32),
            "mags": rng.standard_normal((B, F, NB)).astype(np.float32),
            "noise": (rng.random((B, F, bs)) * 2 - 1).astype(np.float32)}


def harmonic_ref(inp, bs):
    c = no.harmonic_get_controls(inp["param"][..., :1], inp["param"][..., 1:], inp["f0"], SR)
    return no.harmonic_forward(c["amplitudes"], c["harmonic_distribution"], inp["f0"], bs, SR)[0]


def run(dd, inp, bs, sl=slice(None), **kw):
    with torch.no_grad():
        return dd.core.synth_frames(G(inp["f0"][sl]), G(inp["param"][sl]), G(inp["mags"][sl]), bs, SR,
                                    noise=G(inp["noise"][sl]), parts=True, **kw)


BATCH = (4, 128, 20, 9, 64)  # 512 frames: the 4-samples-per-thread form


@pytest.fixture(scope="module")
def batch(dd):
    """both pitch cases at the batch shape: inputs, the launch's (signal, harmonic, noise), the oracle's harmonic"""
    out = {}
    for i, case in enumerate(("low", "high")):
        B, F, H, NB, bs = BATCH
        inp = make_case(case, B, F, H, NB, bs, seed=20 + i)
        out[case] = (inp, run(dd, inp, bs), harmonic_ref(inp, bs))
    return out


@pytest.mark.parametrize("case", ["low", "high"])
def test_oracle_parity_batch_form(batch, case):
    """50-1000 Hz: every frame below the guard (bound <= 1.4 at H = 20).  6-20 kHz on alternate frames: the
    frames above 9 kHz are past it (bound 8 at 9 kHz) and keep one count per sample, those below share."""
    inp, (_, harm, _), ref = batch[case]
    bound = rev_bound(inp["f0"], BATCH[2])
    if case == "low":
        assert (bound < SHARED_REV_LIMIT).all()
    else:
        assert (bound > SHARED_REV_LIMIT).sum() >= 0.25 * bound.size and (bound < SHARED_REV_LIMIT).any()
    e = rms(C(harm), ref)
    print(f"batch form, {case}: rms {e:.3e}, bound on |y| {bound.min():.2f}..{bound.max():.2f}")
    assert e < 1e-6, e


@pytest.mark.parametrize("case", ["low", "high"])
def test_oracle_parity_split_form(dd, case):
    B, F, H, NB, bs = 1, 6, 100, 65, 512
    inp = make_case(case, B, F, H, NB, bs, seed=30)
    bound = rev_bound(inp["f0"], H)
    assert (bound < SHARED_REV_LIMIT).all() if case == "low" else (bound[:, ::2] > SHARED_REV_LIMIT).all()
    e = rms(C(run(dd, inp, bs)[1]), harmonic_ref(inp, bs))
    print(f"split form, {case}: rms {e:.3e}, bound on |y| {bound.min():.2f}..{bound.max():.2f}")
    assert e < 1e-6, e


@pytest.mark.parametrize("case", ["low", "high"])
def test_launch_shape_independence(dd, batch, case):
    """one item alone (128 frames: the SPLIT form) equals its slice of the 512-frame batch bit for bit"""
    inp, full, _ = batch[case]
    bs = BATCH[4]
    for b in range(BATCH[0]):
        one = run(dd, inp, bs, slice(b, b + 1))
        for o, f in zip(one, full):
            assert torch.equal(o, f[b:b + 1]), (case, b)


@pytest.mark.parametrize("B,F", [(1, 8), (4, 128)])  # SPLIT form, 4-samples-per-thread form
def test_guard_edge(dd, B, F):
    """frames just under and just over the guard (about 1800 Hz at H = 100), alternating: both within the
    oracle bound"""
    H, NB, bs = 100, 9, 64
    inp = make_case("low", B, F, H, NB, bs, seed=40)
    edge = (SHARED_REV_LIMIT - 0.5) * SR / (2.0 * ((H + 3) & ~3))  # 0.5 + 2 H4 f0 / sr = limit
    inp["f0"][:, 0::2] = np.float32(edge * 0.99)
    inp["f0"][:, 1::2] = np.float32(edge * 1.01)
    bound = rev_bound(inp["f0"], H)
    assert (bound[:, 0::2] < SHARED_REV_LIMIT).all() and (bound[:, 0::2] > 0.98 * SHARED_REV_LIMIT).all()
    assert (bound[:, 1::2] > SHARED_REV_LIMIT).all() and (bound[:, 1::2] < 1.02 * SHARED_REV_LIMIT).all()
    harm = C(run(dd, inp, bs)[1]).reshape(B, F, bs)
    ref = harmonic_ref(inp, bs).reshape(B, F, bs)
    under, over = rms(harm[:, 0::2], ref[:, 0::2]), rms(harm[:, 1::2], ref[:, 1::2])
    print(f"guard edge B={B} F={F}: under {under:.3e} (bound {bound[0, 0, 0]:.3f}), over {over:.3e} "
          f"(bound {bound[0, 1, 0]:.3f})")
    assert under < 1e-6 and over < 1e-6, (under, over)


@pytest.mark.parametrize("k", [1, 64, 128])
def test_per_sine_bound(dd, k):
    """One loud harmonic (raw +12, every other -25) at H = 128, 900-1000 Hz, so that the harmonic signal is
    that sine up to the others' residue: |harm / A_k - sin_fp64(fl32 argument)| <= 3.2e-7 + 2 pi ulp, the
    recorded hardware-sine error plus the reduction's two roundings of half a spacing each at the frame's
    bound on |y|.  At these pitches harmonics 25 and up are past Nyquist and scaled by 1e-4, the loud one
    included for k = 64 and 128, which leaves the 24 audible ones at up to 1.2e-2 of it: the reference is
    the fp64 sum over the launch's own coefficients A (its controls output), not the loud sine alone."""
    B, F, H, NB, bs = 1, 3, 128, 65, 512
    rng = np.random.default_rng(k)
    inp = make_case("low", B, F, H, NB, bs, seed=50 + k)
    inp["f0"] = (900.0 + 100.0 * rng.random((B, F, 1))).astype(np.float32)
    inp["param"][..., 0] = 0.0
    inp["param"][..., 1:] = -25.0
    inp["param"][..., k] = 12.0
    _, harm, _, ctrl = run(dd, inp, bs, controls=True)
    A = C(ctrl["harmonic_distribution"]).astype(np.float64)                      # [B, F, H]
    w = no.phase(no.upsample(inp["f0"], bs), SR).reshape(B, F, bs, 1)           # fl32 omega, bit-exact
    x = (w * np.arange(1, H + 1, dtype=np.float32)).astype(np.float32)          # fl32(omega k)
    assert x.dtype == np.float32
    ref = (np.sin(x.astype(np.float64)) * A[:, :, None, :]).sum(-1)
    err = np.abs(C(harm).reshape(B, F, bs).astype(np.float64) - ref) / A[:, :, None, k - 1]
    ybound = rev_bound(inp["f0"], H)[..., 0]                                    # [B, F]
    assert (ybound < SHARED_REV_LIMIT).all()
    limit = 3.2e-7 + 2.0 * np.pi * np.spacing(ybound.astype(np.float32)).astype(np.float64)
    others = (A.sum(-1) - A[..., k - 1]) / A[..., k - 1]
    print(f"per-sine k={k}: max error {err.max(-1).max():.3e}, limit {limit.min():.3e}, |y| bound "
          f"{ybound.max():.2f}, other harmonics / A_k {others.max():.2e}")
    assert (err.max(-1) <= limit).all(), (err.max(-1), limit)
