"""The pitch tracker on gfx950 (csrc/pitch.hip: core.extract_pitch, features.analyze(pitch=None), torch.ops.ddsp_hip
.pitch) against the fp64 restatement of tests/pitch_ref.py.

Accuracy gate, per case: f0's relative error and the confidence's absolute error against the fp64 restatement, RMS
and maximum, over the frames whose ``period`` equals the fp64 one's; each statistic <= 4 x max(the fp32
restatement's same statistic, 2^-24).  4 x is the project's margin; 2^-24 is half an fp32 ulp of
the output, below which the GPU's own rounding of an exact result would fail.  Frames whose period differs are left
out of the statistics; there may be at most frames // 50 of them per case (none for any case here, and the inputs
have no near-ties: tests/test_pitch_ref.py).  Every figure is printed before it is asserted (pytest -s).

Measured on MI355X (profiles/pitch_gate.txt): no frame of any case differs in period; f0
relative error <= 2.8e-8 rms and <= 5.5e-8 max, confidence <= 2.0e-8 rms and <= 5.4e-8 max, i.e. the fp32 rounding
of the outputs, against bounds of 2.4e-7 and more.
"""
import numpy as np
import pytest
import torch

import pitch_cases as pc

pytestmark = pytest.mark.gpu

MARGIN = 4.0
FLOOR = 2.0 ** -24


@pytest.fixture(scope="module")
def dd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ddsp_pytorch_amd
    ddsp_pytorch_amd._lib.load()
    return ddsp_pytorch_amd


def _stats(e):
    return (float(np.sqrt(np.mean(e ** 2))), float(np.abs(e).max())) if e.size else (0.0, 0.0)


def gate(label, f0, conf, period, ref):
    """The accuracy gate of this file's docstring on [B, F] arrays; prints the figures, then asserts."""
    f0, conf, period = (np.asarray(a) for a in (f0, conf, period))
    assert f0.dtype == np.float32 and conf.dtype == np.float32 and period.dtype == np.int32
    assert f0.shape == ref["f064"].shape == conf.shape == period.shape
    assert np.isfinite(f0).all() and np.isfinite(conf).all()
    same = period == ref["period64"]
    same32 = ref["period32"] == ref["period64"]
    n_diff = int((~same).sum())
    print(f"{label}: {same.size} frames, {n_diff} with another period than the fp64 restatement's")
    figures = []
    for name, got, r64, r32, rel in (("f0 rel", f0, ref["f064"], ref["f032"], True),
                                     ("confidence abs", conf, ref["conf64"], ref["conf32"], False)):
        scale = r64 if rel else 1.0
        g = _stats(((got.astype(np.float64) - r64) / scale)[same])
        c = _stats(((r32.astype(np.float64) - r64) / scale)[same32])
        for stat, gv, cv in zip(("rms", "max"), g, c):
            bound = MARGIN * max(cv, FLOOR)
            print(f"{label}: {name} {stat}: gpu {gv:.3e} | fp32 cpu {cv:.3e} | bound {bound:.3e}")
            figures.append((name, stat, gv, bound))
    assert n_diff <= same.size // 50, (label, n_diff)
    for name, stat, gv, bound in figures:
        assert gv <= bound, (label, name, stat, gv, bound)


def run(dd, x, sr, block, **kw):
    f0, conf, period = dd.core.extract_pitch(x, sr, block, return_confidence=True, return_period=True, **kw)
    return f0.cpu().numpy(), conf.cpu().numpy(), period.cpu().numpy()


@pytest.mark.parametrize("sr,block,T,B,kind", pc.OFFLINE)
def test_accuracy_against_the_fp64_restatement(dd, sr, block, T, B, kind):
    x, (tmin, tmax), ref = pc.offline_case(sr, block, T, B, kind)
    xg = torch.from_numpy(np.array(x)).cuda()
    F = T // block
    if kind == "one_d":
        f0, conf, period = run(dd, xg[0], sr, block)
        assert f0.shape == conf.shape == period.shape == (F,)
        f0, conf, period = f0[None], conf[None], period[None]
    else:
        f0, conf, period = run(dd, xg, sr, block)
        assert f0.shape == (B, F)
    gate(f"sr {sr} block {block} T {T} B {B} {kind}", f0, conf, period, ref)
    if kind == "zeros":  # the silent item: the values the rules predict, exactly
        assert (period[0] == tmin).all() and (f0[0] == np.float32(sr / tmin)).all() and not conf[0].any()
    if kind == "onset":  # the frames that begin in the leading zeros and end in the tone: d' >= 1 -> tau_min
        early = np.arange(F) * block <= 1500  # y[0..W) = x[f block - W .. f block) lies in the zeros
        assert early.any() and (ref["period64"][0, early] == tmin).all() and (period[0, early] == tmin).all()
        assert (period[0, -4:] > tmin).all() and (conf[0, -4:] > 0.9).all()


# Every transform size is its own instantiation (one to three radix-16 passes, a final radix-1/2/4/8 pass, 32 frames
# to one frame per workgroup, scans and reductions inside a wave or across waves): frame_length at 16 kHz, hop
# L/4 + 1 (odd), T = 3 L + 37, B = 2, fmin = sr / (W - 1) + 1, the drawn f0 with a period between 4 and W/2.
@pytest.mark.parametrize("L", pc.SIZES)
def test_every_transform_size(dd, L):
    hop, T, fmin, _, _ = pc.size_params(L)
    x, (tmin, tmax), ref = pc.size_case(L)
    assert dd.core.pitch_lags(pc.SIZES_SR, fmin, 2000.0, L) == (tmin, tmax)
    xg = torch.from_numpy(np.array(x)).cuda()
    f0, conf, period = run(dd, xg, pc.SIZES_SR, hop, fmin=fmin, frame_length=L)
    gate(f"frame_length {L} hop {hop} T {T} lags {tmin}..{tmax}", f0, conf, period, ref)


def test_bits_are_reproducible_independent_of_the_batch_and_of_the_optional_outputs(dd):
    sr, block, T, B, kind = pc.OFFLINE[1]
    x = pc.offline_case(sr, block, T, B, kind)[0]
    xg = torch.from_numpy(np.array(x)).cuda()
    a = dd.core.extract_pitch(xg, sr, block, return_confidence=True, return_period=True)
    b = dd.core.extract_pitch(xg, sr, block, return_confidence=True, return_period=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # an item alone, and in another place of another batch
    alone = dd.core.extract_pitch(xg[1:2], sr, block, return_confidence=True, return_period=True)
    other = dd.core.extract_pitch(torch.flip(xg, [0]).contiguous(), sr, block, return_confidence=True,
                                  return_period=True)
    for u, v, w in zip(a, alone, other):
        assert torch.equal(u[1:2], v) and torch.equal(u[0], w[B - 1])
    # confidence / period are optional (null pointers in the C-ABI): the same f0 bits
    only = dd.core.extract_pitch(xg, sr, block)
    assert isinstance(only, torch.Tensor) and torch.equal(only, a[0])
    f0c = dd.core.extract_pitch(xg, sr, block, return_confidence=True)
    f0p = dd.core.extract_pitch(xg, sr, block, return_period=True)
    assert len(f0c) == 2 and torch.equal(f0c[0], a[0]) and torch.equal(f0c[1], a[1])
    assert len(f0p) == 2 and torch.equal(f0p[0], a[0]) and torch.equal(f0p[1], a[2]) and f0p[1].dtype == torch.int32
    # a non-contiguous input is made contiguous
    wide = torch.zeros(B, 2 * T, device="cuda")
    wide[:, ::2] = xg
    assert torch.equal(dd.core.extract_pitch(wide[:, ::2], sr, block), a[0])


def test_torch_op_returns_the_python_functions_bits(dd):
    from ddsp_pytorch_amd import script
    script.load_ops()
    sr, block, T, B, kind = pc.OFFLINE[3]
    x, (tmin, tmax), _ = pc.offline_case(sr, block, T, B, kind)
    xg = torch.from_numpy(np.array(x)).cuda()
    want = dd.core.extract_pitch(xg, sr, block, return_confidence=True, return_period=True)
    got = torch.ops.ddsp_hip.pitch(xg, 2048, block, tmin, tmax, float(sr), 0.1)
    for u, v in zip(want, got):
        assert u.dtype == v.dtype and torch.equal(u, v)
    got1 = torch.ops.ddsp_hip.pitch(xg[0], 2048, block, tmin, tmax, float(sr), 0.1)
    assert got1[0].shape == (T // block,) and torch.equal(got1[0], want[0][0])


def test_analyze_computes_the_pitch_and_the_autoencoder_takes_it(dd):
    sr, block, T, B, kind = pc.OFFLINE[0]
    x = pc.offline_case(sr, block, T, B, kind)[0]
    xg = torch.from_numpy(np.array(x)).cuda()
    F = T // block
    batch = dd.features.analyze(xg, None, sr, block)
    assert set(batch) == {"pitch", "loudness", "mfcc"}
    assert batch["pitch"].shape == (B, F, 1) and batch["loudness"].shape == (B, F, 1)
    assert batch["mfcc"].shape == (B, F, 30)
    assert torch.equal(batch["pitch"][..., 0], dd.core.extract_pitch(xg, sr, block))
    # fmin / fmax pass through; a given pitch behaves as before
    narrow = dd.features.analyze(xg, None, sr, block, fmin=100.0, fmax=1000.0)
    assert torch.equal(narrow["pitch"][..., 0], dd.core.extract_pitch(xg, sr, block, fmin=100.0, fmax=1000.0))
    given = dd.features.analyze(xg, batch["pitch"], sr, block)
    for k in batch:
        assert torch.equal(given[k], batch[k])
    torch.manual_seed(0)
    model = dd.DDSPAutoencoder(32, 16, 9, sr, block, False).cuda()
    with torch.no_grad():
        out = model(batch)
    assert out["signal"].shape == (B, T, 1) and bool(torch.isfinite(out["signal"]).all())


def test_bad_arguments_raise(dd):
    x = torch.zeros(2, 4096, device="cuda")
    with pytest.raises(RuntimeError, match="HIP device"):
        dd.core.extract_pitch(x.cpu(), 48000, 512)
    with pytest.raises(RuntimeError, match="audio"):
        dd.core.extract_pitch(x[None], 48000, 512)
    with pytest.raises(RuntimeError, match="block_size"):
        dd.core.extract_pitch(x, 48000, 0)
    with pytest.raises(RuntimeError, match="status 5"):
        dd.core.extract_pitch(x, 48000, 512, frame_length=1000)
    with pytest.raises(RuntimeError, match="status 5"):
        dd.core.extract_pitch(x, 48000, 512, frame_length=32, fmin=4000.0, fmax=24000.0)
    with pytest.raises(RuntimeError, match="status 1"):
        dd.core.extract_pitch(x[:, :1024], 48000, 512)  # reflect padding longer than the signal
    with pytest.raises(RuntimeError, match="no lag"):
        dd.core.extract_pitch(x, 48000, 512, fmin=3000.0, fmax=2000.5, frame_length=64)
    with pytest.raises(RuntimeError, match="positive"):
        dd.core.extract_pitch(x, 48000, 512, fmin=0.0)
