"""The analysis features on gfx950 (csrc/features.hip: core.extract_loudness, core.mfcc, features.analyze, the
torch.ops) against the fp64 restatement of tests/features_ref.py.

Accuracy gate, per case and feature: both the RMS and the maximum error of the GPU against the fp64 restatement
are <= 4 x the same statistic of the fp32 CPU restatement against fp64 on the same input (4 x because the GPU's
FFT factorisation — radix-16 Stockham against pocketfft — and its log differ from the CPU's).  Every figure is
printed before it is asserted (pytest -s shows them; DESIGN.md 3f records the measured ratios).
"""
import functools

import numpy as np
import pytest
import torch

import features_ref as fr

pytestmark = pytest.mark.gpu

MARGIN = 4.0
# (sample rate, block, T, B, input given as a 1-D tensor)
CASES = [
    (48000, 512, 2560, 2, False),
    (48000, 64, 2048, 3, False),   # 33 MFCC frames: an odd count, the last frame has no partner
    (16000, 160, 2080, 1, False),  # hop not a power of two; fmax equals Nyquist
    (44100, 256, 2304, 2, False),
    (48000, 512, 2660, 1, False),  # T % hop != 0
    (48000, 512, 4096, 1, True),   # a 1-D input
]


@pytest.fixture(scope="module")
def dd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ddsp_pytorch_amd
    ddsp_pytorch_amd._lib.load()
    return ddsp_pytorch_amd


def restate(x, sr, block):
    """Both features of x [B, T] item by item, in fp64 and fp32 -> dict of stacked arrays (computed once per
    input and shared; callers must not write to them)."""
    out = {}
    for name, fn in (("loudness", fr.loudness), ("mfcc", fr.mfcc)):
        for tag, dt in (("64", np.float64), ("32", np.float32)):
            a = np.stack([fn(x[b], sr, block, dtype=dt) for b in range(x.shape[0])]).astype(np.float64)
            a.setflags(write=False)
            out[name + tag] = a
    return out


@functools.lru_cache(maxsize=None)
def case_reference(sr, block, T, B):
    x = fr.make_signal(sr, T, B, seed=T + block)
    x.setflags(write=False)
    return x, restate(x, sr, block)


def stats(a, ref):
    e = np.asarray(a, dtype=np.float64) - ref
    return float(np.sqrt(np.mean(e ** 2))), float(np.abs(e).max())


def gate(label, got, ref64, ref32):
    """The accuracy gate of this file's docstring; prints the figures, then asserts."""
    g_rms, g_max = stats(got, ref64)
    c_rms, c_max = stats(ref32, ref64)
    print(f"{label}: gpu rms {g_rms:.3e} max {g_max:.3e} | fp32 cpu rms {c_rms:.3e} max {c_max:.3e} | "
          f"ratios rms {g_rms / c_rms:.2f} max {g_max / c_max:.2f}")
    assert g_rms <= MARGIN * c_rms, (label, "rms", g_rms, c_rms)
    assert g_max <= MARGIN * c_max, (label, "max", g_max, c_max)


@pytest.mark.parametrize("sr,block,T,B,one_d", CASES)
def test_accuracy_against_the_fp64_restatement(dd, sr, block, T, B, one_d):
    """Measured on MI355X (ratios GPU / fp32 CPU, rms and max, in the order of CASES): loudness 0.28/0.16,
    0.35/0.12, 0.33/0.29, 0.02/0.01, 0.60/0.71, 0.61/0.59; MFCC 0.44/0.44, 0.44/0.57, 0.61/0.85, 0.44/0.57,
    0.34/0.50, 0.64/1.00.  (With an fp32 transform the 1-D case's loudness came to 4.16/6.51, all of it in
    frame 0: DESIGN.md 3f.)"""
    x, ref = case_reference(sr, block, T, B)
    xg = torch.from_numpy(np.array(x)).cuda()
    if one_d:
        xg = xg[0]
    loud = dd.core.extract_loudness(xg, sr, block)
    mfcc = dd.core.mfcc(xg, sr, block)
    F = T // block
    assert loud.shape == ((F,) if one_d else (B, F))
    assert mfcc.shape == ((F + 1, 30) if one_d else (B, F + 1, 30))
    if one_d:
        loud, mfcc = loud[None], mfcc[None]
    tag = f"sr {sr} block {block} T {T} B {B}"
    gate(tag + " loudness", loud.cpu().numpy(), ref["loudness64"], ref["loudness32"])
    gate(tag + " mfcc", mfcc.cpu().numpy(), ref["mfcc64"], ref["mfcc32"])


# Every transform size is its own instantiation (one to three radix-16 passes, a final radix-1/2/4/8 pass, 2048 or
# 4096 points per workgroup), and the DCT launch loops differently once frames x n_mfcc passes one task per thread:
# (n_fft, n_mels, n_mfcc) at 16 kHz, hop n_fft/4 + 1 (odd), T no multiple of anything, B = 2.  Same gate.
SIZES = [(16, 4, 4), (32, 8, 5), (64, 16, 16), (128, 32, 13), (256, 64, 30), (512, 128, 30), (2048, 256, 256),
         (4096, 128, 30)]


@pytest.mark.parametrize("n_fft,n_mels,n_mfcc", SIZES)
def test_every_transform_size(dd, n_fft, n_mels, n_mfcc):
    sr, B = 16000, 2
    hop, T = n_fft // 4 + 1, 3 * n_fft + 37
    x = fr.make_signal(sr, T, B, seed=n_fft)
    xg = torch.from_numpy(x).cuda()
    kw = dict(n_mfcc=n_mfcc, n_fft=n_fft, n_mels=n_mels, fmin=20.0, fmax=8000.0)
    loud = dd.core.extract_loudness(xg, sr, hop, n_fft=n_fft).cpu().numpy()
    mfcc = dd.core.mfcc(xg, sr, hop, **kw).cpu().numpy()
    assert loud.shape == (B, T // hop) and mfcc.shape == (B, T // hop + 1, n_mfcc)
    for name, got, fn, args in (("loudness", loud, fr.loudness, dict(n_fft=n_fft)), ("mfcc", mfcc, fr.mfcc, kw)):
        r64 = np.stack([fn(x[b], sr, hop, dtype=np.float64, **args) for b in range(B)])
        r32 = np.stack([fn(x[b], sr, hop, dtype=np.float32, **args) for b in range(B)]).astype(np.float64)
        gate(f"n_fft {n_fft} n_mels {n_mels} n_mfcc {n_mfcc} {name}", got, r64, r32)


@functools.lru_cache(maxsize=None)
def top_db_reference():
    """One full-scale item, the same item x 1e-3, one whose last 40 % of samples are exact zeros."""
    sr, block, T = 48000, 512, 8192
    base = fr.make_signal(sr, T, 2, seed=7)
    tail = base[1].copy()
    tail[int(0.6 * T):] = 0.0
    x = np.stack([base[0], base[0] * np.float32(1e-3), tail])
    x.setflags(write=False)
    return sr, block, T, x, restate(x, sr, block)


def test_top_db_is_per_item_and_clamps(dd):
    sr, block, T, x, ref = top_db_reference()
    xg = torch.from_numpy(np.array(x)).cuda()
    mfcc, D = dd.core.mfcc(xg, sr, block, return_db=True)
    loud = dd.core.extract_loudness(xg, sr, block)
    mfcc, D, loud = mfcc.cpu().numpy(), D.cpu().numpy().astype(np.float64), loud.cpu().numpy()
    for b, name in enumerate(("full scale", "x 1e-3", "zero tail")):
        # each item against the restatement run on that item alone (a batch-wide maximum would clamp the
        # quiet item 60 dB too high)
        gate(f"top_db {name} mfcc", mfcc[b], ref["mfcc64"][b], ref["mfcc32"][b])
        gate(f"top_db {name} loudness", loud[b], ref["loudness64"][b], ref["loudness32"][b])
    # the zero-tailed item: frames whose 1024-sample window lies wholly in the zeros are silent
    first_zero = int(0.6 * T)
    silent = [f for f in range(T // block + 1) if f * block - 512 >= first_zero]
    assert len(silent) >= 5
    floor = D[2].max() - 80.0
    clamped = np.maximum(D[2], floor)
    # 10 log10(amin) = -100 to fp32: the device log10 of fl32(1e-10) may sit an ulp off -10 (4 ulps of 100 allowed)
    assert np.abs(D[2][silent] + 100.0).max() <= 4 * 7.63e-6
    assert (clamped[silent] == floor).all()
    frac = float((clamped == floor).mean())
    print(f"zero-tailed item: {frac:.3f} of the cells clamped at Dmax - 80 = {floor:.3f}")
    assert frac >= 0.25
    # ... and the kernel's clamp is that one: a silent frame's MFCC is the DCT of the constant floor
    want = fr.dct_matrix(30, 128) @ np.full(128, floor)
    assert np.abs(mfcc[2][silent] - want[None, :]).max() <= 1e-3 * 4  # |want[0]| ~ 500: a few fp32 ulps
    # its silent loudness frames (2048-sample windows): ln(1e-7) + mean(A-weighting)
    w = fr.a_weighting(fr.fft_frequencies(sr, 2048))
    silent_l = [f for f in range(T // block) if f * block - 1024 >= first_zero]
    assert len(silent_l) >= 3
    assert np.abs(loud[2][silent_l] - (np.log(1e-7) + w.mean())).max() <= 1e-5


def test_batch_independence_and_determinism(dd):
    sr, block, T, B = 48000, 64, 2048, 3
    x, _ = case_reference(sr, block, T, B)
    xg = torch.from_numpy(np.array(x)).cuda()
    loud, mfcc = dd.core.extract_loudness(xg, sr, block), dd.core.mfcc(xg, sr, block)
    assert torch.equal(loud, dd.core.extract_loudness(xg, sr, block))
    assert torch.equal(mfcc, dd.core.mfcc(xg, sr, block))
    for b in range(B):
        assert torch.equal(dd.core.extract_loudness(xg[b:b + 1], sr, block)[0], loud[b]), b
        assert torch.equal(dd.core.mfcc(xg[b:b + 1], sr, block)[0], mfcc[b]), b
        assert torch.equal(dd.core.mfcc(xg[b], sr, block), mfcc[b]), b


def test_non_contiguous_input(dd):
    sr, block, T, B = 44100, 256, 2304, 2
    x, _ = case_reference(sr, block, T, B)
    xg = torch.from_numpy(np.array(x)).cuda()
    wide = torch.zeros(B, 2 * T, device="cuda")
    wide[:, ::2] = xg
    view = wide[:, ::2]
    assert not view.is_contiguous()
    assert torch.equal(dd.core.extract_loudness(view, sr, block), dd.core.extract_loudness(xg, sr, block))
    assert torch.equal(dd.core.mfcc(view, sr, block), dd.core.mfcc(xg, sr, block))


def test_torch_ops_return_the_python_functions_bits(dd):
    from ddsp_pytorch_amd import script
    script.load_ops()
    sr, block, T, B = 48000, 512, 2560, 2
    x, _ = case_reference(sr, block, T, B)
    xg = torch.from_numpy(np.array(x)).cuda()
    (w,) = dd.core._feature_tables("a_weighting", (float(sr), 2048), xg.device,
                                   lambda: (dd.core.a_weighting_table(sr, 2048),))
    assert torch.equal(torch.ops.ddsp_hip.loudness(xg, w, 2048, block), dd.core.extract_loudness(xg, sr, block))
    assert torch.equal(torch.ops.ddsp_hip.loudness(xg[0], w, 2048, block), dd.core.extract_loudness(xg[0], sr, block))
    # no table: plain mean log magnitude — the weighted result minus the table's mean, to fp32 rounding
    plain = torch.ops.ddsp_hip.loudness(xg, None, 2048, block)
    assert (plain + w.double().mean() - dd.core.extract_loudness(xg, sr, block)).abs().max() < 1e-4
    tabs = dd.core.mfcc_tables(sr, 30, 1024, 128, 20.0, 8000.0, xg.device)
    assert torch.equal(torch.ops.ddsp_hip.mfcc(xg, *tabs, 1024, block, 80.0), dd.core.mfcc(xg, sr, block))


def test_analyze_feeds_the_autoencoder(dd):
    sr, block, T, B = 48000, 512, 8192, 2
    x = torch.from_numpy(fr.make_signal(sr, T, B, seed=3)).cuda()
    F = T // block
    pitch = torch.full((B, F), 220.0, device="cuda")
    batch = dd.features.analyze(x, pitch, sr, block)
    assert set(batch) == {"pitch", "loudness", "mfcc"}
    assert batch["pitch"].shape == (B, F, 1) and batch["loudness"].shape == (B, F, 1)
    assert batch["mfcc"].shape == (B, F, 30)
    assert torch.equal(batch["loudness"][..., 0], dd.core.extract_loudness(x, sr, block))
    assert torch.equal(batch["mfcc"], dd.core.mfcc(x, sr, block)[:, :F])
    torch.manual_seed(0)
    model = dd.DDSPAutoencoder(32, 16, 9, sr, block, False).cuda()
    with torch.no_grad():
        out = model(batch)
    assert out["signal"].shape == (B, T, 1) and bool(torch.isfinite(out["signal"]).all())
    mean, std = -6.5, 1.75
    normed = dd.features.analyze(x, pitch, sr, block, mean_loudness=mean, std_loudness=std)
    assert (normed["loudness"] - (batch["loudness"] - mean) / std).abs().max() <= 1e-6
    assert torch.equal(normed["mfcc"], batch["mfcc"]) and torch.equal(normed["pitch"], batch["pitch"])
    # an input that requires grad is analysed detached
    xr = x.clone().requires_grad_(True)
    assert not dd.core.extract_loudness(xr, sr, block).requires_grad
    assert torch.equal(dd.core.mfcc(xr, sr, block), dd.core.mfcc(x, sr, block))


def test_warmed_up_calls_capture_into_a_hip_graph(dd):
    """After the first call built the tables nothing synchronises with the host: both features record into
    one HIP graph on one stream, and its replay on new audio gives the eager result's bits."""
    sr, block, T, B = 48000, 512, 4096, 2
    x = torch.from_numpy(fr.make_signal(sr, T, B, seed=11)).cuda()
    y = torch.from_numpy(fr.make_signal(sr, T, B, seed=12)).cuda()
    want = dd.core.extract_loudness(y, sr, block), dd.core.mfcc(y, sr, block)  # (also the warm-up)
    buf = x.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = dd.core.extract_loudness(buf, sr, block), dd.core.mfcc(buf, sr, block)
    buf.copy_(y)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
