"""The Viterbi-decoded pitch tracker on gfx950 (csrc/pitch_viterbi.hip: core.pitch_salience, core.viterbi_path,
core.track_pitch, features.analyze(viterbi=True), torch.ops.ddsp_hip.pitch_salience / pitch_viterbi) against the
restatement of tests/viterbi_ref.py.

The decode alone is bit for bit: every operation is one fp64 addition or a comparison, so from the same costs the
path is int32-equal to the restatement's, f0 is the gather of f0c and confidence is 1 - cost, exactly.

The salience's gate is DESIGN.md 3f-pitch's: ``lag`` equals the fp64 restatement's except in at most F NB // 50
entries per item; over the equal entries the cost's absolute and f0c's relative error, RMS and maximum, are each
<= 4 x max(the fp32 restatement's same statistic, 2^-24).  Every figure is printed before it is asserted (pytest -s).

Measured on MI355X (profiles/viterbi_gate.txt): all 672 decoded items equal the restatement;
no lag of any salience case differs and cost and f0c equal the fp64 restatement's fp32 values in every entry (error
0 against bounds of 2.4e-7 and more); on octave and bursts the path equals the fp64 restatement's on all 93 frames,
the decoded f0 is at most 6.2 and 29.3 cents from truth where extract_pitch is off on 58 and 7 of 87 frames.
"""
import numpy as np
import pytest
import torch

import viterbi_cases as vc
import viterbi_ref as vr

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


# ---------------- the decode alone, bit for bit ----------------
def _costs(kind, rng, F, NB):
    if kind == "uniform":
        return rng.uniform(0.0, 1.0, size=(F, NB)).astype(np.float32)
    if kind == "shallow":  # costs small against lambda * k: the path weighs every move
        return rng.uniform(0.0, 0.05, size=(F, NB)).astype(np.float32)
    if kind == "quantised":
        return (rng.integers(0, 5, size=(F, NB)) / 4.0).astype(np.float32)
    return np.ones((F, NB), dtype=np.float32)


def _decode_gpu(dd, cost, f0c, lam, R):
    f0, conf, path = dd.core.viterbi_path(torch.from_numpy(cost).cuda(), torch.from_numpy(f0c).cuda(), lam, R)
    assert f0.dtype == torch.float32 and conf.dtype == torch.float32 and path.dtype == torch.int32
    return f0.cpu().numpy(), conf.cpu().numpy(), path.cpu().numpy()


@pytest.mark.parametrize("NB", [1, 2, 63, 64, 65, 256, 1024])
def test_decode_is_bit_exact(dd, NB):
    G = int(dd._lib.query("pitch_viterbi_chunk_frames", NB))
    assert G == min(32768 // NB, 512) and G * NB <= 32768
    rng = np.random.default_rng(100 + NB)
    n = 0
    for F in (1, 2, G - 1, G, G + 1, 2 * G + 3):
        for R in (0, 1, 12, 127):
            # (costs per item, lambda): a batch of three at the default lambda; one item of dense ties at 1/4
            for kinds, lam in ((("uniform", "shallow", "ones"), 0.02), (("quantised",), 0.25)):
                cost = np.stack([_costs(k, rng, F, NB) for k in kinds])
                f0c = rng.uniform(50.0, 2000.0, size=cost.shape).astype(np.float32)
                f0, conf, path = _decode_gpu(dd, cost, f0c, lam, R)
                assert path.shape == f0.shape == conf.shape == (len(kinds), F)
                t = np.arange(F)
                for b, kind in enumerate(kinds):
                    want = vr.viterbi(cost[b], lam, R)
                    label = (NB, F, R, kind)
                    assert np.array_equal(path[b], want), (label, int((path[b] != want).sum()))
                    assert np.array_equal(f0[b], f0c[b][t, want]), label
                    assert np.array_equal(conf[b], np.float32(1.0) - cost[b][t, want]), label
                    if kind == "ones":
                        assert not path[b].any(), label
                    n += 1
                if len(kinds) == 3 and R == 12:
                    # item 1 of the batch equals the same item run alone; a second run gives the same bits
                    alone = _decode_gpu(dd, cost[1:2], f0c[1:2], lam, R)
                    again = _decode_gpu(dd, cost, f0c, lam, R)
                    for a, b3, c3 in zip(alone, (f0, conf, path), again):
                        assert np.array_equal(a[0], b3[1]) and np.array_equal(b3, c3), (NB, F, R)
    print(f"NB {NB}: chunk {G} frames; {n} decoded items equal the restatement bit for bit")


def test_decode_accepts_one_item_without_a_batch_axis(dd):
    rng = np.random.default_rng(5)
    cost = _costs("uniform", rng, 9, 17)
    f0c = rng.uniform(50.0, 2000.0, size=cost.shape).astype(np.float32)
    f0, conf, path = dd.core.viterbi_path(torch.from_numpy(cost).cuda(), torch.from_numpy(f0c).cuda())
    assert f0.shape == conf.shape == path.shape == (9,)
    assert np.array_equal(path.cpu().numpy(), vr.viterbi(cost, 0.02, 12))


# ---------------- the salience ----------------
def _salience_gate(label, cost, f0c, lag, ref):
    """The gate of this file's docstring on [B, F, NB] arrays; prints the figures, then asserts."""
    assert cost.dtype == np.float32 and f0c.dtype == np.float32 and lag.dtype == np.int32
    assert cost.shape == f0c.shape == lag.shape == ref["lag64"].shape
    assert np.isfinite(cost).all() and np.isfinite(f0c).all()
    assert (cost >= 0.0).all() and (cost <= 1.0).all()
    B, F, NB = lag.shape
    same = lag == ref["lag64"]
    same32 = ref["lag32"] == ref["lag64"]
    n_diff = (~same).sum(axis=(1, 2))
    print(f"{label}: {F} x {NB} entries per item, {n_diff.tolist()} with another lag than the fp64 restatement's "
          f"(allowed {F * NB // 50})")
    figures = []
    for name, got, r64, r32, rel in (("cost abs", cost, ref["cost64"], ref["cost32"], False),
                                     ("f0c rel", f0c, ref["f0c64"], ref["f0c32"], True)):
        r64 = r64.astype(np.float64)
        scale = r64 if rel else 1.0
        g = _stats(((got.astype(np.float64) - r64) / scale)[same])
        c = _stats(((r32.astype(np.float64) - r64) / scale)[same32])
        for stat, gv, cv in zip(("rms", "max"), g, c):
            bound = MARGIN * max(cv, FLOOR)
            print(f"{label}: {name} {stat}: gpu {gv:.3e} | fp32 cpu {cv:.3e} | bound {bound:.3e}")
            figures.append((name, stat, gv, bound))
    assert (n_diff <= F * NB // 50).all(), (label, n_diff.tolist())
    for name, stat, gv, bound in figures:
        assert gv <= bound, (label, name, stat, gv, bound)


@pytest.mark.parametrize("case", list(vc.SALIENCE_CASES))
def test_salience_against_the_fp64_restatement(dd, case):
    name, L = vc.SALIENCE_CASES[case]
    x = torch.from_numpy(np.array(vc.audio(name))).cuda()
    ref = vc.restated(case)
    cost, f0c, lag, f0, conf, period = dd.core.pitch_salience(x, vc.SR, vc.HOP, frame_length=L, return_lag=True,
                                                              return_raw=True)
    _salience_gate(case, cost.cpu().numpy(), f0c.cpu().numpy(), lag.cpu().numpy(), ref)
    # the raw outputs of the same launch are ddsp_hip_pitch's, bit for bit
    e0, ec, ep = dd.core.extract_pitch(x, vc.SR, vc.HOP, frame_length=L, return_confidence=True, return_period=True)
    assert torch.equal(f0, e0) and torch.equal(conf, ec) and torch.equal(period, ep)
    # without them, and without the lag, the salience is the same bits
    c2, g2 = dd.core.pitch_salience(x, vc.SR, vc.HOP, frame_length=L)
    assert torch.equal(c2, cost) and torch.equal(g2, f0c)
    if case == "silence":
        tau_min, tau_max, (lo, hi) = vc.table(L)
        assert (cost[1] == 1.0).all() and torch.isfinite(f0c[1]).all() and (conf[1] == 0.0).all()
        assert np.array_equal(lag[1].cpu().numpy(), np.broadcast_to(lo, lag[1].shape))
        _, dconf, dpath = dd.core.viterbi_path(cost, f0c)
        assert (dconf[1] == 0.0).all() and not dpath[1].any()
    if case == "clean":
        # an item's bits do not depend on its batch; a 1-D signal drops the batch axis
        c1, g1, l1 = dd.core.pitch_salience(x[2], vc.SR, vc.HOP, return_lag=True)
        assert c1.shape == cost.shape[1:]
        assert torch.equal(c1, cost[2]) and torch.equal(g1, f0c[2]) and torch.equal(l1, lag[2])


# ---------------- end to end ----------------
@pytest.mark.parametrize("name,raw_off_at_least", [("octave", 44), ("bursts", 5)])
def test_track_pitch_end_to_end(dd, name, raw_off_at_least):
    x = torch.from_numpy(np.array(vc.audio(name))).cuda()
    truth = vc.signals()[name][1]
    ref = vc.restated(name)
    f0, conf, path = dd.core.track_pitch(x, vc.SR, vc.HOP, return_confidence=True, return_path=True)
    assert f0.shape == conf.shape == path.shape == (1, vc.F)
    want = vr.viterbi(ref["cost64"][0], 0.02, 12)
    n_diff = int((path[0].cpu().numpy() != want).sum())
    dec = vc.cents(f0[0].cpu().numpy(), truth)[vc.INTERIOR]
    raw = vc.cents(dd.core.extract_pitch(x, vc.SR, vc.HOP)[0].cpu().numpy(), truth)[vc.INTERIOR]
    n_raw = int((raw > 50.0).sum())
    print(f"{name}: path differs from the fp64 restatement's in {n_diff} of {vc.F} frames; decoded max "
          f"{dec.max():.1f} cents; extract_pitch more than 50 cents off on {n_raw} of {raw.size} interior frames")
    assert n_diff <= vc.F // 50
    assert (dec <= 50.0).all()
    assert n_raw >= raw_off_at_least
    # a 1-D signal; f0 alone by default
    f1 = dd.core.track_pitch(x[0], vc.SR, vc.HOP)
    assert f1.shape == (vc.F,) and torch.equal(f1, f0[0])


def test_analyze_takes_the_decoded_track_on_request(dd):
    x = torch.from_numpy(np.array(vc.audio("clean"))).cuda()
    a = dd.features.analyze(x, None, vc.SR, vc.HOP, viterbi=True)
    assert a["pitch"].shape == (4, vc.F, 1)
    assert torch.equal(a["pitch"][..., 0], dd.core.track_pitch(x, vc.SR, vc.HOP))
    for kw in ({}, {"viterbi": False}):
        b = dd.features.analyze(x, None, vc.SR, vc.HOP, **kw)
        assert torch.equal(b["pitch"][..., 0], dd.core.extract_pitch(x, vc.SR, vc.HOP))
        assert torch.equal(b["loudness"], a["loudness"]) and torch.equal(b["mfcc"], a["mfcc"])


def test_torch_ops_match_core(dd):
    from ddsp_pytorch_amd import script
    script.load_ops()
    x = torch.from_numpy(np.array(vc.audio("clean"))).cuda()
    tau_min, tau_max, lo, hi = dd.core.pitch_bins(vc.SR, vc.FMIN, vc.FMAX, vc.L)
    lo_d = torch.tensor(lo, dtype=torch.int32, device="cuda")
    hi_d = torch.tensor(hi, dtype=torch.int32, device="cuda")
    cost, f0c, lag = torch.ops.ddsp_hip.pitch_salience(x, lo_d, hi_d, vc.L, vc.HOP, tau_min, tau_max, float(vc.SR))
    c, g, l = dd.core.pitch_salience(x, vc.SR, vc.HOP, return_lag=True)
    assert torch.equal(cost, c) and torch.equal(f0c, g) and torch.equal(lag, l)
    f0, conf, path = torch.ops.ddsp_hip.pitch_viterbi(cost, f0c, 0.02, 12)
    for got, want in zip((f0, conf, path), dd.core.viterbi_path(c, g)):
        assert got.dtype == want.dtype and torch.equal(got, want)
    c1, _, _ = torch.ops.ddsp_hip.pitch_salience(x[1], lo_d, hi_d, vc.L, vc.HOP, tau_min, tau_max, float(vc.SR))
    assert torch.equal(c1, c[1])


def test_track_pitch_in_a_captured_graph(dd):
    x = torch.from_numpy(np.array(vc.audio("clean"))).cuda()
    eager = [t.clone() for t in dd.core.track_pitch(x, vc.SR, vc.HOP, return_confidence=True, return_path=True)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        dd.core.track_pitch(x, vc.SR, vc.HOP)  # warm-up on the capture stream (the tables are cached already)
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            out = dd.core.track_pitch(x, vc.SR, vc.HOP, return_confidence=True, return_path=True)
    # the capture went through: no call synchronised with the host, and nothing but the two launches and torch's
    # allocations was recorded (no entry point here issues a memset or a copy; the workspace needs no zeroing)
    for _ in range(3):
        for t in out:
            t.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(out, eager):
            assert torch.equal(got, want)
