"""The streamed Viterbi pitch tracker on gfx950 (csrc/stream_pitch_viterbi.hip: core.stream_pitch_salience,
core.stream_viterbi_path, core.stream_track_pitch, features.StreamAnalyzer(viterbi=True),
torch.ops.ddsp_hip.pitch_salience_stream / pitch_viterbi_stream) against the restatements of
tests/stream_viterbi_ref.py and tests/viterbi_ref.py.

The decode alone is bit for bit: every operation is one fp64 addition or a comparison, so from the same costs the
path is int32-equal to the restatement's, f0 is the gather of f0c and confidence is 1 - cost, exactly — whatever the
cut into calls, the batch around an item, or a second run of a call before the advance.

The salience's gate is test_gpu_pitch_viterbi.py's, the function itself: ``lag`` equals the fp64
restatement's except in at most F NB // 50 entries per item; over the equal entries the cost's absolute and f0c's
relative error, RMS and maximum, are each <= 4 x max(the fp32 restatement's same statistic, 2^-24).

End to end the cents gates are those of tests/test_stream_viterbi_ref.py (the fp64 restatement passes them there)
and the path may differ from the fp64 restatement's online path in at most F // 50 emitted frames, the offline
test's allowance.  Every figure is printed before it is asserted (pytest -s).
"""
import numpy as np
import pytest
import torch

import stream_viterbi_cases as sc
import stream_viterbi_ref as sv
import viterbi_cases as vc
from test_gpu_pitch_viterbi import _salience_gate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ddsp_pytorch_amd
    ddsp_pytorch_amd._lib.load()
    return ddsp_pytorch_amd


# ---------------- the decode alone, bit for bit ----------------
def _costs(kind, rng, F, NB):
    if kind == "uniform":
        return rng.uniform(0.0, 1.0, size=(F, NB)).astype(np.float32)
    if kind == "shallow":  # costs small against lambda * k: the path weighs every move
        return rng.uniform(0.0, 0.05, size=(F, NB)).astype(np.float32)
    if kind == "quantised":
        return (rng.integers(0, 5, size=(F, NB)) / 4.0).astype(np.float32)
    return np.ones((F, NB), dtype=np.float32)


def _stream_gpu(dd, cost, f0c, R, D, lam, J, state=None, twice=False):
    """cost, f0c [B, F, NB] cut into calls of R frames -> (f0, confidence, path) numpy [B, F].  ``twice``: every
    call runs twice before its advance and both runs' outputs must agree."""
    B, F, NB = cost.shape
    c, g = torch.from_numpy(cost).cuda(), torch.from_numpy(f0c).cuda()
    st = state if state is not None else dd.core.ViterbiStreamState(B, "cuda", R, NB, D)
    outs = []
    for a in range(0, F, R):
        args = (c[:, a:a + R].contiguous(), g[:, a:a + R].contiguous(), st, lam, J)
        out = dd.core.stream_viterbi_path(*args)
        if twice:
            for x, y in zip(out, dd.core.stream_viterbi_path(*args)):
                assert torch.equal(x, y), a
        dd.core.stream_advance(st)
        outs.append(out)
    f0, conf, path = (torch.cat([o[k] for o in outs], 1) for k in range(3))
    assert f0.dtype == torch.float32 and conf.dtype == torch.float32 and path.dtype == torch.int32
    assert f0.shape == conf.shape == path.shape == (B, F)
    return f0.cpu().numpy(), conf.cpu().numpy(), path.cpu().numpy()


def _check_items(label, got, cost, f0c, kinds, R, D, lam, J):
    f0, conf, path = got
    for b, kind in enumerate(kinds):
        w0, wc, wp = sv.stream(cost[b], f0c[b], R, lam, J, D)
        assert np.array_equal(path[b], wp), (label, kind, int((path[b] != wp).sum()))
        m = np.maximum(np.arange(len(wp)) - D, 0)
        assert np.array_equal(f0[b], f0c[b][m, wp]) and np.array_equal(f0[b], w0), (label, kind)
        assert np.array_equal(conf[b], np.float32(1.0) - cost[b][m, wp]) and np.array_equal(conf[b], wc), (label, kind)
        if kind == "ones":
            assert not path[b].any(), (label, kind)


@pytest.mark.parametrize("NB", [1, 63, 64, 65, 256, 1024])
def test_decode_is_bit_exact(dd, NB):
    rng = np.random.default_rng(300 + NB)
    n = 0
    for R in (1, 2, 32):
        for D in (0, 1, 3, 64):
            K = 2 * (D + R) // R + 1  # K R > 2 (D + R): the ring wraps
            F = K * R
            assert F > 2 * (D + R)
            for J in (0, 1, 12, 127):
                # (costs per item, lambda): a batch of three at the default lambda; one item of dense ties at 1/4
                for kinds, lam in ((("uniform", "shallow", "ones"), 0.02), (("quantised",), 0.25)):
                    cost = np.stack([_costs(k, rng, F, NB) for k in kinds])
                    f0c = rng.uniform(50.0, 2000.0, size=cost.shape).astype(np.float32)
                    got = _stream_gpu(dd, cost, f0c, R, D, lam, J)
                    _check_items((NB, R, D, J), got, cost, f0c, kinds, R, D, lam, J)
                    n += len(kinds)
    print(f"NB {NB}: {n} streamed items equal the restatement bit for bit")


def test_decode_batch_cut_rerun_and_reset(dd):
    rng = np.random.default_rng(11)
    NB, J, lam = 65, 12, 0.02
    for D in (0, 3, 64):
        K = 2 * (D + 2) // 2 + 1
        F = 2 * K
        kinds = ("uniform", "shallow", "quantised")
        cost = np.stack([_costs(k, rng, F, NB) for k in kinds])
        f0c = rng.uniform(50.0, 2000.0, size=cost.shape).astype(np.float32)
        two = _stream_gpu(dd, cost, f0c, 2, D, lam, J)
        # item 1 of the batch equals the item run alone
        alone = _stream_gpu(dd, cost[1:2], f0c[1:2], 2, D, lam, J)
        # R = 1 over 2 K calls equals R = 2 over K calls
        one = _stream_gpu(dd, cost, f0c, 1, D, lam, J)
        # every call run twice before its advance: the same outputs, and the stream continues as if it had run once
        st = dd.core.ViterbiStreamState(3, "cuda", 2, NB, D)
        again = _stream_gpu(dd, cost, f0c, 2, D, lam, J, state=st, twice=True)
        assert int(st.counter.item()) == K
        # after reset() the stream repeats itself
        st.reset()
        assert int(st.counter.item()) == 0 and not st.buf.any()
        reset = _stream_gpu(dd, cost, f0c, 2, D, lam, J, state=st)
        for a, t, o, g, r in zip(alone, two, one, again, reset):
            assert np.array_equal(a[0], t[1]), D
            assert np.array_equal(o, t) and np.array_equal(g, t) and np.array_equal(r, t), D
    # "fresh" comes from the counter, not from the stored bits: a state full of garbage at call 0 is a fresh stream
    st = dd.core.ViterbiStreamState(3, "cuda", 2, NB, 64)
    st.buf.fill_(0x7F)
    dirty = _stream_gpu(dd, cost, f0c, 2, 64, lam, J, state=st)
    for d, t in zip(dirty, two):
        assert np.array_equal(d, t)
    # a state for another shape is refused by the host layer
    with pytest.raises(RuntimeError, match="another batch"):
        dd.core.stream_viterbi_path(torch.zeros(3, 2, NB + 1, device="cuda"), torch.zeros(3, 2, NB + 1, device="cuda"),
                                    st)


# ---------------- the salience ----------------
def _salience_stream(dd, case):
    """The case's calls through core.stream_pitch_salience (lag and raw outputs asked for) and, on a state of its
    own, core.stream_pitch: (cost, f0c, lag [B, K R, NB], raw and pitch (f0, confidence, period) [B, K R])."""
    _, K, L, hop = sc.SALIENCE_CASES[case]
    x = torch.from_numpy(np.array(sc.audio(case))).cuda()
    B = x.shape[0]
    ring = dd.core.FeatureStreamState(B, "cuda", sc.N, L, hop)
    ring2 = dd.core.FeatureStreamState(B, "cuda", sc.N, L, hop)
    sal, yin = [], []
    for k in range(K):
        xc = x[:, k * sc.N:(k + 1) * sc.N]
        out = dd.core.stream_pitch_salience(xc, vc.SR, hop, ring, frame_length=L, return_lag=True, return_raw=True)
        if k == 1:  # a call run twice before the advance, and without the optional outputs: the same bits
            for a, b in zip(out, dd.core.stream_pitch_salience(xc, vc.SR, hop, ring, frame_length=L, return_lag=True,
                                                               return_raw=True)):
                assert torch.equal(a, b)
            c2, g2 = dd.core.stream_pitch_salience(xc, vc.SR, hop, ring, frame_length=L)
            assert torch.equal(c2, out[0]) and torch.equal(g2, out[1])
        sal.append(out)
        yin.append(dd.core.stream_pitch(xc, vc.SR, hop, ring2, frame_length=L, return_confidence=True,
                                        return_period=True))
        dd.core.stream_advance(ring)
        dd.core.stream_advance(ring2)
    sal = [torch.cat([o[i] for o in sal], 1) for i in range(6)]
    yin = [torch.cat([o[i] for o in yin], 1) for i in range(3)]
    return sal, yin


@pytest.mark.parametrize("case", ["octave", "clean", "silence", "L64", "hop256"])
def test_salience_against_the_fp64_restatement(dd, case):
    _, K, L, hop = sc.SALIENCE_CASES[case]
    ref = sc.restated(case)
    (cost, f0c, lag, f0, conf, period), yin = _salience_stream(dd, case)
    assert cost.shape[1] == K * (sc.N // hop)
    _salience_gate(case, cost.cpu().numpy(), f0c.cpu().numpy(), lag.cpu().numpy(), ref)
    # the raw outputs of the same launch are ddsp_hip_stream_pitch's, bit for bit
    assert period.dtype == torch.int32
    for got, want in zip((f0, conf, period), yin):
        assert got.dtype == want.dtype and torch.equal(got, want)
    if case == "silence":
        _, _, (lo, hi) = vc.table(L)
        assert (cost[1] == 1.0).all() and torch.isfinite(f0c[1]).all() and (conf[1] == 0.0).all()
        assert np.array_equal(lag[1].cpu().numpy(), np.broadcast_to(lo, lag[1].shape))
        R = sc.N // hop
        st = dd.core.ViterbiStreamState(2, "cuda", R, cost.shape[2], 3)
        for k in range(K):
            _, dconf, dpath = dd.core.stream_viterbi_path(cost[:, k * R:(k + 1) * R], f0c[:, k * R:(k + 1) * R], st)
            dd.core.stream_advance(st)
            assert (dconf[1] == 0.0).all() and not dpath[1].any()
    if case == "clean":  # an item's bits do not depend on its batch
        x = torch.from_numpy(np.array(sc.audio(case))).cuda()
        ring = dd.core.FeatureStreamState(1, "cuda", sc.N, L, hop)
        for k in range(3):
            c1, g1, l1 = dd.core.stream_pitch_salience(x[2:3, k * sc.N:(k + 1) * sc.N], vc.SR, hop, ring,
                                                       return_lag=True)
            dd.core.stream_advance(ring)
            fr = slice(2 * k, 2 * k + 2)
            assert torch.equal(c1[0], cost[2, fr]) and torch.equal(g1[0], f0c[2, fr]) and torch.equal(l1[0], lag[2, fr])


# ---------------- end to end ----------------
@pytest.mark.parametrize("name,raw_off_at_least,over_at_lag0", [("octave", 44, 0), ("bursts", 5, 2)])
def test_stream_analyzer_end_to_end(dd, name, raw_off_at_least, over_at_lag0):
    _, K, L, hop = sc.SALIENCE_CASES[name]
    R = sc.N // hop
    F = K * R
    x = torch.from_numpy(np.array(sc.audio(name))).cuda()
    plain = dd.features.StreamAnalyzer(vc.SR, hop, sc.N, pitch=True)
    raw = torch.cat([plain(x[:, k * sc.N:(k + 1) * sc.N])["pitch"] for k in range(K)], 1)[0, :, 0].cpu().numpy()
    raw_cents = sc.interior(name, raw, 0)
    n_raw = int((raw_cents > 50.0).sum())
    print(f"{name}: StreamAnalyzer(pitch=True) more than 50 cents off on {n_raw} of {raw_cents.size} interior frames")
    figures = {}
    for D in (0, 4):
        an = dd.features.StreamAnalyzer(vc.SR, hop, sc.N, pitch=True, viterbi=True, pitch_lag=D)
        assert an.delay_frames["pitch"] == an.delay_frames["loudness"] + D
        assert an.pitch_state is not an.loudness_state and an.viterbi_state.lag == D
        assert an.viterbi_state.counter is an.counter and an.pitch_state.counter is an.counter
        ring = dd.core.FeatureStreamState(1, "cuda", sc.N, L, hop)
        vit = dd.core.ViterbiStreamState(1, "cuda", R, an.viterbi_state.n_bins, D, counter=ring.counter)
        f0s, paths = [], []
        for k in range(K):
            xc = x[:, k * sc.N:(k + 1) * sc.N]
            out = an(xc)
            f0, conf, path = dd.core.stream_track_pitch(xc, vc.SR, hop, ring, vit, return_confidence=True,
                                                        return_path=True)
            dd.core.stream_advance(ring)
            assert out["pitch"].shape == out["confidence"].shape == (1, R, 1)
            assert torch.equal(out["pitch"][..., 0], f0) and torch.equal(out["confidence"][..., 0], conf), (D, k)
            assert torch.equal(out["loudness"], plain_loudness(dd, name, hop, K)[k]), (D, k)
            f0s.append(f0)
            paths.append(path)
        f0 = torch.cat(f0s, 1)[0].cpu().numpy()
        path = torch.cat(paths, 1)[0].cpu().numpy()
        n_diff = int((path != sc.online(name, D)[2]).sum())
        dec = sc.interior(name, f0, D)
        figures[D] = (n_diff, dec)
        print(f"{name} lag {D}: path differs from the fp64 restatement's online path in {n_diff} of {F} emitted frames "
              f"(allowed {F // 50}); {int((dec > 50.0).sum())} of {dec.size} interior frames more than 50 cents off, "
              f"max {dec.max():.1f} cents")
        # reset() resets the decode state too: the first call repeats itself
        an.reset()
        assert int(an.counter.item()) == 0 and not an.viterbi_state.buf.any() and not an.pitch_state.buf.any()
        again = an(x[:, :sc.N])
        assert torch.equal(again["pitch"][0, :, 0], torch.cat(f0s, 1)[0, :R])
    assert n_raw >= raw_off_at_least
    for D in (0, 4):
        assert figures[D][0] <= F // 50, D
    assert int((figures[0][1] > 50.0).sum()) <= over_at_lag0
    assert (figures[4][1] <= 50.0).all()


_LOUDNESS = {}


def plain_loudness(dd, name, hop, K):
    """StreamAnalyzer()'s loudness of the case, call by call: what viterbi=True must leave as it is."""
    if name not in _LOUDNESS:
        x = torch.from_numpy(np.array(sc.audio(name))).cuda()
        an = dd.features.StreamAnalyzer(vc.SR, hop, sc.N)
        _LOUDNESS[name] = [an(x[:, k * sc.N:(k + 1) * sc.N])["loudness"] for k in range(K)]
    return _LOUDNESS[name]


def test_stream_analyzer_aligned_takes_loudness_and_mfcc_from_their_launch(dd):
    hop, K = 256, 6
    x = torch.from_numpy(np.array(sc.audio("octave"))).cuda()
    base = dd.features.StreamAnalyzer(vc.SR, hop, sc.N, aligned=True)
    an = dd.features.StreamAnalyzer(vc.SR, hop, sc.N, aligned=True, pitch=True, viterbi=True, pitch_lag=2)
    sep = dd.features.StreamAnalyzer(vc.SR, hop, sc.N, pitch=True, viterbi=True, pitch_lag=2)
    assert an.mfcc_state is an.loudness_state and an.pitch_state is not an.loudness_state
    assert an.delay_frames["pitch"] == an.delay_frames["mfcc"] + 2 == an.delay_frames["loudness"] + 2
    for k in range(K):
        xc = x[:, k * sc.N:(k + 1) * sc.N]
        a, b, s = base(xc), an(xc), sep(xc)
        assert torch.equal(a["loudness"], b["loudness"]) and torch.equal(a["mfcc"], b["mfcc"]), k
        assert torch.equal(b["pitch"], s["pitch"]) and torch.equal(b["confidence"], s["confidence"]), k
    assert int(an.counter.item()) == K


# ---------------- torch ops, captured graph ----------------
def test_torch_ops_match_core(dd):
    from ddsp_pytorch_amd import script
    script.load_ops()
    hop, D = 256, 3
    R = sc.N // hop
    x = torch.from_numpy(np.array(sc.audio("clean"))).cuda()
    B = x.shape[0]
    tau_min, tau_max, lo, hi = dd.core.pitch_bins(vc.SR, vc.FMIN, vc.FMAX, vc.L)
    lo_d = torch.tensor(lo, dtype=torch.int32, device="cuda")
    hi_d = torch.tensor(hi, dtype=torch.int32, device="cuda")
    rings = [dd.core.FeatureStreamState(B, "cuda", sc.N, vc.L, hop) for _ in range(2)]
    vits = [dd.core.ViterbiStreamState(B, "cuda", R, len(lo), D, counter=r.counter) for r in rings]
    for k in range(4):
        xc = x[:, k * sc.N:(k + 1) * sc.N]
        cost, f0c, lag = torch.ops.ddsp_hip.pitch_salience_stream(xc, lo_d, hi_d, vc.L, hop, tau_min, tau_max,
                                                                  float(vc.SR), rings[0].counter, rings[0].buf)
        want = dd.core.stream_pitch_salience(xc, vc.SR, hop, rings[1], return_lag=True)
        for got, w in zip((cost, f0c, lag), want):
            assert got.dtype == w.dtype and torch.equal(got, w), k
        got = torch.ops.ddsp_hip.pitch_viterbi_stream(cost, f0c, 0.02, 12, D, vits[0].counter, vits[0].buf)
        for g, w in zip(got, dd.core.stream_viterbi_path(want[0], want[1], vits[1])):
            assert g.dtype == w.dtype and torch.equal(g, w), k
        for r in rings:
            dd.core.stream_advance(r)
    assert torch.equal(rings[0].buf, rings[1].buf) and torch.equal(vits[0].buf, vits[1].buf)


def test_analyzer_call_in_a_captured_graph(dd):
    hop, K, D = 256, 8, 2
    x = torch.from_numpy(np.array(sc.audio("octave"))).cuda()
    keys = ("loudness", "mfcc", "pitch", "confidence")
    eager = dd.features.StreamAnalyzer(vc.SR, hop, sc.N, pitch=True, viterbi=True, pitch_lag=D)
    want = [eager(x[:, k * sc.N:(k + 1) * sc.N]) for k in range(K)]
    an = dd.features.StreamAnalyzer(vc.SR, hop, sc.N, pitch=True, viterbi=True, pitch_lag=D)
    buf = torch.zeros(1, sc.N, device="cuda")
    an(buf)  # warm-up (the tables)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    # the capture goes through: no call synchronises with the host, and nothing but the launches and torch's
    # allocations is recorded (the new entry points issue no memset and no copy; the states are zeroed by reset())
    with torch.cuda.graph(g):
        out = an(buf)
    an.reset()
    for k in range(K):
        buf.copy_(x[:, k * sc.N:(k + 1) * sc.N])
        g.replay()
        torch.cuda.synchronize()
        for key in keys:
            assert torch.equal(out[key], want[k][key]), (k, key)
    assert int(an.counter.item()) == K
