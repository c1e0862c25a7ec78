"""The streamed Viterbi decode's restatement (tests/stream_viterbi_ref.py) against the offline one it is defined by,
and the fp64 end-to-end figures the GPU gates of tests/test_gpu_stream_viterbi.py rest on.  numpy only.

Prefix equality: the decision for emitted frame n at lag D is element max(n - D, 0) of viterbi_ref.viterbi over frames
0 .. n.  Cut independence: the decisions do not depend on how the frames are cut into calls.
End to end (include/ddsp_hip.h "pitch_viterbi_stream"; hop 512, calls of 1024 samples, 46 calls, 92 emitted frames,
lambda 0.02, jumps of 12 bins, 256 bins), more than 50 cents from truth on an interior frame counted as off:
    octave  streamed per-frame YIN 56 of 85 off | online lag 0: 0 off, max 22.4 cents | lag 4: 0 off, max 6.3 cents
    bursts  streamed per-frame YIN  7 of 85 off | online lag 0: 1 off, 53.7 cents     | lag 4: 0 off, max 29.3 cents
"""
import numpy as np
import pytest

import stream_viterbi_cases as sc
import stream_viterbi_ref as sv
import viterbi_ref as vr


def _costs(kind, rng, F, NB):
    if kind == "random":
        return rng.uniform(0.0, 1.0, size=(F, NB)).astype(np.float32)
    if kind == "quantised":  # dense ties
        return (rng.integers(0, 5, size=(F, NB)) / 4.0).astype(np.float32)
    return np.ones((F, NB), dtype=np.float32)


@pytest.mark.parametrize("D", [0, 1, 3, 64])
@pytest.mark.parametrize("NB", [1, 2, 65, 256])
def test_every_decision_is_the_offline_decode_of_the_prefix(NB, D):
    rng = np.random.default_rng(1000 * NB + D)
    F = D + 6  # past frame D, where the walk reaches its full length
    n_checked = 0
    for J in (0, 1, 12, 127):
        for kind, lam in (("random", 0.02), ("quantised", 0.25), ("ones", 0.02)):
            cost = _costs(kind, rng, F, NB)
            f0c = rng.uniform(50.0, 2000.0, size=cost.shape).astype(np.float32)
            f0, conf, path = sv.stream(cost, f0c, 1, lam, J, D)
            assert path.dtype == np.int32 and f0.dtype == np.float32 and conf.dtype == np.float32
            for n in range(F):
                m = max(n - D, 0)
                want = vr.viterbi(cost[:n + 1], lam, J)[m]
                assert path[n] == want, (kind, J, n, int(path[n]), int(want))
                assert f0[n] == f0c[m, want] and conf[n] == np.float32(1.0) - cost[m, want]
                n_checked += 1
            if kind == "ones":
                assert not path.any()
    assert n_checked == 12 * F


@pytest.mark.parametrize("D", [0, 1, 3, 64])
def test_decisions_do_not_depend_on_the_cut_into_calls(D):
    rng = np.random.default_rng(77 + D)
    F, NB = 80, 65
    for kind, lam in (("random", 0.02), ("quantised", 0.25)):
        cost = _costs(kind, rng, F, NB)
        f0c = rng.uniform(50.0, 2000.0, size=cost.shape).astype(np.float32)
        one = sv.stream(cost, f0c, 1, lam, 12, D)
        for R in (2, 5):
            for a, b in zip(one, sv.stream(cost, f0c, R, lam, 12, D)):
                assert np.array_equal(a, b), (kind, R)


@pytest.mark.parametrize("name,raw_off_at_least,over_at_lag0", [("octave", 44, 0), ("bursts", 5, 2)])
def test_end_to_end_figures_in_fp64(name, raw_off_at_least, over_at_lag0):
    raw = sc.interior(name, sc.raw_yin(name), 0)
    n_raw = int((raw > 50.0).sum())
    print(f"{name}: streamed per-frame YIN more than 50 cents off on {n_raw} of {raw.size} interior frames")
    lines = {}
    for D in (0, 4, 8):
        f0, _, path = sc.online(name, D)
        dec = sc.interior(name, f0, D)
        ref = sc.restated(name)
        off = vr.viterbi(ref["cost64"][0], sc.LAM, sc.JUMP)
        n = np.arange(D, len(path))
        same = int((path[n] == off[n - D]).sum())
        lines[D] = (dec, same, n.size)
        print(f"{name} lag {D}: {int((dec > 50.0).sum())} of {dec.size} interior frames off, max {dec.max():.1f} "
              f"cents; equals the offline path on {same} of {n.size} frames")
    assert raw.size == 85 and n_raw >= raw_off_at_least
    assert int((lines[0][0] > 50.0).sum()) <= over_at_lag0
    assert (lines[4][0] <= 50.0).all()
    assert lines[4][1] >= lines[4][2] - 1 and lines[8][1] == lines[8][2]
