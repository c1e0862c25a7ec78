"""features.StreamAnalysisPlan on gfx950: for each of the eleven routes ``run`` returns, bit for bit, what the route's
core functions return when called directly on fresh states of their own; ``delay_frames`` is the streamed features'
delay plus the decode's lag; ``reset()`` gives the same stream again.  The routing is under test, not the kernels."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SR, BS, N, B, K, LAG = 48000, 256, 512, 2, 3, 2
R = N // BS
ROUTES = [(None, None), (None, "own"), (None, "fused"), (None, "viterbi"), ("own", None), ("own", "own"),
          ("own", "fused"), ("own", "viterbi"), ("aligned", None), ("aligned", "fused"), ("aligned", "viterbi")]


@pytest.fixture(scope="module")
def dd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ddsp_pytorch_amd
    ddsp_pytorch_amd._lib.load()
    return ddsp_pytorch_amd


@pytest.fixture(scope="module")
def calls(dd):
    g = torch.Generator().manual_seed(1234)
    t = torch.arange(K * N, dtype=torch.float64) / SR
    tone = torch.stack([torch.sin(2 * math.pi * 220.0 * t), torch.sin(2 * math.pi * 330.0 * t)]).float()
    x = (0.5 * tone + 0.05 * torch.randn(B, K * N, generator=g)).cuda()
    return [x[:, k * N:(k + 1) * N].contiguous() for k in range(K)]


def _direct(core, mfcc, pitch, calls):
    """The route's core calls, made by hand on states of their own (one counter, one advance per call)."""
    main = core.FeatureStreamState(B, "cuda", N, 2048, BS)
    mfcc_ring = core.FeatureStreamState(B, "cuda", N, 1024, BS, counter=main.counter) if mfcc == "own" else None
    pitch_ring = decode = None
    if pitch in ("own", "viterbi"):
        pitch_ring = core.FeatureStreamState(B, "cuda", N, 2048, BS, counter=main.counter)
    if pitch == "viterbi":
        decode = core.ViterbiStreamState(B, "cuda", R, core.stream_pitch_bin_count(SR), LAG, counter=main.counter)
    out = []
    for a in calls:
        m = f0 = conf = None
        if pitch == "viterbi":
            cost, f0c = core.stream_pitch_salience(a, SR, BS, pitch_ring)
            f0, conf, _ = core.stream_viterbi_path(cost, f0c, decode)
        if mfcc == "aligned" and pitch == "fused":
            loud, m, f0, conf = core.stream_analysis_mfcc(a, SR, BS, main, pitch=True, return_confidence=True)
        elif mfcc == "aligned":
            loud, m = core.stream_analysis_mfcc(a, SR, BS, main, pitch=False)
        elif pitch == "fused":
            loud, f0, conf = core.stream_analysis(a, SR, BS, main, return_confidence=True)
        else:
            loud = core.stream_loudness(a, SR, BS, main)
        if mfcc == "own":
            m = core.stream_mfcc(a, SR, BS, mfcc_ring)
        if pitch == "own":
            f0, conf = core.stream_pitch(a, SR, BS, pitch_ring, return_confidence=True)
        core.stream_advance(main)
        out.append((loud, m, f0, conf))
    return out


def _same(got, want):
    return all((g is None and w is None) or (g is not None and w is not None and torch.equal(g, w))
               for g, w in zip(got, want))


@pytest.mark.parametrize("mfcc,pitch", ROUTES)
def test_plan_runs_its_route(dd, calls, mfcc, pitch):
    core, features = dd.core, dd.features
    plan = features.StreamAnalysisPlan(features.stream_analysis_route(mfcc, pitch), SR, BS, N, B, "cuda",
                                       pitch_lag=LAG)
    delay = core.stream_feature_delay
    want_delay = {"loudness": delay(2048, BS)}
    if mfcc:
        want_delay["mfcc"] = delay(1024, BS) if mfcc == "own" else delay(2048, BS)
    if pitch:
        want_delay["pitch"] = delay(2048, BS) + (LAG if pitch == "viterbi" else 0)
    assert plan.delay_frames == want_delay
    assert (plan.viterbi_state is not None) == (pitch == "viterbi")
    states = list(plan.states.values()) + ([plan.viterbi_state] if plan.viterbi_state is not None else [])
    assert all(s.counter is plan.counter for s in states)
    assert len({id(s) for s in plan.states.values()}) == len(set(dict(plan.route.rings).values()))
    want = _direct(core, mfcc, pitch, calls)

    def stream():
        out = []
        for a in calls:
            out.append(plan.run(a))
            core.stream_advance(plan.states["loudness"])
        return out
    first = stream()
    for k in range(K):
        assert len(first[k]) == 4 and _same(first[k], want[k]), k
        loud, m, f0, conf = first[k]
        assert loud.shape == (B, R) and (m is None) == (mfcc is None) and (f0 is None) == (pitch is None)
        assert (conf is None) == (f0 is None)
    assert int(plan.counter.item()) == K
    plan.reset()
    assert int(plan.counter.item()) == 0 and not any(bool(s.buf.any()) for s in states)
    again = stream()
    assert all(_same(again[k], first[k]) for k in range(K))
