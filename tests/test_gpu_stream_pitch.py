"""The streamed pitch tracker on gfx950 (csrc/pitch.hip: core.stream_pitch, features.StreamAnalyzer(pitch=True),
torch.ops.ddsp_hip.pitch_stream) against the fp64 restatement of tests/pitch_ref.py on the stream's frames
(tests/stream_features_ref.py's frame indices), with the gate of test_gpu_pitch.py over every emitted frame —
the frames of zeros before the stream included, which must come out as the silent-frame values exactly."""
import numpy as np
import pytest
import torch

import pitch_cases as pc
import stream_features_ref as sf
from test_gpu_pitch import gate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ddsp_pytorch_amd
    ddsp_pytorch_amd._lib.load()
    return ddsp_pytorch_amd


def run_stream(dd, xg, sr, hop, N, L, state=None):
    """xg [B, K N] through K calls -> (f0, confidence, period) [B, K R] device tensors, and the state."""
    B, K = xg.shape[0], xg.shape[1] // N
    st = state or dd.core.FeatureStreamState(B, "cuda", N, L, hop)
    outs = []
    for k in range(K):
        outs.append(dd.core.stream_pitch(xg[:, k * N:(k + 1) * N], sr, hop, st, frame_length=L,
                                         return_confidence=True, return_period=True))
        dd.core.stream_advance(st)
    assert int(st.counter.item()) == K
    return tuple(torch.cat([o[i] for o in outs], 1) for i in range(3)), st


@pytest.mark.parametrize("sr,hop,N,B,L,K", pc.STREAM)
def test_accuracy_against_the_fp64_restatement(dd, sr, hop, N, B, L, K):
    x, (tmin, tmax), ref = pc.stream_case(sr, hop, N, B, L, K)
    if (sr, hop, N) == (48000, 256, 1024):
        assert sf.sizes(L, hop, N)[3] == 2816 and sf.ring_wraps(L, hop, N, K) >= 2.0
    xg = torch.from_numpy(np.array(x)).cuda()
    (f0, conf, period), _ = run_stream(dd, xg, sr, hop, N, L)
    f0, conf, period = f0.cpu().numpy(), conf.cpu().numpy(), period.cpu().numpy()
    gate(f"stream sr {sr} hop {hop} N {N} B {B} L {L} K {K}", f0, conf, period, ref)
    # the frames before the stream (f = -d + 1 .. -1): silent frames, exactly
    before = sf.sizes(L, hop, N)[1] - 1
    assert before >= 1
    assert (period[:, :before] == tmin).all() and (f0[:, :before] == np.float32(sr / tmin)).all()
    assert not conf[:, :before].any()


def test_a_call_run_twice_before_the_advance(dd):
    sr, hop, N, B, L, K = pc.STREAM[0]
    x = pc.stream_case(sr, hop, N, B, L, K)[0]
    xg = torch.from_numpy(np.array(x)).cuda()
    once = dd.core.FeatureStreamState(B, "cuda", N, L, hop)
    twice = dd.core.FeatureStreamState(B, "cuda", N, L, hop)
    for k in range(K):
        xc = xg[:, k * N:(k + 1) * N]
        a = dd.core.stream_pitch(xc, sr, hop, once, frame_length=L, return_confidence=True, return_period=True)
        b1 = dd.core.stream_pitch(xc, sr, hop, twice, frame_length=L, return_confidence=True, return_period=True)
        b2 = dd.core.stream_pitch(xc, sr, hop, twice, frame_length=L, return_confidence=True, return_period=True)
        for u, v, w in zip(a, b1, b2):
            assert torch.equal(u, v) and torch.equal(u, w), k
        assert torch.equal(once.buf, twice.buf), k  # the ring as one run leaves it
        assert int(twice.counter.item()) == k        # the call reads the counter and never writes it
        dd.core.stream_advance(once)
        dd.core.stream_advance(twice)
    # confidence / period are optional
    st = dd.core.FeatureStreamState(B, "cuda", N, L, hop)
    only = dd.core.stream_pitch(xg[:, :N, None], sr, hop, st, frame_length=L)
    first = dd.core.stream_pitch(xg[:, :N], sr, hop, dd.core.FeatureStreamState(B, "cuda", N, L, hop),
                                 frame_length=L, return_confidence=True)
    assert isinstance(only, torch.Tensor) and torch.equal(only, first[0])
    # a state built for another geometry is refused
    with pytest.raises(RuntimeError, match="another batch"):
        dd.core.stream_pitch(xg[:, :N], sr, hop, dd.core.FeatureStreamState(B, "cuda", N, 1024, hop), frame_length=L)


def test_stream_analyzer_with_pitch(dd):
    sr, hop, N, B, L, K = pc.STREAM[0]
    x, _, ref = pc.stream_case(sr, hop, N, B, L, K)
    xg = torch.from_numpy(np.array(x)).cuda()
    plain = dd.features.StreamAnalyzer(sr, hop, N, batch=B)
    full = dd.features.StreamAnalyzer(sr, hop, N, batch=B, pitch=True)
    assert set(plain.delay_frames) == {"loudness", "mfcc"} and plain.pitch_state is None
    assert full.delay_frames["pitch"] == full.delay_frames["loudness"] == 3
    assert full.first_frame["pitch"] == -3 and full.pitch_state.counter is full.counter
    (want, _, _), _ = run_stream(dd, xg, sr, hop, N, L)
    R = N // hop
    for k in range(K):
        xc = xg[:, k * N:(k + 1) * N]
        a, b = plain(xc), full(xc)
        assert set(a) == {"loudness", "mfcc"}
        assert set(b) == {"loudness", "mfcc", "pitch", "confidence"}
        assert torch.equal(a["loudness"], b["loudness"]) and torch.equal(a["mfcc"], b["mfcc"]), k
        assert b["pitch"].shape == b["confidence"].shape == (B, R, 1)
        assert torch.equal(b["pitch"][..., 0], want[:, k * R:(k + 1) * R]), k
    assert int(full.counter.item()) == K == int(plain.counter.item())
    full.reset()
    assert int(full.counter.item()) == 0 and not full.pitch_state.buf.any()
    assert torch.equal(full(xg[:, :N])["pitch"][..., 0], want[:, :R])


def test_a_shared_stream_counter_with_advance_off(dd):
    sr, hop, N, B, L, K = pc.STREAM[0]
    x = pc.stream_case(sr, hop, N, B, L, K)[0]
    xg = torch.from_numpy(np.array(x)).cuda()
    (want, _, _), _ = run_stream(dd, xg, sr, hop, N, L)
    synth = dd.core.StreamState(B, "cuda")
    an = dd.features.StreamAnalyzer(sr, hop, N, batch=B, counter=synth.counter, advance=False, pitch=True)
    assert an.pitch_state.counter is synth.counter
    R = N // hop
    for k in range(3):
        out = an(xg[:, k * N:(k + 1) * N])
        assert int(synth.counter.item()) == k  # the analyzer did not advance
        assert torch.equal(out["pitch"][..., 0], want[:, k * R:(k + 1) * R]), k
        dd.core.stream_advance(synth)           # the stream's own advance ends the call for all three states


def test_torch_op_returns_the_python_functions_bits(dd):
    from ddsp_pytorch_amd import script
    script.load_ops()
    sr, hop, N, B, L, K = pc.STREAM[2]
    x, (tmin, tmax), _ = pc.stream_case(sr, hop, N, B, L, K)
    xg = torch.from_numpy(np.array(x)).cuda()
    (f0, conf, period), _ = run_stream(dd, xg, sr, hop, N, L)
    st = dd.core.FeatureStreamState(B, "cuda", N, L, hop)
    R = N // hop
    for k in range(K):
        xc = xg[:, k * N:(k + 1) * N]
        got = torch.ops.ddsp_hip.pitch_stream(xc.unsqueeze(-1), L, hop, tmin, tmax, float(sr), 0.1, st.counter, st.buf)
        for u, v in zip(got, (f0, conf, period)):
            assert u.dtype == v.dtype and torch.equal(u, v[:, k * R:(k + 1) * R]), k
        dd.core.stream_advance(st)
