"""The streamed loudness and the streamed pitch of one call in one launch over one state on gfx950
(csrc/stream_analysis.hip: core.stream_analysis, torch.ops.ddsp_hip.analysis_stream,
features.StreamAnalyzer(pitch=True, fused=True), RealtimeGraph(pitch_from_audio=True)).

Two kinds of check.  Accuracy: the gates of test_gpu_pitch.py and test_gpu_features.py against the fp64 restatements
(tests/pitch_ref.py, tests/stream_features_ref.py), unchanged.  Identity: the fused launch runs the per-frame code of
the two separate launches (csrc/analysis_bodies.h) with every reduction order fixed, so every output and the ring
must equal theirs bit for bit — for every transform size, each being its own instantiation."""
import functools

import numpy as np
import pytest
import torch

import pitch_cases as pc
import pitch_ref as pr
import stream_features_ref as sf
from test_gpu_features import gate as loudness_gate
from test_gpu_pitch import gate as pitch_gate

pytestmark = pytest.mark.gpu

ALL = dict(return_confidence=True, return_period=True)


@pytest.fixture(scope="module")
def dd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ddsp_pytorch_amd
    ddsp_pytorch_amd._lib.load()
    return ddsp_pytorch_amd


def run_fused(dd, xg, sr, hop, N, L, fmin=50.0):
    """xg [B, K N] through K calls -> ((loudness, f0, confidence, period) [B, K R] device tensors, the state)."""
    B, K = xg.shape[0], xg.shape[1] // N
    st = dd.core.FeatureStreamState(B, "cuda", N, L, hop)
    outs = []
    for k in range(K):
        outs.append(dd.core.stream_analysis(xg[:, k * N:(k + 1) * N], sr, hop, st, fmin=fmin, frame_length=L, **ALL))
        dd.core.stream_advance(st)
    assert int(st.counter.item()) == K
    return tuple(torch.cat([o[i] for o in outs], 1) for i in range(4)), st


@functools.lru_cache(maxsize=None)
def loudness_reference(sr, hop, N, B, L, K):
    """The streamed loudness of pc.stream_case's input at n_fft = L in fp64 and fp32, [B, K R] each, read-only."""
    x = pc.stream_case(sr, hop, N, B, L, K)[0]
    out = []
    for dt in (np.float64, np.float32):
        a = np.stack([sf.loudness(x[b], sr, hop, N, n_fft=L, dtype=dt).reshape(-1) for b in range(B)])
        a = a.astype(np.float64)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


@pytest.mark.parametrize("sr,hop,N,B,L,K", pc.STREAM)
def test_accuracy_against_the_fp64_restatements(dd, sr, hop, N, B, L, K):
    x, (tmin, tmax), ref = pc.stream_case(sr, hop, N, B, L, K)
    if (sr, hop, N) == (48000, 256, 1024):
        assert sf.sizes(L, hop, N)[3] == 2816 and sf.ring_wraps(L, hop, N, K) >= 2.0
    xg = torch.from_numpy(np.array(x)).cuda()
    (loud, f0, conf, period), _ = run_fused(dd, xg, sr, hop, N, L)
    assert loud.shape == f0.shape == conf.shape == period.shape == (B, K * (N // hop))
    loud, f0, conf, period = (t.cpu().numpy() for t in (loud, f0, conf, period))
    tag = f"fused stream sr {sr} hop {hop} N {N} B {B} L {L} K {K}"
    pitch_gate(tag, f0, conf, period, ref)
    ref64, ref32 = loudness_reference(sr, hop, N, B, L, K)
    assert loud.dtype == np.float32
    loudness_gate(tag + " loudness", loud, ref64, ref32)
    # the frames before the stream (f = -d + 1 .. -1): silent frames, exactly
    before = sf.sizes(L, hop, N)[1] - 1
    assert before >= 1
    assert (period[:, :before] == tmin).all() and (f0[:, :before] == np.float32(sr / tmin)).all()
    assert not conf[:, :before].any()


def assert_the_separate_launches_bits(dd, xg, sr, hop, N, L, fmin=50.0):
    B, K = xg.shape[0], xg.shape[1] // N
    fused = dd.core.FeatureStreamState(B, "cuda", N, L, hop)
    sl = dd.core.FeatureStreamState(B, "cuda", N, L, hop)
    sp = dd.core.FeatureStreamState(B, "cuda", N, L, hop, counter=sl.counter)
    for k in range(K):
        xc = xg[:, k * N:(k + 1) * N]
        got = dd.core.stream_analysis(xc, sr, hop, fused, fmin=fmin, frame_length=L, **ALL)
        want = (dd.core.stream_loudness(xc, sr, hop, sl, n_fft=L),) + \
            dd.core.stream_pitch(xc, sr, hop, sp, fmin=fmin, frame_length=L, **ALL)
        assert len(got) == len(want) == 4
        for name, u, v in zip(("loudness", "f0", "confidence", "period"), got, want):
            assert u.dtype == v.dtype and u.shape == v.shape and torch.equal(u, v), (L, k, name)
        dd.core.stream_advance(fused)
        dd.core.stream_advance(sl)
    assert torch.equal(fused.buf, sl.buf) and torch.equal(fused.buf, sp.buf), L


@pytest.mark.parametrize("sr,hop,N,B,L,K", pc.STREAM)
def test_same_bits_as_the_two_separate_launches(dd, sr, hop, N, B, L, K):
    x = pc.stream_case(sr, hop, N, B, L, K)[0]
    assert_the_separate_launches_bits(dd, torch.from_numpy(np.array(x)).cuda(), sr, hop, N, L)


@pytest.mark.parametrize("L", [64, 128, 256, 512, 1024, 2048, 4096])
def test_same_bits_at_every_transform_size(dd, L):
    """Each L is its own instantiation of the kernel; hop L/4 + 1 (odd), N = 3 hop, B = 2, K = 4 at 16 kHz."""
    hop, _, fmin, f_lo, f_hi = pc.size_params(L)
    N, B, K = 3 * hop, 2, 4
    x = pr.make_voiced(pc.SIZES_SR, K * N, B, seed=L, f_lo=f_lo, f_hi=f_hi)
    assert_the_separate_launches_bits(dd, torch.from_numpy(x).cuda(), pc.SIZES_SR, hop, N, L, fmin=fmin)


def test_a_call_run_twice_before_the_advance(dd):
    sr, hop, N, B, L, K = pc.STREAM[0]
    x = pc.stream_case(sr, hop, N, B, L, K)[0]
    xg = torch.from_numpy(np.array(x)).cuda()
    once = dd.core.FeatureStreamState(B, "cuda", N, L, hop)
    twice = dd.core.FeatureStreamState(B, "cuda", N, L, hop)
    for k in range(K):
        xc = xg[:, k * N:(k + 1) * N]
        a = dd.core.stream_analysis(xc, sr, hop, once, frame_length=L, **ALL)
        b1 = dd.core.stream_analysis(xc, sr, hop, twice, frame_length=L, **ALL)
        b2 = dd.core.stream_analysis(xc, sr, hop, twice, frame_length=L, **ALL)
        for u, v, w in zip(a, b1, b2):
            assert torch.equal(u, v) and torch.equal(u, w), k
        assert torch.equal(once.buf, twice.buf), k  # the ring as one run leaves it
        assert int(twice.counter.item()) == k        # the call reads the counter and never writes it
        dd.core.stream_advance(once)
        dd.core.stream_advance(twice)
    # confidence / period are optional: the same loudness and f0 bits without them
    first = dd.core.stream_analysis(xg[:, :N], sr, hop, dd.core.FeatureStreamState(B, "cuda", N, L, hop),
                                    frame_length=L, **ALL)
    only = dd.core.stream_analysis(xg[:, :N, None], sr, hop, dd.core.FeatureStreamState(B, "cuda", N, L, hop),
                                   frame_length=L)
    assert len(only) == 2 and torch.equal(only[0], first[0]) and torch.equal(only[1], first[1])
    with_conf = dd.core.stream_analysis(xg[:, :N], sr, hop, dd.core.FeatureStreamState(B, "cuda", N, L, hop),
                                        frame_length=L, return_confidence=True)
    assert len(with_conf) == 3 and torch.equal(with_conf[2], first[2])
    # a state built for another geometry is refused
    with pytest.raises(RuntimeError, match="another batch"):
        dd.core.stream_analysis(xg[:, :N], sr, hop, dd.core.FeatureStreamState(B, "cuda", N, 1024, hop),
                                frame_length=L)


def test_an_items_bits_do_not_depend_on_its_batch(dd):
    sr, hop, N, B, L, K = pc.STREAM[2]
    assert B == 3
    x = pc.stream_case(sr, hop, N, B, L, K)[0]
    xg = torch.from_numpy(np.array(x)).cuda()
    whole, _ = run_fused(dd, xg, sr, hop, N, L)
    for b in range(B):
        alone, _ = run_fused(dd, xg[b:b + 1].contiguous(), sr, hop, N, L)
        for u, v in zip(alone, whole):
            assert torch.equal(u[0], v[b]), b


def test_torch_op_returns_the_python_functions_bits(dd):
    from ddsp_pytorch_amd import script
    script.load_ops()
    sr, hop, N, B, L, K = pc.STREAM[2]
    x, (tmin, tmax), _ = pc.stream_case(sr, hop, N, B, L, K)
    xg = torch.from_numpy(np.array(x)).cuda()
    want, _ = run_fused(dd, xg, sr, hop, N, L)
    (w,) = dd.core._feature_tables("a_weighting", (float(sr), L), xg.device,
                                   lambda: (dd.core.a_weighting_table(sr, L),))
    st = dd.core.FeatureStreamState(B, "cuda", N, L, hop)
    R = N // hop
    for k in range(K):
        xc = xg[:, k * N:(k + 1) * N]
        got = torch.ops.ddsp_hip.analysis_stream(xc.unsqueeze(-1), w, L, hop, tmin, tmax, float(sr), 0.1, st.counter,
                                                 st.buf)
        assert len(got) == 4
        for u, v in zip(got, want):
            assert u.dtype == v.dtype and torch.equal(u, v[:, k * R:(k + 1) * R]), k
        dd.core.stream_advance(st)


KEYS = ("loudness", "mfcc", "pitch", "confidence")


def test_stream_analyzer_fused(dd):
    """StreamAnalyzer(pitch=True, fused=True): the bits of StreamAnalyzer(pitch=True) call by call, one state for
    the loudness and the pitch; a call captures into one HIP graph after a warm-up call; reset() restarts it."""
    sr, hop, N, K = 48000, 256, 1024, 6
    x = torch.from_numpy(pr.make_voiced(sr, K * N, 1, seed=17)).cuda()
    kw = dict(mean_loudness=-6.5, std_loudness=1.75, pitch=True)
    separate = dd.features.StreamAnalyzer(sr, hop, N, **kw)
    fused = dd.features.StreamAnalyzer(sr, hop, N, fused=True, **kw)
    assert fused.pitch_state is fused.loudness_state and separate.pitch_state is not separate.loudness_state
    assert fused.delay_frames == separate.delay_frames and fused.first_frame == separate.first_frame
    want = []
    for k in range(K):
        xc = x[:, k * N:(k + 1) * N]
        a, b = separate(xc), fused(xc)
        assert set(a) == set(b) == set(KEYS)
        for key in KEYS:
            assert a[key].shape == b[key].shape and torch.equal(a[key], b[key]), (k, key)
        want.append(a)
    assert int(fused.counter.item()) == K
    fused.reset()
    assert int(fused.counter.item()) == 0 and not fused.loudness_state.buf.any() and not fused.mfcc_state.buf.any()
    first = fused(x[:, :N])
    for key in KEYS:
        assert torch.equal(first[key], want[0][key]), key
    # one HIP graph: the fused launch, the MFCC, the advance
    an = dd.features.StreamAnalyzer(sr, hop, N, fused=True, **kw)
    buf = torch.zeros(1, N, device="cuda")
    an(buf)  # warm-up (the tables)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = an(buf)
    an.reset()
    for k in range(K):
        buf.copy_(x[:, k * N:(k + 1) * N])
        g.replay()
        torch.cuda.synchronize()
        for key in KEYS:
            assert torch.equal(out[key], want[k][key]), (k, key)
    assert int(an.counter.item()) == K


def _small_model(dd, seed=0):
    torch.manual_seed(seed)
    m = dd.DDSPDecoder(64, 16, 9, 48000, 256, False).eval()
    with torch.no_grad():
        m.decoder.cache_gru.normal_(0, 0.1)
    return m.cuda()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("continuous", [False, True])
def test_realtime_graph_from_audio_alone(dd, continuous, fused):
    """RealtimeGraph(pitch_from_audio=True, loudness_from_audio=True) fed the audio alone equals, bit for bit, a plain
    RealtimeGraph of the same model and seed whose pitch and loudness inputs carry, at every 256th sample, the
    'pitch' and 'loudness' of a separate StreamAnalyzer(pitch=True) run on the same audio: the same kernels on the
    same values.  Three rounds with reset() between them: device tensors in, host tensors in, device tensors again
    (reset() zeroes the GRU state the model came with, so the rounds after a reset are the ones to compare)."""
    from ddsp_pytorch_amd.realtime import RealtimeGraph
    sr, hop, N, K = 48000, 256, 1024, 6
    R = N // hop
    kw = dict(mean_loudness=-6.5, std_loudness=1.75, seed=99, continuous=continuous, reverb=continuous, fused=fused)
    rt = RealtimeGraph(_small_model(dd), N, loudness_from_audio=True, pitch_from_audio=True, **kw)
    rt_plain = RealtimeGraph(_small_model(dd), N, **kw)
    assert rt.pitch_delay_samples == rt.loudness_delay_samples == 768
    assert rt_plain.pitch_delay_samples == 0 and rt_plain.f0 is None and rt_plain.confidence is None
    assert rt.f0.shape == rt.confidence.shape == (1, R) and rt.f0.is_cuda and rt.confidence.is_cuda
    f0_buf, conf_buf = rt.f0.data_ptr(), rt.confidence.data_ptr()
    if continuous:
        assert rt.analysis.counter is rt.stream.counter
    an = dd.features.StreamAnalyzer(sr, hop, N, pitch=True)
    audio = torch.from_numpy(pr.make_voiced(sr, K * N, 1, seed=41)).cuda()
    rounds = []
    for rnd in range(3):
        ys = []
        for k in range(K):
            a = audio[:, k * N:(k + 1) * N].reshape(1, N, 1)
            feats = an(a)
            pitch = torch.zeros(1, N, 1, device="cuda")
            loud = torch.zeros(1, N, 1, device="cuda")
            pitch[:, ::hop] = feats["pitch"]
            loud[:, ::hop] = feats["loudness"]
            y = rt(a.cpu()).cuda() if rnd == 1 else rt(a).clone()
            y_plain = rt_plain(pitch, loud).clone()
            assert y.shape == (1, N, 1) and bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
            assert torch.equal(y, y_plain), (rnd, k)
            assert torch.equal(rt.f0, feats["pitch"][..., 0]), (rnd, k)
            assert torch.equal(rt.confidence, feats["confidence"][..., 0]), (rnd, k)
            ys.append(y)
        assert float(rt.confidence.max()) > 0.5  # voiced audio: the tracker is sure of the last call's frames
        rounds.append(torch.cat(ys, 1))
        rt.reset()
        rt_plain.reset()
        an.reset()
    assert torch.equal(rounds[1], rounds[2])  # host input and device input: the same audio
    assert (rt.f0.data_ptr(), rt.confidence.data_ptr()) == (f0_buf, conf_buf)  # static buffers


def test_realtime_graph_refuses_what_it_cannot_take(dd):
    from ddsp_pytorch_amd.realtime import RealtimeGraph
    N = 1024
    with pytest.raises(RuntimeError, match="needs loudness_from_audio=True"):
        RealtimeGraph(_small_model(dd), N, pitch_from_audio=True)
    rt = RealtimeGraph(_small_model(dd), N, loudness_from_audio=True, pitch_from_audio=True)
    a = torch.zeros(1, N, 1, device="cuda")
    with pytest.raises(RuntimeError, match="one input"):
        rt(a, a)
    for shape in ((1, N), (1, N // 2, 1), (2, N, 1)):
        with pytest.raises(RuntimeError, match="audio must be"):
            rt(torch.zeros(*shape, device="cuda"))
        with pytest.raises(RuntimeError, match="audio must be"):
            rt(torch.zeros(*shape))
