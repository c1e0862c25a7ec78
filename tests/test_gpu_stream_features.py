"""The streaming analysis on gfx950 (csrc/features.hip: core.stream_loudness, core.stream_mfcc,
features.StreamAnalyzer, the torch.ops, RealtimeGraph(loudness_from_audio=True)) against the fp64 restatement of
tests/stream_features_ref.py.

The accuracy gate is the one of tests/test_gpu_features.py, imported unchanged: RMS and maximum error of the GPU
against fp64 <= 4 x the same statistic of the fp32 CPU restatement against fp64 on the same input; every figure is
printed before it is asserted (pytest -s; DESIGN.md 3f-stream records the measured ratios).  It runs over every frame a
stream emits, the ones before the stream's start included.
"""
import functools

import numpy as np
import pytest
import torch

import features_ref as fr
import stream_features_ref as sf
from test_gpu_features import gate

pytestmark = pytest.mark.gpu

LOUD_FFT, MFCC_FFT = 2048, 1024  # core.stream_loudness's and core.stream_mfcc's defaults


@pytest.fixture(scope="module")
def dd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ddsp_pytorch_amd
    ddsp_pytorch_amd._lib.load()
    return ddsp_pytorch_amd


def run_stream(dd, x, sr, hop, N, loud_kw=None, mfcc_kw=None, wrap_input=None):
    """x [B, K N] (numpy) through K calls of both features -> (loudness [B, K, R], mfcc [B, K, R, n_mfcc]) as
    device tensors.  ``wrap_input``: what to do to each call's device tensor before it is passed on."""
    loud_kw, mfcc_kw = dict(loud_kw or {}), dict(mfcc_kw or {})
    B, K = x.shape[0], x.shape[1] // N
    xg = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    sl = dd.core.FeatureStreamState(B, "cuda", N, loud_kw.get("n_fft", LOUD_FFT), hop)
    sm = dd.core.FeatureStreamState(B, "cuda", N, mfcc_kw.get("n_fft", MFCC_FFT), hop, counter=sl.counter)
    loud, mfcc = [], []
    for k in range(K):
        xc = xg[:, k * N:(k + 1) * N]
        if wrap_input is not None:
            xc = wrap_input(xc)
        loud.append(dd.core.stream_loudness(xc, sr, hop, sl, **loud_kw))
        mfcc.append(dd.core.stream_mfcc(xc, sr, hop, sm, **mfcc_kw))
        dd.core.stream_advance(sl)
    assert int(sl.counter.item()) == K
    return torch.stack(loud, 1), torch.stack(mfcc, 1)


def restate(x, sr, hop, N, loud_kw=None, mfcc_kw=None):
    """Both features of x [B, K N] item by item in fp64 and fp32 (computed once per input and shared; read-only)."""
    loud_kw, mfcc_kw = dict(loud_kw or {}), dict(mfcc_kw or {})
    out = {}
    for name, fn, kw in (("loudness", sf.loudness, loud_kw), ("mfcc", sf.mfcc, mfcc_kw)):
        for tag, dt in (("64", np.float64), ("32", np.float32)):
            a = np.stack([fn(x[b], sr, hop, N, dtype=dt, **kw) for b in range(x.shape[0])]).astype(np.float64)
            a.setflags(write=False)
            out[name + tag] = a
    return out


# (sample rate, hop, N, B, K calls).  The fourth row runs K = 4 calls, not the 3 first planned for it: 3 calls of
# 2048 take the loudness's ring of 4032 floats round 1.52 times, short of the two wraps asserted below (the first
# three calls are the same calls either way).
CASES = [
    (48000, 256, 1024, 1, 8),   # the realtime shape
    (48000, 512, 512, 2, 10),   # R = 1: every frame rides alone
    (16000, 160, 480, 3, 12),   # R odd, hop not a power of two, n_fft/2 not a multiple of hop
    (44100, 64, 2048, 1, 4),    # R = 32, the cap
]


@functools.lru_cache(maxsize=None)
def case_reference(sr, hop, N, B, K):
    x = fr.make_signal(sr, K * N, B, seed=N + hop)
    x.setflags(write=False)
    return x, restate(x, sr, hop, N)


@pytest.mark.parametrize("sr,hop,N,B,K", CASES)
def test_accuracy_against_the_fp64_restatement(dd, sr, hop, N, B, K):
    """Measured on MI355X (ratios GPU / fp32 CPU, rms and max, in the order of CASES): see DESIGN.md 3f-stream."""
    for n_fft in (LOUD_FFT, MFCC_FFT):
        assert sf.ring_wraps(n_fft, hop, N, K) >= 2.0, n_fft
    x, ref = case_reference(sr, hop, N, B, K)
    loud, mfcc = run_stream(dd, x, sr, hop, N)
    R = N // hop
    assert loud.shape == (B, K, R) and mfcc.shape == (B, K, R, 30)
    tag = f"stream sr {sr} hop {hop} N {N} B {B} K {K}"
    gate(tag + " loudness", loud.cpu().numpy(), ref["loudness64"], ref["loudness32"])
    gate(tag + " mfcc", mfcc.cpu().numpy(), ref["mfcc64"], ref["mfcc32"])


# every transform size is its own instantiation of both kernels: (n_fft, n_mels, n_mfcc) as in
# tests/test_gpu_features.py, hop n_fft/4 + 1 (odd), N = 3 hop, B = 2
SIZES = [(16, 4, 4), (32, 8, 5), (64, 16, 16), (128, 32, 13), (256, 64, 30), (512, 128, 30), (2048, 256, 256),
         (4096, 128, 30)]


@pytest.mark.parametrize("n_fft,n_mels,n_mfcc", SIZES)
def test_every_transform_size(dd, n_fft, n_mels, n_mfcc):
    sr, B = 16000, 2
    hop = n_fft // 4 + 1
    N = 3 * hop
    K = -(-2 * sf.sizes(n_fft, hop, N)[3] // N) + 1
    assert sf.ring_wraps(n_fft, hop, N, K) >= 2.0
    x = fr.make_signal(sr, K * N, B, seed=n_fft)
    lkw = dict(n_fft=n_fft)
    mkw = dict(n_mfcc=n_mfcc, n_fft=n_fft, n_mels=n_mels, fmin=20.0, fmax=8000.0)
    loud, mfcc = run_stream(dd, x, sr, hop, N, lkw, mkw)
    assert loud.shape == (B, K, 3) and mfcc.shape == (B, K, 3, n_mfcc)
    ref = restate(x, sr, hop, N, lkw, mkw)
    tag = f"stream n_fft {n_fft} n_mels {n_mels} n_mfcc {n_mfcc}"
    gate(tag + " loudness", loud.cpu().numpy(), ref["loudness64"], ref["loudness32"])
    gate(tag + " mfcc", mfcc.cpu().numpy(), ref["mfcc64"], ref["mfcc32"])


def test_causal_clamp_is_per_item(dd):
    """Item 0: make_signal x 1e-6 for four calls, x 1 for four, x 1e-6 for four; item 1 loud throughout; top_db 80.

    What the fp64 restatement shows for item 0 (asserted before the device is touched): in the late segment most
    values are clamped (measured 0.81 of them) and in the loud one none is; the early segment's clamp level
    (running maximum -98.0 dB, level -178.0) differs from the offline one (global maximum 18.6 dB, level -61.4),
    which would have clamped every early value.  Under the causal clamp NO early value can be clamped with this
    input, and none in the loud segment either: 10 log10(max(1e-10, .)) bounds D below by -100 dB, so a level of
    (running maximum - 80) only bites once the running maximum has passed -20 dB, and the loud segment's own floor,
    its white noise (-57.3 dB at the least), lies above its level of -61.4.  "Some values clamped in every
    segment" therefore holds for the late segment only; the assertions below state what does hold."""
    sr, hop, N, seg = 48000, 256, 1024, 4
    K = 3 * seg
    base = fr.make_signal(sr, K * N, 2, seed=5)
    scale = np.repeat(np.array([1e-6, 1.0, 1e-6], dtype=np.float32), seg * N)
    x = np.stack([base[0] * scale, base[1]])
    D = np.stack([sf.mel_db(x[b], sr, hop, N) for b in range(2)])  # [2, K, R, 128]
    level = np.stack([sf.causal_clamp(D[b], 80.0)[1] for b in range(2)]) - 80.0  # [2, K]
    clamped = D < level[:, :, None, None]
    early, loud_, late = (slice(s * seg, (s + 1) * seg) for s in range(3))
    assert clamped[0, late].mean() >= 0.5
    assert (~clamped[0, loud_]).any()
    offline_level = D[0].max() - 80.0
    assert level[0, early].max() < offline_level - 100.0      # the early level is not the offline one ...
    assert (D[0, early] < offline_level).all() and not clamped[0, early].any()  # ... which would clamp all of it
    assert abs(level[0, late].min() - offline_level) == 0.0   # once the loudest frame has passed: the offline clamp
    assert level[1, 0] > -70.0 and level[0, 0] < -170.0       # item 1 is loud from its first call, item 0 is not
    loud, mfcc = run_stream(dd, x, sr, hop, N)
    ref = restate(x, sr, hop, N)
    for b, name in enumerate(("quiet-loud-quiet", "loud throughout")):
        gate(f"causal clamp {name} mfcc", mfcc[b].cpu().numpy(), ref["mfcc64"][b], ref["mfcc32"][b])
        gate(f"causal clamp {name} loudness", loud[b].cpu().numpy(), ref["loudness64"][b], ref["loudness32"][b])
    # a batch-wide maximum would clamp item 0's early segment at item 1's level: its MFCC would be the DCT of a
    # constant.  It is not: the early frames keep their shape (coefficient 1 is far from 0)
    want_flat = fr.dct_matrix(30, 128) @ np.full(128, level[1, 0])
    got_early = mfcc[0, early].cpu().numpy().reshape(-1, 30)
    assert np.abs(got_early - want_flat[None, :]).max() > 50.0


def test_state_behaviour(dd):
    sr, hop, N, B, K = 16000, 160, 480, 3, 12
    x, _ = case_reference(sr, hop, N, B, K)
    loud, mfcc = run_stream(dd, np.array(x), sr, hop, N)
    xg = torch.from_numpy(np.array(x)).cuda()
    sl = dd.core.FeatureStreamState(B, "cuda", N, LOUD_FFT, hop)
    sm = dd.core.FeatureStreamState(B, "cuda", N, MFCC_FFT, hop, counter=sl.counter)
    for rnd in range(2):  # the second round: reset() then a replay gives the first run's bits
        for k in range(K):
            xc = xg[:, k * N:(k + 1) * N]
            for rep in range(2):  # a call run twice before the advance gives equal bits
                assert torch.equal(dd.core.stream_loudness(xc, sr, hop, sl), loud[:, k]), (rnd, k, rep)
                assert torch.equal(dd.core.stream_mfcc(xc, sr, hop, sm), mfcc[:, k]), (rnd, k, rep)
            dd.core.stream_advance(sl)
        sl.reset()
        sm.reset()
        assert int(sm.counter.item()) == 0
    # item b's bits do not depend on the batch around it
    for b in range(B):
        lb, mb = run_stream(dd, np.array(x[b:b + 1]), sr, hop, N)
        assert torch.equal(lb[0], loud[b]) and torch.equal(mb[0], mfcc[b]), b
    # a non-contiguous [B, N, 1] input is accepted
    def strided(xc):
        wide = torch.zeros(xc.shape[0], xc.shape[1], 2, device="cuda")
        wide[..., 0] = xc
        view = wide[..., :1]
        assert not view.is_contiguous() and view.shape == (xc.shape[0], N, 1)
        return view
    ls, ms = run_stream(dd, np.array(x), sr, hop, N, wrap_input=strided)
    assert torch.equal(ls, loud) and torch.equal(ms, mfcc)


def test_two_streams_interleaved_do_not_interact(dd):
    sr, hop, N, K = 48000, 256, 1024, 6
    xa = fr.make_signal(sr, K * N, 1, seed=21)
    xb = fr.make_signal(sr, K * N, 1, seed=22) * np.float32(0.01)
    alone = [run_stream(dd, x, sr, hop, N) for x in (xa, xb)]
    an = [dd.features.StreamAnalyzer(sr, hop, N) for _ in range(2)]
    assert an[0].delay_frames == {"loudness": 3, "mfcc": 1} and an[0].first_frame == {"loudness": -3, "mfcc": -1}
    got = [[], []]
    for k in range(K):
        for i, x in enumerate((xa, xb)):
            got[i].append(an[i](torch.from_numpy(x[:, k * N:(k + 1) * N]).cuda()))
    for i in range(2):
        loud = torch.stack([g["loudness"] for g in got[i]], 1)
        mfcc = torch.stack([g["mfcc"] for g in got[i]], 1)
        assert loud.shape == (1, K, 4, 1) and mfcc.shape == (1, K, 4, 30)
        assert torch.equal(loud[..., 0], alone[i][0]) and torch.equal(mfcc, alone[i][1]), i
    # the normalisation of analyze
    an_n = dd.features.StreamAnalyzer(sr, hop, N, mean_loudness=-6.5, std_loudness=1.75)
    out = an_n(torch.from_numpy(xa[:, :N]).cuda())
    assert (out["loudness"][..., 0] - (alone[0][0][:, 0] + 6.5) / 1.75).abs().max() <= 1e-6
    an_n.reset()
    assert torch.equal(an_n(torch.from_numpy(xa[:, :N]).cuda())["loudness"], out["loudness"])


def test_torch_ops_return_the_python_functions_bits(dd):
    from ddsp_pytorch_amd import script
    script.load_ops()
    sr, hop, N, B, K = 48000, 512, 512, 2, 10
    x, _ = case_reference(sr, hop, N, B, K)
    loud, mfcc = run_stream(dd, np.array(x), sr, hop, N)
    xg = torch.from_numpy(np.array(x)).cuda()
    (w,) = dd.core._feature_tables("a_weighting", (float(sr), LOUD_FFT), xg.device,
                                   lambda: (dd.core.a_weighting_table(sr, LOUD_FFT),))
    tabs = dd.core.mfcc_tables(sr, 30, MFCC_FFT, 128, 20.0, 8000.0, xg.device)
    sl = dd.core.FeatureStreamState(B, "cuda", N, LOUD_FFT, hop)
    sm = dd.core.FeatureStreamState(B, "cuda", N, MFCC_FFT, hop, counter=sl.counter)
    for k in range(K):
        xc = xg[:, k * N:(k + 1) * N]
        assert torch.equal(torch.ops.ddsp_hip.loudness_stream(xc, w, LOUD_FFT, hop, sl.counter, sl.buf), loud[:, k]), k
        got = torch.ops.ddsp_hip.mfcc_stream(xc.unsqueeze(-1), *tabs, MFCC_FFT, hop, 80.0, sm.counter, sm.buf)
        assert torch.equal(got, mfcc[:, k]), k
        dd.core.stream_advance(sl)


def test_stream_analyzer_captures_into_a_hip_graph(dd):
    """After a warm-up call (the tables) a StreamAnalyzer call — both features and the advance — records into one
    HIP graph on one stream; six replays equal six eager calls bit for bit."""
    sr, hop, N, K = 48000, 256, 1024, 6
    x = torch.from_numpy(fr.make_signal(sr, K * N, 1, seed=31)).cuda()
    eager = dd.features.StreamAnalyzer(sr, hop, N)
    want = [eager(x[:, k * N:(k + 1) * N]) for k in range(K)]
    an = dd.features.StreamAnalyzer(sr, hop, N)
    buf = torch.zeros(1, N, device="cuda")
    an(buf)  # warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = an(buf)
    an.reset()
    for k in range(K):
        buf.copy_(x[:, k * N:(k + 1) * N])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["loudness"], want[k]["loudness"]) and torch.equal(out["mfcc"], want[k]["mfcc"]), k
    assert int(an.counter.item()) == K


def _small_model(dd, seed=0):
    torch.manual_seed(seed)
    m = dd.DDSPDecoder(64, 16, 9, 48000, 256, False).eval()
    with torch.no_grad():
        m.decoder.cache_gru.normal_(0, 0.1)
    return m.cuda()


@pytest.mark.parametrize("continuous", [False, True])
def test_realtime_graph_takes_its_loudness_from_audio(dd, continuous):
    """RealtimeGraph(loudness_from_audio=True) fed (pitch, audio) equals, bit for bit, a plain RealtimeGraph of the
    same model and seed whose loudness input carries, at every 256th sample, the output of a separate StreamAnalyzer
    run on the same audio: both run the same kernels on the same values."""
    from ddsp_pytorch_amd.realtime import RealtimeGraph
    sr, hop, N, K = 48000, 256, 1024, 6
    kw = dict(mean_loudness=-6.5, std_loudness=1.75, seed=99, continuous=continuous, reverb=continuous)
    rt_audio = RealtimeGraph(_small_model(dd), N, loudness_from_audio=True, **kw)
    rt_plain = RealtimeGraph(_small_model(dd), N, **kw)
    assert rt_audio.loudness_delay_samples == 768 and rt_plain.loudness_delay_samples == 0
    if continuous:
        assert rt_audio.analysis.counter is rt_audio.stream.counter
    an = dd.features.StreamAnalyzer(sr, hop, N)
    audio = torch.from_numpy(fr.make_signal(sr, K * N, 1, seed=41)).cuda()
    g = torch.Generator().manual_seed(3)
    for rnd in range(2):  # the second round after reset(): the analysis state is reset with the rest
        for k in range(K):
            pitch = (80.0 * 10.0 ** torch.rand(1, N, 1, generator=g)).cuda()
            a = audio[:, k * N:(k + 1) * N].reshape(1, N, 1)
            loud = torch.zeros(1, N, 1, device="cuda")
            loud[:, ::hop] = an(a)["loudness"]
            y_audio = rt_audio(pitch, a).clone()
            y_plain = rt_plain(pitch, loud).clone()
            assert bool(torch.isfinite(y_audio).all()) and float(y_audio.abs().max()) > 0
            assert torch.equal(y_audio, y_plain), (rnd, k)
        rt_audio.reset()
        rt_plain.reset()
        an.reset()
