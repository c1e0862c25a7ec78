"""The streamed loudness, MFCC and pitch of one call in one launch over one state, on one time axis, on gfx950
(csrc/stream_analysis.hip: core.stream_analysis_mfcc, torch.ops.ddsp_hip.analysis_mfcc_stream,
features.StreamAnalyzer(aligned=True)).

Identity: the launch runs the per-call code of the separate launches (csrc/analysis_bodies.h) with every reduction
order fixed, so the loudness, the pitch and the ring equal core.stream_analysis' bit for bit, and the MFCC equals
core.stream_mfcc(n_fft=M) fed the same stream delayed by D = (delay(L) - delay(M)) hop samples
(tests/aligned_mfcc_ref.py; test_stream_analysis_mfcc_abi.py proves that identity in fp64) — for every pair
(L, M), each being its own instantiation.  Accuracy: the imported gates against the fp64 restatements, every figure
printed before it is asserted (pytest -s; DESIGN.md 3f-aligned records the measured ratios)."""
import functools

import numpy as np
import pytest
import torch

import aligned_mfcc_ref as am
import pitch_cases as pc
import pitch_ref as pr
import stream_features_ref as sf
from test_gpu_features import gate as loudness_gate
from test_gpu_pitch import gate as pitch_gate
from test_gpu_stream_analysis import loudness_reference
from test_gpu_stream_features import gate as mfcc_gate

pytestmark = pytest.mark.gpu

ALL = dict(return_confidence=True, return_period=True)
NAMES = ("loudness", "mfcc", "f0", "confidence", "period")
# (n_mels, n_mfcc) per MFCC transform size, as tests/test_gpu_stream_features.py pairs them
MELS = {32: (8, 5), 64: (16, 16), 128: (32, 13), 256: (64, 30), 512: (128, 30), 1024: (128, 30), 2048: (256, 256)}


@pytest.fixture(scope="module")
def dd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ddsp_pytorch_amd
    ddsp_pytorch_amd._lib.load()
    return ddsp_pytorch_amd


def mfcc_kw(M, default=False):
    if default:
        return dict(mfcc_n_fft=M)
    n_mels, n_mfcc = MELS[M]
    return dict(mfcc_n_fft=M, n_mels=n_mels, n_mfcc=n_mfcc)


def run_aligned(dd, xg, sr, hop, N, L, fmin=50.0, pitch=True, **mkw):
    """xg [B, K N] through K calls -> (the outputs concatenated over the calls [B, K R, ...], the state)."""
    B, K = xg.shape[0], xg.shape[1] // N
    st = dd.core.FeatureStreamState(B, "cuda", N, L, hop)
    outs = []
    for k in range(K):
        outs.append(dd.core.stream_analysis_mfcc(xg[:, k * N:(k + 1) * N], sr, hop, st, pitch=pitch, fmin=fmin,
                                                 frame_length=L, **(ALL if pitch else {}), **mkw))
        dd.core.stream_advance(st)
    assert int(st.counter.item()) == K
    return tuple(torch.cat([o[i] for o in outs], 1) for i in range(len(outs[0]))), st


def assert_the_separate_launches_bits(dd, x, sr, hop, N, L, M, fmin=50.0, default=False):
    B, K = x.shape[0], x.shape[1] // N
    xg = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    xd = torch.from_numpy(np.ascontiguousarray(am.delayed(x, L, M, hop))).cuda()
    mkw = mfcc_kw(M, default)
    skw = {("n_fft" if k == "mfcc_n_fft" else k): v for k, v in mkw.items()}
    one = dd.core.FeatureStreamState(B, "cuda", N, L, hop)
    two = dd.core.FeatureStreamState(B, "cuda", N, L, hop)
    sm = dd.core.FeatureStreamState(B, "cuda", N, M, hop)
    ring_bytes = 4 * B * sf.sizes(L, hop, N)[3]
    for k in range(K):
        xc = xg[:, k * N:(k + 1) * N]
        got = dd.core.stream_analysis_mfcc(xc, sr, hop, one, fmin=fmin, frame_length=L, **ALL, **mkw)
        sep = dd.core.stream_analysis(xc, sr, hop, two, fmin=fmin, frame_length=L, **ALL)
        mf = dd.core.stream_mfcc(xd[:, k * N:(k + 1) * N], sr, hop, sm, **skw)
        want = (sep[0], mf) + tuple(sep[1:])
        assert len(got) == len(want) == 5
        for name, u, v in zip(NAMES, got, want):
            assert u.dtype == v.dtype and u.shape == v.shape and torch.equal(u, v), (L, M, k, name)
        for s in (one, two, sm):
            dd.core.stream_advance(s)
    assert torch.equal(one.buf[:ring_bytes], two.buf[:ring_bytes]), (L, M)
    # the running maximum behind the rings is the separate MFCC stream's
    assert torch.equal(one.buf[ring_bytes:ring_bytes + 4 * B],
                       sm.buf[4 * B * sf.sizes(M, hop, N)[3]:][:4 * B]), (L, M)


@pytest.mark.parametrize("sr,hop,N,B,L,K", pc.STREAM)
def test_same_bits_as_the_separate_launches(dd, sr, hop, N, B, L, K):
    x = np.array(pc.stream_case(sr, hop, N, B, L, K)[0])
    assert_the_separate_launches_bits(dd, x, sr, hop, N, L, L // 2, default=True)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("L", [64, 128, 256, 512, 1024, 2048])
def test_same_bits_at_every_transform_size(dd, L, half):
    """Each (L, M) is its own instantiation; hop L/4 + 1 (odd), N = 3 hop, B = 2 at 16 kHz, calls for two ring
    wraps."""
    hop, _, fmin, f_lo, f_hi = pc.size_params(L)
    N, B = 3 * hop, 2
    K = -(-2 * sf.sizes(L, hop, N)[3] // N) + 1
    assert sf.ring_wraps(L, hop, N, K) >= 2.0
    x = pr.make_voiced(pc.SIZES_SR, K * N, B, seed=L, f_lo=f_lo, f_hi=f_hi)
    assert_the_separate_launches_bits(dd, x, pc.SIZES_SR, hop, N, L, L // 2 if half else L, fmin=fmin)


@functools.lru_cache(maxsize=None)
def mfcc_reference(sr, hop, N, B, L, K):
    """The aligned MFCC (M = L/2, default tables) of pc.stream_case's input in fp64 and fp32, [B, K, R, 30]."""
    x = pc.stream_case(sr, hop, N, B, L, K)[0]
    out = []
    for dt in (np.float64, np.float32):
        a = np.stack([am.aligned_mfcc(x[b], sr, L, L // 2, hop, N, dtype=dt) for b in range(B)]).astype(np.float64)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


@pytest.mark.parametrize("sr,hop,N,B,L,K", pc.STREAM)
def test_accuracy_against_the_fp64_restatements(dd, sr, hop, N, B, L, K):
    x, _, ref = pc.stream_case(sr, hop, N, B, L, K)
    xg = torch.from_numpy(np.array(x)).cuda()
    (loud, mfcc, f0, conf, period), _ = run_aligned(dd, xg, sr, hop, N, L, mfcc_n_fft=L // 2)
    R = N // hop
    assert loud.shape == f0.shape == conf.shape == period.shape == (B, K * R) and mfcc.shape == (B, K * R, 30)
    tag = f"aligned stream sr {sr} hop {hop} N {N} B {B} L {L} M {L // 2} K {K}"
    m64, m32 = mfcc_reference(sr, hop, N, B, L, K)
    mfcc_gate(tag + " mfcc", mfcc.reshape(B, K, R, 30).cpu().numpy(), m64, m32)
    pitch_gate(tag, f0.cpu().numpy(), conf.cpu().numpy(), period.cpu().numpy(), ref)
    ref64, ref32 = loudness_reference(sr, hop, N, B, L, K)
    loudness_gate(tag + " loudness", loud.cpu().numpy(), ref64, ref32)


@pytest.mark.parametrize("sr,hop,N,B,L,K", pc.STREAM[::2])
def test_without_pitch(dd, sr, hop, N, B, L, K):
    xg = torch.from_numpy(np.array(pc.stream_case(sr, hop, N, B, L, K)[0])).cuda()
    full, sa = run_aligned(dd, xg, sr, hop, N, L, mfcc_n_fft=L // 2)
    got, sb = run_aligned(dd, xg, sr, hop, N, L, pitch=False, mfcc_n_fft=L // 2)
    assert len(got) == 2 and torch.equal(got[0], full[0]) and torch.equal(got[1], full[1])
    assert torch.equal(sa.buf, sb.buf)
    with pytest.raises(RuntimeError, match="pitch=True"):
        dd.core.stream_analysis_mfcc(xg[:, :N], sr, hop, sb, pitch=False, frame_length=L, mfcc_n_fft=L // 2,
                                     return_confidence=True)


def test_a_call_run_twice_before_the_advance_and_reset(dd):
    sr, hop, N, B, L, K = pc.STREAM[0]
    xg = torch.from_numpy(np.array(pc.stream_case(sr, hop, N, B, L, K)[0])).cuda()
    once = dd.core.FeatureStreamState(B, "cuda", N, L, hop)
    twice = dd.core.FeatureStreamState(B, "cuda", N, L, hop)
    first = []
    for k in range(K):
        xc = xg[:, k * N:(k + 1) * N]
        a = dd.core.stream_analysis_mfcc(xc, sr, hop, once, **ALL)
        b1 = dd.core.stream_analysis_mfcc(xc, sr, hop, twice, **ALL)
        b2 = dd.core.stream_analysis_mfcc(xc, sr, hop, twice, **ALL)
        for u, v, w in zip(a, b1, b2):
            assert torch.equal(u, v) and torch.equal(u, w), k
        assert torch.equal(once.buf, twice.buf), k   # the rings and the running maximum as one run leaves them
        assert int(twice.counter.item()) == k         # the call reads the counter and never writes it
        dd.core.stream_advance(once)
        dd.core.stream_advance(twice)
        first.append(a)
    once.reset()
    assert int(once.counter.item()) == 0 and not once.buf.any()
    for k in range(K):
        again = dd.core.stream_analysis_mfcc(xg[:, k * N:(k + 1) * N], sr, hop, once, **ALL)
        for u, v in zip(again, first[k]):
            assert torch.equal(u, v), k
        dd.core.stream_advance(once)
    with pytest.raises(RuntimeError, match="another batch"):
        dd.core.stream_analysis_mfcc(xg[:, :N], sr, hop, dd.core.FeatureStreamState(B, "cuda", N, 1024, hop))


def test_an_items_bits_do_not_depend_on_its_batch(dd):
    sr, hop, N, B, L, K = pc.STREAM[2]
    assert B == 3
    xg = torch.from_numpy(np.array(pc.stream_case(sr, hop, N, B, L, K)[0])).cuda()
    whole, _ = run_aligned(dd, xg, sr, hop, N, L, mfcc_n_fft=L // 2)
    for b in range(B):
        alone, _ = run_aligned(dd, xg[b:b + 1].contiguous(), sr, hop, N, L, mfcc_n_fft=L // 2)
        for u, v in zip(alone, whole):
            assert torch.equal(u[0], v[b]), b


def test_torch_op_returns_the_python_functions_bits(dd):
    from ddsp_pytorch_amd import script
    script.load_ops()
    sr, hop, N, B, L, K = pc.STREAM[2]
    M = L // 2
    x, (tmin, tmax), _ = pc.stream_case(sr, hop, N, B, L, K)
    xg = torch.from_numpy(np.array(x)).cuda()
    want, _ = run_aligned(dd, xg, sr, hop, N, L, mfcc_n_fft=M)
    (w,) = dd.core._feature_tables("a_weighting", (float(sr), L), xg.device,
                                   lambda: (dd.core.a_weighting_table(sr, L),))
    tabs = dd.core.mfcc_tables(sr, 30, M, 128, 20.0, 8000.0, xg.device)
    R = N // hop
    for pitch in (True, False):
        st = dd.core.FeatureStreamState(B, "cuda", N, L, hop)
        for k in range(K):
            xc = xg[:, k * N:(k + 1) * N]
            got = torch.ops.ddsp_hip.analysis_mfcc_stream(xc.unsqueeze(-1), w, *tabs, L, M, hop, 80.0, pitch, tmin,
                                                          tmax, float(sr), 0.1, st.counter, st.buf)
            assert len(got) == 5
            for name, u, v in zip(NAMES, got, want):
                if pitch or name in ("loudness", "mfcc"):
                    assert u.dtype == v.dtype and torch.equal(u, v[:, k * R:(k + 1) * R]), (pitch, k, name)
                else:
                    assert u.numel() == 0, name
            dd.core.stream_advance(st)


KEYS = ("loudness", "mfcc", "pitch", "confidence")


def test_stream_analyzer_aligned(dd):
    """StreamAnalyzer(pitch=True, aligned=True): core.stream_analysis_mfcc's bits call by call from one state, every
    delay equal; without the pitch the same loudness and MFCC; a call captures into one HIP graph after a warm-up
    call; reset() restarts it.  aligned=False is untouched: three states, the MFCC 512 samples ahead."""
    sr, hop, N, K = 48000, 256, 1024, 6
    x = torch.from_numpy(pr.make_voiced(sr, K * N, 1, seed=17)).cuda()
    kw = dict(mean_loudness=-6.5, std_loudness=1.75)
    an = dd.features.StreamAnalyzer(sr, hop, N, pitch=True, aligned=True, **kw)
    nop = dd.features.StreamAnalyzer(sr, hop, N, aligned=True, **kw)
    old = dd.features.StreamAnalyzer(sr, hop, N, pitch=True, **kw)
    assert an.mfcc_state is an.loudness_state and an.pitch_state is an.loudness_state
    assert nop.mfcc_state is nop.loudness_state and nop.pitch_state is None
    assert an.delay_frames == {"loudness": 3, "mfcc": 3, "pitch": 3} and nop.delay_frames == {"loudness": 3, "mfcc": 3}
    assert old.delay_frames == {"loudness": 3, "mfcc": 1, "pitch": 3} and old.mfcc_state is not old.loudness_state
    st = dd.core.FeatureStreamState(1, "cuda", N, 2048, hop)
    want = []
    for k in range(K):
        xc = x[:, k * N:(k + 1) * N]
        loud, mfcc, f0, conf = dd.core.stream_analysis_mfcc(xc, sr, hop, st, return_confidence=True)
        dd.core.stream_advance(st)
        w = {"loudness": ((loud - kw["mean_loudness"]) / kw["std_loudness"]).unsqueeze(-1), "mfcc": mfcc,
             "pitch": f0.unsqueeze(-1), "confidence": conf.unsqueeze(-1)}
        a, b = an(xc), nop(xc)
        assert set(a) == set(KEYS) and set(b) == {"loudness", "mfcc"}
        for key in KEYS:
            assert a[key].shape == w[key].shape and torch.equal(a[key], w[key]), (k, key)
        assert torch.equal(b["loudness"], w["loudness"]) and torch.equal(b["mfcc"], w["mfcc"]), k
        want.append(w)
    assert int(an.counter.item()) == K
    an.reset()
    assert int(an.counter.item()) == 0 and not an.loudness_state.buf.any()
    first = an(x[:, :N])
    for key in KEYS:
        assert torch.equal(first[key], want[0][key]), key
    # one HIP graph: the launch and the advance
    an = dd.features.StreamAnalyzer(sr, hop, N, pitch=True, aligned=True, **kw)
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
