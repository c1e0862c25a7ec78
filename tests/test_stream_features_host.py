"""The streaming analysis without a GPU: the numpy restatement of its semantics (tests/stream_features_ref.py)
against the offline restatement (tests/features_ref.py), and the argument checks of its C-ABI entry points
(include/ddsp_hip.h, "streaming analysis")."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import features_ref as fr
import stream_features_ref as sr_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12  # fp64: both sides run the same formulas on the same windows

# (n_fft, hop, N) -> (R, d, Hs, first frame of call 0), written out, not computed
GEOMETRY = {
    (2048, 256, 1024): (4, 4, 1792, -3),    # the realtime shape
    (2048, 512, 512): (1, 2, 1536, -1),     # one frame per call
    (2048, 160, 480): (3, 7, 1984, -6),     # hop not a power of two, n_fft/2 not a multiple of hop
    (1024, 64, 2048): (32, 8, 960, -7),     # the frame cap
    (16, 5, 15): (3, 2, 13, -1),            # the smallest transform
}
SAMPLE_RATE = 16000


def calls_for(n_fft, hop, N):
    """Enough calls for the ring to go round twice, and at least three."""
    L = sr_.sizes(n_fft, hop, N)[3]
    return max(3, -(-2 * L // N) + 1)


def offline_input(x_all, n_fft, hop):
    """concat(zeros(Z), x_all), Z = hop ceil(n_fft / hop): stream frame f is offline frame f + Z / hop, and every
    compared window is clear of the reflect padding at both ends."""
    Z = hop * -(-n_fft // hop)
    return np.concatenate([np.zeros(Z), np.asarray(x_all, dtype=np.float64)]), Z // hop


@pytest.mark.parametrize("n_fft,hop,N", list(GEOMETRY))
def test_index_arithmetic(n_fft, hop, N):
    R, d, Hs, first = GEOMETRY[(n_fft, hop, N)]
    assert sr_.sizes(n_fft, hop, N) == (R, d, Hs, Hs + N)
    assert sr_.first_frame(n_fft, hop, N) == first
    assert sr_.first_frame(n_fft, hop, N, k=5) == 5 * R + first
    # the newest sample the last frame of call k needs is inside the call; the oldest is Hs before it
    k = 3
    newest = (k * R - d + 1 + R - 1) * hop - n_fft // 2 + n_fft - 1
    oldest = (k * R - d + 1) * hop - n_fft // 2
    assert newest <= (k + 1) * N - 1 and oldest == k * N - Hs
    # the lag the features carry: d - 1 frames (768 samples at the realtime shape)
    from ddsp_pytorch_amd import core
    assert core.stream_feature_delay(n_fft, hop) == d - 1 == -first
    if (n_fft, hop) == (2048, 256):
        assert (d - 1) * hop == 768


@pytest.mark.parametrize("n_fft,hop,N", list(GEOMETRY))
def test_ring_bookkeeping_is_race_free_and_wraps(n_fft, hop, N):
    """With a ring of Hs + N floats the positions a call writes are disjoint from those it reads (so the copy
    needs no ordering), and the windows are those of the concatenated stream."""
    K = calls_for(n_fft, hop, N)
    assert sr_.ring_wraps(n_fft, hop, N, K) >= 2.0
    x = fr.make_signal(SAMPLE_RATE, K * N, 1, seed=n_fft + hop)[0].astype(np.float64)
    st = sr_.Stream(n_fft, hop, N)
    R, d, Hs, L = sr_.sizes(n_fft, hop, N)
    padded = np.concatenate([np.zeros(Hs), x])  # sample s at s + Hs
    for k in range(K):
        w = st.windows(x[k * N:(k + 1) * N])
        assert not (st.reads & st.writes), k
        assert len(st.writes) == N
        for j in range(R):
            f = k * R - d + 1 + j
            s0 = f * hop - n_fft // 2 + Hs
            assert s0 >= 0
            assert np.array_equal(w[j], padded[s0:s0 + n_fft]), (k, j)
        st.advance()


@pytest.mark.parametrize("n_fft,hop,N", list(GEOMETRY))
def test_stream_loudness_is_the_offline_loudness_of_the_zero_prefixed_stream(n_fft, hop, N):
    K = calls_for(n_fft, hop, N)
    x = fr.make_signal(SAMPLE_RATE, K * N, 1, seed=n_fft + hop + 1)[0]
    got = sr_.loudness(x, SAMPLE_RATE, hop, N, n_fft=n_fft).reshape(-1)
    xz, shift = offline_input(x, n_fft, hop)
    S = np.abs(fr.stft(xz, n_fft, hop))
    want_all = np.mean(np.log(S + 1e-7) + fr.a_weighting(fr.fft_frequencies(SAMPLE_RATE, n_fft))[None, :], axis=1)
    f0 = sr_.first_frame(n_fft, hop, N)
    idx = f0 + np.arange(got.size) + shift
    assert idx.min() >= 0 and idx.max() < len(want_all)
    assert np.abs(got - want_all[idx]).max() <= TOL


def mel_shape(n_fft):
    n_mels = 128 if n_fft >= 512 else max(4, n_fft // 4)
    return n_mels, min(30, n_mels)


@pytest.mark.parametrize("n_fft,hop,N", list(GEOMETRY))
def test_stream_mfcc_is_the_offline_mel_db_under_the_causal_clamp(n_fft, hop, N):
    K = calls_for(n_fft, hop, N)
    R = N // hop
    n_mels, n_mfcc = mel_shape(n_fft)
    x = fr.make_signal(SAMPLE_RATE, K * N, 1, seed=n_fft + hop + 2)[0]
    # a quiet start, so that the running maximum moves during the stream
    x = x * np.where(np.arange(K * N) < (K // 2) * N, np.float32(1e-3), np.float32(1.0))
    kw = dict(n_fft=n_fft, n_mels=n_mels, fmin=20.0, fmax=8000.0)
    got = sr_.mfcc(x, SAMPLE_RATE, hop, N, n_mfcc=n_mfcc, top_db=80.0, **kw)
    xz, shift = offline_input(x, n_fft, hop)
    D_all = fr.mel_db(xz, SAMPLE_RATE, hop, **kw)
    f0 = sr_.first_frame(n_fft, hop, N)
    idx = f0 + np.arange(K * R) + shift
    assert idx.min() >= 0 and idx.max() < len(D_all)
    D = D_all[idx].reshape(K, R, n_mels)
    assert np.abs(D - sr_.mel_db(x, SAMPLE_RATE, hop, N, **kw)).max() <= 1e-9  # dB of a 128-term BLAS sum
    run = -np.inf
    want = np.empty((K, R, n_mfcc))
    runs = []
    for k in range(K):
        run = max(run, D[k].max())
        runs.append(run)
        want[k] = np.maximum(D[k], run - 80.0) @ fr.dct_matrix(n_mfcc, n_mels).T
    assert runs[-1] > runs[0] + 30.0  # the clamp level did move
    scale = max(1.0, np.abs(want).max())
    assert np.abs(got - want).max() <= TOL * scale


# ---------------------------------------------------------------------------------------------------------
# the C-ABI
# ---------------------------------------------------------------------------------------------------------
NEW = ("ddsp_hip_stream_features_state_bytes", "ddsp_hip_stream_loudness", "ddsp_hip_stream_mfcc")
EINVAL, EWS, ERANGE = 1, 4, 5


@pytest.fixture(scope="module")
def lib():
    from ddsp_pytorch_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", ROOT, "-j4"], check=True)
    return _lib.load()


def test_entry_points_are_declared_exported_and_bound(lib):
    from ddsp_pytorch_amd import _lib
    header = open(os.path.join(ROOT, "include", "ddsp_hip.h")).read()
    declared = set(re.findall(r"\b(ddsp_hip_\w+)\s*\(", header))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                        check=True).stdout
    for name in NEW:
        assert name in declared, name
        assert re.search(rf"\b{name}\b", nm), name
        assert name in _lib.SIGNATURES, name
    assert lib.ddsp_hip_version() >= 105
    # the header states the frame index formula and cites the reference
    section = header[header.index("streaming analysis"):]
    assert "f = k R - d + 1 + j" in section and "core.py:81-97" in section and "preprocess.py:30-32" in section


def state_bytes_by_the_documented_layout(B, N, n_fft, hop):
    """Per item a ring of Hs + N floats, then one float per item, rounded up to 16 bytes."""
    Hs = (-(-(n_fft // 2) // hop) - 1) * hop + n_fft // 2
    return -(-4 * (B * (Hs + N) + B) // 16) * 16


def test_state_bytes(lib):
    q = lib.ddsp_hip_stream_features_state_bytes
    assert q(1, 1024, 2048, 256) == 11280 == state_bytes_by_the_documented_layout(1, 1024, 2048, 256)
    for (n_fft, hop, N) in GEOMETRY:
        for B in (1, 3, 65535):
            assert q(B, N, n_fft, hop) == state_bytes_by_the_documented_layout(B, N, n_fft, hop), (B, N, n_fft, hop)
    # outside the envelope: 0
    for args in [(0, 1024, 2048, 256), (-1, 1024, 2048, 256), (65536, 1024, 2048, 256),  # batch
                 (1, 1024, 1000, 250), (1, 1024, 8, 256), (1, 1024, 8192, 256),         # n_fft
                 (1, 1024, 2048, 0), (1, 1000, 2048, 256), (1, 0, 2048, 256),           # hop, N % hop, N
                 (1, 33 * 64, 2048, 64)]:                                               # R = 33
        assert q(*args) == 0, args
    assert q(1, 32 * 64, 2048, 64) > 0  # R = 32: the cap itself


def test_stream_entry_points_reject_bad_arguments_without_launching(lib):
    """Every call below returns before any HIP call (there is no device here): the documented code each."""
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(256)  # p: never dereferenced
    big = 1 << 30

    def loud(x=p, w=p, out=p, counter=p, state=p, nbytes=big, B=1, N=1024, n_fft=2048, hop=256):
        return lib.ddsp_hip_stream_loudness(x, w, out, counter, state, nbytes, B, N, n_fft, hop, null)

    def mfcc(x=p, bs=p, bc=p, bw=p, n_w=100, dct=p, out=p, counter=p, state=p, nbytes=big, B=1, N=1024, n_fft=1024,
             hop=256, n_mels=128, n_mfcc=30, top_db=80.0):
        return lib.ddsp_hip_stream_mfcc(x, bs, bc, bw, n_w, dct, out, counter, state, nbytes, B, N, n_fft, hop, n_mels,
                                        n_mfcc, top_db, null)

    for fn in (loud, mfcc):
        assert fn(n_fft=1000) == ERANGE and fn(n_fft=8) == ERANGE and fn(n_fft=8192) == ERANGE
        assert fn(hop=0) == EINVAL and fn(hop=-256) == EINVAL
        assert fn(N=1000) == EINVAL  # not a multiple of hop
        assert fn(N=0) == EINVAL and fn(N=-1024) == EINVAL
        assert fn(N=33 * 64, hop=64) == ERANGE  # 33 frames per call
        assert fn(B=65536) == ERANGE and fn(B=-1) == EINVAL
        assert fn(B=0, x=null, out=null, counter=null, state=null, nbytes=0) == 0  # an empty batch: a no-op
        for missing in ("x", "out", "counter", "state"):
            assert fn(**{missing: null}) == EINVAL, missing
        need = lib.ddsp_hip_stream_features_state_bytes(1, 1024, 2048 if fn is loud else 1024, 256)
        assert fn(nbytes=need - 1) == EWS and fn(nbytes=0) == EWS
        # the envelope comes before the pointers and the state
        assert fn(n_fft=1000, x=null, nbytes=0) == ERANGE
    assert mfcc(n_mels=257, n_mfcc=30) == ERANGE
    assert mfcc(n_mels=0) == EINVAL and mfcc(n_mfcc=0) == EINVAL and mfcc(n_mfcc=129) == EINVAL
    assert mfcc(top_db=-1.0) == EINVAL and mfcc(top_db=float("nan")) == EINVAL
    assert mfcc(n_w=-1) == EINVAL
    for missing in ("bs", "bc", "bw", "dct"):
        assert mfcc(**{missing: null}) == EINVAL, missing


def test_cpu_tensors_raise():
    import ddsp_pytorch_amd as dd
    state = types.SimpleNamespace(batch=1, call_samples=1024, n_fft=2048, hop=256)  # never reached
    x = torch.zeros(1, 1024)
    with pytest.raises(RuntimeError, match="HIP device"):
        dd.core.stream_loudness(x, 48000, 256, state)
    state.n_fft = 1024
    with pytest.raises(RuntimeError, match="HIP device"):
        dd.core.stream_mfcc(x, 48000, 256, state)
    with pytest.raises(RuntimeError, match="HIP device"):
        dd.core.FeatureStreamState(1, "cpu", 1024, 2048, 256)
    with pytest.raises(RuntimeError, match="HIP device"):
        dd.features.StreamAnalyzer(48000, 256, 1024, device="cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        dd.StreamAnalyzer(48000, 256, 1024, device="cpu")
