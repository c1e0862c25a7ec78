"""The streamed Viterbi pitch tracker's boundary on the CPU: the three entry points are declared, exported and bound,
answer the documented code for every bad argument before any HIP call, in the documented order (there is no device
here), the state-size formula is the header's, and the host layer refuses CPU tensors and bad options."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ddsp_hip_stream_pitch_salience", "ddsp_hip_stream_viterbi_state_bytes", "ddsp_hip_stream_pitch_viterbi")
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
    # the header carries the definition: the fixed-lag decision, the state and its rerun argument, the horizon; and
    # the offline section points to it
    section = header[header.index("pitch_viterbi_stream:"):]
    for phrase in ("min(D, n) steps back", "counter == 0", "P = D + R", "never renormalised",
                   "run twice before the advance"):
        assert phrase in section, phrase
    offline = header[header.index("pitch_viterbi: a Viterbi-decoded"):header.index("pitch_viterbi_stream:")]
    assert "decode needs the future" in offline and '"pitch_viterbi_stream"' in offline


def test_state_size_formula(lib):
    size = lib.ddsp_hip_stream_viterbi_state_bytes

    def want(B, R, NB, D):  # per item delta[2][NB] fp64, then (D + R) frames of f0c, cost (fp32) and bp (int8)
        item = (16 * NB + 9 * (D + R) * NB + 7) // 8 * 8
        return (B * item + 15) // 16 * 16

    for B, R, NB, D in ((1, 4, 256, 0), (1, 4, 256, 4), (3, 1, 1, 0), (3, 2, 63, 3), (2, 32, 1024, 64), (5, 1, 65, 1),
                        (7, 3, 1, 64)):
        assert size(B, R, NB, D) == want(B, R, NB, D), (B, R, NB, D)
    assert size(1, 4, 256, 0) == 13312 and size(3, 1, 1, 0) == 96  # roundup8(25) = 32 per item
    # outside the envelope, and without a batch: 0
    for args in ((0, 4, 256, 0), (-1, 4, 256, 0), (1, 0, 256, 0), (1, 33, 256, 0), (1, 4, 0, 0), (1, 4, 1025, 0),
                 (1, 4, 256, -1), (1, 4, 256, 65)):
        assert size(*args) == 0, args
    # the salience's ring is the streamed features' state
    assert lib.ddsp_hip_stream_features_state_bytes(1, 1024, 2048, 256) == 11280


def test_salience_rejects_bad_arguments_in_order_without_launching(lib):
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(256)  # p: never dereferenced
    big = 1 << 30

    def sal(x=p, lo=p, hi=p, cost=p, f0c=p, lag=p, f0=p, conf=p, period=p, counter=p, state=p, nbytes=big, B=1,
            N=1024, L=2048, hop=256, tmin=24, tmax=960, NB=256, sr=48000.0, thr=0.1):
        return lib.ddsp_hip_stream_pitch_salience(x, lo, hi, cost, f0c, lag, f0, conf, period, counter, state, nbytes,
                                                  B, N, L, hop, tmin, tmax, NB, sr, thr, null)

    # the streaming envelope
    assert sal(B=-1) == EINVAL and sal(N=0) == EINVAL and sal(hop=0) == EINVAL and sal(N=1000) == EINVAL
    assert sal(N=33 * 64, hop=64) == ERANGE and sal(B=65536) == ERANGE and sal(L=8192, tmin=1, tmax=2) == ERANGE
    # the pitch parameters
    assert sal(L=32, tmin=1, tmax=2) == ERANGE  # inside the streaming envelope, below the pitch's
    assert sal(tmin=0) == EINVAL and sal(tmin=961) == EINVAL and sal(tmax=1024) == EINVAL
    assert sal(sr=0.0) == EINVAL and sal(sr=float("nan")) == EINVAL
    # n_bins in [1, 1024]
    assert sal(NB=0) == EINVAL and sal(NB=-4) == EINVAL and sal(NB=1025) == ERANGE
    # confidence or period without f0
    assert sal(f0=null) == EINVAL and sal(f0=null, conf=null) == EINVAL and sal(f0=null, period=null) == EINVAL
    # batch 0: a no-op success, whatever the buffers
    assert sal(B=0, x=null, lo=null, hi=null, cost=null, f0c=null, counter=null, state=null, nbytes=0) == 0
    # null pointers (lag, and f0 with confidence and period, may be null: these get as far as the state's size)
    for name in ("x", "lo", "hi", "cost", "f0c", "counter", "state"):
        assert sal(**{name: null}) == EINVAL, name
    need = lib.ddsp_hip_stream_features_state_bytes(1, 1024, 2048, 256)
    assert sal(lag=null, f0=null, conf=null, period=null, nbytes=need - 1) == EWS
    # a short state
    assert sal(nbytes=need - 1) == EWS and sal(nbytes=0) == EWS and sal(B=3, nbytes=need) == EWS
    # the order: each refusal hides the ones after it
    assert sal(N=1000, tmin=0, NB=0, f0=null, x=null, nbytes=0) == EINVAL      # the envelope
    assert sal(N=33 * 64, hop=64, tmin=0, NB=0) == ERANGE                      # the envelope before the parameters
    assert sal(L=32, tmin=1, tmax=2, NB=0) == ERANGE                           # the parameters before n_bins
    assert sal(NB=1025, f0=null, x=null) == ERANGE                             # n_bins before the pairing and nulls
    assert sal(B=0, NB=1025) == ERANGE and sal(B=0, f0=null) == EINVAL         # all of them before batch 0
    assert sal(x=null, nbytes=0) == EINVAL                                     # nulls before the state's size


def test_decode_rejects_bad_arguments_in_order_without_launching(lib):
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(256)
    big = 1 << 30

    def dec(cost=p, f0c=p, f0=p, conf=p, path=p, counter=p, state=p, nbytes=big, B=1, R=4, NB=256, J=12, D=0,
            lam=0.02):
        return lib.ddsp_hip_stream_pitch_viterbi(cost, f0c, f0, conf, path, counter, state, nbytes, B, R, NB, J, D,
                                                 lam, null)

    # negative sizes, R < 1, a transition that is negative, infinite or NaN
    assert dec(B=-1) == EINVAL and dec(R=0) == EINVAL and dec(R=-2) == EINVAL and dec(NB=0) == EINVAL
    assert dec(J=-1) == EINVAL and dec(D=-1) == EINVAL
    assert dec(lam=-0.5) == EINVAL and dec(lam=float("inf")) == EINVAL and dec(lam=float("nan")) == EINVAL
    assert dec(lam=0.0, nbytes=0) == EWS  # zero is a transition
    # the caps
    assert dec(R=33) == ERANGE and dec(NB=1025) == ERANGE and dec(J=128) == ERANGE and dec(D=65) == ERANGE
    assert dec(R=32, NB=1024, J=127, D=64, nbytes=0) == EWS  # the caps themselves are inside
    # batch 0
    assert dec(B=0, cost=null, f0c=null, f0=null, path=null, counter=null, state=null, nbytes=0) == 0
    # null pointers (confidence may be null)
    for name in ("cost", "f0c", "f0", "path", "counter", "state"):
        assert dec(**{name: null}) == EINVAL, name
    need = lib.ddsp_hip_stream_viterbi_state_bytes(1, 4, 256, 0)
    assert dec(conf=null, nbytes=need - 1) == EWS
    # a short state
    assert dec(nbytes=need - 1) == EWS and dec(D=1, nbytes=need) == EWS and dec(B=2, nbytes=need) == EWS
    # the order
    assert dec(R=33, lam=-1.0) == EINVAL and dec(R=33, D=-1) == EINVAL     # EINVAL before ERANGE
    assert dec(B=0, R=33) == ERANGE and dec(B=0, lam=-1.0) == EINVAL       # both before batch 0
    assert dec(cost=null, nbytes=0) == EINVAL                              # nulls before the state's size


def test_host_layer_refuses_cpu_tensors_and_bad_options():
    import ddsp_pytorch_amd as dd
    for name in ("ViterbiStreamState", "stream_pitch_salience", "stream_viterbi_path", "stream_track_pitch"):
        assert name in dd.core.__all__, name
    with pytest.raises(RuntimeError, match="HIP device"):
        dd.core.ViterbiStreamState(1, "cpu", 4, 256, 0)
    with pytest.raises(RuntimeError, match="HIP device"):
        dd.core.stream_viterbi_path(torch.zeros(1, 4, 8), torch.zeros(1, 4, 8), None)
    assert dd.core.stream_pitch_bin_count(48000, 50.0, 2000.0, 2048) == 256
    with pytest.raises(ValueError, match="needs pitch=True"):
        dd.features.StreamAnalyzer(48000, 256, 1024, viterbi=True)
    with pytest.raises(ValueError, match="viterbi=True takes the pitch"):
        dd.features.StreamAnalyzer(48000, 256, 1024, pitch=True, fused=True, viterbi=True)
    sig = inspect.signature(dd.features.StreamAnalyzer.__init__)
    assert (sig.parameters["viterbi"].default, sig.parameters["pitch_lag"].default) == (False, 0)
    from ddsp_pytorch_amd.realtime import RealtimeGraph
    sig = inspect.signature(RealtimeGraph.__init__)
    want = dict(pitch_viterbi=False, pitch_lag=0, pitch_transition=0.02, pitch_max_jump=12)
    assert {k: sig.parameters[k].default for k in want} == want
    sig = inspect.signature(dd.core.stream_viterbi_path)
    assert (sig.parameters["transition"].default, sig.parameters["max_jump"].default) == (0.02, 12)
    sig = inspect.signature(dd.core.ViterbiStreamState.__init__)
    assert list(sig.parameters)[1:] == ["batch", "device", "frames_per_call", "n_bins", "lag", "counter"]
