"""The fused streamed analysis' boundary on the CPU (ddsp_hip_stream_analysis: the streamed loudness and the streamed
pitch of one call in one launch over one state): the entry point is declared, exported and bound, answers the
documented code for every bad argument before any HIP call (there is no device here), and the host layers refuse
what they cannot run."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ddsp_hip_stream_analysis"
EINVAL, EWS, ERANGE = 1, 4, 5


@pytest.fixture(scope="module")
def lib():
    from ddsp_pytorch_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", ROOT, "-j4"], check=True)
    return _lib.load()


def test_entry_point_is_declared_exported_and_bound(lib):
    from ddsp_pytorch_amd import _lib
    header = open(os.path.join(ROOT, "include", "ddsp_hip.h")).read()
    assert NAME in set(re.findall(r"\b(ddsp_hip_\w+)\s*\(", header))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                        check=True).stdout
    assert re.search(rf"\b{NAME}\b", nm)
    assert NAME in _lib.SIGNATURES
    assert lib.ddsp_hip_version() >= 107


def test_entry_point_rejects_bad_arguments_without_launching(lib):
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(256)  # p: never dereferenced
    big = 1 << 30

    def fn(x=p, w=p, loud=p, f0=p, conf=p, period=p, counter=p, state=p, nbytes=big, B=1, N=1024, L=2048, hop=256,
           tmin=24, tmax=960, sr=48000.0, thr=0.1):
        return lib.ddsp_hip_stream_analysis(x, w, loud, f0, conf, period, counter, state, nbytes, B, N, L, hop, tmin,
                                            tmax, sr, thr, null)

    # frame length outside the pitch's envelope [64, 4096] or not a power of two (the lags are valid for any L >= 8)
    assert fn(L=32, tmin=1, tmax=2) == ERANGE
    assert fn(L=8192, tmin=1, tmax=2) == ERANGE
    assert fn(L=96, tmin=1, tmax=2) == ERANGE
    # the call is whole hops, at most 32 of them
    assert fn(N=1000) == EINVAL and fn(N=0) == EINVAL and fn(hop=0) == EINVAL
    assert fn(N=33 * 64, hop=64) == ERANGE
    # tau bounds: 1 <= tau_min <= tau_max <= L/2 - 1; the sample rate
    assert fn(tmin=0) == EINVAL and fn(tmin=961) == EINVAL and fn(tmax=1024) == EINVAL
    assert fn(sr=0.0) == EINVAL and fn(sr=-48000.0) == EINVAL and fn(sr=float("nan")) == EINVAL
    # the streaming envelope is checked before the pitch parameters
    assert fn(N=1000, tmin=0) == EINVAL and fn(N=33 * 64, hop=64, tmin=0) == ERANGE
    # batch 0: a no-op success, whatever the buffers; a negative batch is not
    assert fn(B=0, x=null, w=null, loud=null, f0=null, conf=null, period=null, counter=null, state=null) == 0
    assert fn(B=-1) == EINVAL and fn(B=65536) == ERANGE
    # null buffers
    for name in ("x", "f0", "loud", "counter", "state"):
        assert fn(**{name: null}) == EINVAL, name
    # a short state; confidence, period (and the weights) may be null: such a call gets as far as the workspace check
    need = lib.ddsp_hip_stream_features_state_bytes(1, 1024, 2048, 256)
    assert need == 11280
    assert fn(nbytes=need - 16) == EWS and fn(nbytes=0) == EWS and fn(B=3, nbytes=need) == EWS
    assert fn(conf=null, nbytes=need - 16) == EWS and fn(period=null, nbytes=need - 16) == EWS
    assert fn(conf=null, period=null, w=null, nbytes=need - 16) == EWS


def test_host_layers_refuse_what_they_cannot_run():
    import ddsp_pytorch_amd as dd
    assert "stream_analysis" in dd.core.__all__
    sig = inspect.signature(dd.core.stream_analysis)
    assert list(sig.parameters)[:4] == ["x", "sample_rate", "block_size", "state"]
    want = dict(fmin=50.0, fmax=2000.0, frame_length=2048, threshold=0.1, return_confidence=False,
                return_period=False)
    assert {k: sig.parameters[k].default for k in want} == want

    class State:  # a CPU tensor is refused before the state is looked at
        pass
    with pytest.raises(RuntimeError, match="HIP device"):
        dd.core.stream_analysis(torch.zeros(1, 1024), 48000, 256, State())
    # RealtimeGraph on a CPU model: the error of before, whatever the new options
    from ddsp_pytorch_amd.realtime import RealtimeGraph
    model = dd.DDSPDecoder(64, 16, 9, 48000, 256, False)
    for kw in ({}, {"pitch_from_audio": True, "loudness_from_audio": True}):
        with pytest.raises(RuntimeError, match="the model must be on a HIP device"):
            RealtimeGraph(model, call_samples=1024, **kw)
    sig = inspect.signature(RealtimeGraph.__init__)
    want = dict(pitch_from_audio=False, pitch_fmin=50.0, pitch_fmax=2000.0, pitch_threshold=0.1)
    assert {k: sig.parameters[k].default for k in want} == want
    # StreamAnalyzer(fused=True) is the loudness and the pitch in one launch: without the pitch there is nothing to fuse
    sig = inspect.signature(dd.features.StreamAnalyzer.__init__)
    assert sig.parameters["fused"].default is False
    with pytest.raises(ValueError, match="pitch=True"):
        dd.features.StreamAnalyzer(48000, 256, 1024, device="cpu", fused=True)
