"""The pitch tracker's boundary on the CPU: the two entry points are declared, exported and bound, answer the
documented code for every bad argument before any HIP call (there is no device here), and the host layer refuses
CPU tensors."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ddsp_hip_pitch", "ddsp_hip_stream_pitch")
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
    assert lib.ddsp_hip_version() >= 106
    # the header carries the definition: the floor, the lag bounds and what the reference's extract_pitch is
    section = header[header.index("pitch: YIN"):]
    assert "2^-40" in section and "tau_min <= tau_max <= W - 1" in section and "core.py:100-119" in section


def test_entry_points_reject_bad_arguments_without_launching(lib):
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(256)  # p: never dereferenced
    big = 1 << 30

    def off(x=p, f0=p, conf=p, period=p, B=1, T=4096, L=2048, hop=512, tmin=24, tmax=960, sr=48000.0, thr=0.1):
        return lib.ddsp_hip_pitch(x, f0, conf, period, B, T, L, hop, tmin, tmax, sr, thr, null)

    def st(x=p, f0=p, conf=p, period=p, counter=p, state=p, nbytes=big, B=1, N=1024, L=2048, hop=256, tmin=24,
           tmax=960, sr=48000.0, thr=0.1):
        return lib.ddsp_hip_stream_pitch(x, f0, conf, period, counter, state, nbytes, B, N, L, hop, tmin, tmax, sr,
                                         thr, null)

    for fn in (off, st):
        # null buffers (confidence and period may be null: see batch 0 below for a call that gets that far)
        assert fn(x=null) == EINVAL and fn(f0=null) == EINVAL
        # sizes
        assert fn(B=-1) == EINVAL and fn(hop=0) == EINVAL and fn(hop=-256) == EINVAL and fn(L=0) == EINVAL
        # tau bounds: 1 <= tau_min <= tau_max <= W - 1
        assert fn(tmin=0) == EINVAL and fn(tmin=961) == EINVAL and fn(tmax=1024) == EINVAL
        assert fn(tmin=-3, tmax=-1) == EINVAL
        assert fn(L=64, tmin=1, tmax=32) == EINVAL
        # sample rate
        assert fn(sr=0.0) == EINVAL and fn(sr=-48000.0) == EINVAL and fn(sr=float("nan")) == EINVAL
        # frame_length outside the envelope (the lags are valid for any L >= 8)
        assert fn(L=48, tmin=1, tmax=2) == ERANGE and fn(L=8192, tmin=1, tmax=2) == ERANGE
        assert fn(L=32, tmin=1, tmax=2) == ERANGE
        assert fn(B=65536) == ERANGE
        # batch 0: a no-op success, whatever the buffers
        assert fn(B=0, x=null, f0=null, conf=null, period=null) == 0
    assert off(T=0) == EINVAL and off(T=1024) == EINVAL      # reflect padding needs T > L/2
    assert off(T=1025, x=null) == EINVAL                      # the padding fits; then the buffers
    assert st(N=0) == EINVAL and st(N=1000) == EINVAL         # N % hop
    assert st(N=33 * 64, hop=64) == ERANGE                    # R = 33
    assert st(counter=null) == EINVAL and st(state=null) == EINVAL
    need = lib.ddsp_hip_stream_features_state_bytes(1, 1024, 2048, 256)
    assert need == 11280
    assert st(nbytes=need - 1) == EWS and st(nbytes=0) == EWS
    assert st(B=3, nbytes=need) == EWS


def test_host_layer_refuses_cpu_tensors_and_bad_ranges():
    import ddsp_pytorch_amd as dd
    with pytest.raises(RuntimeError, match="HIP device"):
        dd.core.extract_pitch(torch.zeros(2, 4096), 48000, 512)
    with pytest.raises(RuntimeError, match="HIP device"):
        dd.features.analyze(torch.zeros(2, 4096), None, 48000, 512)
    with pytest.raises(RuntimeError, match="HIP device"):
        dd.core.FeatureStreamState(1, "cpu", 1024, 2048, 256)
    for name in ("extract_pitch", "stream_pitch", "pitch_lags"):
        assert name in dd.core.__all__


def test_signatures():
    import ddsp_pytorch_amd as dd
    sig = inspect.signature(dd.features.analyze)
    assert sig.parameters["pitch"].default is None
    assert "fmin" in sig.parameters and "fmax" in sig.parameters
    assert list(sig.parameters)[:4] == ["signal", "pitch", "sample_rate", "block_size"]
    with pytest.raises(TypeError, match="sample_rate and block_size"):
        dd.features.analyze(torch.zeros(1, 4096))
    sig = inspect.signature(dd.core.extract_pitch)
    want = dict(fmin=50.0, fmax=2000.0, frame_length=2048, threshold=0.1, return_confidence=False,
                return_period=False)
    assert {k: sig.parameters[k].default for k in want} == want
    assert list(sig.parameters)[:3] == ["signal", "sample_rate", "block_size"]
    sig = inspect.signature(dd.features.StreamAnalyzer.__init__)
    assert sig.parameters["pitch"].default is False
    assert (sig.parameters["fmin"].default, sig.parameters["fmax"].default) == (50.0, 2000.0)
    assert dd.features.StreamAnalyzer.N_FFT["pitch"] == 2048
    # install() does not rebind extract_pitch: the reference's is the CREPE network on host numpy
    import importlib
    inst = importlib.import_module("ddsp_pytorch_amd.install")
    assert "extract_pitch" not in inst.FUNCTIONS + inst.LOSS_FUNCTIONS
