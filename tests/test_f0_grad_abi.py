"""The pitch gradient's boundary on the CPU: its entry points are declared, exported and bound, answer the
documented code for every bad argument and for a short workspace before any HIP call (there is no device here), and
the host layer keeps refusing a per-sample f0 that requires grad only in core.harmonic_synth."""
import ctypes
import os
import re
import subprocess

import pytest

import f0_grad_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ddsp_hip_frame_pitch_grad_workspace_size", "ddsp_hip_frame_pitch_grad_scan_chunk",
       "ddsp_hip_harmonic_synth_frames_pitch_grad", "ddsp_hip_harmonic_synth_params_pitch_grad")
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
    assert lib.ddsp_hip_version() >= 108
    assert lib.ddsp_hip_frame_pitch_grad_scan_chunk() == fr.SCAN_CHUNK


def test_workspace_size(lib):
    size = lib.ddsp_hip_frame_pitch_grad_workspace_size
    assert size(2, 8) == 2 * 8 * 16          # (Q, R) as two doubles per frame
    assert size(1, 512) == 512 * 16
    assert size(1, 513) == 513 * 24          # and the phase prefix past 512 frames per item
    assert size(0, 8) == 0 and size(2, 0) == 0 and size(-1, 8) == 0


def test_entry_points_reject_bad_arguments_without_launching(lib):
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(256)  # p: never dereferenced
    big = 1 << 30

    def frames(f0=p, amp=p, dist=p, g=p, d=p, B=2, F=8, H=100, bs=512, sr=48000.0, ws=p, nbytes=big):
        return lib.ddsp_hip_harmonic_synth_frames_pitch_grad(f0, amp, dist, g, d, B, F, H, bs, sr, ws, nbytes, null)

    def params(f0=p, amp=p, dist=p, g=p, d=p, B=2, F=8, H=100, bs=512, sr=48000.0, ws=p, nbytes=big):
        return lib.ddsp_hip_harmonic_synth_params_pitch_grad(f0, amp, g, d, B, F, H, bs, sr, ws, nbytes, null)

    for fn in (frames, params):
        # null buffers
        assert fn(f0=null) == EINVAL and fn(amp=null) == EINVAL and fn(g=null) == EINVAL and fn(d=null) == EINVAL
        assert fn(ws=null) == EINVAL
        assert fn(ws=ctypes.c_void_p(260)) == EINVAL  # doubles: 8-byte aligned
        # sizes
        assert fn(B=-1) == EINVAL and fn(F=-1) == EINVAL and fn(bs=0) == EINVAL and fn(H=0) == EINVAL
        assert fn(sr=0.0) == EINVAL and fn(sr=-48000.0) == EINVAL and fn(sr=float("nan")) == EINVAL
        # the envelope
        assert fn(H=4097) == ERANGE and fn(bs=8193) == ERANGE and fn(B=65536) == ERANGE
        # a short workspace
        need = lib.ddsp_hip_frame_pitch_grad_workspace_size(2, 8)
        assert fn(nbytes=need - 1) == EWS and fn(nbytes=0) == EWS
        need = lib.ddsp_hip_frame_pitch_grad_workspace_size(1, 513)
        assert fn(B=1, F=513, nbytes=513 * 16) == EWS and fn(B=1, F=513, nbytes=need - 1) == EWS
        # nothing to do: a no-op success, whatever the buffers
        assert fn(B=0, f0=null, amp=null, g=null, d=null, ws=null, nbytes=0) == 0
        assert fn(F=0, f0=null, amp=null, g=null, d=null, ws=null, nbytes=0) == 0
    assert frames(dist=null) == EINVAL


def test_only_the_per_sample_op_refuses():
    """core.harmonic_synth is the one caller of grad.refuse_f0_grad left"""
    import inspect

    from ddsp_pytorch_amd import core, grad
    src = inspect.getsource(core)
    assert src.count("refuse_f0_grad") == 1
    assert "refuse_f0_grad" in inspect.getsource(core.harmonic_synth)
    assert "per-sample" in inspect.getsource(grad.refuse_f0_grad)
