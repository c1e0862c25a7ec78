"""ddsp_hip_synth_frames_route: which form of the fused frame kernel a launch takes, read from the launch plan
(synth_frame.hip frame_plan) without a device.  The fixed-shape kernel is taken exactly for 65 bands at block
512 when the launch is not split; a neighbouring shape must never reach it (it reads no shape argument)."""
import ctypes

import pytest

ANY, SPLIT, FIXED = 0, 1, 2  # enum ddsp_hip_synth_route
EINVAL, ERANGE = 1, 5


@pytest.fixture(scope="module")
def lib():
    from ddsp_pytorch_amd import _lib
    return _lib.load()


def route(lib, batch, frames, H, NB, bs, prefix=0):
    r = ctypes.c_int(-1)
    st = lib.ddsp_hip_synth_frames_route(batch, frames, H, NB, bs, prefix, ctypes.byref(r))
    return st, r.value


def test_header_names_the_routes():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                             "ddsp_hip.h")).read()
    for name, value in (("ANY", ANY), ("SPLIT", SPLIT), ("FIXED", FIXED)):
        assert f"DDSP_HIP_SYNTH_ROUTE_{name} = {value}" in text


@pytest.mark.parametrize("batch,frames", [(64, 200), (1, 512), (512, 1), (2, 256), (65535, 1)])
@pytest.mark.parametrize("H", [1, 7, 100, 128, 1024])
def test_shipped_shape_takes_the_fixed_form(lib, batch, frames, H):
    assert route(lib, batch, frames, H, 65, 512) == (0, FIXED)


@pytest.mark.parametrize("batch,frames", [(1, 511), (1, 1), (7, 73), (2, 255)])
def test_few_frames_split(lib, batch, frames):
    assert route(lib, batch, frames, 100, 65, 512) == (0, SPLIT)


@pytest.mark.parametrize("NB,bs", [(64, 512), (66, 512), (65, 508), (65, 516), (65, 256), (65, 1024), (9, 64)])
def test_neighbouring_shapes_stay_any_shape(lib, NB, bs):
    st, many = route(lib, 4, 512, 100, NB, bs)
    assert (st, many) == (0, ANY)
    st, few = route(lib, 1, 4, 100, NB, bs)
    assert st == 0 and few in (ANY, SPLIT) and few == (SPLIT if bs <= 512 else ANY)  # 4 * nt <= 256 threads
    assert route(lib, 1, 4, 100, NB, bs, prefix=1) == (0, ANY)


@pytest.mark.parametrize("batch,frames", [(1, 1), (1, 511), (1, 512), (3, 5625)])
def test_prefix_launch_is_never_split(lib, batch, frames):
    assert route(lib, batch, frames, 100, 65, 512, prefix=1) == (0, FIXED)


def test_invalid_sizes_and_envelope(lib):
    for args in ((-1, 1, 100, 65, 512), (1, -1, 100, 65, 512), (1, 1, 0, 65, 512), (1, 1, 100, 1, 512),
                 (1, 1, 100, 65, 0)):
        assert route(lib, *args) == (EINVAL, -1), args
    for args in ((1, 1, 100, 65, 510), (1, 1, 100, 65, 1028), (1, 1, 1025, 65, 512), (1, 1, 100, 1026, 512),
                 (65536, 1, 100, 65, 512), (1, 1 << 31, 100, 65, 512)):
        assert route(lib, *args) == (ERANGE, -1), args
    assert lib.ddsp_hip_synth_frames_route(1, 512, 100, 65, 512, 0, None) == EINVAL
    # the answer is the envelope's: every shape ddsp_hip_synth_frames_supported takes has a route
    for NB, bs in ((65, 512), (2, 4), (1025, 1024)):
        assert lib.ddsp_hip_synth_frames_supported(1, 100, NB, bs) == 1
        assert route(lib, 1, 1, 100, NB, bs)[0] == 0
