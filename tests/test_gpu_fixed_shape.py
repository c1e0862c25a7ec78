"""The fixed-shape fused synthesis kernel (synth_frame.hip FixedShape: 65 bands, block 512) against the any-shape
code, bit for bit.  A launch of 512 frames at that shape takes the fixed form, one of 511 frames the SPLIT form,
which is any-shape, and a frame's bits do not depend on the launch shape (test_gpu_shared_reduction.py relies
on the same), so the first 511 frames of the two launches must be equal: signal, both parts and the controls,
with injected and with device noise (item 0 of both launches draws the same Philox counters), on every
oscillator branch.  Every output buffer starts as NaN, so a sample the kernel did not write shows.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import numpy_oracle as no

pytestmark = pytest.mark.gpu

SR, NB, BS, F = 48000, 65, 512, 512
ANY, SPLIT, FIXED = 0, 1, 2        # enum ddsp_hip_synth_route
SHARED_REV_LIMIT = 8.0             # kSharedRevLimit
FAST_ARG_LIMIT = 8.0e6             # kFastArgLimit
SECTIONS = (200, 350)              # frames [0, 200) below the shared-count guard, [200, 350) above it, then hot


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from ddsp_pytorch_amd import _lib
    _lib.load()
    return _lib


def route(lib, frames, H, prefix=0):
    r = ctypes.c_int(-1)
    assert lib.load().ddsp_hip_synth_frames_route(1, frames, H, NB, BS, prefix, ctypes.byref(r)) == 0
    return r.value


def make_case(H, seed):
    """One item of 512 frames whose f0 rows walk the oscillator's three branches, chosen from the guards
    themselves: below the shared-count guard's edge pitch (0.5 + 2 H4 f0 / sr = 8: 1800 Hz at H = 100), above it
    while |omega| H4 is still below kFastArgLimit, then so high that |omega| H4 passes the limit within about 50
    frames (2.4e6 / H4 Hz), after which every frame is on the general loop."""
    rng = np.random.default_rng(seed)
    H4 = (H + 3) & ~3
    edge = (SHARED_REV_LIMIT - 0.5) * SR / (2.0 * H4)
    a, b = SECTIONS
    f0 = np.empty((1, F, 1), np.float32)
    f0[0, :a, 0] = 50.0 * (0.9 * edge / 50.0) ** rng.random(a)
    f0[0, a:b, 0] = edge * (1.05 + 0.95 * rng.random(b - a))
    f0[0, b:, 0] = max(2.0 * edge, 2.4e6 / H4) * (1.0 + rng.random(F - b))
    return {"f0": f0, "param": rng.standard_normal((1, F, H + 1)).astype(np.float32),
            "mags": rng.standard_normal((1, F, NB)).astype(np.float32),
            "noise": (rng.random((1, F, BS)) * 2 - 1).astype(np.float32)}


def branches(f0, H):
    """per frame: 0 shared count, 1 one count per sample, 2 general loop, -1 a frame the limit crosses or nears"""
    H4 = (H + 3) & ~3
    inc = no.phase_increment(f0[0, :, 0].astype(np.float32), SR).astype(np.float64)
    bound = 0.5 + 2.0 * H4 * np.abs(inc) / (2.0 * np.pi)
    start = np.concatenate([[0.0], np.cumsum(inc * BS)[:-1]])
    end = start + inc * BS
    br = np.full(F, -1)
    fast = end * H4 < 0.99 * FAST_ARG_LIMIT
    br[fast & (bound < 0.99 * SHARED_REV_LIMIT)] = 0
    br[fast & (bound > 1.01 * SHARED_REV_LIMIT)] = 1
    br[start * H4 > 1.01 * FAST_ARG_LIMIT] = 2
    return br


def launch(lib, inp, frames, device_noise, controls, prefix=False):
    """ddsp_hip_synth_frames_controls_prefix on the first `frames` frames into NaN-filled buffers"""
    dev = torch.device("cuda")
    H = inp["param"].shape[-1] - 1
    f0, param, mags, noise = (torch.as_tensor(inp[k][:, :frames]).contiguous().to(dev)
                              for k in ("f0", "param", "mags", "noise"))
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    out, harm, nz = nan(frames * BS), nan(frames * BS), nan(frames * BS)
    ctrl = nan(frames * (1 + H + NB)) if controls else None
    pre = None
    if prefix:
        pre = torch.full((frames,), float("nan"), dtype=torch.float64, device=dev)
        lib.call("frame_phase_prefix", lib.ptr(f0), 1, frames, BS, float(SR), lib.ptr(pre), lib.stream_of(out))
    lib.call("synth_frames_controls_prefix", lib.ptr(f0), lib.ptr(param), H + 1, lib.ptr(mags), NB, -5.0,
             lib.ptr(None if device_noise else noise), 1234, 77, lib.ptr(out), lib.ptr(harm), lib.ptr(nz),
             lib.ptr(ctrl), lib.ptr(pre), 1, frames, H, NB, BS, float(SR), lib.stream_of(out))
    torch.cuda.synchronize()
    res = {"signal": out, "harmonic": harm, "noise": nz}
    if controls:
        res.update(amplitudes=ctrl[:frames], harmonic_distribution=ctrl[frames:frames * (1 + H)].view(frames, H),
                   magnitudes=ctrl[frames * (1 + H):].view(frames, NB))
    return res


def assert_same_frames(a, b, frames, what):
    """the first `frames` frames of two launches' outputs (every output is frame-major)"""
    assert a.keys() == b.keys()
    for k in a:
        per = BS if k in ("signal", "harmonic", "noise") else a[k].numel() // a["amplitudes"].numel()
        x, y = a[k].reshape(-1)[:frames * per], b[k].reshape(-1)[:frames * per]
        assert x.numel() == frames * per == y.numel()
        assert not torch.isnan(x).any() and not torch.isnan(y).any(), (what, k)
        assert torch.equal(x, y), (what, k, int((x != y).sum()))


@pytest.mark.parametrize("device_noise", [False, True], ids=["inject", "philox"])
@pytest.mark.parametrize("H", [100, 7, 128])
def test_fixed_form_equals_any_shape_form(lib, H, device_noise):
    inp = make_case(H, seed=60 + H)
    assert route(lib, F, H) == FIXED and route(lib, F - 1, H) == SPLIT
    br = branches(inp["f0"], H)[:F - 1]
    counts = [int((br == i).sum()) for i in range(3)]
    print(f"H={H}: frames on the shared-count / per-sample / general loop: {counts}")
    assert min(counts) >= 50, counts
    for controls in (False, True):
        fixed = launch(lib, inp, F, device_noise, controls)
        anyshape = launch(lib, inp, F - 1, device_noise, controls)
        assert not any(torch.isnan(v).any() for v in fixed.values())   # frame 511 too
        assert_same_frames(fixed, anyshape, F - 1, (H, device_noise, controls))


@pytest.mark.parametrize("device_noise", [False, True], ids=["inject", "philox"])
def test_fixed_prefix_form_equals_fixed_form(lib, device_noise):
    """The PREFIX instantiation reads the frame's phase prefix, the other sums it: the same bits while every
    partial sum is exact in fp64 (test_gpu_long_render.py's condition).  Here the increments span 50 Hz to 48 kHz,
    10 bits, beside 24 significant bits and 18 bits of frames * block_size: 52 <= 53."""
    H = 100
    inp = make_case(H, seed=71)
    assert inp["f0"].min() >= 50.0 and inp["f0"].max() <= 50.0 * 2 ** 10
    assert route(lib, F, H, prefix=1) == FIXED and route(lib, F, H) == FIXED
    for controls in (False, True):
        a = launch(lib, inp, F, device_noise, controls, prefix=True)
        b = launch(lib, inp, F, device_noise, controls)
        assert_same_frames(a, b, F, (device_noise, controls))
