"""The synthesis VJP kernels (csrc/backward.hip: harmonic_vjp_kernel, noise_vjp_kernel, noise_vjp_wave_kernel) at every
branch their shape arithmetic takes, against the high-precision references of tests/vjp_ref.py, checked PER FRAME:
max over (b, f) of ||got - ref||_2 / ||ref||_2 <= GRAD_REL (1e-5, the project's gradient tolerance), and the
whole-tensor relative L2 as well.  One wrong frame among hundreds, or one wrong band of one frame (a partly empty
last workgroup, the Nyquist band, the DC band's factor, the last lag segment), passes a whole-tensor check; it does
not pass this one.  The scalar grad_amplitudes of HMODE 1 is a signed sum: |got - ref| is measured against the
sum's condition scale sum_k |dA_k u_k| from the fp64 reference.  tests/test_vjp_ref.py shows that the reference's
own fp32 autograd meets GRAD_REL / 2 per frame on every case's inputs, so the bound is a fair one in every frame.

The kernels are called directly (grad.params_backward, grad.noise_backward, ddsp_hip_harmonic_synth_frames_backward
as SynthFramesHarmonicFn.backward calls it), so the forward kernels' envelopes do not limit the shapes; cases 2, a
and c run through the public autograd route too.  Sample rate 48000, f0 = 50 * 20**U per frame, upstream randn.

Harmonic part, (B, F, H, bs), harmonic_vjp_kernel<true> (raw param, "HMODE 2" below) and <false> (frame controls,
"HMODE 1").  harmonic_backward_shape (csrc/harmonic_frame.h) works
from kq = ceil(H/4), ns = clamp(min(128/kq, bs), 1, 64), nt = min(512, roundup64(kq ns)), SL = ((bs+ns-1)/ns+1)&~1.
Per frame the kernel takes its padded hardware-sine loop when H bs inc >= 16 rad and max |omega| H < 8e6 (`fast_s`),
else the general loop (polynomial sine, sin_slow past 8e6): "fast" / "general" below says which one the case's
pitches give:
   1  (1, 3, 1, 64)      kq = 1, ns = 64, nt = 64, SL = 2; general (its fast twin is case 11)
   2  (2, 5, 17, 441)    odd bs, ns = 25, SL = 18, padded WGN = 450, H % 4 = 1 (the 4 kq + c < H tail); fast
   3  (1, 2, 5, 3)       bs < 128/kq: ns = 3, segments that are all padding; general
   4  (1, 4, 3, 1)       bs = 1; general
   5  (1, 3, 1024, 64)   kq = 256 > 128: ns = 1, nt = 256; fast
   6  (1, 2, 2052, 16)   kq = 513 > nt = 512: the item loop wraps, with a one-item tail; fast
   7  (1, 2, 4096, 8)    the envelope's cap, two full passes; fast
   8  (1, 600, 8, 4)     nt = 64: the strided fp64 phase-prefix sum over 600 frames (> FRAME_PREFIX_MIN_FRAMES);
                         general: 32 sines per frame, whose gradient cancels to a few percent of its terms in some
                         frames (the case that moved such frames off the hardware sine: 1.1e-5 with it)
   9  (1, 8, 1024, 512)  HMODE 1, f0 alternating 21 / 23 kHz: frames 0-4 on the fast sine, 5-7 on sin_slow
                         (max |omega| H = 1.2e7 > 8e6), in one launch
  10  (2, 6, 8, 64)      HMODE 2, f0 = 0 in frames 0-1 and 4, 30 kHz in frame 3 (every harmonic masked): frames with
                         an exactly zero reference gradient come back exactly zero; both loops
  11  (1, 3, 1, 64)      case 1's shape at f0 = 2000 * 10**U: the fast loop with SL = 2 and its segments s >= 32 all
                         padding

Noise part, (B, F, bs, NB), n = 2 (NB - 1) taps, raw_bias = -5.0 (RAW) and None, injected noise:
   a  (2, 3, 441, 18)    per-tap path (n/2 = 17), odd bs, modular cosine transform (n = 34)
   b  (2, 3, 441, 17)    n = 32 qualifies for `quads`, bs % 4 != 0 does not: per-tap path
   c  (1, 3, 64, 65)     n > bs: cropped taps, NSEG = 2
   d  (1, 2, 7, 9)       n > 2 bs: the tap index wraps, NSEG = 8 > bs
   e  (2, 3, 100, 21)    quads with n = 40 (modular transform), 16 segments of 8 lags, the last ones empty
   f  (2, 5, 64, 33)     quads with n == bs
   g  (1, 3, 8, 2)       NB = 2: empty cosine loop, DC and Nyquist bands only
   h  (1, 2, 1024, 513)  nqh = 128: NSEG = 1, 256 items on 128 threads
   i  (1, 2, 512, 129)   NSEG = 3, seglen = 172
   j  (1, 5, 512, 65)    upstream gradient 4 bytes into its buffer: the generic kernel at the reference's shape
                         (NSEG = 7); the aligned run of the same values takes the wave kernel
   k  (1, 5, 640, 65), (2, 3, 1024, 65)   wave kernel, Philox noise (seed 77, offset 2^32 + 5)
   l  (2, 3, 441, 18), (1, 3, 30, 33)     generic kernel, Philox noise at bs % 4 != 0, same seed and offset
   m  (1, 2, 8, 65)      n = 128 > 9 bs + 8: the cosine transform's n partial sums need more than the NSEG * bs = 64
                         floats of the correlation's partials (they used to run past the workgroup's LDS)

Largest per-frame error measured on an MI355X (a record; the assertion is GRAD_REL), beside the fp32 oracle's on the
CPU (tests/test_vjp_ref.py):
  harmonic, HMODE 2 (cases 1-8, 10, 11):  device 3.9e-6 (case 8; 1.1e-6 elsewhere)   oracle 1.8e-6 (case 8)
  harmonic, HMODE 1 (cases 1-9, 11):      device 2.5e-6 (case 8; 4.9e-7 elsewhere)   oracle 1.8e-6 (case 8)
                                          amplitude against its scale: device 1.6e-6, oracle 7.2e-7
  noise (a-m, both biases):               device 1.1e-6                              oracle 1.6e-6
"""
import math

import pytest
import torch

import vjp_ref as vr

pytestmark = pytest.mark.gpu

GRAD_REL = vr.GRAD_REL
EINVAL, ERANGE = 1, 5  # DDSP_HIP_EINVAL, DDSP_HIP_ERANGE (include/ddsp_hip.h)


@pytest.fixture(scope="module")
def dd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ddsp_pytorch_amd
    ddsp_pytorch_amd._lib.load()
    return ddsp_pytorch_amd


def poison(*shapes):
    """The kernels write into torch.empty buffers: leave NaNs in the allocator's free blocks of these sizes, so
    that a band or a frame the kernel skips does not come back holding an earlier run's correct value."""
    for s in shapes:
        torch.full(s, math.nan, dtype=torch.float32, device="cuda")


def check(got, ref, what):
    e, w = vr.max_frame_relerr(got, ref), vr.relerr(got, ref)
    print(f"{what}: per frame {e:.2e}, whole {w:.2e}")
    assert e <= GRAD_REL, (what, e)
    assert w <= GRAD_REL, (what, w)


# ------------------------------------------------------------------------------------------ harmonic part
def params_backward(dd, c):
    poison(c["param"].shape)
    return dd.grad.params_backward(c["f0"].cuda(), c["param"].cuda(), c["g"].cuda(), c["bs"], vr.SR)


def frames_backward(dd, c):
    """ddsp_hip_harmonic_synth_frames_backward as grad.SynthFramesHarmonicFn.backward calls it"""
    from ddsp_pytorch_amd import _lib
    B, F, H = c["dist"].shape
    f0, amp, dist, g = (c[k].cuda().contiguous() for k in ("f0", "amp", "dist", "g"))
    da = torch.full((B, F, 1), math.nan, dtype=torch.float32, device="cuda")
    du = torch.full((B, F, H), math.nan, dtype=torch.float32, device="cuda")
    _lib.call("harmonic_synth_frames_backward", _lib.ptr(f0), _lib.ptr(amp), _lib.ptr(dist), _lib.ptr(g),
              _lib.ptr(da), _lib.ptr(du), B, F, H, c["bs"], float(vr.SR), _lib.stream_of(g))
    return da, du


def check_frames(dd, case):
    c = vr.harmonic_case(case)
    da, du = frames_backward(dd, c)
    check(du, c["grad_dist"], f"harmonic case {case} HMODE 1 distribution")
    ea = vr.scaled_err(da, c["grad_amp"], c["amp_scale"])
    print(f"harmonic case {case} HMODE 1 amplitude vs its condition scale: {float(ea.max()):.2e}")
    assert float(ea.max()) <= GRAD_REL, (case, float(ea.max()))
    # whole tensor: the error's norm against the scale's
    assert float((da.double().cpu() - c["grad_amp"]).norm() / c["amp_scale"].norm()) <= GRAD_REL


@pytest.mark.parametrize("case", sorted(vr.HARMONIC_CASES))
def test_harmonic_params_vjp(dd, case):
    c = vr.harmonic_case(case)
    check(params_backward(dd, c), c["grad_param"], f"harmonic case {case} HMODE 2")


@pytest.mark.parametrize("case", sorted(vr.HARMONIC_CASES))
def test_harmonic_frames_vjp(dd, case):
    check_frames(dd, case)


def test_harmonic_high_pitch_short_segments(dd):
    """case 11: every frame on the padded hardware-sine loop (H bs inc >= 16 rad)"""
    c = vr.harmonic_case(11)
    inc = 2 * math.pi * c["f0"] / vr.SR
    assert float((c["H"] * c["bs"] * inc).min()) >= 16.0
    check(params_backward(dd, c), c["grad_param"], "harmonic case 11 HMODE 2")
    check_frames(dd, 11)


def test_harmonic_slow_sine_frames(dd):
    """case 9: fast-sine and sin_slow frames in one launch"""
    c = vr.harmonic_case(9)
    _, omega, _ = vr.harmonic_fp32_points(c["f0"], c["H"], c["bs"])
    assert float(omega.abs().max()) * c["H"] > 8e6
    check_frames(dd, 9)


def test_harmonic_masked_and_silent_frames(dd):
    """case 10: exact zeros where the reference's gradient is exactly zero"""
    c = vr.harmonic_case(10)
    got = params_backward(dd, c)
    zero = (c["grad_param"] == 0).all(-1)
    assert zero[:, :2].all() and not zero[:, 2:].any()
    assert (got.cpu()[zero] == 0).all()
    check(got, c["grad_param"], "harmonic case 10 HMODE 2")  # (a zero row that is not zero in got reads inf)


# ------------------------------------------------------------------------------------------ noise part
def noise_backward(dd, c, raw_bias, noise="inject", g=None):
    poison(c["mags"].shape)
    nz = c["noise"].cuda() if noise == "inject" else None
    seed, offset = (0, 0) if noise == "inject" else (vr.PHILOX_SEED, vr.PHILOX_OFFSET)
    g = c["g"].cuda() if g is None else g
    return dd.grad.noise_backward(c["mags"].cuda(), nz, seed, offset, raw_bias, g, c["bs"])


@pytest.mark.parametrize("raw_bias", vr.RAW_BIASES)
@pytest.mark.parametrize("name", [n for n in sorted(vr.NOISE_CASES) if n != "j"])
def test_noise_vjp(dd, name, raw_bias):
    c = vr.noise_case(name)
    check(noise_backward(dd, c, raw_bias), c["ref"][raw_bias], f"noise case {name} bias {raw_bias}")


@pytest.mark.parametrize("raw_bias", vr.RAW_BIASES)
def test_noise_vjp_unaligned_upstream(dd, raw_bias):
    """case j: the same values through the wave kernel (aligned) and the generic kernel (4 bytes off)"""
    c = vr.noise_case("j")
    g = c["g"].cuda()
    assert g.data_ptr() % 16 == 0
    check(noise_backward(dd, c, raw_bias, g=g), c["ref"][raw_bias], f"noise case j aligned bias {raw_bias}")
    buf = torch.zeros(g.numel() + 4, dtype=torch.float32, device="cuda")
    gv = buf[1:1 + g.numel()].view(g.shape)
    gv.copy_(g)
    assert gv.is_contiguous() and gv.data_ptr() % 16 == 4
    check(noise_backward(dd, c, raw_bias, g=gv), c["ref"][raw_bias], f"noise case j unaligned bias {raw_bias}")


@pytest.mark.parametrize("raw_bias", vr.RAW_BIASES)
@pytest.mark.parametrize("name", sorted(vr.PHILOX_CASES))
def test_noise_vjp_philox(dd, name, raw_bias):
    """cases k, l: the kernels regenerate the noise; the reference takes oracle.philox's"""
    c = vr.noise_case(name)
    check(noise_backward(dd, c, raw_bias, noise="philox"), c["ref"][raw_bias], f"noise case {name} bias {raw_bias}")


# ------------------------------------------------------------------------------------------ envelope, routes
def test_envelope_answers(dd):
    """Host-only answers of the launcher (nothing is launched): ERANGE past the envelope, EINVAL for no shape"""
    from ddsp_pytorch_amd import _lib
    allow = (EINVAL, ERANGE)
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")  # noqa: E731
    st = _lib.stream_of(z(1))

    def params(H, bs):
        f0, p, g, dp = z(1, 1, 1), z(1, 1, H + 1), z(1, max(bs, 1), 1), z(1, 1, H + 1)
        return _lib.call("harmonic_synth_params_backward", _lib.ptr(f0), _lib.ptr(p), _lib.ptr(g), _lib.ptr(dp),
                         1, 1, H, bs, float(vr.SR), st, allow=allow)

    def frames(H, bs):
        f0, a, u, g, da, du = z(1, 1, 1), z(1, 1, 1), z(1, 1, H), z(1, max(bs, 1), 1), z(1, 1, 1), z(1, 1, H)
        return _lib.call("harmonic_synth_frames_backward", _lib.ptr(f0), _lib.ptr(a), _lib.ptr(u), _lib.ptr(g),
                         _lib.ptr(da), _lib.ptr(du), 1, 1, H, bs, float(vr.SR), st, allow=allow)

    def noise(NB, bs, raw):
        m, nz, g, dm = z(1, 1, max(NB, 1)), z(1, 1, max(bs, 1)), z(1, max(bs, 1), 1), z(1, 1, max(NB, 1))
        return _lib.call("filtered_noise_backward", _lib.ptr(m), _lib.ptr(nz), 0, 0, raw, -5.0, _lib.ptr(g),
                         _lib.ptr(dm), 1, 1, NB, bs, st, allow=allow)

    for harm in (params, frames):
        assert harm(4097, 64) == ERANGE
        assert harm(8, 8193) == ERANGE
        assert harm(8, 0) == EINVAL
    for raw in (0, 1):
        assert noise(65, 8193, raw) == ERANGE
        assert noise(4098, 64, raw) == ERANGE
        assert noise(1, 64, raw) == EINVAL
        assert noise(65, 0, raw) == EINVAL


def test_public_route_harmonic(dd):
    """case 2 through core.harmonic_synth_params under autograd: the same kernel, outside the fused envelope"""
    c = vr.harmonic_case(2)
    p = c["param"].cuda().requires_grad_(True)
    poison(c["param"].shape)
    (dd.core.harmonic_synth_params(c["f0"].cuda(), p, c["bs"], vr.SR) * c["g"].cuda()).sum().backward()
    check(p.grad, c["grad_param"], "harmonic case 2 through core.harmonic_synth_params")


@pytest.mark.parametrize("raw_bias", vr.RAW_BIASES)
@pytest.mark.parametrize("name", ["a", "c"])
def test_public_route_noise(dd, name, raw_bias):
    """cases a and c through core.filtered_noise under autograd"""
    c = vr.noise_case(name)
    m = c["mags"].cuda().requires_grad_(True)
    poison(c["mags"].shape)
    (dd.core.filtered_noise(m, c["bs"], noise=c["noise"].cuda(), raw_bias=raw_bias) * c["g"].cuda()).sum().backward()
    check(m.grad, c["ref"][raw_bias], f"noise case {name} bias {raw_bias} through core.filtered_noise")
