"""The pitch (f0) gradient of the frame-rate synthesis (csrc/pitch_grad.hip: frame_pitch_grad_kernel and
pitch_grad_scan_kernel) against the closed form of tests/f0_grad_ref.py, through the three public routes that
return it — core.harmonic_synth_params, core.harmonic_synth_frames, core.synth_signal (core.synth_frames inside the
fused envelope, the two module kernels outside it) — with a random upstream gradient.

Bounds, both the project's: the whole-tensor relative L2 error <= GRAD_REL = 1e-5 (tests/test_gpu_grad.py), and PER
FRAME |got - ref| <= 2e-6 (synth_ref.HARM_FRAME_TOL, the forward oscillator's bound for the same kind of sum: H bs
hardware-transcendental terms in fp32 against the sum of their magnitudes) of the frame's condition scale
c (Rbar_f + bs sum_{f'>f} Qbar_{f'}) from the reference.  tests/test_f0_grad_ref.py shows that the reference's own
fp32 autograd uses less than a quarter of either on every case.

Cases (H, bs, B, F, pitch), sample rate 48000.  The frame kernel's geometry is kq = ceil(H/4), ns = clamp(min(128/kq,
bs), 1, 64) sample segments of SL = ((bs+ns-1)/ns+1)&~1 samples, nt = min(512, roundup64(kq ns)) threads:
  c8          (100, 512, 2, 8, low)     the config shape: kq = 25, ns = 5, SL = 104 (8 padded samples)
  m16         (16, 64, 2, 16, low)      mid size
  b4          (8, 4, 3, 7, low)         smallest block; the upstream gradient of the last two frames is zero, so their
                                        scale and gradient are exactly zero
  odd         (5, 12, 2, 9, low)        H not a multiple of 4 (the 4 kq + c < H tail); the sample segments pad
  h1          (1, 4, 1, 64, low)        one harmonic
  high        (100, 64, 2, 16, high)    most harmonics masked
  nyq         (48, 64, 1, 64, nyquist)  products exactly at sr/2; silent frames; a zero-pitch frame after the phase
                                        has moved
  sub         (1024, 64, 1, 8, sub)     H at the fused envelope's cap: kq = 256, ns = 1, nt = 256
  f441        (17, 441, 2, 5, low)      outside the fused envelope (bs % 4): odd bs, padded segments
  f1          (3, 1, 2, 5, low)         outside the fused envelope: bs = 1
  slow        (1024, 441, 1, 13, 20k)   arguments past kFastArgLimit partway: the general loop and the fp64 cosine
  long        (16, 64, 1, 520, low)     F > 512: the frames read the phase-prefix buffer; three scan chunks
  scan_below  (4, 4, 2, chunk - 1, low) the reverse scan one frame below its chunk length ...
  scan_above  (4, 4, 2, chunk + 1, low) ... and one above (a chunk of one frame, then a full one)

Largest errors measured on an MI355X are recorded in DESIGN.md (the pitch gradient's section).
"""
import math

import pytest
import torch

import f0_grad_ref as fr
import vjp_ref as vr
from oracle import torch_ref as tr

pytestmark = pytest.mark.gpu

SR = fr.SR
GRAD_REL, NET_REL = fr.GRAD_REL, 1e-4
NAMES = sorted(fr.CASES)


@pytest.fixture(scope="module")
def dd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ddsp_pytorch_amd
    ddsp_pytorch_amd._lib.load()
    return ddsp_pytorch_amd


def poison(*shapes):
    """The kernels write into torch.empty buffers: leave NaNs in the allocator's free blocks of these sizes, so that
    a frame a kernel skips does not come back holding an earlier run's correct value."""
    for s in shapes:
        torch.full(s, math.nan, dtype=torch.float32, device="cuda")


def check(got, ref, scale, what):
    assert got is not None and got.shape == ref.shape, what
    e, w = float(fr.frame_err(got, ref, scale).max()), vr.relerr(got, ref)
    print(f"{what}: per frame {e:.2e} of the scale, whole {w:.2e}")
    assert e <= fr.FRAME_TOL, (what, e)
    assert w <= GRAD_REL, (what, w)


def cuda_leaf(t):
    return t.cuda().requires_grad_(True)


def route_params(dd, c, f0, param):
    return dd.core.harmonic_synth_params(f0, param, c["bs"], SR)


def route_frames(dd, c, f0, amp, dist):
    return dd.core.harmonic_synth_frames(f0, amp, dist, c["bs"], SR, write_back=False)


def route_signal(dd, c, f0, param, mags):
    return dd.core.synth_signal(f0, param, mags, c["bs"], SR, noise=c["noise"].cuda())


# ------------------------------------------------------------------------------------------ the three routes
@pytest.mark.parametrize("name", NAMES)
def test_params_route(dd, name):
    c = fr.case(name)
    f0 = cuda_leaf(c["f0"])
    poison(c["f0"].shape)
    (route_params(dd, c, f0, c["param"].cuda()) * c["g"].cuda()).sum().backward()
    check(f0.grad, c["grad_params"], c["scale_params"], f"{name} harmonic_synth_params")


@pytest.mark.parametrize("name", NAMES)
def test_frames_route(dd, name):
    c = fr.case(name)
    f0 = cuda_leaf(c["f0"])
    poison(c["f0"].shape)
    (route_frames(dd, c, f0, c["amp"].cuda(), c["dist"].cuda()) * c["g"].cuda()).sum().backward()
    check(f0.grad, c["grad_frames"], c["scale_frames"], f"{name} harmonic_synth_frames")


@pytest.mark.parametrize("name", NAMES)
def test_signal_route(dd, name):
    """core.synth_signal with injected noise: the fused kernel's Function inside its envelope, harmonic_synth_params
    and filtered_noise outside it (f441, f1, slow)"""
    c = fr.case(name)
    fused = dd.core.synth_frames_in_envelope(c["H"], fr.NB, c["bs"], c["B"])
    assert fused == (name not in ("f441", "f1", "slow"))
    f0 = cuda_leaf(c["f0"])
    poison(c["f0"].shape)
    (route_signal(dd, c, f0, c["param"].cuda(), c["mags"].cuda()) * c["g"].cuda()).sum().backward()
    check(f0.grad, c["grad_params"], c["scale_params"], f"{name} synth_signal ({'fused' if fused else 'modules'})")


def test_zero_scale_frames_come_back_zero(dd):
    c = fr.case("b4")
    tail = fr.ZERO_TAIL["b4"]
    assert (c["scale_params"][:, -tail:] == 0).all()
    f0 = cuda_leaf(c["f0"])
    poison(c["f0"].shape)
    (route_params(dd, c, f0, c["param"].cuda()) * c["g"].cuda()).sum().backward()
    assert (f0.grad[:, -tail:] == 0).all() and (f0.grad[:, :-tail] != 0).all()


# ------------------------------------------------------------------------------------------ (a) the other gradients
@pytest.mark.parametrize("name", ["c8", "f441"])
def test_other_gradients_are_unchanged(dd, name):
    """param / mags / amplitude / distribution gradients of a backward that also returns the pitch gradient are bit
    for bit those of the same backward with f0.detach()"""
    c = fr.case(name)
    g = c["g"].cuda()

    def run(route, with_f0, *ops):
        f0 = cuda_leaf(c["f0"])
        leaves = [cuda_leaf(t) for t in ops]
        (route(dd, c, f0 if with_f0 else f0.detach(), *leaves) * g).sum().backward()
        assert (f0.grad is not None) == with_f0
        return [t.grad for t in leaves]

    for route, ops in ((route_params, (c["param"],)), (route_frames, (c["amp"], c["dist"])),
                       (route_signal, (c["param"], c["mags"]))):
        a, b = run(route, True, *ops), run(route, False, *ops)
        for x, y in zip(a, b):
            assert x is not None and torch.equal(x, y), route.__name__


# ------------------------------------------------------------------------------------------ (b) launches
def test_plain_pitch_issues_no_pitch_grad_call(dd, monkeypatch):
    """A pitch that does not require grad costs nothing: no *pitch_grad* entry point is called; one that does calls
    exactly one per backward."""
    from ddsp_pytorch_amd import _lib
    c = fr.case("m16")
    g = c["g"].cuda()
    calls = []
    real = _lib.call

    def spy(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)

    monkeypatch.setattr(_lib, "call", spy)
    for route, ops in ((route_params, (c["param"],)), (route_frames, (c["amp"], c["dist"])),
                       (route_signal, (c["param"], c["mags"]))):
        for with_f0 in (False, True):
            del calls[:]
            f0 = c["f0"].cuda().requires_grad_(with_f0)
            (route(dd, c, f0, *(cuda_leaf(t) for t in ops)) * g).sum().backward()
            n = [x for x in calls if "pitch_grad" in x]
            assert any("backward" in x for x in calls), calls
            assert len(n) == int(with_f0), (route.__name__, with_f0, calls)


# ------------------------------------------------------------------------------------------ (c) composition
def test_synth_path_with_reverb(dd):
    """SynthPath (fused synthesis, then modules.Reverb) with a pitch leaf against the oracle's synth_path_autograd
    on the CPU: the pitch gradient through the reverb's input gradient, and the other leaves beside it"""
    from ddsp_pytorch_amd.synth import SynthPath
    B, F, H, bs, L = 2, 8, 16, 64, 256  # F * bs = 512 >= L
    gen = torch.Generator().manual_seed(31)
    f0 = 50.0 * 20.0 ** torch.rand(B, F, 1, generator=gen)
    param = torch.randn(B, F, H + 1, generator=gen)
    mags = torch.randn(B, F, fr.NB, generator=gen)
    nz = torch.rand(B, F, bs, generator=gen) * 2 - 1
    w = torch.randn(B, F * bs, 1, generator=gen)
    syn = SynthPath(bs, SR, reverb_length=L, noise_mode="inject")
    with torch.no_grad():
        syn.reverb.wet.fill_(0.5)
    rv = tr.Reverb(*(p.detach().clone() for p in (syn.reverb.noise, syn.reverb.decay, syn.reverb.wet)), L, SR)
    fc, pc, mc = (t.clone().requires_grad_(True) for t in (f0, param, mags))
    (tr.synth_path_autograd(fc, pc, mc, nz, rv, bs, SR) * w).sum().backward()
    syn = syn.cuda()
    fg, pg, mg = cuda_leaf(f0), cuda_leaf(param), cuda_leaf(mags)
    out = syn(fg, pg, mg, nz.cuda())
    assert out.requires_grad
    (out * w.cuda()).sum().backward()
    for what, a, b in (("f0", fg, fc), ("param", pg, pc), ("mags", mg, mc)):
        e = vr.relerr(a.grad, b.grad)
        print(f"SynthPath {what} gradient: {e:.2e}")
        assert e <= GRAD_REL, (what, e)
    # inputs that need no gradient: inference, as before, whatever the reverb's parameters say
    assert not syn(f0.cuda(), param.cuda(), mags.cuda(), nz.cuda()).requires_grad


# ------------------------------------------------------------------------------------------ (d) the decoder
def test_decoder_pitch_gradient(dd):
    """DDSPDecoder at a small native size with a pitch leaf: pitch.grad is the control network's share (torch
    autograd) plus the synthesis share, against the oracle's gru_decoder_forward + decoder_synthesis autograd"""
    hidden, H, NBd, bs, B, F = 64, 16, 9, 64, 2, 12
    torch.manual_seed(11)
    m = dd.DDSPDecoder(hidden, H, NBd, SR, bs, False)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    gen = torch.Generator().manual_seed(12)
    f0 = 50.0 * 20.0 ** torch.rand(B, F, 1, generator=gen)
    loud = torch.randn(B, F, 1, generator=gen)
    w = torch.randn(B, F * bs, 1, generator=gen)
    torch.manual_seed(123)
    nz = torch.rand(B, F, bs) * 2 - 1  # what FilteredNoise.draw_noise draws below
    fc = f0.clone().requires_grad_(True)
    hid = tr.gru_decoder_forward(sd, fc, loud)
    sig = tr.decoder_synthesis.__wrapped__(sd, fc, hid, nz, bs, SR)[0]  # (the function under its no_grad)
    (sig * w).sum().backward()
    m = m.cuda()
    pitch = cuda_leaf(f0)
    torch.manual_seed(123)
    out = m({"pitch": pitch, "loudness": loud.cuda()})
    (out["signal"] * w.cuda()).sum().backward()
    e = vr.relerr(pitch.grad, fc.grad)
    print(f"DDSPDecoder pitch gradient: {e:.2e}")
    assert e <= NET_REL, e
    # the synthesis share is not a rounding error of the sum: without it the gradient is far off
    pitch2 = cuda_leaf(f0)
    torch.manual_seed(123)
    hid_g = m.decoder(pitch2, loud.cuda())
    sig2 = m.synthesize(hid_g, pitch2.detach())[0]
    (sig2 * w.cuda()).sum().backward()
    assert vr.relerr(pitch2.grad, fc.grad) > 0.1


# ------------------------------------------------------------------------------------------ (e) graph reuse
@pytest.mark.parametrize("route", ["params", "frames", "signal"])
def test_retain_graph_and_double_backward(dd, route):
    c = fr.case("m16")
    ops = {"params": (route_params, (c["param"],)), "frames": (route_frames, (c["amp"], c["dist"])),
           "signal": (route_signal, (c["param"], c["mags"]))}
    fn, tensors = ops[route]
    f0 = cuda_leaf(c["f0"])
    out = fn(dd, c, f0, *(t.cuda() for t in tensors))
    loss = (out * c["g"].cuda()).sum()
    (g1,) = torch.autograd.grad(loss, f0, retain_graph=True)
    (g2,) = torch.autograd.grad(loss, f0, retain_graph=True)
    assert torch.equal(g1, g2) and float(g1.abs().sum()) > 0
    # first order only: a gradient taken with create_graph=True cannot be back-propagated through
    out = fn(dd, c, f0, *(t.cuda() for t in tensors))
    (g3,) = torch.autograd.grad(out.pow(2).sum(), f0, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g3.pow(2).sum().backward()
