"""Multiscale STFT magnitudes and the training loss on gfx950 kernels,
against torch.stft on the CPU (the reference's own call, ddsp/core.py:27-41) and the reference's
golden loss and gradient (g7, tests/golden/make_goldens.py).

Tolerances: spectrogram relative L2 error <= 1e-5 (fp32 FFTs of different structure);
gradient of sum(M * W) <= 2e-5; the loss value <= 1e-5; the loss gradient <= 1e-3 on the golden's
small case and <= 1e-4 for the squared linear-magnitude form at config 2's length (see the last test
for why the L1 / log form's gradient is not a well-conditioned comparison there).
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import torch_ref as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ddsp_pytorch_amd
    ddsp_pytorch_amd._lib.load()
    return ddsp_pytorch_amd


def relerr(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def ref_stft(x, n, hop):
    return torch.stft(x, n, hop, n, torch.hann_window(n), True, normalized=True, return_complex=True).abs()


@pytest.mark.parametrize("n", [16, 32, 64, 128, 256, 512, 1024, 2048, 4096])
@pytest.mark.parametrize("T,hop_div", [(10000, 4), (9001, 4), (5000, 2), (4097, 8)])
def test_stft_magnitude(dd, n, T, hop_div):
    if n // 2 >= T:
        pytest.skip("reflect padding needs T > n/2")
    hop = max(1, n // hop_div)
    x = torch.randn(3, T, generator=torch.Generator().manual_seed(n + T)) * 0.3
    ref = ref_stft(x, n, hop)
    got = dd.core.stft_magnitude(x.cuda(), n, hop)
    assert got.shape == ref.shape
    assert relerr(got, ref) < 1e-5, relerr(got, ref)


@pytest.mark.parametrize("n,T", [(16, 12000), (32, 12000), (64, 12000), (128, 12000), (256, 12000), (512, 12000),
                                 (1024, 12000), (2048, 12000), (4096, 12000), (128, 102400), (4096, 102400)])
def test_stft_magnitude_grad(dd, n, T):
    hop = n // 4
    g = torch.Generator().manual_seed(n)
    x = torch.randn(2, T, generator=g) * 0.3
    ref_m = ref_stft(x, n, hop)
    W = torch.randn(ref_m.shape, generator=g)
    xc = x.clone().requires_grad_(True)
    (ref_stft(xc, n, hop) * W).sum().backward()
    xg = x.cuda().requires_grad_(True)
    (dd.core.stft_magnitude(xg, n, hop) * W.cuda()).sum().backward()
    assert relerr(xg.grad, xc.grad) < 2e-5, relerr(xg.grad, xc.grad)


def test_spectral_loss_golden(dd):
    g = load_golden("g7_stft_loss")
    scales, overlap = [int(s) for s in g["scales"]], float(g["overlap"])
    from ddsp_pytorch_amd import loss as L
    rec = torch.as_tensor(g["rec"]).cuda().requires_grad_(True)
    sig = torch.as_tensor(g["sig"]).cuda()
    rs = dd.core.multiscale_fft(rec, scales, overlap)
    for s, m in zip(scales, rs):
        assert relerr(m, g[f"stft_{s}"]) < 1e-5, (s, relerr(m, g[f"stft_{s}"]))
    val = L.multiscale_spec_loss(dd.core.multiscale_fft(sig, scales, overlap), rs)
    assert relerr(val, g["loss"]) < 1e-5, (float(val), float(g["loss"]))
    val.backward()
    # the golden gradient itself is 3.5e-4 from the fp64 gradient of the same loss (ill-conditioned
    # log-term weights of the smallest bins); the 1e-5 comparison on the well-conditioned bins is
    # test_spectral_loss_grad_well_conditioned_bins
    assert relerr(rec.grad, g["grad_rec"]) < 1e-3, relerr(rec.grad, g["grad_rec"])


def test_spectral_loss_config2_size(dd):
    """config 2's signal length (T = 102400) and batch 4, against the oracle on the CPU.

    The loss value is compared directly.  Its gradient is compared on the linear-magnitude part
    in squared form: train.py's L1 terms take sign(|X| - |Y|), decided by transform round-off for
    bins whose magnitudes agree to fp32 precision, and its log terms weight each bin by
    1/(|X| + 1e-7), so the few smallest of ~10^6 bins per scale dominate that gradient and carry
    the fp32 transform's relative error of those tiny magnitudes (two correct fp32 transforms
    differ there by several percent of the gradient norm).  Both are conditioning of the loss,
    not of the kernels, whose vector-Jacobian product is checked directly in
    test_stft_magnitude_grad (including at this length)."""
    g = torch.Generator().manual_seed(3)
    sig = torch.randn(4, 102400, generator=g) * 0.3
    rec = sig + 0.05 * torch.randn(4, 102400, generator=g)
    scales = [4096, 2048, 1024, 512, 256, 128]
    from ddsp_pytorch_amd import loss as L
    lc = tr.multiscale_spec_loss(tr.multiscale_fft(sig, scales, 0.75), tr.multiscale_fft(rec, scales, 0.75))
    lg = L.spectral_loss(sig.cuda(), rec.cuda())
    assert relerr(lg, lc) < 1e-5

    def lin_sq(ori, rs):
        out = 0
        for s_x, s_y in zip(ori, rs):
            out = out + ((s_x - s_y) ** 2).mean()
        return out

    rc = rec.clone().requires_grad_(True)
    lin_sq(tr.multiscale_fft(sig, scales, 0.75), tr.multiscale_fft(rc, scales, 0.75)).backward()
    rg = rec.cuda().requires_grad_(True)
    lin_sq(dd.core.multiscale_fft(sig.cuda(), scales, 0.75), dd.core.multiscale_fft(rg, scales, 0.75)).backward()
    assert relerr(rg.grad, rc.grad) < 1e-4, relerr(rg.grad, rc.grad)


def test_fused_spectral_loss_matches_unfused(dd):
    """ddsp_hip_spectral_loss (one fused pass per scale) against the spectrogram route on the same
    kernels: same loss, and the same gradient up to the sign-flip ambiguity of the L1 terms
    (checked on the golden's small case, where no bin pair is within rounding)."""
    from ddsp_pytorch_amd import loss as L
    g = load_golden("g7_stft_loss")
    scales, overlap = [int(s) for s in g["scales"]], float(g["overlap"])
    sig = torch.as_tensor(g["sig"]).cuda()
    rec = torch.as_tensor(g["rec"]).cuda().requires_grad_(True)
    lf = L.spectral_loss(sig, rec, scales, overlap)
    lf.backward()
    assert relerr(lf, g["loss"]) < 1e-5, (float(lf), float(g["loss"]))
    assert relerr(rec.grad, g["grad_rec"]) < 1e-3, relerr(rec.grad, g["grad_rec"])
    with torch.no_grad():
        l0 = L.spectral_loss(sig, rec.detach(), scales, overlap)
    assert torch.equal(l0, lf.detach())
    # config 2's length: the loss value against the oracle
    gg = torch.Generator().manual_seed(3)
    s2 = torch.randn(4, 102400, generator=gg) * 0.3
    r2 = s2 + 0.05 * torch.randn(4, 102400, generator=gg)
    lc = tr.multiscale_spec_loss(tr.multiscale_fft(s2, scales, 0.75), tr.multiscale_fft(r2, scales, 0.75))
    assert relerr(L.spectral_loss(s2.cuda(), r2.cuda()), lc) < 1e-5


def test_fused_spectral_loss_small_scales(dd):
    """The fused loss at the transform sizes below 128 (one radix-16 pass alone, then a radix-2 and a radix-4
    tail), an odd length and an odd frame count: the value against the oracle on the CPU, bit-equal with and
    without a gradient, and the gradient against the spectrogram route on the same kernels."""
    from ddsp_pytorch_amd import loss as L
    scales, overlap = [64, 32, 16], 0.75
    g = torch.Generator().manual_seed(3)
    sig = torch.randn(2, 3001, generator=g) * 0.3
    rec = sig + 0.05 * torch.randn(2, 3001, generator=g)
    lc = tr.multiscale_spec_loss(tr.multiscale_fft(sig, scales, overlap), tr.multiscale_fft(rec, scales, overlap))
    rf = rec.cuda().requires_grad_(True)
    lf = L.spectral_loss(sig.cuda(), rf, scales, overlap)
    lf.backward()
    ru = rec.cuda().requires_grad_(True)
    L.multiscale_spec_loss(dd.core.multiscale_fft(sig.cuda(), scales, overlap),
                           dd.core.multiscale_fft(ru, scales, overlap)).backward()
    print("small scales: value", relerr(lf, lc), "gradient", relerr(rf.grad, ru.grad))
    assert relerr(lf, lc) < 1e-5, (float(lf), float(lc))
    with torch.no_grad():
        l0 = L.spectral_loss(sig.cuda(), rec.cuda(), scales, overlap)
    assert torch.equal(l0, lf.detach())
    assert relerr(rf.grad, ru.grad) < 1e-3, relerr(rf.grad, ru.grad)


def test_spectral_loss_grad_well_conditioned_bins(dd):
    """Golden g7's gradient at 1e-5 on the bins where it is defined to that precision.

    train.py's log-L1 term weights each bin by 1/(|Y| + 1e-7), so the loss gradient is dominated
    by the few smallest magnitudes, whose fp32 transform round-off is of their own size: the
    reference's own fp32 gradient (the golden) is 3.5e-4 (relative L2) from the same loss evaluated
    in fp64, and no sign of an L1 term is a tie on g7 (tools/exp_loss_grad.py).  Masking the bins
    with |X| or |Y| below 1 % of the spectrogram's RMS (0.14 % of all bins, mask taken from the
    fp64 magnitudes) makes the reference's fp32 gradient agree with fp64 to 2.7e-6; on the
    remaining bins the kernels' gradient must match the reference's at 1e-5.  The fused loss
    (no mask input) is held to the reference's own accuracy against the fp64 gradient."""
    from ddsp_pytorch_amd import loss as L
    g = load_golden("g7_stft_loss")
    scales, ov = [int(s) for s in g["scales"]], float(g["overlap"])
    sig32, rec32 = torch.as_tensor(g["sig"]), torch.as_tensor(g["rec"])
    ori64 = tr.multiscale_fft(sig32.double(), scales, ov)
    my64 = tr.multiscale_fft(rec32.double(), scales, ov)
    masks = []
    for mx, my in zip(ori64, my64):
        floor = 1e-2 * float(my.pow(2).mean().sqrt())
        masks.append(((my > floor) & (mx > floor)).float())

    def masked_loss(ori, rec_stft, log):
        lo = 0
        for m, mx, my in zip(masks, ori, rec_stft):
            m = m.to(my)
            lo = lo + (m * (mx - my).abs()).mean() + (m * (log(mx) - log(my)).abs()).mean()
        return lo

    def oracle_grad(dtype):
        rc = rec32.to(dtype).clone().requires_grad_(True)
        masked_loss(tr.multiscale_fft(sig32.to(dtype), scales, ov), tr.multiscale_fft(rc, scales, ov),
                    tr.safe_log).backward()
        return rc.grad
    ref32, ref64 = oracle_grad(torch.float32), oracle_grad(torch.float64)
    assert relerr(ref32, ref64) < 5e-6  # the reference's fp32 gradient is well conditioned here
    rg = rec32.cuda().requires_grad_(True)
    masked_loss(dd.core.multiscale_fft(sig32.cuda(), scales, ov), dd.core.multiscale_fft(rg, scales, ov),
                dd.core.safe_log).backward()
    assert relerr(rg.grad, ref32) < 1e-5, relerr(rg.grad, ref32)
    # ... and against the reference itself: golden g7b is this masked loss's gradient computed by the
    # reference's multiscale_fft / safe_log (tests/golden/make_goldens.py masked_loss_golden), its masks
    # stored with it
    g7b = load_golden("g7b_stft_loss_masked")
    for s_, m in zip(scales, masks):
        assert torch.equal(torch.as_tensor(g7b[f"mask_{s_}"]).float(), m), s_
    assert relerr(rg.grad, g7b["grad_rec"]) < 1e-5, relerr(rg.grad, g7b["grad_rec"])
    # unmasked: the fused kernel's gradient is as close to the fp64 gradient as the reference's own
    rc64 = rec32.double().clone().requires_grad_(True)
    tr.multiscale_spec_loss(tr.multiscale_fft(sig32.double(), scales, ov), tr.multiscale_fft(rc64, scales, ov)).backward()
    golden_err = relerr(g["grad_rec"], rc64.grad)
    rf = rec32.cuda().requires_grad_(True)
    L.spectral_loss(sig32.cuda(), rf, scales, ov).backward()
    assert relerr(rf.grad, rc64.grad) < 2.0 * golden_err, (relerr(rf.grad, rc64.grad), golden_err)
