"""ddsp_hip_dense_rows' widened envelope on gfx950 (csrc/dense.hip): K up to 1536 (the 24-chunk instantiation: the
z-conditioned decoder's GRU input projection, three LayerNorm + LeakyReLU segments of 512), a LayerNorm segment
without the activation (the MFCC encoder's ``norm``), three problems per launch.

The accuracy gate is the project's: the GPU's error against torch in fp64 on the CPU is at most 4 x
the error of the same computation by torch in fp32 on the CPU, in RMS and in maximum; every figure is printed
before it is asserted (pytest -s; DESIGN.md 3f-aligned records the measured ratios)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def core():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ddsp_pytorch_amd
    ddsp_pytorch_amd._lib.load()
    return ddsp_pytorch_amd.core


def gate(tag, got, ref64, ref32):
    eg, e32 = got.double().cpu() - ref64, ref32.double() - ref64
    rms = lambda e: float(e.pow(2).mean().sqrt())
    r_rms, r_max = rms(eg) / rms(e32), float(eg.abs().max()) / float(e32.abs().max())
    print(f"{tag}: rms gpu {rms(eg):.3e} fp32 {rms(e32):.3e} ratio {r_rms:.2f}; max gpu {float(eg.abs().max()):.3e} "
          f"fp32 {float(e32.abs().max()):.3e} ratio {r_max:.2f}")
    assert rms(e32) > 0 and r_rms <= 4.0 and r_max <= 4.0, tag


def reference(xs, norms, lin, act, dtype):
    """Linear(concat_s [LeakyReLU](LayerNorm(x_s))) by torch on the CPU in ``dtype``."""
    segs = []
    for x, ln in zip(xs, norms):
        h = F.layer_norm(x.to(dtype), (x.shape[-1],), ln.weight.detach().to(dtype), ln.bias.detach().to(dtype), 1e-5)
        segs.append(F.leaky_relu(h, 0.01) if act else h)
    return F.linear(torch.cat(segs, -1), lin.weight.detach().to(dtype), lin.bias.detach().to(dtype))


def make(widths, out, rows, seed):
    torch.manual_seed(seed)
    norms = [torch.nn.LayerNorm(w) for w in widths]
    for ln in norms:
        with torch.no_grad():
            ln.weight.normal_(1.0, 0.2)
            ln.bias.normal_(0.0, 0.2)
    lin = torch.nn.Linear(sum(widths), out)
    xs = [torch.randn(rows, w) * 2.0 + 0.5 for w in widths]
    return xs, norms, lin


def run(core, xs, norms, lin, act, rows):
    dev = torch.device("cuda")
    gn, gl = [ln.to(dev) for ln in norms], lin.to(dev)
    gx = [x.to(dev) for x in xs]
    y = torch.full((rows, lin.out_features), float("nan"), device=dev)
    core.dense_rows([([core.dense_input(x, norm=ln, activation=act) for x, ln in zip(gx, gn)], gl, y)], rows, dev)
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("rows", [1, 8])
def test_k_1536(core, rows):
    import copy
    xs, norms, lin = make([512, 512, 512], 1536, rows, seed=rows)
    ref64, ref32 = (reference(xs, norms, lin, True, dt) for dt in (torch.float64, torch.float32))
    y = run(core, xs, copy.deepcopy(norms), copy.deepcopy(lin), True, rows)
    assert y.shape == (rows, 1536) and bool(torch.isfinite(y).all())
    gate(f"dense_rows K 1536 rows {rows}", y, ref64, ref32)


@pytest.mark.parametrize("rows", [1, 8])
def test_plain_norm_segment(core, rows):
    import copy
    xs, norms, lin = make([30], 192, rows, seed=10 + rows)
    ref64, ref32 = (reference(xs, norms, lin, False, dt) for dt in (torch.float64, torch.float32))
    y = run(core, xs, copy.deepcopy(norms), copy.deepcopy(lin), False, rows)
    gate(f"dense_rows LayerNorm(30) without activation rows {rows}", y, ref64, ref32)
    # the flag is what makes the difference: with the activation the values differ wherever the norm is negative
    y_act = run(core, xs, copy.deepcopy(norms), copy.deepcopy(lin), True, rows)
    assert not torch.equal(y, y_act)
    with pytest.raises(RuntimeError, match="goes with a norm"):
        core.dense_input(xs[0].cuda(), activation=False)


def test_three_problems_in_one_launch(core):
    """f0_mlp's, loudness_mlp's and z_mlp's second blocks side by side equal the same three one per launch; a wide
    problem beside narrow ones runs all three on the 24-chunk code and still gives each alone's bits."""
    dev, rows = torch.device("cuda"), 4
    for widths in ([[64], [64], [64]], [[512, 512, 512], [30], [64, 64]]):
        probs = []
        for i, ws in enumerate(widths):
            xs, norms, lin = make(ws, 200 + 8 * i + 3, rows, seed=20 + i)
            probs.append(([x.to(dev) for x in xs], [ln.to(dev) for ln in norms], lin.to(dev)))

        def problem(p, y):
            return ([core.dense_input(x, norm=ln) for x, ln in zip(p[0], p[1])], p[2], y)

        together = [torch.full((rows, p[2].out_features), float("nan"), device=dev) for p in probs]
        core.dense_rows([problem(p, y) for p, y in zip(probs, together)], rows, dev)
        for p, y in zip(probs, together):
            # (a narrow problem beside a wide one runs the 24-chunk code, alone the 17-chunk code: the same fma
            # chain per lane over the chunks that exist)
            alone = torch.full_like(y, float("nan"))
            core.dense_rows([problem(p, alone)], rows, dev)
            assert bool(torch.isfinite(y).all()) and torch.equal(y, alone)
    with pytest.raises(RuntimeError, match="1 to 3 problems"):
        core.dense_rows([problem(probs[0], together[0])] * 4, rows, dev)
    with pytest.raises(RuntimeError):  # K = 1537
        xs, norms, lin = make([512, 512, 513], 8, rows, seed=3)
        core.dense_rows([([core.dense_input(x.to(dev)) for x in xs], lin.to(dev),
                          torch.empty(rows, 8, device=dev))], rows, dev)
