"""The layer between torch's autograd engine and the backward kernels (ddsp_pytorch_amd/grad.py and the
dispatch in decoder.py), in the forms the kernel-level gradient tests never take:

A. partial ``requires_grad`` — frozen leaves, single leaves, single outputs of multi-output Functions;
B. upstream gradients that are not dense, aligned and contiguous — zero-stride (the expanded scalar of
   ``out.sum()``), strided, and 4 bytes off a 16-byte boundary, handed to the outputs directly; and the
   slice losses ``(out[:, 1::2] * w).sum()`` and ``(out[:, 1:] * w).sum()``, which arrive dense;
C. graph reuse — ``backward(retain_graph=True)`` twice, one module applied twice in one graph;
D. double backward is refused (every ``backward`` is ``once_differentiable``);
E. dtypes and autocast under autograd — the fp32 network kernels step aside for torch's modules.

Every reference is torch's own autograd on the CPU (oracle/torch_ref.py, torch.nn.functional), at the bound
the Function already has in the suite: relative L2 error <= 1e-5 for the synthesis path and the GRU
(tests/test_gpu_grad.py GRAD_REL, tests/test_gpu_gru.py), 2e-5 for the STFT magnitude
(tests/test_gpu_stft.py), and for the decoder's network Functions (LinearFn, ProjectionsFn, LNLeakyFn)
"within 2x of torch's fp32 error against an fp64 evaluation" with the floors of tests/test_gpu_mlp.py.
Forward outputs are held to relative L2 1e-5 (the GRU tests' forward bound; the synthesis kernels' sine
and scale_function approximations are 2e-7 / 1e-6 relative).  The route assertions (a spy on ``_lib.call``)
are the only ones not made against a reference.
"""
import contextlib
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import torch_ref as tr

pytestmark = pytest.mark.gpu

GRAD_REL = 1e-5   # tests/test_gpu_grad.py, tests/test_gpu_gru.py
STFT_REL = 2e-5   # tests/test_gpu_stft.py test_stft_magnitude_grad
FWD_REL = 1e-5
SR = 48000


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


def rms(e):
    return float(e.double().pow(2).mean().sqrt()) if e.numel() else 0.0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def f0_frames(B, F_, seed=0):
    return 50.0 * 20.0 ** torch.rand(B, F_, 1, generator=_gen(seed))


class Case:
    """One Function at one shape: ``leaves`` (name -> CPU fp32 value), ``ours(dd, L)`` on cuda leaves and
    ``ref(L)`` on the reference's, both -> tuple of outputs.  ``mode`` "rel": relative L2 <= ``bound`` against
    torch's CPU fp32 autograd; "mlp": error against an fp64 CPU evaluation of ``ref`` within 2x of the error of
    ``ref`` in fp32 on the device (torch's kernels), + ``floor(rms of the fp64 value)``."""

    def __init__(self, leaves, ours, ref, mode="rel", bound=GRAD_REL, floor=None):
        self.leaves, self.ours, self.ref, self.mode, self.bound, self.floor = leaves, ours, ref, mode, bound, floor


# Upstream gradients handed straight to the outputs (torch.autograd.backward(outs, grads)), so that the
# Function's backward receives exactly this tensor:
#   dense         contiguous, 16-byte aligned (what every other gradient test delivers)
#   sum           a scalar one expanded to the output's shape, every stride 0: what out.sum().backward() delivers
#   strided       every second column (dim 1) of a buffer twice as wide: not contiguous
#   offset        a contiguous view that starts one float into its buffer: 4 bytes off a 16-byte boundary
#   offset_rows   columns 1.. (dim 1) of a buffer one column wider: not contiguous, and off by that column
# and the issue's two slice losses, (out[:, 1::2] * w).sum() and (out[:, 1:] * w).sum().  Those do NOT hand
# over a strided or misaligned gradient — autograd's slice backward writes the slice's gradient into a fresh,
# dense, aligned zero tensor — they are dense gradients with zeros in them, kept as the sparse-pattern cases:
#   slice_strided, slice_offset
LAYOUTS = ("sum", "strided", "offset", "offset_rows")
SLICE_LOSSES = ("slice_strided", "slice_offset")


def _upstream(o, kind, seed):
    """the gradient for output ``o``: values drawn on the CPU in fp32, the same for every evaluation and — but
    for "sum" — for every layout, the dense one included, so that the layout is all that differs between them
    (the scalar gradients of the reverb's decay and wet are sums that cancel: on a draw that left d wet 20 x
    below its usual size the CPU reference's own fp32 value was 7.8e-6 from its fp64 one, no yardstick for a
    1e-5 bound).  The view is taken on ``o``'s device, so that its strides and offset are the ones named."""
    shape = list(o.shape)
    w = torch.randn(shape, generator=_gen(seed))
    if kind == "dense":
        return w.to(o)
    if kind == "sum":
        return torch.ones((), dtype=o.dtype, device=o.device).expand(shape)
    if kind == "strided":
        big = torch.zeros(shape[0], 2 * shape[1], *shape[2:])
        big[:, ::2] = w
        return big.to(o)[:, ::2]
    if kind == "offset":
        return torch.cat([torch.zeros(1), w.flatten()]).to(o)[1:].view(shape)
    if kind == "offset_rows":
        big = torch.zeros(shape[0], shape[1] + 1, *shape[2:])
        big[:, 1:] = w
        return big.to(o)[:, 1:]
    raise ValueError(kind)


def _expected_layout(g, kind):
    """what ``_upstream`` promises, checked where the gradient is built and (test_layouts_reach_backward)
    where a backward receives it"""
    if kind == "sum":
        return all(s == 0 for s in g.stride())
    if kind == "strided":
        return not g.is_contiguous()
    if kind == "offset":
        return g.is_contiguous() and g.data_ptr() % 16 == 4
    if kind == "offset_rows":  # (off by one column: 4 bytes times the trailing dimensions; one row is contiguous)
        return g.storage_offset() > 0 and (g.shape[0] == 1 or not g.is_contiguous())
    return g.is_contiguous() and g.data_ptr() % 16 == 0


def _evaluate(fn, vals, req, dtype, device, which, kind, repeat=1, seed=1234):
    L = {k: torch.nn.Parameter(v.to(device=device, dtype=dtype), requires_grad=k in req) for k, v in vals.items()}
    outs = fn(L)
    outs = outs if isinstance(outs, tuple) else (outs,)
    which = list(which if which is not None else range(len(outs)))
    if kind in SLICE_LOSSES:
        loss = 0
        for i in which:
            v = outs[i][:, 1::2] if kind == "slice_strided" else outs[i][:, 1:]
            loss = loss + (v * torch.randn(v.shape, generator=_gen(seed + i)).to(v)).sum()
        for r in range(repeat):
            loss.backward(retain_graph=r + 1 < repeat)
    else:
        which = [i for i in which if outs[i].requires_grad]  # (an output no chosen leaf reaches: as in a loss, unused)
        grads = [_upstream(outs[i], kind, seed + i) for i in which]
        if device == "cuda":
            assert all(_expected_layout(g, kind) for g in grads), (kind, [(g.stride(), g.storage_offset()) for g in grads])
        for r in range(repeat):
            torch.autograd.backward([outs[i] for i in which], grads, retain_graph=r + 1 < repeat)
    return [o.detach() for o in outs], {k: p.grad for k, p in L.items()}


def check(dd, case, req=None, which=None, kind="dense", repeat=1, zero=()):
    """Forward outputs and every leaf's gradient against the reference; frozen leaves get no gradient.
    ``repeat``: that many backward passes over one retained graph, against ``repeat`` x the reference's.
    ``zero``: leaves whose gradient under this loss is identically zero (the reference's is its own round-off,
    no yardstick): held to ``bound`` x the norm of the reference's gradient under the dense loss instead."""
    req = set(case.leaves) if req is None else set(req)
    go, gg = _evaluate(lambda L: case.ours(dd, L), case.leaves, req, torch.float32, "cuda", which, kind, repeat)
    if case.mode == "rel":
        ro, rg = _evaluate(case.ref, case.leaves, req, torch.float32, "cpu", which, kind)
        yard_o = yard_g = None
    else:
        ro, rg = _evaluate(case.ref, case.leaves, req, torch.float64, "cpu", which, kind)
        yard_o, yard_g = _evaluate(case.ref, case.leaves, req, torch.float32, "cuda", which, kind)

    def close(name, got, ref, yard, scale):
        ref = ref.double() * scale
        if case.mode == "rel":
            err = relerr(got, ref)
            print(f"{name}: relerr {err:.3e} (bound {case.bound:.0e})")
            assert err <= case.bound, (name, err)
        else:
            e, ey = rms(got.double().cpu() - ref), rms(yard.double().cpu() * scale - ref)
            print(f"{name}: rms error {e:.3e}, torch fp32 {ey:.3e}")
            assert e <= 2 * ey + case.floor(rms(ref)), (name, e, ey)

    assert len(go) == len(ro)
    for i, (a, b) in enumerate(zip(go, ro)):
        assert a.shape == b.shape and a.dtype == torch.float32
        if case.mode == "rel":
            err = relerr(a, b)
            print(f"out{i}: relerr {err:.3e}")
            assert err <= FWD_REL, (i, err)
        else:
            close(f"out{i}", a, b, yard_o[i], 1)
    for k in case.leaves:
        if k not in req:
            assert gg[k] is None, f"frozen leaf {k} received a gradient"
        elif k in zero:
            _, dense = _evaluate(case.ref, case.leaves, req, torch.float32, "cpu", which, "dense")
            size = float(gg[k].double().norm()) / float(dense[k].double().norm())
            print(f"d{k}: {size:.3e} of the dense loss's gradient (the reference's: "
                  f"{float(rg[k].double().norm()) / float(dense[k].double().norm()):.3e})")
            assert size <= case.bound, (k, size)
        elif rg[k] is None:  # no path from the chosen outputs to this leaf: nothing, or a materialised zero
            assert gg[k] is None or not bool(gg[k].any()), k
        else:
            assert gg[k] is not None and gg[k].shape == rg[k].shape, k
            close(f"d{k}", gg[k], rg[k], None if yard_g is None else yard_g[k], repeat)


def subsets(names, extra=()):
    """each single leaf, every "all but one" subset, all of them, and ``extra``"""
    names = list(names)
    out = [(n,) for n in names]
    if len(names) > 2:
        out += [tuple(m for m in names if m != n) for n in names]
    if len(names) > 1:
        out.append(tuple(names))
    return out + [s for s in extra if s not in out]


def reaching(cases, paths):
    """drop the (leaves, outputs) choices in which no chosen leaf reaches a chosen output (``paths``: leaf -> the
    outputs that depend on it): such a loss has no graph, on the reference either"""
    return [(r, w) for r, w in cases if any(set(paths.get(n, w)) & set(w) for n in r)]


def _spy(monkeypatch):
    from ddsp_pytorch_amd import _lib
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: calls.append(name) or real(name, *a, **k))
    return calls


def ids(v):
    return "+".join(map(str, v)) if isinstance(v, (tuple, list, range)) else str(v)


# ------------------------------------------------------------------------------------------ the cases
def case_scale():
    x = torch.randn(3, 1001, generator=_gen(0)) * 4
    return Case({"x": x}, lambda dd, L: dd.core.scale_with_bias(L["x"], -5.0), lambda L: tr.scale_function(L["x"] + (-5.0)))


def case_nyquist():
    f0 = f0_frames(2, 7, 1)
    a = torch.rand(2, 7, 33, generator=_gen(1))
    return Case({"a": a}, lambda dd, L: dd.core.remove_above_nyquist(L["a"], f0.cuda(), SR),
                lambda L: tr.remove_above_nyquist(L["a"], f0, SR))


def case_upsample():
    s = torch.randn(2, 7, 5, generator=_gen(2))
    return Case({"s": s}, lambda dd, L: dd.core.upsample(L["s"], 64), lambda L: tr.upsample(L["s"], 64))


def case_harmonic_synth():
    f0 = tr.upsample(f0_frames(2, 4, 3), 64)
    a = torch.rand(2, 256, 16, generator=_gen(3)) / 16
    return Case({"a": a}, lambda dd, L: dd.core.harmonic_synth(f0.cuda(), L["a"], SR),
                lambda L: tr.harmonic_synth(f0, L["a"], SR))


def case_impulse_response():
    amp = torch.rand(3, 5, 17, generator=_gen(4))
    return Case({"amp": amp}, lambda dd, L: dd.core.amp_to_impulse_response(L["amp"], 40),
                lambda L: tr.amp_to_impulse_response(L["amp"], 40))


def case_fft_convolve(rows=4, krows=1, N=100):
    g = _gen(rows * N + krows)
    s = torch.randn(rows, N, generator=g)
    k = torch.randn(krows, N, generator=g) * 0.1
    return Case({"s": s, "k": k}, lambda dd, L: dd.core.fft_convolve(L["s"], L["k"]),
                lambda L: tr.fft_convolve(L["s"], L["k"]))


def case_controls():
    f0 = f0_frames(2, 5, 5)
    g = _gen(5)
    a, d = torch.randn(2, 5, 1, generator=g), torch.randn(2, 5, 17, generator=g)
    return Case({"a": a, "d": d}, lambda dd, L: dd.core.harmonic_controls(L["a"], L["d"], f0.cuda(), SR),
                lambda L: tr.harmonic_controls(L["a"], L["d"], f0, SR))


def case_harmonic_frames():
    f0 = f0_frames(2, 5, 6)
    g = _gen(6)
    a = torch.rand(2, 5, 1, generator=g) + 0.1
    d = torch.rand(2, 5, 17, generator=g) / 17
    return Case({"a": a, "d": d},
                lambda dd, L: dd.core.harmonic_synth_frames(f0.cuda(), L["a"], L["d"], 64, SR, write_back=False),
                lambda L: tr.harmonic_forward(L["a"], L["d"] * 1.0, f0, 64, SR))  # (its in-place *= on a copy)


def _ref_harmonic(param, f0, bs):
    a, d = tr.harmonic_controls(param[..., :1], param[..., 1:], f0, SR)
    return tr.harmonic_forward(a, d, f0, bs, SR)


def case_harmonic_params():
    f0 = f0_frames(2, 5, 7)
    p = torch.randn(2, 5, 18, generator=_gen(7))
    return Case({"param": p}, lambda dd, L: dd.core.harmonic_synth_params(f0.cuda(), L["param"], 64, SR),
                lambda L: _ref_harmonic(L["param"], f0, 64))


def case_filtered_noise(B=2, F_=4, bs=64, NB=17):
    g = _gen(8)
    m = torch.randn(B, F_, NB, generator=g)
    add = torch.randn(B, F_ * bs, 1, generator=g)
    nz = torch.rand(B, F_, bs, generator=g) * 2 - 1

    def ref(L):
        n = tr.noise_forward(tr.scale_function(L["m"] + (-5.0)), nz, bs)
        return n + L["add"], n

    return Case({"m": m, "add": add},
                lambda dd, L: dd.core.filtered_noise(L["m"], bs, noise=nz.cuda(), add=L["add"], return_noise=True,
                                                     raw_bias=-5.0), ref)


def case_synth_frames(parts, B=2, F_=5, H=17, NB=9, bs=64):
    g = _gen(9)
    f0 = f0_frames(B, F_, 9)
    p = torch.randn(B, F_, H + 1, generator=g)
    m = torch.randn(B, F_, NB, generator=g)
    nz = torch.rand(B, F_, bs, generator=g) * 2 - 1

    def ref(L):
        h = _ref_harmonic(L["param"], f0, bs)
        n = tr.noise_forward(tr.scale_function(L["mags"] + (-5.0)), nz, bs)
        return (h + n, h, n) if parts else h + n

    return Case({"param": p, "mags": m},
                lambda dd, L: dd.core.synth_frames(f0.cuda(), L["param"], L["mags"], bs, SR, noise=nz.cuda(), parts=parts),
                ref)


def _reverb_values(T, L):
    g = _gen(T + L)
    return {"noise": (torch.rand(L, generator=g) * 2 - 1).unsqueeze(-1), "decay": torch.tensor(4.0),
            "wet": torch.tensor(0.3)}


def _reverb_module(dd, L, length):
    rv = dd.modules.Reverb(length, SR).cuda()
    rv.noise, rv.decay, rv.wet = L["noise"], L["decay"], L["wet"]
    return rv


def case_reverb(B=2, T=4096, L=3000):
    vals = {"x": torch.randn(B, T, 1, generator=_gen(B * T + L)) * 0.3, **_reverb_values(T, L)}
    return Case(vals, lambda dd, P: _reverb_module(dd, P, L)(P["x"]),
                lambda P: tr.Reverb(P["noise"], P["decay"], P["wet"], L, SR)(P["x"]))


def case_reverb_apply(B=2, T=4096, L=3000):
    p = _reverb_values(T, L)
    imp = tr.Reverb(p["noise"], p["decay"], p["wet"], L, SR).build_impulse().detach()
    x = torch.randn(B, T, 1, generator=_gen(11)) * 0.3

    def ours(dd, P):
        with torch.no_grad():
            spec = dd.core.reverb_spectrum(imp.cuda(), T)
        return dd.core.reverb_apply(P["x"], spec, L)

    return Case({"x": x}, ours, lambda P: tr.fft_convolve(P["x"].squeeze(-1), F.pad(imp, (0, 0, 0, T - L)).squeeze(-1)).unsqueeze(-1))


def case_build_impulse(L=300):
    return Case(_reverb_values(0, L), lambda dd, P: dd.core.reverb_build_impulse(P["noise"], P["decay"], P["wet"], SR),
                lambda P: tr.Reverb(P["noise"], P["decay"], P["wet"], L, SR).build_impulse())


def case_stft(n=128):
    x = torch.randn(2, 12000, generator=_gen(n)) * 0.3
    return Case({"x": x}, lambda dd, L: dd.core.stft_magnitude(L["x"], n, n // 4),
                lambda L: torch.stft(L["x"], n, n // 4, n, torch.hann_window(n), True, normalized=True,
                                     return_complex=True).abs(), bound=STFT_REL)


def case_linear(rows, K, N):
    """(33, 512, 512): ddsp_hip_linear; (7, 514, 512): torch.addmm inside LinearFn (K outside the kernel's)."""
    torch.manual_seed(rows + K)
    lin = torch.nn.Linear(K, N)
    vals = {"x": torch.randn(rows, K), "w": lin.weight.detach().clone(), "b": lin.bias.detach().clone()}

    def ours(dd, L):
        from ddsp_pytorch_amd.grad import LinearFn
        return LinearFn.apply(L["x"], L["w"], L["b"])

    return Case(vals, ours, lambda L: F.linear(L["x"], L["w"], L["b"]), mode="mlp", floor=lambda r: 1e-12)


def _projection_values(rows, n1, n2):
    torch.manual_seed(rows)
    l1, l2 = torch.nn.Linear(512, n1), torch.nn.Linear(512, n2)
    return {"x": torch.randn(rows, 512), "w1": l1.weight.detach().clone(), "b1": l1.bias.detach().clone(),
            "w2": l2.weight.detach().clone(), "b2": l2.bias.detach().clone()}


def case_projections(rows=37):
    """through decoder_projections on a fresh DDSPDecoder(512, 100, 65, 48000, 64, False): the dispatch is under
    test too.  Its two outputs are column slices of ProjectionsFn's, so whatever gradient they are given,
    ProjectionsFn's backward receives the dense one that the slices' backward builds (case_projections_fn)."""
    vals = _projection_values(rows, 101, 65)

    def ours(dd, L):
        m = dd.DDSPDecoder(512, 100, 65, SR, 64, False).cuda()
        m.harmonic_proj.weight, m.harmonic_proj.bias = L["w1"], L["b1"]
        m.noise_proj.weight, m.noise_proj.bias = L["w2"], L["b2"]
        return dd.decoder.decoder_projections(m, L["x"])

    return Case(vals, ours, lambda L: (F.linear(L["x"], L["w1"], L["b1"]), F.linear(L["x"], L["w2"], L["b2"])),
                mode="mlp", floor=lambda r: 1e-12)


def case_projections_fn(rows=37):
    """ProjectionsFn itself, so that its backward receives the upstream gradient as given: 101 + 67 outputs, a
    multiple of 4, so that its one output buffer has no padding columns (with 101 + 65 the buffer is 168 wide
    and its last two columns are never written)."""
    vals = _projection_values(rows, 101, 67)

    def ours(dd, L):
        from ddsp_pytorch_amd.grad import ProjectionsFn
        return ProjectionsFn.apply(L["x"], L["w1"], L["b1"], L["w2"], L["b2"])

    return Case(vals, ours, lambda L: torch.cat([F.linear(L["x"], L["w1"], L["b1"]), F.linear(L["x"], L["w2"], L["b2"])], -1),
                mode="mlp", floor=lambda r: 1e-12)


def case_ln_leaky(rows, cols):
    g = _gen(rows + cols)
    vals = {"g": torch.randn(rows, cols, generator=g) * 1.7 + 0.4, "gamma": 1 + 0.3 * torch.randn(cols, generator=g),
            "beta": 0.2 * torch.randn(cols, generator=g)}

    def ours(dd, L):
        from ddsp_pytorch_amd.grad import LNLeakyFn
        return LNLeakyFn.apply(L["g"], L["gamma"], L["beta"], 1e-5, 0.01)

    return Case(vals, ours, lambda L: F.leaky_relu(F.layer_norm(L["g"], (cols,), L["gamma"], L["beta"], 1e-5), 0.01),
                mode="mlp", floor=lambda r: 1e-7 * (1 + r))


def case_gru(B, T, I, H):
    """(3, 5, 1024, 512): the persistent launches; (3, 5, 32, 64): the step kernels."""
    torch.manual_seed(B + T + H)
    g = torch.nn.GRU(I, H, batch_first=True)
    vals = {"x": torch.randn(B, T, I), "w_ih": g.weight_ih_l0.detach().clone(), "w_hh": g.weight_hh_l0.detach().clone(),
            "b_ih": g.bias_ih_l0.detach().clone(), "b_hh": g.bias_hh_l0.detach().clone(), "h0": torch.randn(1, B, H) * 0.5}

    def ours(dd, L):
        mod = types.SimpleNamespace(num_layers=1, batch_first=True, bidirectional=False, bias=True, hidden_size=H,
                                    weight_ih_l0=L["w_ih"], weight_hh_l0=L["w_hh"], bias_ih_l0=L["b_ih"],
                                    bias_hh_l0=L["b_hh"])
        return dd.core.gru(L["x"], mod, L["h0"])

    def ref(L):
        return torch.func.functional_call(g, {"weight_ih_l0": L["w_ih"], "weight_hh_l0": L["w_hh"],
                                              "bias_ih_l0": L["b_ih"], "bias_hh_l0": L["b_hh"]}, (L["x"], L["h0"]))

    return Case(vals, ours, ref)


# ------------------------------------------------------------------------------------------ A. partial requires_grad
_LN = ("g", "gamma", "beta")


@pytest.mark.parametrize("req", subsets(_LN), ids=ids)
@pytest.mark.parametrize("rows,cols", [(37, 512), (5, 1024)])
def test_partial_ln_leaky(dd, rows, cols, req):
    """LNLeakyFn: gamma and beta both frozen (no partial sums, no sum kernel), one of them frozen (the sum
    kernel's null branches), the input frozen."""
    check(dd, case_ln_leaky(rows, cols), req)


@pytest.mark.parametrize("req", subsets(("x", "w", "b")), ids=ids)
@pytest.mark.parametrize("rows,K,N", [(33, 512, 512), (7, 514, 512)])
def test_partial_linear(dd, rows, K, N, req):
    check(dd, case_linear(rows, K, N), req)


@pytest.mark.parametrize("req,which", reaching([(r, w) for r in subsets(("x", "w1", "b1", "w2", "b2"))
                                                 for w in ((0, 1), (0,), (1,))],
                                                {"w1": (0,), "b1": (0,), "w2": (1,), "b2": (1,)}), ids=ids)
def test_partial_projections(dd, monkeypatch, req, which):
    """ProjectionsFn through decoder_projections (the dispatch under test too): fp32 outside autocast takes the
    one-launch kernel, whichever leaves are frozen."""
    calls = _spy(monkeypatch)
    check(dd, case_projections(), req, which)
    assert calls[0] == "projections" and "linear" not in calls, calls
    assert ("linear_weight_grad" in calls) == bool({"w1", "w2"} & set(req)), calls


_GRU = ("x", "w_ih", "w_hh", "b_ih", "b_hh", "h0")


@pytest.mark.parametrize("req,which", [(r, (0, 1)) for r in subsets(_GRU)] + [(_GRU, (0,)), (_GRU, (1,)), (("x",), (1,))],
                         ids=ids)
@pytest.mark.parametrize("B,T,I,H", [(3, 5, 1024, 512), (3, 5, 32, 64)])
def test_partial_gru(dd, B, T, I, H, req, which):
    """GRUFn: frozen weights with x requiring grad, h0 given but frozen, the loss on ``out`` alone and on
    ``h_T`` alone (where the gradient of ``out`` arrives as materialised zeros)."""
    check(dd, case_gru(B, T, I, H), req, which)
    dev = torch.cuda.current_device()
    assert dd.core._GRU_LAST[dev][0] == ("persistent" if H == 512 else "steps")


_RV = ("x", "noise", "decay", "wet")


@pytest.mark.parametrize("req", subsets(_RV, extra=[("noise", "decay", "wet")]), ids=ids)
@pytest.mark.parametrize("B,T,L", [(2, 4096, 3000), (1, 2048, 4800)])
def test_partial_reverb(dd, B, T, L, req):
    """ReverbFn through modules.Reverb: parameters without x (no input gradient out of the backward), x with
    all three parameters frozen (the signal-only route); (1, 2048, 4800) crops the IR, whose tail gets a
    zero gradient."""
    check(dd, case_reverb(B, T, L), req)


_SF = ("param", "mags")


@pytest.mark.parametrize("parts,req,which", [(False, r, (0,)) for r in subsets(_SF)] + [(True, r, w) for r, w in reaching(
    [(r, w) for r in subsets(_SF) for w in ((0, 1, 2), (0,), (1,), (2,))], {"param": (0, 1), "mags": (0, 2)})], ids=ids)
def test_partial_synth_frames(dd, parts, req, which):
    """SynthFramesFn with injected noise: one projection frozen; with ``parts`` the loss on the sum alone, on
    the harmonic part alone and on the noise part alone (a part that does not depend on a leaf leaves it no
    gradient, or a zero one)."""
    check(dd, case_synth_frames(parts), req, which)


@pytest.mark.parametrize("req,which", reaching([(r, w) for r in subsets(("m", "add")) for w in ((0, 1), (0,), (1,))],
                                                {"add": (0,)}), ids=ids)
def test_partial_filtered_noise(dd, req, which):
    """FilteredNoiseFn with ``add`` and ``return_noise``: ``add`` requiring grad while the magnitudes do not."""
    check(dd, case_filtered_noise(), req, which)


@pytest.mark.parametrize("req", subsets(("s", "k")), ids=ids)
@pytest.mark.parametrize("rows,krows,N", [(4, 1, 100), (4, 4, 100)])
def test_partial_fft_convolve(dd, rows, krows, N, req):
    """FFTConvolveFn: a broadcast kernel (krows == 1) with only the signal requiring grad, and the reverse."""
    check(dd, case_fft_convolve(rows, krows, N), req)


# ------------------------------------------------------------------------------------------ B. upstream layouts
LAYOUT_CASES = {
    "scale": case_scale, "nyquist": case_nyquist, "upsample": case_upsample, "harmonic_synth": case_harmonic_synth,
    "impulse_response": case_impulse_response, "fft_convolve": case_fft_convolve, "controls": case_controls,
    "harmonic_frames": case_harmonic_frames, "harmonic_params": case_harmonic_params,
    "filtered_noise": case_filtered_noise, "synth_frames": lambda: case_synth_frames(False),
    "synth_frames_parts": lambda: case_synth_frames(True), "reverb_apply": case_reverb_apply, "reverb": case_reverb,
    "reverb_crop": lambda: case_reverb(1, 2048, 4800), "build_impulse": case_build_impulse, "stft": case_stft,
    "linear": lambda: case_linear(33, 512, 512), "linear_addmm": lambda: case_linear(7, 514, 512),
    "projections": case_projections, "projections_fn": case_projections_fn, "ln_leaky": lambda: case_ln_leaky(37, 512),
    "ln_leaky_1024": lambda: case_ln_leaky(5, 1024), "gru_persistent": lambda: case_gru(3, 5, 1024, 512),
    "gru_steps": lambda: case_gru(3, 5, 32, 64),
}


@pytest.mark.parametrize("kind", LAYOUTS + SLICE_LOSSES)
@pytest.mark.parametrize("name", list(LAYOUT_CASES))
def test_upstream_gradient_layout(dd, name, kind):
    """Every Function in grad.py with an upstream gradient, on each of its outputs, that is zero-stride (what
    ``out.sum()`` hands over), strided, contiguous but 4 bytes off a 16-byte boundary, or both strided and off
    (LAYOUTS: given to the outputs directly, so the backward receives that very tensor); and the two slice
    losses, whose gradients arrive dense with zeros in them."""
    # the normalised distribution's rows sum to one: d(sum of the controls) / d(distribution) = 0 identically
    zero = ("d",) if (name, kind) == ("controls", "sum") else ()
    check(dd, LAYOUT_CASES[name](), kind=kind, zero=zero)


@pytest.mark.parametrize("kind", ("dense",) + LAYOUTS)
def test_layouts_reach_backward(kind):
    """The premise of test_upstream_gradient_layout: torch's engine hands a Function's backward the gradient
    given to its output as it is — same strides, same storage offset, no copy."""
    seen = []

    class Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 2

        @staticmethod
        def backward(ctx, g):
            seen.append(g)
            return g * 2

    x = torch.randn(6, 10, 3, device="cuda", requires_grad=True)
    out = Probe.apply(x)
    g = _upstream(out, kind, 1)
    out.backward(g)
    assert len(seen) == 1 and seen[0].data_ptr() == g.data_ptr() and seen[0].stride() == g.stride()
    assert _expected_layout(seen[0], kind), (kind, seen[0].stride(), seen[0].data_ptr() % 16)


# ------------------------------------------------------------------------------------------ C. graph reuse
@pytest.mark.parametrize("name", ["reverb", "reverb_crop", "synth_frames_parts", "filtered_noise", "gru_persistent",
                                  "gru_steps"])
def test_backward_twice_over_a_retained_graph(dd, name):
    """backward(retain_graph=True) twice accumulates twice the reference's gradient: what a backward needs from
    its forward (the reverb's input spectra) lives as long as the graph."""
    check(dd, LAYOUT_CASES[name](), repeat=2)


def test_one_reverb_two_inputs_one_backward(dd):
    """One Reverb module applied to two inputs of the same length in one graph (one IR cache, two forward
    workspaces), a single backward."""
    B, T, L = 2, 4096, 3000
    g = _gen(77)
    xs = [torch.randn(B, T, 1, generator=g) * 0.3 for _ in range(2)]
    ws = [torch.randn(B, T, 1, generator=g) for _ in range(2)]
    vals = _reverb_values(T, L)
    pc = {k: v.clone().requires_grad_(True) for k, v in vals.items()}
    pg = {k: torch.nn.Parameter(v.cuda()) for k, v in vals.items()}
    xc = [x.clone().requires_grad_(True) for x in xs]
    xg = [x.cuda().requires_grad_(True) for x in xs]
    ref = tr.Reverb(pc["noise"], pc["decay"], pc["wet"], L, SR)
    sum((ref(x) * w).sum() for x, w in zip(xc, ws)).backward()
    rv = _reverb_module(dd, pg, L)
    sum((rv(x) * w.cuda()).sum() for x, w in zip(xg, ws)).backward()
    for a, b in zip(xg, xc):
        assert relerr(a.grad, b.grad) <= GRAD_REL, relerr(a.grad, b.grad)
    for k in vals:
        assert relerr(pg[k].grad, pc[k].grad) <= GRAD_REL, (k, relerr(pg[k].grad, pc[k].grad))


# ------------------------------------------------------------------------------------------ D. double backward
def _double_cases(dd):
    f0 = f0_frames(2, 5, 9).cuda()

    def leaf(*shape, scale=1.0):
        return (torch.randn(*shape, device="cuda") * scale).requires_grad_(True)

    def scale():
        x = leaf(3, 100)
        return x, dd.core.scale_function(x)

    def fft_convolve():
        s = leaf(4, 100)
        return s, dd.core.fft_convolve(s, torch.randn(1, 100, device="cuda") * 0.1)

    def nyquist():
        a = leaf(2, 5, 33)
        return a, dd.core.remove_above_nyquist(a, f0, SR)

    def synth_frames():
        p = leaf(2, 5, 18)
        return p, dd.core.synth_frames(f0, p, torch.randn(2, 5, 9, device="cuda"), 64, SR,
                                       noise=torch.rand(2, 5, 64, device="cuda") * 2 - 1)

    def reverb():
        x = leaf(2, 4096, 1, scale=0.3)
        return x, dd.modules.Reverb(3000, SR).cuda()(x)

    return {"scale": scale, "fft_convolve": fft_convolve, "nyquist": nyquist, "synth_frames": synth_frames,
            "reverb": reverb}


@pytest.mark.parametrize("loss", ["sum", "square"])
@pytest.mark.parametrize("name", ["scale", "fft_convolve", "nyquist", "synth_frames", "reverb"])
def test_double_backward_is_refused(dd, name, loss):
    """A first-order gradient taken with create_graph=True cannot be back-propagated through: RuntimeError, not
    a silently truncated second-order gradient.  ``out.sum()`` hands the backward a constant upstream gradient
    and the penalty is back-propagated alone; ``(out ** 2).sum()`` hands it one that itself requires grad, and
    the penalty is back-propagated together with a first-order term, as a training step would: without the
    refusal NyquistFn / FFTConvolveFn re-dispatched into themselves and the kernels' fresh buffers cut the
    graph, so that step ran and dropped the penalty's gradient."""
    torch.manual_seed(5)
    leaf, out = _double_cases(dd)[name]()
    first = out.sum() if loss == "sum" else out.pow(2).sum()
    (g,) = torch.autograd.grad(first, leaf, create_graph=True)
    assert g.shape == leaf.shape and bool(torch.isfinite(g).all())
    penalty = g.pow(2).sum() if loss == "sum" else g.pow(2).sum() + out.sum()
    # "square": the refusal itself.  "sum": the first-order gradient has no graph at all (nothing in it
    # requires grad), which is torch's own error — the same with or without once_differentiable; it shows only
    # that such a penalty cannot be back-propagated silently when it stands alone
    with pytest.raises(RuntimeError, match="once_differentiable" if loss == "square" else "does not require grad"):
        penalty.backward()


# ------------------------------------------------------------------------------------------ E. dtypes and autocast
# Two evaluations of a Linear (or of its gradients: GEMMs as well) in a dtype with epsilon eps, accumulated in
# fp32 or wider: each rounds its result once to that dtype, <= eps/2 of the value, and accumulates K <= 512
# products with an error far below that for bf16 / fp16 (512 * 2^-24 = 3e-5 of the terms' scale) and of the
# order of sqrt(K) * eps/2 of a term, i.e. of eps/2 of the result's scale, when the dtype accumulates in
# itself (fp64).  Two such results differ by at most ~ 2 * (eps/2 + eps/2) = 2 eps of the scale; x 4 headroom
# for the element whose partial sums run largest: 8 eps * max |reference|.
def _eps_bound(ref, dtype):
    return 8 * torch.finfo(dtype).eps * float(ref.detach().abs().max())


def _assert_within(got, ref, dtype, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype)
    err = float((got.detach().double() - ref.detach().double()).abs().max())
    print(f"{what}: max abs error {err:.3e} (bound {_eps_bound(ref, dtype):.3e})")
    assert err <= _eps_bound(ref, dtype), (what, err, _eps_bound(ref, dtype))


@pytest.mark.parametrize("setting", ["autocast_fp32_hidden", "autocast_bf16_hidden", "half_model", "double_model"])
def test_projections_dtype_and_autocast_under_autograd(dd, monkeypatch, setting):
    """decoder_projections with autograd outside the fp32 kernels' dtype: torch's two Linears run (no C-ABI
    call), so the outputs have their dtype and values, and the five gradients are theirs."""
    torch.manual_seed(3)
    model_dtype = {"half_model": torch.float16, "double_model": torch.float64}.get(setting, torch.float32)
    m = dd.DDSPDecoder(512, 100, 65, SR, 64, False).cuda().to(model_dtype)
    auto = setting.startswith("autocast")
    hidden_dtype = torch.bfloat16 if setting == "autocast_bf16_hidden" else model_dtype
    round_dtype = torch.bfloat16 if auto else model_dtype  # the dtype the Linears compute and round in
    h0 = torch.randn(37, 512, device="cuda").to(hidden_dtype)
    w1 = torch.randn(37, 101, device="cuda")
    w2 = torch.randn(37, 65, device="cuda")
    ps = [m.harmonic_proj.weight, m.harmonic_proj.bias, m.noise_proj.weight, m.noise_proj.bias]

    def run(fn):
        h = h0.clone().requires_grad_(True)
        for p in ps:
            p.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16) if auto else contextlib.nullcontext():
            a, b = fn(h)
            ((a.float() * w1).sum() + (b.float() * w2).sum()).backward()
        return a, b, [h.grad] + [p.grad.clone() for p in ps]

    ra, rb, rgrads = run(lambda h: (m.harmonic_proj(h), m.noise_proj(h)))
    calls = _spy(monkeypatch)
    a, b, grads = run(lambda h: dd.decoder.decoder_projections(m, h))
    assert calls == [], calls
    _assert_within(a, ra, round_dtype, "harmonic_proj")
    _assert_within(b, rb, round_dtype, "noise_proj")
    for name, g, r in zip(("hidden", "hp.weight", "hp.bias", "np.weight", "np.bias"), grads, rgrads):
        _assert_within(g, r, round_dtype, "d" + name)


def test_gru_decoder_autocast_under_autograd(dd, monkeypatch):
    """gru_decoder_forward under autocast with grad enabled: the MLPs and the GRU stay on torch's modules (no
    C-ABI call); the output and every parameter's gradient are those of the module chain (decoder.py:43-68)."""
    torch.manual_seed(4)
    dec = dd.decoder.GRUDecoder(512).cuda()
    f0 = torch.rand(2, 6, 1, device="cuda") * 800 + 50
    lo = torch.randn(2, 6, 1, device="cuda")
    w = torch.randn(2, 6, 512, device="cuda")
    ps = dict(dec.named_parameters())

    def chain(f0, lo):
        hidden = torch.cat([dec.f0_mlp(f0), dec.loudness_mlp(lo)], -1)
        return dec.out_mlp(torch.cat([dec.gru(hidden)[0], f0, lo], -1))

    def run(fn):
        for p in ps.values():
            p.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = fn(f0, lo)
            (y.float() * w).sum().backward()
        return y, {k: p.grad.clone() for k, p in ps.items()}

    ry, rg = run(chain)
    calls = _spy(monkeypatch)
    y, g = run(dec)
    assert calls == [], calls
    _assert_within(y, ry, torch.bfloat16, "out")
    for k in ps:
        _assert_within(g[k], rg[k], torch.bfloat16, "d" + k)


def test_projections_fp32_training_route(dd, monkeypatch):
    """fp32 outside autocast, with autograd: still ProjectionsFn (one ddsp_hip_projections launch, the weight
    gradient on ddsp_hip_linear_weight_grad)."""
    torch.manual_seed(6)
    m = dd.DDSPDecoder(512, 100, 65, SR, 64, False).cuda()
    h = torch.randn(37, 512, device="cuda", requires_grad=True)
    calls = _spy(monkeypatch)
    a, b = dd.decoder.decoder_projections(m, h)
    assert calls == ["projections"], calls
    assert a.dtype == b.dtype == torch.float32 and a.grad_fn is not None
    (a.sum() + b.sum()).backward()
    assert calls == ["projections", "linear_weight_grad"], calls
