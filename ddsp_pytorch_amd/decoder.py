"""Caller of the hot path: a ``DDSPDecoder`` with the reference's architecture and
state_dict keys (ddsp/models/decoder.py:9-136, ddsp/core.py:122-133), wired to the gfx950
synth modules.

The control network before the path runs at inference on gfx950 kernels
too: each MLP block is one matrix-core launch with its LayerNorm + LeakyReLU (core.mlp_block), the
GRU's input projection for every step one matrix-core launch (core.linear) and its recurrence one
persistent launch per layer (core.gru), the two projections one matrix-core launch reading both layers'
parameters in place (core.projections), and the synthesis section of ``forward`` (decoder.py:106-125) one
fused launch before the reverb.  Under autograd the MLP blocks' Linears run their forward, input gradient
and weight gradient on the matrix-core kernels (grad.LinearFn), their LayerNorm + LeakyReLU forward and
backward on this package's kernels (grad.LNLeakyFn), the projections one grad.ProjectionsFn (forward in one
matrix-core launch, weight gradient on the matrix cores), and the GRU's BPTT is one persistent
launch with its weight gradients on the matrix cores.

Which of these a call takes is decided in one place per layer: ``mlp_route`` once per MLP and forward
("kernels", "autograd" or "modules"), ``_gru`` for the recurrence, ``decoder_projections`` for the two
projections.  They share two questions: is somebody observing the modules (``_observed``: then the module
calls stay), and must autograd record the call (``core._wants_grad``).  A kernel's shapes are named beside
its wrapper in ``core`` (MLP_MATRIX_MIN_IN, LN_LEAKY_COLS) or answered by the launch itself (ERANGE).
"""
import torch
import torch.nn as nn

from . import core, grad
from .modules import NOISE_MODES, FilteredNoise, HarmonicSynth, Reverb


def mlp(in_size, hidden_size, n_layers):
    """ddsp/core.py:122-129: (Linear, LayerNorm, LeakyReLU) x n_layers."""
    sizes = [in_size] + n_layers * [hidden_size]
    layers = []
    for i in range(n_layers):
        layers += [nn.Linear(sizes[i], sizes[i + 1]), nn.LayerNorm(sizes[i + 1]), nn.LeakyReLU()]
    return nn.Sequential(*layers)


class GRUDecoder(nn.Module):
    """ddsp/models/decoder.py:9-68, incl. the optional z conditioning (z_dim: a z_mlp whose output joins
    the GRU input, decoder.py:31-39) that DDSPAutoencoder uses."""

    def __init__(self, hidden_size: int, z_dim: int = None):
        super().__init__()
        self.register_buffer("cache_gru", torch.zeros(1, 1, hidden_size))
        self.f0_mlp = mlp(1, hidden_size, 3)
        self.loudness_mlp = mlp(1, hidden_size, 3)
        self.add_z = z_dim is not None
        if self.add_z:
            self.z_mlp = mlp(z_dim, hidden_size, 3)
        self.gru = nn.GRU((3 if self.add_z else 2) * hidden_size, hidden_size, batch_first=True)
        self.out_mlp = mlp(hidden_size + 2, hidden_size, 3)

    def forward(self, f0, loudness, z=None, realtime: bool = False):
        return gru_decoder_forward(self, f0, loudness, z, realtime)


def _gru(mod, hidden, h0):
    """mod.gru(hidden[, h0]) with the recurrence (and, under autograd, its BPTT) on the gfx950 step
    kernels; torch's GRU only for shapes outside the kernel's (hidden % 64 != 0)."""
    if hidden.is_cuda and core.gru_supported(mod.gru) and _fp32_inference_ok(hidden, (mod.gru,)):
        return core.gru(hidden, mod.gru, h0)
    return mod.gru(hidden, h0) if h0 is not None else mod.gru(hidden)


def _observed(*mods):
    """Somebody watches these module calls: forward (pre-)hooks on one of them or registered globally.  Such a
    call stays a module call."""
    from torch.nn.modules import module as _m
    return bool(_m._global_forward_hooks or _m._global_forward_pre_hooks or
                any(m._forward_hooks or m._forward_pre_hooks for m in mods))


def _blocks(seq):
    """The (Linear, LayerNorm, LeakyReLU) triples of a ddsp/core.py:122-129 chain."""
    mods = list(seq)
    return [mods[i:i + 3] for i in range(0, len(mods), 3)]


def _mlp_params(seq):
    """The parameters of an unobserved (Linear, LayerNorm, LeakyReLU) x n chain, or None where ``seq`` is not one:
    the plain torch classes, affine LayerNorms, Linears with biases, no hooks on the chain or in it — nothing
    can tell its kernels from its module calls.  (Read off the blocks: walking the module tree with
    ``parameters()`` costs more than every other question mlp_route asks.)"""
    if (type(seq) is not nn.Sequential or type(seq).forward is not nn.Sequential.forward or len(seq) % 3
            or _observed(seq, *seq)):
        return None
    params = []
    for lin, ln, act in _blocks(seq):
        if (type(lin) is not nn.Linear or type(ln) is not nn.LayerNorm or type(act) is not nn.LeakyReLU or
                lin.bias is None or not ln.elementwise_affine or ln.bias is None):
            return None
        params += [lin.weight, lin.bias, ln.weight, ln.bias]
    return params


def mlp_route(seq, x, extras=()):
    """How mlp_forward runs seq(cat([x, *extras])), decided once per MLP and forward: "kernels" (an unobserved
    block chain in fp32 on the GPU that autograd need not record: the inference kernels), "autograd" (the same
    chain recorded: grad.LinearFn / grad.LNLeakyFn per block, on the concatenated input) or "modules" (torch's
    modules, as the reference calls them).  ``extras`` do not change the first answer — at inference a
    non-fp32 one is core's TypeError — but the autograd route takes the concatenation, in the dtype torch.cat
    gives it."""
    params = _mlp_params(seq) if x.is_cuda else None
    if params is None:
        return "modules"
    if _fp32_ok(x.dtype, x.device.type, params) and not core._wants_grad(x, *params):
        return "kernels"
    dtype = x.dtype
    for e in extras:
        dtype = torch.promote_types(dtype, e.dtype)
    return "autograd" if _fp32_ok(dtype, x.device.type, params) else "modules"


def _block_kernels(lin, ln, act, h, extras, out):
    """One block at inference: a one-feature Linear folds into the LayerNorm kernel, a block in core.mlp_block's
    shapes is that one launch, others run their GEMM then the LayerNorm kernel, or torch's modules outside it.
    ``out`` is written where the kernel can address it (the caller copies otherwise)."""
    y = None
    if lin.in_features == 1 and not extras:
        y = core.layer_norm_leaky_relu(h, ln, act, out=out, w1=lin.weight[:, 0], b1=lin.bias)
    elif lin.in_features >= core.MLP_MATRIX_MIN_IN:
        y = core.mlp_block(h, lin, ln, act, out=out, extras=extras)
    if y is None:
        hin = torch.cat([h, *extras], -1) if extras else h
        g = torch.nn.functional.linear(hin, lin.weight, lin.bias)
        y = core.layer_norm_leaky_relu(g, ln, act, out=out)
        if y is None:
            y = act(ln(g))
    return y


def _block_autograd(lin, ln, act, y):
    """One block under autograd: the Linear on grad.LinearFn (the one-feature first Linear stays torch's), its
    LayerNorm + LeakyReLU on grad.LNLeakyFn at the kernel's widths, else torch's modules."""
    g = grad.LinearFn.apply(y, lin.weight, lin.bias) if lin.in_features >= core.MLP_MATRIX_MIN_IN else lin(y)
    if lin.out_features in core.LN_LEAKY_COLS and tuple(ln.normalized_shape) == (lin.out_features,):
        return grad.LNLeakyFn.apply(g, ln.weight, ln.bias, ln.eps, act.negative_slope)
    return act(ln(g))


def mlp_forward(seq, x, out=None, extras=(), route=None):
    """seq(torch.cat([x, *extras], -1)) for a core.py:122-129 MLP, on ``route`` (mlp_route; computed if not
    given).  On the GPU at inference a block with 512 outputs is ONE launch (core.mlp_block: the Linear on the
    matrix cores, LayerNorm + LeakyReLU in its epilogue; ``extras`` — per-row [..., 1] inputs appended to x,
    the out_mlp's f0 and loudness — enter the first block's epilogue, so the concatenation is never built), a
    one-feature first Linear folds into the LayerNorm kernel (core.layer_norm_leaky_relu), other blocks run
    their GEMM then that kernel; the last block may write into ``out`` (e.g. a column slice of the GRU input
    concatenation).  On the other routes ``out`` receives a copy."""
    if route is None:
        route = mlp_route(seq, x, extras)
    if route == "kernels":
        y, blocks = x, _blocks(seq)
        for i, blk in enumerate(blocks):
            y = _block_kernels(*blk, y, extras if i == 0 else (), out if i == len(blocks) - 1 else None)
    else:
        y = torch.cat([x, *extras], -1) if extras else x
        if route == "autograd":
            for blk in _blocks(seq):
                y = _block_autograd(*blk, y)
        else:
            y = seq(y)
    if out is not None and y is not out:
        out.copy_(y)
        y = out
    return y


def gru_decoder_forward(self, f0, loudness, z=None, realtime=False):
    """ddsp/models/decoder.py:43-68 GRUDecoder.forward (incl. the optional z projection), the GRU on
    the step kernel for inference.  install() binds it to the reference's GRUDecoder too.  At inference
    on the GPU the MLP blocks' LayerNorm + LeakyReLU run fused and the input MLPs write straight into
    the GRU's input concatenation (mlp_forward): only when every one of them is on the kernels."""
    mlps = [(self.f0_mlp, f0), (self.loudness_mlp, loudness)]
    if getattr(self, "add_z", False):
        assert z is not None
        mlps.append((self.z_mlp, z))
    routes = [mlp_route(m, x) for m, x in mlps]
    widths = [m[-3].out_features if len(m) >= 3 else -1 for m, _ in mlps]
    if all(r == "kernels" for r in routes) and len(set(widths)) == 1:
        W = widths[0]
        hidden = torch.empty(*f0.shape[:-1], W * len(mlps), dtype=torch.float32, device=f0.device)
        for i, (m, x) in enumerate(mlps):
            mlp_forward(m, x, out=hidden[..., i * W:(i + 1) * W], route="kernels")
    else:
        hidden = torch.cat([mlp_forward(m, x, route=r) for (m, x), r in zip(mlps, routes)], -1)
    if realtime:
        gru_out, cache = _gru(self, hidden, self.cache_gru)
        self.cache_gru.copy_(cache)
    else:
        gru_out = _gru(self, hidden, None)[0]
    return mlp_forward(self.out_mlp, gru_out, extras=(f0, loudness))


def _hooked(m):
    """A module call that must stay a module call: observed (_observed), or a subclass / wrapper whose forward
    is not nn.Linear's."""
    return _observed(m) or type(m).forward is not torch.nn.Linear.forward


def _synth_overridden(m, cls):
    """The synth module's calls must stay module calls: observed (_observed), or a class whose forward /
    get_controls is not this package's (``cls``; install() binds the same functions to the reference's
    classes, so an installed reference module is not overridden)."""
    t = type(m)
    return _observed(m) or any(getattr(t, n, None) is not cls.__dict__[n] for n in ("forward", "get_controls"))


def _fp32_ok(dtype, device_type, params):
    """The fp32 network kernels apply: float32 input and parameters, and no autocast region (under
    torch.autocast torch's modules run in the autocast dtype; these kernels compute in fp32 only)."""
    return (dtype == torch.float32 and all(p.dtype == torch.float32 for p in params)
            and not torch.is_autocast_enabled(device_type))


def _fp32_inference_ok(x, mods):
    """_fp32_ok for input x and the parameters of ``mods``."""
    return _fp32_ok(x.dtype, x.device.type, (p for m in mods for p in m.parameters()))


def decoder_projections(self, hidden):
    """decoder.py:106-117: harmonic_proj(hidden), noise_proj(hidden).  On the GPU at inference ONE GEMM
    (core.projections: both layers' parameters stacked fresh on every call into a zero-padded buffer, then
    hipBLASLt — nothing is cached on or rebound in the modules, so every write to a parameter, through
    ``.data`` included, is seen by the next call); the two outputs are column slices of one buffer, which
    the fused synthesis kernel reads with its row stride.  Under autograd the concatenated weights keep the call
    differentiable, so the parameters receive their gradients as the reference's do: at 512 inputs
    grad.ProjectionsFn (the forward on ddsp_hip_projections, the weight gradient on ddsp_hip_linear_weight_grad),
    elsewhere grad.LinearFn over the concatenated parameters.  Both are fp32 kernels: for any other dtype of
    the input or the parameters, and inside an autocast region, the two module calls run (_fp32_ok),
    with or without autograd."""
    hp, npj = self.harmonic_proj, self.noise_proj
    ps = (hp.weight, hp.bias, npj.weight, npj.bias)
    if (not hidden.is_cuda or hp.bias is None or npj.bias is None or _hooked(hp) or _hooked(npj)
            or not _fp32_ok(hidden.dtype, hidden.device.type, ps)):
        # module hooks see the calls the reference makes; other dtypes and autocast regions run torch's Linears,
        # in their dtype, with their autograd
        return hp(hidden), npj(hidden)
    h1, n = hp.out_features, hp.out_features + npj.out_features
    if core._wants_grad(hidden, *ps):
        if hidden.shape[-1] == 512 and all(p.dim() and p.stride(-1) == 1 for p in ps) \
                and hp.in_features == npj.in_features == 512:
            out = grad.ProjectionsFn.apply(hidden, hp.weight, hp.bias, npj.weight, npj.bias)
        else:
            w, b = torch.cat([hp.weight, npj.weight]), torch.cat([hp.bias, npj.bias])  # differentiable
            out = grad.LinearFn.apply(hidden, w, b)
        return out[..., :h1], out[..., h1:n]
    return core.projections(hidden, hp, npj)


def decoder_synthesize(self, hidden, f0):
    """decoder.py:106-125, the synthesis section of DDSPDecoder.forward: controls -> harmonic + noise
    (+ reverb).  On the fused kernel (one launch for both synths, their controls, the sum and the
    returned control dicts) whenever the shapes are in its envelope: the reference's noise stream
    (``noise_mode = "torch"``: torch.rand(B, F, bs) drawn as modules.py:119-123 draws it, injected)
    or on-device Philox (``"device"``).  Outside the envelope the modules run one by one (still on the
    gfx950 kernels).  Works on this package's DDSPDecoder and, through install(), on the reference's.
    Returns (signal, harmonic, noise, harmonic_ctrls, noise_ctrls)."""
    hs, ns = self.harmonic_synth, self.noise_synth
    param, mags = decoder_projections(self, hidden)
    H, NB, bs = param.shape[-1] - 1, mags.shape[-1], int(hs.block_size)
    fused = (param.is_cuda and int(ns.block_size) == bs and param.shape[0] <= 65535
             and core.synth_frames_in_envelope(H, NB, bs, param.shape[0])
             and not _synth_overridden(hs, HarmonicSynth) and not _synth_overridden(ns, FilteredNoise))
    if fused:
        mode = getattr(ns, "noise_mode", "torch")
        if mode not in NOISE_MODES:
            raise ValueError(f"noise_mode must be one of {NOISE_MODES}")
        noise_in = FilteredNoise.draw_noise(ns, mags) if mode == "torch" else None
        signal, harmonic, noise, ctrl = core.synth_frames(
            f0, param, mags, bs, hs.sample_rate, bias=float(ns.initial_bias), noise=noise_in, parts=True,
            controls=True)
        harmonic_ctrls = {"f0": f0, "harmonic_distribution": ctrl["harmonic_distribution"],
                          "amplitudes": ctrl["amplitudes"]}
        noise_ctrls = {"magnitudes": ctrl["magnitudes"]}
    else:
        harmonic_ctrls = hs.get_controls(param[..., :1], param[..., 1:], f0)
        harmonic = hs(**harmonic_ctrls)
        noise_ctrls = ns.get_controls(mags)
        noise = ns(**noise_ctrls)
        signal = harmonic + noise
    if self.has_reverb:
        signal = self.reverb(signal)
    return signal, harmonic, noise, harmonic_ctrls, noise_ctrls


def decoder_forward(self, batch: dict):
    """decoder.py:101-136 DDSPDecoder.forward with the synthesis section fused (decoder_synthesize);
    install() binds it to the reference's DDSPDecoder."""
    f0, loudness = batch["pitch"], batch["loudness"]
    hidden = self.decoder(f0, loudness)
    signal, harmonic, noise, hc, nc = decoder_synthesize(self, hidden, f0)
    return {"f0": f0, "loudness": loudness, "signal": signal, "noise": noise,
            "harmonic_audio": harmonic, "noise_ctrls": nc, "harmonic_ctrls": hc}


class DDSPDecoder(nn.Module):
    """ddsp/models/decoder.py:70-136 with the synthesis on gfx950 kernels."""

    def __init__(self, hidden_size: int, n_harmonic: int, n_bands: int, sample_rate: int,
                 block_size: int, has_reverb: bool):
        super().__init__()
        self.register_buffer("sample_rate", torch.tensor(sample_rate))
        self.register_buffer("block_size", torch.tensor(block_size))
        self.decoder = GRUDecoder(hidden_size)
        self.harmonic_proj = nn.Linear(hidden_size, n_harmonic + 1)
        self.noise_proj = nn.Linear(hidden_size, n_bands)
        self.harmonic_synth = HarmonicSynth(block_size=block_size, sample_rate=sample_rate)
        self.noise_synth = FilteredNoise(block_size=block_size, window_size=n_bands)
        self.has_reverb = has_reverb
        self.reverb = Reverb(sample_rate, sample_rate)
        self.register_buffer("phase", torch.zeros(1))

    synthesize = decoder_synthesize
    forward = decoder_forward
