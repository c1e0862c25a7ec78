"""Which C-ABI entry points the control network (the three MLPs, the GRU, the two projections) launches, and in
which order, on every route: the kernels at inference, the Functions under autograd, each ERANGE fallback, the
module calls when somebody observes a module or the dtype is not the kernels', and RealtimeGraph's capture.

The expected sequences (EXPECTED) are literal: they were recorded by running these same bodies (the ``run_*``
functions) on the commit before decoder.mlp_route existed, so they pin the routes that commit took (DESIGN.md,
"Control network: one route per layer").  Shapes are the smallest that reach every route: batch 2 x 8 frames,
block size 256, 20 harmonics, 17 bands."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

SR, BS, HARM, BANDS = 48000, 256, 20, 17
# the network's entry points (the synthesis, reverb and loss have traces of their own in their tests)
BLOCK, LIN, DW, DENSE = "mlp_block", "linear", "linear_weight_grad", "dense_rows"
LN, LN_B = "layer_norm_leaky_relu", "layer_norm_leaky_relu_backward"
PROJ, STACK = "projections", "stack_rows"
GRU_P, GRU_S, GRU_BP, GRU_BS = "gru_forward_persistent", "gru_forward", "gru_backward_persistent", "gru_backward"
NETWORK = (BLOCK, LIN, DW, DENSE, LN, LN_B, PROJ, STACK, GRU_P, GRU_S, GRU_BP, GRU_BS)
CAT = "torch.cat"


@pytest.fixture(scope="module")
def dd():
    import ddsp_pytorch_amd
    return ddsp_pytorch_amd


@contextlib.contextmanager
def traced(count_cat=False):
    """The network entry points called inside the block, in order (with ``count_cat``: and "torch.cat" for every
    concatenation made from Python)."""
    from ddsp_pytorch_amd import _lib
    names, real, cat = [], _lib.call, torch.cat

    def call(name, *a, **k):
        if name in NETWORK:
            names.append(name)
        return real(name, *a, **k)

    def spy_cat(*a, **k):
        names.append(CAT)
        return cat(*a, **k)

    _lib.call = call
    if count_cat:
        torch.cat = spy_cat
    try:
        yield names
    finally:
        _lib.call, torch.cat = real, cat


def batch():
    g = torch.Generator().manual_seed(3)
    return {"pitch": (50.0 * 20.0 ** torch.rand(2, 8, 1, generator=g)).cuda(),
            "loudness": torch.randn(2, 8, 1, generator=g).cuda()}


def model(dd, hidden, train=False):
    torch.manual_seed(0)
    return dd.DDSPDecoder(hidden, HARM, BANDS, SR, BS, False).cuda().train(train)


def run_inference(m):
    """-> (trace, {"signal": ...}) of one no_grad forward."""
    with traced() as t, torch.no_grad():
        torch.manual_seed(7)
        out = m(batch())
    return list(t), {"signal": out["signal"]}


def run_training(m):
    """-> (trace, signal and every parameter gradient) of one forward + backward."""
    with traced() as t:
        torch.manual_seed(7)
        out = m(batch())
        out["signal"].pow(2).mean().backward()
    res = {"signal": out["signal"].detach()}
    res.update({"d" + k: p.grad for k, p in m.named_parameters() if p.grad is not None})
    return list(t), res


def run_gru_decoder(dd, hook=False):
    """GRUDecoder(512, z_dim=16) at inference -> (trace with the concatenations, output, hook calls)."""
    torch.manual_seed(0)
    dec = dd.decoder.GRUDecoder(512, z_dim=16).cuda().eval()
    b = batch()
    z = torch.randn(2, 8, 16, generator=torch.Generator().manual_seed(5)).cuda()
    seen = []
    h = dec.f0_mlp[0].register_forward_hook(lambda mod, i, o: seen.append(tuple(o.shape))) if hook else None
    try:
        with traced(count_cat=True) as t, torch.no_grad():
            y = dec(b["pitch"], b["loudness"], z)
    finally:
        if h is not None:
            h.remove()
    return list(t), y, seen


def run_other_dtype(dd, setting):
    """The network alone (decoder + projections) at inference under bf16 autocast or as a .half() model."""
    m = model(dd, 512)
    b = batch()
    f0, lo = b["pitch"], b["loudness"]
    if setting == "half":
        m, f0, lo = m.half(), f0.half(), lo.half()
    ctx = torch.autocast("cuda", dtype=torch.bfloat16) if setting == "autocast" else contextlib.nullcontext()
    with traced() as t, torch.no_grad(), ctx:
        hidden = m.decoder(f0, lo)
        p, n = dd.decoder.decoder_projections(m, hidden)
    return list(t), (hidden.dtype, p.dtype, n.dtype)


def outcome(fn):
    """("returns", dtype) or ("raises", exception type name) of fn()."""
    try:
        return ("returns", str(fn().dtype))
    except Exception as e:  # noqa: BLE001 (the type is the result)
        return ("raises", type(e).__name__)


def run_fp64_extra(dd, grad, double_model=False):
    """mlp_forward(out_mlp, x, extras=(f0, loudness.double())) -> (trace, outcome, outcome of the module chain on
    the concatenation)."""
    torch.manual_seed(2)
    seq = dd.decoder.mlp(514, 512, 3).cuda()
    if double_model:
        seq = seq.double()
    b = batch()
    x = torch.randn(2, 8, 512, device="cuda")
    extras = (b["pitch"], b["loudness"].double())
    with traced() as t, torch.set_grad_enabled(grad):
        got = outcome(lambda: dd.decoder.mlp_forward(seq, x, extras=extras))
        ref = outcome(lambda: seq(torch.cat([x, *extras], -1)))
    return list(t), got, ref


def run_realtime(dd, route):
    """-> (trace of RealtimeGraph's construction: one warm-up forward and the captured one, gru_route_taken)."""
    from ddsp_pytorch_amd.realtime import RealtimeGraph
    m = model(dd, 512)
    with traced() as t:
        rt = RealtimeGraph(m, call_samples=4 * BS, warmup=1, gru_route=route)
    return list(t), rt.gru_route_taken


# ------------------------------------------------------------------------------------------ the recorded routes
EXPECTED = {
    # hidden 512, inference: each input MLP's K = 1 block in the LayerNorm kernel and two block launches, the GRU's
    # input projection and its persistent recurrence, the out_mlp's three block launches, one projections launch
    "infer512": [LN, BLOCK, BLOCK, LN, BLOCK, BLOCK, LIN, GRU_P, BLOCK, BLOCK, BLOCK, PROJ],
    # hidden 512, forward + backward: LinearFn / LNLeakyFn per block (the K = 1 Linears are torch's), GRUFn,
    # ProjectionsFn; then their backwards, last layer first
    "train512": [LN, LIN, LN, LIN, LN, LN, LIN, LN, LIN, LN, LIN, GRU_P, LIN, LN, LIN, LN, LIN, LN, PROJ,
                 DW, LN_B, LIN, DW, LN_B, LIN, DW, LN_B, LIN, DW, GRU_BP, LIN, DW, DW,
                 LN_B, LIN, DW, LN_B, LIN, DW, LN_B, LN_B, LIN, DW, LN_B, LIN, DW, LN_B],
    # hidden 64: every launch below answers ERANGE and its fallback runs — the LayerNorm kernel (torch's modules),
    # the linear kernel (addmm), the persistent GRU (the step kernels), the projections (stack_rows + one GEMM;
    # under autograd LinearFn over the concatenated parameters)
    "infer64": [LN, LN, LN, LN, LN, LN, LN, LN, LIN, GRU_P, GRU_S, LN, LN, LN, PROJ, STACK],
    "train64": [LIN, LIN, LIN, LIN, LIN, GRU_P, GRU_S, LIN, LIN, LIN, LIN,
                LIN, DW, LIN, DW, LIN, DW, LIN, DW, GRU_BP, GRU_BS, LIN, DW, DW, LIN, DW, LIN, DW, LIN, DW, LIN, DW],
    # GRUDecoder(512, z_dim=16): three input MLPs, no concatenation (each writes its slice of the GRU input)
    "gru_decoder": [LN, BLOCK, BLOCK, LN, BLOCK, BLOCK, BLOCK, BLOCK, BLOCK, LIN, GRU_P, BLOCK, BLOCK, BLOCK],
    # the same with a forward hook on f0_mlp[0]: that MLP is module calls, the GRU input is concatenated
    "gru_decoder_hooked": [LN, BLOCK, BLOCK, BLOCK, BLOCK, BLOCK, CAT, LIN, GRU_P, BLOCK, BLOCK, BLOCK],
    "hooked_model": [LN, BLOCK, BLOCK, LIN, GRU_P, BLOCK, BLOCK, BLOCK, PROJ],
    # RealtimeGraph's construction: one warm-up forward and the captured one
    "realtime_steps": 2 * [DENSE, DENSE, DENSE, GRU_S, DENSE, DENSE, DENSE, DENSE],
    "realtime_persistent": 2 * [DENSE, DENSE, DENSE, GRU_P, DENSE, DENSE, DENSE, DENSE],
}


@pytest.mark.parametrize("hidden", [512, 64])
def test_inference_routes(dd, hidden):
    trace, res = run_inference(model(dd, hidden))
    assert trace == EXPECTED[f"infer{hidden}"], trace
    assert bool(torch.isfinite(res["signal"]).all())


@pytest.mark.parametrize("hidden", [512, 64])
def test_training_routes(dd, hidden):
    m = model(dd, hidden, train=True)
    trace, res = run_training(m)
    assert trace == EXPECTED[f"train{hidden}"], trace
    assert all(bool(torch.isfinite(v).all()) for v in res.values())
    # every parameter of the network has its gradient (the reverb is off in this model)
    assert {k for k, _ in m.named_parameters() if not k.startswith("reverb.")} == {k[1:] for k in res if k != "signal"}


def test_three_input_mlps_fill_one_buffer(dd):
    trace, y, seen = run_gru_decoder(dd)
    assert trace == EXPECTED["gru_decoder"], trace
    assert y.shape == (2, 8, 512) and not seen


def test_hooked_mlp_keeps_its_module_calls(dd):
    """A forward hook on f0_mlp[0]: that MLP runs as modules (the hook fires), the others stay on the kernels, the
    GRU input is concatenated; the values are the unhooked run's (the bounds of
    test_gpu_decoder_route.test_hooked_synth_module_keeps_module_calls)."""
    from ddsp_pytorch_amd.decoder import mlp_route
    trace, y, seen = run_gru_decoder(dd, hook=True)
    assert trace == EXPECTED["gru_decoder_hooked"], trace
    assert seen == [(2, 8, 512)]
    torch.testing.assert_close(y, run_gru_decoder(dd)[1], rtol=1e-5, atol=2e-6)
    m = model(dd, 512)
    plain = run_inference(m)[1]["signal"]
    fired = []
    h = m.decoder.f0_mlp[0].register_forward_hook(lambda mod, i, o: fired.append(1))
    try:
        with torch.no_grad():
            assert mlp_route(m.decoder.f0_mlp, batch()["pitch"]) == "modules"
            assert mlp_route(m.decoder.loudness_mlp, batch()["loudness"]) == "kernels"
        trace, hooked = run_inference(m)
    finally:
        h.remove()
    assert trace == EXPECTED["hooked_model"], trace
    assert len(fired) == 1
    torch.testing.assert_close(hooked["signal"], plain, rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("setting", ["autocast", "half"])
def test_other_dtypes_run_the_modules(dd, setting):
    trace, dtypes = run_other_dtype(dd, setting)
    assert trace == []
    low = torch.bfloat16 if setting == "autocast" else torch.float16
    # (inside an autocast region layer_norm computes in fp32: the decoder's output, an MLP block's, is fp32)
    assert dtypes == ((torch.float32 if setting == "autocast" else low), low, low)


def test_fp64_extra(dd):
    """An fp64 ``extras`` tensor.  Under autograd the concatenated input is fp64, so the call is the module chain
    on it: torch's own dtype error with the fp32 MLP (no kernel was tried), an fp64 result with an fp64 one.  At
    inference the kernels' TypeError (core._dev), as for any non-fp32 tensor handed to them."""
    from ddsp_pytorch_amd.decoder import mlp, mlp_route
    trace, got, ref = run_fp64_extra(dd, grad=True)
    assert trace == [] and got == ref == ("raises", "RuntimeError")
    trace, got, ref = run_fp64_extra(dd, grad=True, double_model=True)
    assert trace == [] and got == ref == ("returns", "torch.float64")
    trace, got, _ = run_fp64_extra(dd, grad=False)
    assert trace == [] and got == ("raises", "TypeError")
    seq, b = mlp(514, 512, 3).cuda(), batch()
    x, extras = torch.randn(2, 8, 512, device="cuda"), (b["pitch"], b["loudness"].double())
    assert mlp_route(seq, x, extras) == "modules" and mlp_route(seq, x, (b["pitch"], b["loudness"])) == "autograd"
    with torch.no_grad():
        assert mlp_route(seq, x, extras) == "kernels"


@pytest.mark.parametrize("route", ["steps", "persistent"])
def test_realtime_graph_routes(dd, route):
    trace, taken = run_realtime(dd, route)
    assert trace == EXPECTED["realtime_" + route], trace
    assert taken == route
    assert (GRU_P in trace) == (route == "persistent")
