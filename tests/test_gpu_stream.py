"""The seamless realtime stream on the GPU (ddsp_hip_stream_*, core.StreamState, RealtimeGraph(continuous=True,
reverb=True), ScriptDDSP(streaming=True)): K calls of N samples render what one call of K N samples renders.
References: oracle/numpy_oracle.py and the fp64 stream models of tests/stream_ref.py (checked against the oracle
on the CPU by tests/test_stream_host.py)."""
import numpy as np
import pytest
import torch

from conftest import rms
from oracle import numpy_oracle as no
import stream_ref as sr

gpu = pytest.mark.gpu
SR = 48000.0
SYNTH_SHAPES = [(2, 32, 4, 16, 9, 12), (1, 256, 4, 64, 65, 6)]  # B, bs, R, H, NB, K (the second: config 3's call)
_inputs = {}


def _dev():
    return torch.device("cuda", 0)


def _synth_inputs(shape):
    """Inputs and CPU references of a synthesis stream, computed once per shape and never changed."""
    if shape not in _inputs:
        B, bs, R, H, NB, K = shape
        F = K * R
        rng = np.random.default_rng(1000 + bs + H)
        f0 = rng.uniform(50.0, 2000.0, (B, F, 1)).astype(np.float32)
        f0[0] = rng.uniform(1990.0, 2000.0, (F, 1)).astype(np.float32)  # item 0: omega passes 400 rad
        param = rng.standard_normal((B, F, H + 1)).astype(np.float32)
        mags = rng.standard_normal((B, F, NB)).astype(np.float32)
        noise = rng.uniform(-1.0, 1.0, (B, F, bs)).astype(np.float32)
        c = no.harmonic_get_controls(param[..., :1], param[..., 1:], f0, SR)
        oracle = no.harmonic_forward(c["amplitudes"], c["harmonic_distribution"], f0, bs, SR)[0][..., 0]
        amps = (c["harmonic_distribution"] * c["amplitudes"]).astype(np.float32)
        _inputs[shape] = dict(f0=f0, param=param, mags=mags, noise=noise, oracle=oracle, amps=amps)
    return _inputs[shape]


def _run_stream(shape, wrap, carry0=None, calls=None):
    """The stream through core, call by call -> (signal, harmonic, noise) [B, calls*R*bs] on the host, state."""
    from ddsp_pytorch_amd import core
    B, bs, R, H, NB, K = shape
    inp = _synth_inputs(shape)
    dev = _dev()
    t = {k: torch.from_numpy(inp[k]).to(dev) for k in ("f0", "param", "mags", "noise")}
    st = core.StreamState(B, dev)
    if carry0 is not None:
        st.carry.copy_(torch.as_tensor(carry0, dtype=torch.float64))
    outs = []
    for k in range(K if calls is None else calls):
        s = slice(k * R, (k + 1) * R)
        outs.append(core.stream_synth_frames(t["f0"][:, s], t["param"][:, s], t["mags"][:, s], bs, SR, st,
                                             noise=t["noise"][:, s], wrap=wrap, parts=True))
        core.stream_advance(st, t["f0"][:, s], bs, SR, wrap=wrap)
        assert int(st.counter.item()) == k + 1
    return tuple(torch.cat([o[i] for o in outs], 1)[..., 0].cpu() for i in range(3)), st


@gpu
@pytest.mark.parametrize("shape", SYNTH_SHAPES)
def test_stream_synthesis_chunked_equals_one_shot(shape):
    """T1, wrap=False, injected noise: K streamed calls against one launch over all K R frames."""
    from ddsp_pytorch_amd import core
    B, bs, R, H, NB, K = shape
    inp = _synth_inputs(shape)
    dev = _dev()
    (sig, harm, nz), st = _run_stream(shape, wrap=False)
    one = core._synth_frames_launch(*(torch.from_numpy(inp[k]).to(dev) for k in ("f0", "param", "mags")), bs, SR,
                                    -5.0, torch.from_numpy(inp["noise"]).to(dev), True, 0, 0)
    sig1, harm1, nz1 = (o[..., 0].cpu() for o in one)
    d_h = float((harm - harm1).abs().max())
    r_o = rms(harm.numpy(), inp["oracle"])
    print(f"T1 {shape}: noise equal {torch.equal(nz, nz1)}, harmonic max|d| {d_h:.3e}, rms vs oracle {r_o:.3e}")
    assert torch.equal(nz, nz1)          # frames are independent and run the same code
    assert d_h <= 1e-6
    assert r_o < 1e-6                    # the project's g1 bound
    assert float((sig - (harm + nz)).abs().max()) <= 1e-6
    # the carry is the exact fp64 phase of everything rendered
    inc = no.phase_increment(inp["f0"], SR)[..., 0].astype(np.float64)
    assert np.array_equal(st.carry.cpu().numpy(), bs * inc.sum(-1))


@gpu
@pytest.mark.parametrize("shape", SYNTH_SHAPES)
def test_stream_synthesis_wrapped_carry(shape):
    """T2, wrap=True: against the fp64 numpy model of the definition; the carry stays below 2 pi."""
    B, bs, R, H, NB, K = shape
    inp = _synth_inputs(shape)
    (_, harm, _), st = _run_stream(shape, wrap=True)
    ref, carry, _ = sr.harmonic_stream(inp["amps"], inp["f0"], bs, SR, R, wrap=True)
    r = rms(harm.numpy(), ref)
    c = st.carry.cpu().numpy()
    print(f"T2 {shape}: rms vs wrapped model {r:.3e}, carry {c}, model {carry}")
    assert r < 1e-6
    assert np.all(c >= 0) and np.all(c < 2 * np.pi) and np.abs(c - carry).max() < 1e-9


@gpu
def test_stream_wrap_makes_the_carry_shift_invariant():
    """T2: streams preset to c and c + 2 pi 10^6 agree with wrap (the carry is reduced before use) and differ
    without it (omega = fl32(6.28e6 + ...) has an ulp of 0.5 rad) — why wrap is the realtime default."""
    shape = SYNTH_SHAPES[0]
    c = np.array([1.0, 2.5])
    big = c + 2 * np.pi * 1e6
    (_, a, _), _ = _run_stream(shape, True, c, calls=1)
    (_, b, _), _ = _run_stream(shape, True, big, calls=1)
    (_, a0, _), _ = _run_stream(shape, False, c, calls=1)
    (_, b0, _), _ = _run_stream(shape, False, big, calls=1)
    print(f"T2 shift: wrapped rms {rms(a.numpy(), b.numpy()):.3e}, unwrapped rms {rms(a0.numpy(), b0.numpy()):.3e}")
    assert rms(a.numpy(), b.numpy()) <= 1e-6
    assert rms(a0.numpy(), b0.numpy()) > 1e-3


@gpu
@pytest.mark.parametrize("N,L,K,B", [(128, 1000, 12, 2), (64, 192, 8, 1), (2048, 300, 3, 1), (1024, 48000, 50, 1),
                                     (256, 700, 5, 1), (512, 1500, 5, 2)])
def test_stream_reverb_matches_fp64_convolution(N, L, K, B):
    """T3: the K calls laid end to end against numpy_oracle.reverb on the whole input (ragged last partition,
    ring wrap and per-item state; L a multiple of N; P = 1; the real size with 47 partitions; N = 256 and 512, so
    that every transform size the dispatch can take runs)."""
    from ddsp_pytorch_amd import core
    dev = _dev()
    rng = np.random.default_rng(N + L)
    x = (rng.standard_normal((B, K * N, 1)) * 0.3).astype(np.float32)
    h = (rng.standard_normal(L) * np.exp(-np.arange(L) / 8000.0)).astype(np.float32)
    h[0] = 1.0
    ref = no.reverb(x, h)
    scale = float(np.sqrt(np.mean(ref.astype(np.float64) ** 2)))
    xd = torch.from_numpy(x).to(dev)
    spec = core.stream_spectrum(torch.from_numpy(h).to(dev), N)
    st = core.StreamState(B, dev, N, L)

    def run():
        ys = []
        for k in range(K):
            ys.append(core.stream_reverb(xd[:, k * N:(k + 1) * N], spec, st))
            core.stream_advance(st)
        return torch.cat(ys, 1).cpu()
    y = run()
    assert int(st.counter.item()) == K
    err = rms(y.numpy(), ref)
    print(f"T3 N={N} L={L} K={K} B={B}: rms {err:.3e} = {err / scale:.3e} x rms(ref)")
    assert y.shape == (B, K * N, 1)
    assert err < 1e-6 * scale, (err, scale)
    st.reset()
    assert int(st.counter.item()) == 0 and not bool(st.buf.any())
    assert torch.equal(run(), y)
    # in place (y = x): the same samples
    st.reset()
    xi = xd[:, :N].contiguous()
    assert core.stream_reverb(xi, spec, st, out=xi) is xi
    assert torch.equal(xi.cpu(), y[:, :N])


@gpu
def test_stream_reverb_refuses_before_launching():
    """T3: call sizes outside the range and a state one byte short: the status, and nothing was launched (the
    output and the state are untouched)."""
    from ddsp_pytorch_amd import _lib, core
    lib = _lib.load()
    dev = _dev()
    L = 1000
    for N, status in ((96, 5), (4096, 5), (128, 4)):
        x = torch.randn(1, N, device=dev)
        y = torch.full((1, N), 7.0, device=dev)
        nbytes = int(lib.ddsp_hip_stream_state_bytes(1, 128, L))
        state = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        spec = torch.ones(int(lib.ddsp_hip_stream_spectrum_floats(128, L)), device=dev)
        counter = torch.zeros(1, dtype=torch.int64, device=dev)
        given = nbytes - 1 if status == 4 else nbytes
        st = lib.ddsp_hip_stream_reverb(_lib.ptr(x), _lib.ptr(spec), spec.numel(), _lib.ptr(counter), _lib.ptr(state),
                                        given, _lib.ptr(y), 1, N, L, _lib.stream_of(x))
        torch.cuda.synchronize()
        assert st == status, (N, st)
        assert bool((y == 7.0).all()) and not bool(state.any())
        imp = torch.zeros(L, device=dev)
        assert lib.ddsp_hip_stream_spectrum(_lib.ptr(imp), L, N, _lib.ptr(spec), spec.numel(),
                                            _lib.stream_of(x)) == (0 if N == 128 else 5)
    with pytest.raises(RuntimeError):
        core.StreamState(1, dev, 96, L)
    with pytest.raises(RuntimeError):
        core.stream_spectrum(torch.zeros(L, device=dev), 4096)


# ---------------------------------------------------------------- RealtimeGraph and the exported graph
BS, H, NB, N = 256, 64, 65, 1024  # tests/test_gpu_realtime.py's model shape


def _model(hidden=512, seed=0, reverb_length=4800):
    import ddsp_pytorch_amd as dd
    torch.manual_seed(seed)
    m = dd.DDSPDecoder(hidden, H, NB, 48000, BS, False)
    m.reverb = dd.Reverb(reverb_length, 48000)
    m = m.eval()
    with torch.no_grad():  # a non-zero initial stream state
        m.decoder.cache_gru.normal_(0, 0.1)
    return m


def _calls(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        pitch = 80.0 * 10.0 ** torch.rand(1, N, 1, generator=g)
        loud = torch.randn(1, N, 1, generator=g) - 2.0
        out.append((pitch, loud))
    return out


def _network(m, pitch, loud, mean, std):
    """export.py:33-40 up to the projections, run eagerly -> (f0 [1,R,1], param, mags)."""
    from ddsp_pytorch_amd.decoder import gru_decoder_forward
    p = pitch[:, ::BS].contiguous()
    l = (loud[:, ::BS] - mean) / std
    hidden = gru_decoder_forward(m.decoder, p, l, None, realtime=True)
    return p, m.harmonic_proj(hidden), m.noise_proj(hidden)


@gpu
def test_realtime_graph_continuous_with_reverb_matches_eager_stream():
    """T4: graph replays of RealtimeGraph(continuous=True, reverb=True) against the same stream run eagerly through
    core, call for call (the fused control network's bounds); the pre-reverb harmonic part of all 8 calls against
    the oracle on the concatenated controls.  The oracle rounds the unwrapped omega to fp32 by contract, so it is
    the reference of the stream with wrap=False; the graph's wrapped stream (the default) is held to the same
    bound against the wrapped definition (stream_ref.harmonic_stream)."""
    from ddsp_pytorch_amd import core
    from ddsp_pytorch_amd.realtime import RealtimeGraph
    dev = _dev()
    mean, std, seed, K = -3.0, 1.5, 77, 8
    mg, me = _model().to(dev), _model().to(dev)
    rt = RealtimeGraph(mg, N, mean, std, seed=seed, continuous=True, reverb=True)
    assert rt.wrap and int(rt.counter.item()) == 0 and not bool(rt.stream.buf.any())
    L = int(me.reverb.length)
    st = core.StreamState(1, dev, N, L)
    st_nowrap = core.StreamState(1, dev)
    f0s, params, harm_w, harm_u = [], [], [], []
    with torch.no_grad():
        spec = core.stream_spectrum(me.reverb.build_impulse(), N)
        for k, (pitch, loud) in enumerate(_calls(K)):
            y = rt(pitch, loud).clone()
            p, param, mags = _network(me, pitch.to(dev), loud.to(dev), mean, std)
            sig, harm, _ = core.stream_synth_frames(p, param, mags, BS, SR, st, seed, parts=True)
            ye = core.stream_reverb(sig, spec, st).cpu()
            core.stream_advance(st, p, BS, SR)
            hu = core.stream_synth_frames(p, param, mags, BS, SR, st_nowrap, seed, wrap=False, parts=True)[1]
            core.stream_advance(st_nowrap, p, BS, SR, wrap=False)
            r, d = rms(y.numpy(), ye.numpy()), float((y - ye).abs().max())
            print(f"T4 call {k}: rms {r:.3e} max {d:.3e}")
            assert y.shape == (1, N, 1) and not y.is_cuda
            assert r <= 1e-5 and d <= 1e-4, k
            assert torch.allclose(mg.decoder.cache_gru, me.decoder.cache_gru, atol=1e-5)
            f0s.append(p.cpu().numpy()), params.append(param.cpu().numpy())
            harm_w.append(harm.cpu().numpy()[..., 0]), harm_u.append(hu.cpu().numpy()[..., 0])
        assert int(rt.counter.item()) == K
        assert torch.allclose(rt.stream.carry, st.carry, atol=1e-9)
    f0, param = np.concatenate(f0s, 1), np.concatenate(params, 1)
    c = no.harmonic_get_controls(param[..., :1], param[..., 1:], f0, SR)
    oracle = no.harmonic_forward(c["amplitudes"], c["harmonic_distribution"], f0, BS, SR)[0][..., 0]
    model = sr.harmonic_stream(c["harmonic_distribution"] * c["amplitudes"], f0, BS, SR, N // BS, wrap=True)[0]
    r_u, r_w = rms(np.concatenate(harm_u, 1), oracle), rms(np.concatenate(harm_w, 1), model)
    print(f"T4 harmonic: unwrapped vs oracle {r_u:.3e}, wrapped vs wrapped model {r_w:.3e}")
    assert r_u < 1e-6
    assert r_w < 1e-6
    # reset: a fresh stream
    rt.reset()
    assert int(rt.counter.item()) == 0 and not bool(rt.stream.buf.any())


@gpu
def test_realtime_graph_continuous_arguments():
    from ddsp_pytorch_amd.realtime import RealtimeGraph
    dev = _dev()
    with pytest.raises(RuntimeError, match="continuous"):
        RealtimeGraph(_model().to(dev), N, reverb=True)
    with pytest.raises(RuntimeError, match="power-of-two"):
        RealtimeGraph(_model().to(dev), 768, continuous=True, reverb=True)  # 3 frames: not a power of two


@gpu
def test_realtime_graph_defaults_still_stateless():
    """T4: RealtimeGraph with default arguments still equals the stateless eager calls (noise offset = call
    index, every call from phase zero)."""
    from ddsp_pytorch_amd import core
    from ddsp_pytorch_amd.realtime import RealtimeGraph
    dev = _dev()
    mean, std, seed = -3.0, 1.5, 77
    mg, me = _model().to(dev), _model().to(dev)
    rt = RealtimeGraph(mg, N, mean, std, seed=seed)
    assert rt.stream is None and not rt.continuous and not rt.wrap
    with torch.no_grad():
        for k, (pitch, loud) in enumerate(_calls(3)):
            y = rt(pitch, loud).clone()
            p, param, mags = _network(me, pitch.to(dev), loud.to(dev), mean, std)
            ye = core._synth_frames_launch(p, param, mags, BS, SR, -5.0, None, False, seed, k).cpu()
            assert rms(y.numpy(), ye.numpy()) <= 1e-5, k
            assert float((y - ye).abs().max()) <= 1e-4, k


@gpu
@pytest.mark.parametrize("reverb", [False, True])
def test_exported_streaming_graph_matches_realtime_graph(tmp_path, reverb):
    """T5: the exported streaming=True graph, loaded with torch.jit.load, against
    RealtimeGraph(continuous=True, fused=False): device noise, the same seed, max |d| <= 1e-6; reset_stream()
    against reset().  With the streamed reverb in the exported graph (stream_reverb=True) its output must be, bit
    for bit, the dry exported graph's output sent through core.stream_reverb (the same kernel on the same samples),
    and it is held against RealtimeGraph(reverb=True) too: the reverb is linear, so the two dry signals' 1e-6
    becomes at most 1e-6 x sum|h| behind it (the reverb's own rounding, 2.5e-7 relative, is far below that)."""
    from ddsp_pytorch_amd import core
    from ddsp_pytorch_amd.realtime import RealtimeGraph
    from ddsp_pytorch_amd.script import export
    dev = _dev()
    mean, std = -3.0, 1.5
    mg, me = _model().to(dev), _model().to(dev)
    path, dry_path = str(tmp_path / "stream.ts"), str(tmp_path / "dry.ts")
    bound = 1e-6
    with torch.no_grad():
        export(me, path, mean, std, realtime=True, noise_mode="device", streaming=True, stream_reverb=reverb,
               call_samples=N)
        if reverb:
            export(me, dry_path, mean, std, realtime=True, noise_mode="device", streaming=True, call_samples=N)
            dry = torch.jit.load(dry_path, map_location=dev)
            imp = me.reverb.build_impulse()
            spec, st = core.stream_spectrum(imp, N), core.StreamState(1, dev, N, int(me.reverb.length))
            bound = 1e-6 * float(imp.abs().sum())
            assert torch.equal(torch.ops.ddsp_hip.stream_spectrum(imp, N), spec)  # the op the C++ host has
    loaded = torch.jit.load(path, map_location=dev)
    rt = RealtimeGraph(mg, N, mean, std, fused=False, continuous=True, reverb=reverb)
    with torch.no_grad():
        for k, (pitch, loud) in enumerate(_calls(4)):
            y = rt(pitch, loud).clone()
            ys = loaded(pitch.to(dev), loud.to(dev))
            if reverb:
                yd = core.stream_reverb(dry(pitch.to(dev), loud.to(dev)), spec, st)
                core.stream_advance(st)
                assert torch.equal(ys, yd), k
            d = float((y - ys.cpu()).abs().max())
            print(f"T5 reverb={reverb} call {k}: max|d| {d:.3e} (bound {bound:.3e})")
            assert ys.shape == (1, N, 1)
            assert d <= bound, k
    assert int(loaded.ddsp.stream_counter.item()) == 4
    # a fresh stream on both sides renders the first call again
    pitch, loud = _calls(1)[0]
    with torch.no_grad():
        first = []
        for _ in range(2):
            loaded.reset_stream()
            loaded.ddsp.decoder.cache_gru.zero_()
            assert int(loaded.ddsp.stream_counter.item()) == 0 and not bool(loaded.ddsp.stream_state.any())
            first.append(loaded(pitch.to(dev), loud.to(dev)).cpu())
        assert torch.equal(first[0], first[1])
        rt.reset()
        assert float((rt(pitch, loud) - first[0]).abs().max()) <= bound
    with pytest.raises(Exception, match="batch 1"):
        loaded(pitch.to(dev).repeat(2, 1, 1), loud.to(dev).repeat(2, 1, 1))
