"""RealtimeGraph over a DDSPAutoencoder on gfx950 (ddsp_pytorch_amd/realtime.py): audio in, audio out for the
z-conditioned model.  The graph runs core.stream_analysis_mfcc (loudness, MFCC and, from audio, the pitch of the same
frames in one launch), the MFCC encoder with its GRU state carried in ``rt.encoder_state``, the decoder with z, the
projections and the synthesis.

fused=False replays the package's eager kernels, so every call equals, bit for bit, the same public calls made by
the test.  fused=True runs the network on ddsp_hip_dense_rows and the GRU step kernels (another fp32 summation
order) and is held to the bounds test_gpu_realtime.py holds the decoder to: audio RMS 1e-5 / max 1e-4, states and z
atol 1e-5."""
import functools

import pytest
import torch

import pitch_ref as pr
from conftest import rms

pytestmark = pytest.mark.gpu

SR, BS, N, K = 48000, 256, 1024, 5
R = N // BS
MEAN, STD, SEED = -6.5, 1.75, 99


@pytest.fixture(scope="module")
def dd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ddsp_pytorch_amd
    ddsp_pytorch_amd._lib.load()
    return ddsp_pytorch_amd


def make_model(dd, big=False, seed=0):
    torch.manual_seed(seed)
    m = (dd.DDSPAutoencoder(512, 64, 65, SR, BS, False) if big else dd.DDSPAutoencoder(64, 16, 9, SR, BS, False)).eval()
    with torch.no_grad():
        m.decoder.cache_gru.normal_(0, 0.1)
    return m.cuda()


@functools.lru_cache(maxsize=None)
def inputs():
    """(audio [1, K N] voiced, pitch [K][1, N, 1]) on the host, read-only."""
    audio = torch.from_numpy(pr.make_voiced(SR, K * N, 1, seed=41))
    g = torch.Generator().manual_seed(5)
    pitch = [80.0 * 10.0 ** torch.rand(1, N, 1, generator=g) for _ in range(K)]
    return audio, pitch


class Eager:
    """The same stream by the package's public calls, one call at a time."""

    def __init__(self, dd, model, continuous, pitch_from_audio):
        self.core, self.m, self.continuous, self.pfa = dd.core, model, continuous, pitch_from_audio
        dev = torch.device("cuda")
        self.stream = dd.core.StreamState(1, dev, N, 0) if continuous else None
        self.counter = self.stream.counter if continuous else torch.zeros(1, dtype=torch.int64, device=dev)
        self.analysis = dd.core.FeatureStreamState(1, dev, N, 2048, BS, counter=self.counter)
        self.enc = torch.zeros(1, 1, model.encoder.gru.hidden_size, device=dev)
        self.bias = float(model.noise_synth.initial_bias)

    def reset(self):
        self.m.decoder.cache_gru.zero_()
        self.enc.zero_()
        self.counter.zero_()
        self.analysis.reset()
        if self.stream is not None:
            self.stream.reset()

    @torch.no_grad()
    def __call__(self, audio, pitch):
        """-> dict of the call's audio, z, f0 [1, R], mfcc, param, mags."""
        from ddsp_pytorch_amd.decoder import gru_decoder_forward
        core, m = self.core, self.m
        got = core.stream_analysis_mfcc(audio, SR, BS, self.analysis, pitch=self.pfa, return_confidence=self.pfa)
        loud, mfcc = got[:2]
        f0 = got[2] if self.pfa else pitch[:, ::BS, 0].contiguous()
        x, h = core.gru(m.encoder.norm(mfcc), m.encoder.gru, self.enc)
        self.enc.copy_(h)
        z = m.encoder.proj(x)
        p = f0.view(1, -1, 1)
        ln = (loud.view(1, -1, 1) - MEAN) / STD
        hidden = gru_decoder_forward(m.decoder, p, ln, z, realtime=True)
        param, mags = m.harmonic_proj(hidden), m.noise_proj(hidden)
        if self.continuous:
            y = core.stream_synth_frames(p.contiguous(), param, mags, BS, float(SR), self.stream, SEED,
                                         bias=self.bias, wrap=True)
            core.stream_advance(self.stream, p.contiguous(), BS, float(SR), wrap=True)
        else:
            y = core.synth_frames_counter(p.contiguous(), param, mags, BS, float(SR), self.counter, SEED,
                                          bias=self.bias)
        return {"y": y, "z": z, "f0": f0, "mfcc": mfcc, "param": param, "mags": mags}


def graph(dd, model, continuous, pfa, **kw):
    from ddsp_pytorch_amd.realtime import RealtimeGraph
    return RealtimeGraph(model, N, MEAN, STD, seed=SEED, continuous=continuous, loudness_from_audio=True,
                         pitch_from_audio=pfa, **kw)


def call(rt, pfa, a, p, host=False):
    if host:
        y = rt(a.cpu()) if pfa else rt(p.cpu(), a.cpu())
        return y.cuda()
    return (rt(a) if pfa else rt(p, a)).clone()


@pytest.mark.parametrize("pfa", [True, False])
@pytest.mark.parametrize("continuous", [False, True])
def test_unfused_graph_equals_the_eager_calls(dd, continuous, pfa):
    audio, pitch = inputs()
    audio = audio.cuda()
    mg, me = make_model(dd), make_model(dd)
    rt = graph(dd, mg, continuous, pfa, fused=False)
    assert rt.autoencoder and rt.mfcc_delay_samples == rt.loudness_delay_samples == 768
    assert rt.encoder_state.shape == (1, 1, 64) and not rt.encoder_state.any()
    assert "encoder_state" not in mg.state_dict() and set(mg.state_dict()) == set(me.state_dict())
    assert torch.equal(mg.decoder.cache_gru, me.decoder.cache_gru)  # capture leaves the stream state untouched
    eg = Eager(dd, me, continuous, pfa)
    rounds = []
    for rnd in range(3):
        ys = []
        for k in range(K):
            a = audio[:, k * N:(k + 1) * N].reshape(1, N, 1)
            p = pitch[k].cuda()
            y = call(rt, pfa, a, p, host=rnd == 1)
            want = eg(a, p)
            assert y.shape == (1, N, 1) and bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
            assert torch.equal(y, want["y"]), (rnd, k)
            assert rt.z.shape == (1, R, 16) and torch.equal(rt.z, want["z"]), (rnd, k)
            if pfa:
                assert torch.equal(rt.f0, want["f0"]), (rnd, k)
            assert torch.equal(rt.encoder_state, eg.enc), (rnd, k)
            assert torch.equal(mg.decoder.cache_gru, me.decoder.cache_gru), (rnd, k)
            ys.append(y)
        assert float(rt.encoder_state.abs().max()) > 0
        rounds.append(torch.cat(ys, 1))
        rt.reset()
        eg.reset()
        assert not rt.encoder_state.any() and int(rt.counter.item()) == 0
    assert torch.equal(rounds[1], rounds[2])  # host input and device input: the same audio


@pytest.mark.parametrize("big,route", [(False, "steps"), (False, "persistent"), (True, "steps"), (True, "persistent")])
def test_fused_graph_matches_the_eager_calls(dd, big, route):
    """hidden 64: the decoder GRU's input projection has K = 192; hidden 512 with 64 harmonics and 65 bands: K = 1536,
    the 24-chunk dense_rows instantiation."""
    audio, pitch = inputs()
    audio = audio.cuda()
    mg, me = make_model(dd, big), make_model(dd, big)
    rt = graph(dd, mg, False, True, fused=True, gru_route=route)
    assert mg.decoder.gru.input_size == (1536 if big else 192)
    eg = Eager(dd, me, False, True)
    for k in range(K):
        a = audio[:, k * N:(k + 1) * N].reshape(1, N, 1)
        y = call(rt, True, a, None)
        want = eg(a, None)
        err = (y - want["y"]).abs()
        print(f"fused autoencoder hidden {512 if big else 64} {route} call {k}: audio rms "
              f"{rms(y.cpu().numpy(), want['y'].cpu().numpy()):.3e} max {float(err.max()):.3e}; z max "
              f"{float((rt.z - want['z']).abs().max()):.3e}; encoder state max "
              f"{float((rt.encoder_state - eg.enc).abs().max()):.3e}; cache_gru max "
              f"{float((mg.decoder.cache_gru - me.decoder.cache_gru).abs().max()):.3e}")
        assert rms(y.cpu().numpy(), want["y"].cpu().numpy()) <= 1e-5, k
        assert float(err.max()) <= 1e-4, k
        assert torch.equal(rt.f0, want["f0"]), k
        assert torch.allclose(rt.z, want["z"], atol=1e-5, rtol=0), k
        assert torch.allclose(rt.encoder_state, eg.enc, atol=1e-5, rtol=0), k
        assert torch.allclose(mg.decoder.cache_gru, me.decoder.cache_gru, atol=1e-5, rtol=0), k


@pytest.mark.parametrize("fused", [False, True])
def test_the_stream_carries_the_encoder(dd, fused):
    """The z of K calls, concatenated, is model.encoder run once, offline, on the concatenated streamed MFCC frames,
    and the last call's encoder_state is that pass's final state."""
    audio, _ = inputs()
    audio = audio.cuda()
    m = make_model(dd)
    rt = graph(dd, m, True, True, fused=fused)
    st = dd.core.FeatureStreamState(1, "cuda", N, 2048, BS)
    zs, mfccs = [], []
    for k in range(K):
        a = audio[:, k * N:(k + 1) * N].reshape(1, N, 1)
        rt(a)
        zs.append(rt.z.clone())
        mfccs.append(dd.core.stream_analysis_mfcc(a, SR, BS, st, pitch=False)[1])
        dd.core.stream_advance(st)
    mfcc = torch.cat(mfccs, 1)
    with torch.no_grad():
        want = m.encoder(mfcc)
        _, h = dd.core.gru(m.encoder.norm(mfcc), m.encoder.gru, None)
    got = torch.cat(zs, 1)
    assert got.shape == want.shape == (1, K * R, 16)
    print(f"encoder over the stream fused {fused}: z max {float((got - want).abs().max()):.3e}; state max "
          f"{float((rt.encoder_state - h).abs().max()):.3e}")
    assert torch.allclose(got, want, atol=1e-5, rtol=0)
    assert torch.allclose(rt.encoder_state, h, atol=1e-5, rtol=0)


def test_refusals(dd):
    from ddsp_pytorch_amd.realtime import RealtimeGraph
    for kw in ({}, {"pitch_from_audio": True}, {"continuous": True}):
        with pytest.raises(RuntimeError, match="needs loudness_from_audio=True"):
            RealtimeGraph(make_model(dd), N, **kw)
    with pytest.raises(RuntimeError, match="at most 8 frames"):
        RealtimeGraph(make_model(dd), 9 * BS, loudness_from_audio=True, pitch_from_audio=True, fused=True)
    a = torch.zeros(1, N, 1, device="cuda")
    rt = RealtimeGraph(make_model(dd), N, loudness_from_audio=True, pitch_from_audio=True)
    with pytest.raises(RuntimeError, match="one input"):
        rt(a, a)
    for shape in ((1, N), (1, N // 2, 1), (2, N, 1)):
        with pytest.raises(RuntimeError, match="audio must be"):
            rt(torch.zeros(*shape, device="cuda"))
        with pytest.raises(RuntimeError, match="audio must be"):
            rt(torch.zeros(*shape))
    rt = RealtimeGraph(make_model(dd), N, loudness_from_audio=True)
    with pytest.raises(RuntimeError, match="two inputs"):
        rt(a)
    for shape in ((1, N), (1, N // 2, 1), (2, N, 1)):
        with pytest.raises(RuntimeError, match="must be"):
            rt(torch.zeros(*shape, device="cuda"), torch.zeros(*shape, device="cuda"))
        with pytest.raises(RuntimeError, match="must be"):
            rt(a, torch.zeros(*shape))
