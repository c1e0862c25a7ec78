"""RealtimeGraph(pitch_from_audio=True, pitch_viterbi=True) on gfx950: the graph's f0 is the streamed Viterbi decode's
(features.StreamAnalyzer(viterbi=True)'s, bit for bit, call by call), for the decoder and for the autoencoder; the
defaults leave the graph's per-frame route as it was."""
import numpy as np
import pytest
import torch

import stream_viterbi_cases as sc
import viterbi_cases as vc

pytestmark = pytest.mark.gpu

BS, N, K = 256, 1024, 12
R = N // BS


@pytest.fixture(scope="module")
def dd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ddsp_pytorch_amd
    ddsp_pytorch_amd._lib.load()
    return ddsp_pytorch_amd


def _model(dd, autoencoder, seed=0):
    torch.manual_seed(seed)
    cls = dd.DDSPAutoencoder if autoencoder else dd.DDSPDecoder
    m = cls(64, 16, 9, vc.SR, BS, False).eval()
    with torch.no_grad():
        m.decoder.cache_gru.normal_(0, 0.1)
    return m.cuda()


def _calls():
    x = torch.from_numpy(np.array(sc.audio("octave"))).cuda()
    return [x[:, k * N:(k + 1) * N].reshape(1, N, 1) for k in range(K)]


@pytest.mark.parametrize("autoencoder,continuous,lag,fused", [(False, False, 0, True), (False, True, 3, True),
                                                              (True, False, 2, True), (False, False, 1, False),
                                                              (True, True, 0, False)])
def test_graph_f0_is_the_decoded_one(dd, autoencoder, continuous, lag, fused):
    from ddsp_pytorch_amd.realtime import RealtimeGraph
    rt = RealtimeGraph(_model(dd, autoencoder), N, -6.5, 1.75, seed=99, continuous=continuous, reverb=continuous,
                       fused=fused, loudness_from_audio=True, pitch_from_audio=True, pitch_viterbi=True, pitch_lag=lag)
    assert rt.loudness_delay_samples == 768 and rt.pitch_delay_samples == 768 + lag * BS
    assert rt.viterbi.lag == lag and rt.viterbi.counter is rt.counter and rt.pitch_ring.counter is rt.counter
    an = dd.features.StreamAnalyzer(vc.SR, BS, N, pitch=True, viterbi=True, pitch_lag=lag, aligned=autoencoder)
    runs = []
    for rnd in range(3):
        ys, f0s = [], []
        for k, a in enumerate(_calls()):
            y = rt(a).clone()
            feats = an(a)
            assert y.shape == (1, N, 1) and bool(torch.isfinite(y).all()), (rnd, k)
            assert rt.f0.shape == rt.confidence.shape == (1, R)
            assert torch.equal(rt.f0, feats["pitch"][..., 0]), (rnd, k)
            assert torch.equal(rt.confidence, feats["confidence"][..., 0]), (rnd, k)
            ys.append(y)
            f0s.append(rt.f0.clone())
        assert int(rt.counter.item()) == K
        runs.append((torch.cat(ys, 1), torch.cat(f0s, 1)))
        rt.reset()
        an.reset()
        assert int(rt.counter.item()) == 0 and not rt.viterbi.buf.any() and not rt.pitch_ring.buf.any()
    # reset() gives a fresh decode: the f0 track repeats itself (the audio too once the GRU state the model came with
    # is gone, i.e. between two runs that both follow a reset — the first run started from that state)
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[1][1], runs[2][1])
    assert torch.equal(runs[1][0], runs[2][0])
    assert float(runs[0][0].abs().max()) > 0


def test_without_pitch_viterbi_the_graph_is_the_per_frame_route(dd):
    from ddsp_pytorch_amd.realtime import RealtimeGraph
    rt = RealtimeGraph(_model(dd, False), N, loudness_from_audio=True, pitch_from_audio=True, pitch_viterbi=False)
    assert rt.viterbi is None and rt.pitch_ring is None and rt.pitch_delay_samples == rt.loudness_delay_samples
    state = dd.core.FeatureStreamState(1, "cuda", N, 2048, BS)
    for k, a in enumerate(_calls()):
        rt(a)
        _, f0, conf = dd.core.stream_analysis(a, vc.SR, BS, state, return_confidence=True)
        dd.core.stream_advance(state)
        assert torch.equal(rt.f0, f0) and torch.equal(rt.confidence, conf), k
    with pytest.raises(RuntimeError, match="needs pitch_from_audio=True"):
        RealtimeGraph(_model(dd, False), N, loudness_from_audio=True, pitch_viterbi=True)
