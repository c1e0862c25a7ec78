"""CPU checks of the analysis features' yardstick and host layer (no launch): tests/features_ref.py is tied to
independent sources (torch.stft, scipy's window and DCT, the A-weighting curve's published values), the host
table builders of ddsp_pytorch_amd.core agree with it, and ddsp_hip_loudness / ddsp_hip_mfcc answer their
envelope (include/ddsp_hip.h) with status codes before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch

import features_ref as fr


@pytest.mark.parametrize("n_fft,hop,T", [(1024, 512, 2560), (2048, 160, 2080), (64, 24, 1000), (16, 5, 101)])
def test_stft_matches_torch(n_fft, hop, T):
    x = np.random.default_rng(n_fft + hop).standard_normal(T)
    ref = torch.stft(torch.from_numpy(x), n_fft, hop, n_fft, torch.hann_window(n_fft, dtype=torch.float64),
                     center=True, pad_mode="reflect", normalized=False, return_complex=True).numpy().T
    got = fr.stft(x, n_fft, hop)
    assert got.shape == ref.shape == (1 + T // hop, n_fft // 2 + 1)
    assert np.abs(got - ref).max() <= 1e-10


def test_hann_and_dct_match_scipy():
    signal = pytest.importorskip("scipy.signal")
    fft = pytest.importorskip("scipy.fft")
    for n in (16, 1024, 2048):
        assert np.abs(fr.hann(n) - signal.get_window("hann", n, fftbins=True)).max() <= 1e-15
    for n_mfcc, n_mels in ((30, 128), (7, 7), (1, 40)):
        ref = fft.dct(np.eye(n_mels), type=2, norm="ortho", axis=0)[:n_mfcc]
        assert np.abs(fr.dct_matrix(n_mfcc, n_mels) - ref).max() <= 1e-14


def test_a_weighting_values():
    w = fr.a_weighting([0.0, 100.0, 1000.0])
    assert w[0] == -80.0
    assert abs(w[1] - (-19.1)) <= 0.2
    assert abs(w[2]) <= 0.05
    assert fr.a_weighting(fr.fft_frequencies(48000, 2048))[0] == -80.0


def test_mel_filterbank_rows():
    for sr in (48000, 16000):
        fb = fr.mel_filterbank(sr, 1024)
        assert fb.shape == (128, 513) and (fb >= 0).all()
        assert ((fb > 0).sum(axis=1) >= 1).all(), sr  # every mel row is non-empty
    fb = fr.mel_filterbank(48000, 1024)
    assert not fb[:, 171:].any()  # fmax 8 kHz: no weight above bin 170
    assert fb[:, 170].any()
    # Slaney's normalisation: a triangle of height 2/width over a comb of spacing df has area ~ df^-1
    edges = fr.mel_to_hz(np.linspace(fr.hz_to_mel(20.0), fr.hz_to_mel(8000.0), 130))
    assert abs(fr.hz_to_mel(1000.0) - 15.0) < 1e-12 and abs(fr.mel_to_hz(fr.hz_to_mel(4321.0)) - 4321.0) < 1e-9
    assert np.all(np.diff(edges) > 0) and abs(edges[0] - 20.0) < 1e-9 and abs(edges[-1] - 8000.0) < 1e-9


def rel(a, b):
    return float(np.abs(np.asarray(a) - b).max() / np.abs(b).max())


@pytest.mark.parametrize("sr,n_fft", [(48000, 1024), (16000, 1024), (44100, 2048), (48000, 512)])
def test_host_tables_match_the_yardstick(sr, n_fft):
    from ddsp_pytorch_amd import core
    assert rel(core.a_weighting_table(sr, n_fft), fr.a_weighting(fr.fft_frequencies(sr, n_fft))) <= 1e-7
    fb = fr.mel_filterbank(sr, n_fft, 128, 20.0, 8000.0)
    dense = core.mel_filterbank_table(sr, n_fft, 128, 20.0, 8000.0)
    assert dense.shape == fb.shape and rel(dense, fb) <= 1e-7
    assert rel(core.dct_table(30, 128), fr.dct_matrix(30, 128)) <= 1e-7
    # the bands hold the dense table: unpacked they give it back, and nothing non-zero is left out
    start, count, packed = core.mel_bands(dense)
    assert start.dtype == count.dtype == np.int32 and packed.size == count.sum()
    back = np.zeros_like(dense)
    off = 0
    for m in range(128):
        back[m, start[m]:start[m] + count[m]] = packed[off:off + count[m]]
        off += count[m]
    assert rel(back, fb) <= 1e-7 and (start + count <= n_fft // 2 + 1).all()


def test_restatement_clamps_the_zero_tailed_item():
    """top_db really clamps: in an item whose last 40 % is exact zeros, the silent frames' D is Dmax - 80."""
    x = fr.make_signal(48000, 8192, 1)[0].copy()
    x[int(0.6 * 8192):] = 0.0
    D = fr.mel_db(x, 48000, 512)
    clamped = np.maximum(D, D.max() - 80.0)
    assert (D[-4:] == -100.0).all() and (clamped[-4:] == D.max() - 80.0).all()
    assert (clamped == D.max() - 80.0).mean() >= 0.25
    w = fr.a_weighting(fr.fft_frequencies(48000, 2048))
    assert np.abs(fr.loudness(x, 48000, 512)[-3:] - (np.log(1e-7) + w.mean())).max() <= 1e-5


EINVAL, EWORKSPACE, ERANGE = 1, 4, 5


def test_envelope_through_ctypes_without_launching():
    from ddsp_pytorch_amd import _lib
    lib = _lib.load()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(256)  # p: never dereferenced, every call returns before a launch
    assert lib.ddsp_hip_version() >= 104

    def loud(B, T, n_fft, hop, x=p, out=p):
        return lib.ddsp_hip_loudness(x, null, out, B, T, n_fft, hop, null)

    def mfcc(B, T, n_fft, hop, n_mels=128, n_mfcc=30, x=p, ws=null, ws_bytes=0, top_db=80.0, n_w=336):
        return lib.ddsp_hip_mfcc(x, p, p, p, n_w, p, p, B, T, n_fft, hop, n_mels, n_mfcc, top_db, ws, ws_bytes, null)

    for f in (loud, mfcc):
        assert f(1, 4096, 1000, 512) == ERANGE    # n_fft not a power of two
        assert f(1, 4096, 8, 4) == ERANGE         # below 16
        assert f(1, 100000, 8192, 512) == ERANGE  # above 4096
        assert f(1, 512, 1024, 512) == EINVAL     # T <= n_fft/2: no reflect padding
        assert f(1, 4096, 1024, 0) == EINVAL      # hop < 1
        assert f(-1, 4096, 1024, 512) == EINVAL
        assert f(1, -4096, 1024, 512) == EINVAL
        assert f(65536, 4096, 1024, 512) == ERANGE
        assert f(0, 4096, 1024, 512) == 0         # empty batch: a no-op success
        assert f(0, 4096, 1024, 512, x=null) == 0
        assert f(2, 4096, 1024, 512, x=null) == EINVAL
    assert loud(2, 4096, 2048, 512, out=null) == EINVAL
    assert loud(2, 1025, 2048, 8192) == 0         # T // hop == 0 frames: nothing to do
    # the MFCC's own rows: 1 <= n_mfcc <= n_mels <= 256, top_db >= 0, the workspace
    assert mfcc(2, 4096, 1024, 512, n_mels=257) == ERANGE
    assert mfcc(2, 4096, 1024, 512, n_mels=128, n_mfcc=129) == EINVAL
    assert mfcc(2, 4096, 1024, 512, n_mfcc=0) == EINVAL
    assert mfcc(2, 4096, 1024, 512, n_mels=0, n_mfcc=0) == EINVAL
    assert mfcc(2, 4096, 1024, 512, top_db=-1.0) == EINVAL
    assert mfcc(2, 4096, 1024, 512, n_w=-1) == EINVAL
    assert mfcc(2, 4096, 1024, 512) == EWORKSPACE
    assert mfcc(2, 4096, 1024, 512, n_mels=256, n_mfcc=256) == EWORKSPACE  # the caps themselves are inside
    assert mfcc(65535, 4096, 16, 7, n_mels=1, n_mfcc=1) == EWORKSPACE
    need = lib.ddsp_hip_mfcc_workspace_size(2, 4096, 1024, 512, 128)
    assert need >= 4 * 2 * 9 * 128
    assert mfcc(2, 4096, 1024, 512, ws=p, ws_bytes=need - 1) == EWORKSPACE
    for B, T, n_fft, hop, n_mels in ((16, 192000, 1024, 512, 128), (3, 2048, 1024, 64, 128), (1, 2080, 1024, 160, 40)):
        assert lib.ddsp_hip_mfcc_workspace_size(B, T, n_fft, hop, n_mels) >= 4 * B * (1 + T // hop) * n_mels
    assert lib.ddsp_hip_mfcc_workspace_size(2, 4096, 1000, 512, 128) == 0  # outside the envelope


def test_analysis_has_no_cpu_fallback():
    import ddsp_pytorch_amd as dd
    x = torch.zeros(2, 4096)
    with pytest.raises(RuntimeError, match="HIP device"):
        dd.core.extract_loudness(x, 48000, 512)
    with pytest.raises(RuntimeError, match="HIP device"):
        dd.core.mfcc(x, 48000, 512)
    with pytest.raises(RuntimeError, match="HIP device"):
        dd.features.analyze(x, torch.zeros(2, 8), 48000, 512)
    assert dd.analyze is dd.features.analyze
