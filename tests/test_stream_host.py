"""CPU-side checks of the seamless realtime stream (ddsp_hip_stream_*): every entry point validates before any
HIP call, the size queries grow as the state does, and the numpy stream models that tests/test_gpu_stream.py uses
as references satisfy "chunked equals one-shot" against oracle/numpy_oracle.py — known good before a GPU is
involved."""
import ctypes
import io

import numpy as np
import pytest
import torch

from conftest import rms
from oracle import numpy_oracle as no
import stream_ref as sr

EINVAL, EWS, ERANGE = 1, 4, 5
null = ctypes.c_void_p(0)
one = ctypes.c_void_p(256)  # non-null placeholder: every call below returns before any launch


@pytest.fixture(scope="module")
def lib():
    from ddsp_pytorch_amd import _lib
    return _lib.load()


def test_size_queries(lib):
    sb, sf = lib.ddsp_hip_stream_state_bytes, lib.ddsp_hip_stream_spectrum_floats
    # the carry alone: 8 bytes per item, any call size
    assert sb(1, 1024, 0) == 8 and sb(3, 1000, 0) == 24 and sb(0, 0, 0) == 0
    # with a reverb: the history (N floats) and P = ceil(L / N) spectra of N + 1 complex bins per item
    assert sb(1, 1024, 48000) >= 8 + 4 * 1024 + 47 * 1025 * 8
    assert sb(1, 1024, 48000) < 8 + 4 * 1024 + 47 * 1025 * 8 + 64
    assert sb(2, 1024, 48000) > sb(1, 1024, 48000)                       # grows with B
    assert sb(1, 1024, 1024) < sb(1, 1024, 1025) == sb(1, 1024, 2048)    # and with ceil(L / N)
    assert sb(1, 128, 1000) - sb(1, 128, 896) == 129 * 8
    assert sf(1024, 48000) == 47 * 1025 * 2 and sf(64, 192) == 3 * 65 * 2 and sf(2048, 300) == 2049 * 2
    # outside the reverb's range: no size
    for n in (96, 4096, 32, 0, -64):
        assert sb(1, n, 100) == 0 and sf(n, 100) == 0
    assert sf(1024, 0) == 0 and sb(-1, 1024, 0) == 0 and sb(1, 1024, -5) == 0


def test_stream_entry_points_reject_bad_arguments_without_launching(lib):
    # IR spectra
    spec = lib.ddsp_hip_stream_spectrum
    assert spec(null, 100, 128, one, 10 ** 6, null) == EINVAL
    assert spec(one, 100, 128, null, 10 ** 6, null) == EINVAL
    assert spec(one, 0, 128, one, 10 ** 6, null) == EINVAL
    assert spec(one, -3, 128, one, 10 ** 6, null) == EINVAL
    assert spec(one, 100, 96, one, 10 ** 6, null) == ERANGE
    assert spec(one, 100, 4096, one, 10 ** 6, null) == ERANGE
    assert spec(one, 100, 128, one, 129 * 2 - 1, null) == EWS
    # streamed synthesis
    syn = lib.ddsp_hip_stream_synth_frames

    def synth(f0=one, param=one, mags=one, noise=one, counter=one, state=one, nbytes=64, out=one, B=1, F=4, H=16,
              NB=9, bs=32, rate=48000.0):
        return syn(f0, param, mags, -5.0, noise, 0, counter, state, nbytes, 1, out, null, null, B, F, H, NB, bs,
                   rate, null)
    assert synth(f0=null) == EINVAL and synth(param=null) == EINVAL and synth(mags=null) == EINVAL
    assert synth(out=null) == EINVAL and synth(state=null) == EINVAL
    assert synth(noise=null, counter=null) == EINVAL  # device noise needs the counter
    assert synth(B=-1) == EINVAL and synth(F=-1) == EINVAL and synth(H=0) == EINVAL and synth(NB=1) == EINVAL
    assert synth(bs=0) == EINVAL and synth(rate=0.0) == EINVAL
    assert synth(bs=30) == ERANGE and synth(bs=2048) == ERANGE and synth(H=2000) == ERANGE
    assert synth(B=70000) == ERANGE
    assert synth(B=2, nbytes=15) == EWS
    assert synth(B=0) == 0 and synth(F=0) == 0
    # streamed reverb
    rev = lib.ddsp_hip_stream_reverb

    def reverb(x=one, sp=one, floats=10 ** 9, counter=one, state=one, nbytes=10 ** 9, y=one, B=1, N=128, L=1000):
        return rev(x, sp, floats, counter, state, nbytes, y, B, N, L, null)
    assert reverb(x=null) == EINVAL and reverb(sp=null) == EINVAL and reverb(counter=null) == EINVAL
    assert reverb(state=null) == EINVAL and reverb(y=null) == EINVAL
    assert reverb(B=-1) == EINVAL and reverb(L=0) == EINVAL and reverb(N=0) == EINVAL and reverb(N=-128) == EINVAL
    assert reverb(N=96) == ERANGE and reverb(N=4096) == ERANGE and reverb(N=32) == ERANGE
    need = lib.ddsp_hip_stream_state_bytes(1, 128, 1000)
    assert reverb(nbytes=need - 1) == EWS
    assert reverb(floats=lib.ddsp_hip_stream_spectrum_floats(128, 1000) - 1) == EWS
    assert reverb(B=0) == 0
    # advance
    adv = lib.ddsp_hip_stream_advance
    assert adv(one, null, one, 64, 1, 1, 4, 32, 48000.0, null) == EINVAL
    assert adv(null, one, one, 64, 1, 1, 4, 32, 48000.0, null) == EINVAL
    assert adv(one, one, null, 64, 1, 1, 4, 32, 48000.0, null) == EINVAL
    assert adv(one, one, one, 64, 1, -1, 4, 32, 48000.0, null) == EINVAL
    assert adv(one, one, one, 64, 1, 1, -4, 32, 48000.0, null) == EINVAL
    assert adv(one, one, one, 64, 1, 1, 4, 0, 48000.0, null) == EINVAL
    assert adv(one, one, one, 64, 1, 1, 4, 32, 0.0, null) == EINVAL
    assert adv(one, one, one, 64, 1, 1 << 40, 4, 32, 48000.0, null) == ERANGE
    assert adv(one, one, one, 15, 1, 2, 4, 32, 48000.0, null) == EWS


def test_python_layer_refuses_without_a_device():
    from ddsp_pytorch_amd import core
    with pytest.raises(RuntimeError, match="HIP device"):
        core.StreamState(1, "cpu")
    with pytest.raises(RuntimeError, match="power-of-two"):
        core.StreamState(1, "cpu", 96, 1000)
    with pytest.raises(RuntimeError, match="HIP device"):
        core.stream_spectrum(torch.zeros(100), 128)


def test_streaming_export_scripts_and_keeps_the_state_dict():
    """ScriptDDSP(streaming=True) scripts, saves and loads (on the CPU: no call), its stream buffers stay out
    of the state dict, and the arguments that cannot work are refused at construction."""
    import ddsp_pytorch_amd as dd
    from ddsp_pytorch_amd.script import ScriptDDSP
    m = dd.DDSPDecoder(64, 16, 9, 48000, 32, False).eval()
    plain = ScriptDDSP(m, realtime=True)
    s = ScriptDDSP(m, realtime=True, noise_mode="device", streaming=True, call_samples=128)
    assert set(s.state_dict()) == set(plain.state_dict())
    buf = io.BytesIO()
    torch.jit.save(torch.jit.script(s.eval()), buf)
    buf.seek(0)
    loaded = torch.jit.load(buf)
    assert loaded.ddsp.stream_state.dtype == torch.uint8 and loaded.ddsp.stream_counter.dtype == torch.int64
    assert "synthesize_stream" in loaded.ddsp.code
    with pytest.raises(RuntimeError, match="realtime"):
        ScriptDDSP(m, streaming=True)
    with pytest.raises(RuntimeError, match="streaming"):
        ScriptDDSP(m, realtime=True, stream_reverb=True)


# ---------------------------------------------------------------- the GPU tests' references
def _controls(rng, B, F, H):
    f0 = rng.uniform(50.0, 2000.0, (B, F, 1)).astype(np.float32)
    param = rng.standard_normal((B, F, H + 1)).astype(np.float32)
    c = no.harmonic_get_controls(param[..., :1], param[..., 1:], f0, 48000)
    return f0, (c["harmonic_distribution"] * c["amplitudes"]).astype(np.float32), c


@pytest.mark.parametrize("B,bs,R,H,K", [(2, 32, 4, 16, 12), (1, 256, 4, 64, 6)])
def test_harmonic_stream_model_chunked_equals_one_shot(B, bs, R, H, K):
    rng = np.random.default_rng(bs + H)
    f0, amps, c = _controls(rng, B, K * R, H)
    ref, _ = no.harmonic_forward(c["amplitudes"], c["harmonic_distribution"], f0, bs, 48000)
    out, carry, wmax = sr.harmonic_stream(amps, f0, bs, 48000, R, wrap=False)
    assert rms(out, ref[..., 0]) < 1e-6
    inc = no.phase_increment(f0, 48000)[..., 0].astype(np.float64)
    assert np.array_equal(carry, bs * inc.sum(-1))  # exact fp64 sums
    # wrapped: the same oscillator with omega below 2 pi + one call's phase.  Against the ideal oscillator (no
    # fp32 rounding) the error of fl32(omega) and of fl32(omega k) is at most 2^-24 omega k each, so
    # |error| <= sum_k A_k 2 k omega_max 2^-24 — and the wrapped stream sits far inside the one-shot's bound
    ideal, _, _ = sr.harmonic_stream(amps, f0, bs, 48000, R, wrap=False, exact=True)
    wr, cw, wmax_w = sr.harmonic_stream(amps, f0, bs, 48000, R, wrap=True)
    k = np.arange(1, H + 1)
    bound = lambda w: float(((amps.astype(np.float64) * k).sum(-1) * 2.0 * w * 2.0 ** -24).max())
    assert wmax_w < wmax and wmax_w < 2 * np.pi + R * bs * inc.max() + 1e-9
    assert np.abs(wr - ideal).max() <= bound(wmax_w)
    assert np.abs(out - ideal).max() <= bound(wmax)
    assert np.all(cw >= 0) and np.all(cw < 2 * np.pi)
    assert np.abs(np.sin(cw) - np.sin(carry)).max() < 1e-9 and np.abs(np.cos(cw) - np.cos(carry)).max() < 1e-9
    # a stream whose phase never reaches 2 pi: wrapping changes nothing
    f0s = (f0 * 0 + 20.0).astype(np.float32)[:, :R * 2]
    a, _, _ = sr.harmonic_stream(amps[:, :R * 2], f0s, 8, 48000, R, wrap=True)
    b, _, _ = sr.harmonic_stream(amps[:, :R * 2], f0s, 8, 48000, R, wrap=False)
    assert np.array_equal(a, b)


def test_harmonic_stream_model_carry_shift_invariance():
    """sin(k omega) does not change when the carry moves by a multiple of 2 pi — once it is wrapped."""
    rng = np.random.default_rng(7)
    f0, amps, _ = _controls(rng, 2, 4, 16)
    c = np.array([1.0, 2.5])
    a, _, _ = sr.harmonic_stream(amps, f0, 32, 48000, 4, wrap=True, carry0=c)
    b, _, _ = sr.harmonic_stream(amps, f0, 32, 48000, 4, wrap=True, carry0=c + 2 * np.pi * 1e6)
    assert rms(a, b) < 1e-6
    a, _, _ = sr.harmonic_stream(amps, f0, 32, 48000, 4, wrap=False, carry0=c)
    b, _, _ = sr.harmonic_stream(amps, f0, 32, 48000, 4, wrap=False, carry0=c + 2 * np.pi * 1e6)
    assert rms(a, b) > 1e-3


@pytest.mark.parametrize("N,L,K,B", [(128, 1000, 12, 2), (64, 192, 8, 1), (2048, 300, 3, 1)])
def test_reverb_stream_model_chunked_equals_one_shot(N, L, K, B):
    rng = np.random.default_rng(N + L)
    x = (rng.standard_normal((B, K * N)) * 0.3).astype(np.float32)
    h = (rng.standard_normal(L) * np.exp(-np.arange(L) / 8000.0)).astype(np.float32)
    h[0] = 1.0
    ref = no.reverb(x[..., None], h)[..., 0]
    scale = float(np.sqrt(np.mean(ref.astype(np.float64) ** 2)))
    assert rms(sr.reverb_stream(x, h, N), ref) < 1e-6 * scale
