"""The three-feature streamed analysis' boundary on the CPU (ddsp_hip_stream_analysis_mfcc: the streamed loudness,
MFCC and pitch of one call in one launch over one state, on one time axis) and ddsp_hip_dense_rows' widened
envelope: the entry point is declared, exported and bound, answers the documented code for every bad argument
before any HIP call in the documented order (there is no device here), the delay identity the GPU tests lean on
holds exactly in fp64, and the host layers refuse what they cannot run."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import aligned_mfcc_ref as am
import pitch_cases as pc
import pitch_ref as pr
import stream_features_ref as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ddsp_hip_stream_analysis_mfcc"
EINVAL, EWS, ERANGE = 1, 4, 5


@pytest.fixture(scope="module")
def lib():
    from ddsp_pytorch_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", ROOT, "-j4"], check=True)
    return _lib.load()


def test_entry_point_is_declared_exported_and_bound(lib):
    from ddsp_pytorch_amd import _lib
    header = open(os.path.join(ROOT, "include", "ddsp_hip.h")).read()
    assert NAME in set(re.findall(r"\b(ddsp_hip_\w+)\s*\(", header))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                        check=True).stdout
    assert re.search(rf"\b{NAME}\b", nm)
    assert NAME in _lib.SIGNATURES
    assert lib.ddsp_hip_version() == 108


def test_entry_point_rejects_bad_arguments_without_launching(lib):
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(256)  # p: never dereferenced
    big = 1 << 30

    def fn(x=p, w=p, loud=p, bs=p, bc=p, bw=p, n_w=1000, dct=p, mfcc=p, f0=p, conf=p, period=p, counter=p, state=p,
           nbytes=big, B=1, N=1024, L=2048, M=1024, hop=256, n_mels=128, n_mfcc=30, top_db=80.0, tmin=24, tmax=960,
           sr=48000.0, thr=0.1):
        return lib.ddsp_hip_stream_analysis_mfcc(x, w, loud, bs, bc, bw, n_w, dct, mfcc, f0, conf, period, counter,
                                                 state, nbytes, B, N, L, M, hop, n_mels, n_mfcc, top_db, tmin, tmax,
                                                 sr, thr, null)

    nopitch = dict(f0=null, conf=null, period=null)
    # 1. the streaming envelope: L a power of two in [64, 2048], with or without the pitch
    for kw in ({}, nopitch):
        assert fn(L=4096, M=2048, **kw) == ERANGE and fn(L=32, M=32, tmin=1, tmax=2, **kw) == ERANGE
        assert fn(L=96, M=48, tmin=1, tmax=2, **kw) == ERANGE
        assert fn(N=1000, **kw) == EINVAL and fn(N=0, **kw) == EINVAL and fn(hop=0, **kw) == EINVAL
        assert fn(N=33 * 64, hop=64, **kw) == ERANGE
    # 2. the pitch parameters, after the envelope and before the MFCC's
    assert fn(tmin=0) == EINVAL and fn(tmin=961) == EINVAL and fn(tmax=1024) == EINVAL
    assert fn(sr=0.0) == EINVAL and fn(sr=float("nan")) == EINVAL
    assert fn(N=33 * 64, hop=64, tmin=0) == ERANGE          # envelope first
    assert fn(tmin=0, M=512) == EINVAL                       # pitch before the MFCC's M (ERANGE)
    #    f0 NULL: confidence and period must be NULL too; the pitch parameters are then not looked at
    assert fn(f0=null) == EINVAL and fn(f0=null, conf=null) == EINVAL and fn(f0=null, period=null) == EINVAL
    assert fn(tmin=0, tmax=0, sr=0.0, nbytes=0, **nopitch) == EWS
    # 3. the MFCC parameters: M in {L, L/2}; ddsp_hip_stream_mfcc's limits
    assert fn(M=512) == ERANGE and fn(M=4096) == ERANGE and fn(M=2048, nbytes=0) == EWS
    assert fn(n_mels=0) == EINVAL and fn(n_mfcc=0) == EINVAL and fn(n_mfcc=129) == EINVAL
    assert fn(top_db=-1.0) == EINVAL and fn(top_db=float("nan")) == EINVAL and fn(n_w=-1) == EINVAL
    assert fn(n_mels=257, n_mfcc=30) == ERANGE
    # 4. batch 0: a no-op success, whatever the buffers; a negative batch is not
    nulls = {k: null for k in ("x", "w", "loud", "bs", "bc", "bw", "dct", "mfcc", "f0", "conf", "period", "counter",
                               "state")}
    assert fn(B=0, **nulls) == 0
    assert fn(B=0, M=512, **nulls) == ERANGE                 # the parameters are checked before batch 0
    assert fn(B=-1) == EINVAL and fn(B=65536) == ERANGE
    # 5. null buffers (before the state's size)
    for name in ("x", "loud", "bs", "bc", "bw", "dct", "mfcc", "counter", "state"):
        assert fn(nbytes=0, **{name: null}) == EINVAL, name
    # 6. the state: ddsp_hip_stream_features_state_bytes(batch, N, L, hop), one byte short is short
    need = lib.ddsp_hip_stream_features_state_bytes(1, 1024, 2048, 256)
    assert need == 11280
    assert fn(nbytes=need - 1) == EWS and fn(nbytes=0) == EWS and fn(B=3, nbytes=need) == EWS
    assert fn(w=null, conf=null, period=null, nbytes=need - 1) == EWS and fn(nbytes=need - 1, **nopitch) == EWS


def test_dense_rows_envelope(lib):
    from ddsp_pytorch_amd import _lib
    assert _lib.DENSE_MAX_PROBLEMS == 3
    header = open(os.path.join(ROOT, "include", "ddsp_hip.h")).read()
    assert re.search(r"#define\s+DDSP_HIP_DENSE_MAX_PROBLEMS\s+3\b", header)
    assert [f[0] for f in _lib.DenseInput._fields_][-1] == "plain_norm"
    p = 256  # never dereferenced

    def problem(widths):
        P = _lib.DenseProblem()
        for j, wd in enumerate(widths):
            P.inputs[j].x, P.inputs[j].ld, P.inputs[j].width = p, wd, wd
        P.n_inputs, P.weight, P.y, P.ldy, P.out_features = len(widths), p, p, 8, 8
        return P

    def call(problems, n=None, rows=4):
        arr = (_lib.DenseProblem * max(len(problems), 1))(*problems)
        return lib.ddsp_hip_dense_rows(arr, len(problems) if n is None else n, rows, ctypes.c_void_p(0))

    assert call([problem([512, 512, 513])]) == ERANGE        # K = 1537
    assert call([problem([1089])]) == ERANGE                 # one segment is at most 1088 wide, as before
    assert call([problem([64])] * 3, rows=0) == 0            # three problems are taken ...
    assert call([problem([64])] * 4) == EINVAL               # ... four get the error three got before
    assert call([problem([64])], rows=9) == ERANGE


CASES = list(pc.STREAM) + [(sr, hop, N, B, L // 2, K) for sr, hop, N, B, L, K in pc.STREAM if L // 2 >= 64]


@pytest.mark.parametrize("sr,hop,N,B,L,K", CASES)
@pytest.mark.parametrize("half", [True, False])
def test_delay_identity(sr, hop, N, B, L, K, half):
    """The aligned MFCC built directly (M-sample windows centred at (k R - delay(L) + j) hop of the zero-preceded
    stream) equals stream_features_ref.mfcc of the same stream delayed by D = (delay(L) - delay(M)) hop samples,
    exactly, in fp64: the windows are the same samples, so everything after them is the same arithmetic."""
    M = L // 2 if half else L
    x = pr.make_voiced(sr, K * N, B, seed=N + hop + L)
    D = am.delay_samples(L, M, hop)
    assert D == (sf.sizes(L, hop, N)[1] - sf.sizes(M, hop, N)[1]) * hop and D >= 0
    assert (D == 0) == (M == L or sf.sizes(L, hop, N)[1] == sf.sizes(M, hop, N)[1])
    if (sr, hop, L, M) == (48000, 256, 2048, 1024):
        assert D == 512 and am.delay(L, hop) * hop == 768 and am.delay(M, hop) * hop == 256
    for b in range(B):
        xd = am.delayed(x[b], L, M, hop)
        assert xd.shape == x[b].shape and not xd[:D].any() and np.array_equal(xd[D:], x[b][:len(xd) - D])
        # the windows themselves, then the feature
        assert np.array_equal(am.aligned_windows(x[b], L, M, hop, N), sf.stream_windows(xd, M, hop, N))
        got = am.aligned_mfcc(x[b], sr, L, M, hop, N)
        want = sf.mfcc(xd, sr, hop, N, n_fft=M)
        assert got.dtype == want.dtype == np.float64 and got.shape == (K, N // hop, 30)
        assert np.array_equal(got, want), (b, np.abs(got - want).max())


def test_host_layers_refuse_what_they_cannot_run():
    import ddsp_pytorch_amd as dd
    assert "stream_analysis_mfcc" in dd.core.__all__
    sig = inspect.signature(dd.core.stream_analysis_mfcc)
    assert list(sig.parameters)[:5] == ["x", "sample_rate", "block_size", "state", "pitch"]
    want = dict(pitch=True, fmin=50.0, fmax=2000.0, frame_length=2048, threshold=0.1, return_confidence=False,
                return_period=False, n_mfcc=30, mfcc_n_fft=1024, n_mels=128, mel_fmin=20.0, mel_fmax=8000.0,
                top_db=80.0)
    assert {k: sig.parameters[k].default for k in want} == want
    assert inspect.signature(dd.core.dense_input).parameters["activation"].default is True

    class State:  # a CPU tensor is refused before the state is looked at
        pass
    with pytest.raises(RuntimeError, match="HIP device"):
        dd.core.stream_analysis_mfcc(torch.zeros(1, 1024), 48000, 256, State())
    sig = inspect.signature(dd.features.StreamAnalyzer.__init__)
    assert sig.parameters["aligned"].default is False
    for pitch in (False, True):
        with pytest.raises(RuntimeError, match="HIP device"):
            dd.features.StreamAnalyzer(48000, 256, 1024, device="cpu", pitch=pitch, aligned=True)
    # RealtimeGraph on a CPU autoencoder: the device error of the decoder's, whatever the options
    from ddsp_pytorch_amd.realtime import RealtimeGraph
    model = dd.DDSPAutoencoder(64, 16, 9, 48000, 256, False)
    assert model.decoder.add_z and "encoder.gru.weight_hh_l0" in model.state_dict()
    for kw in ({}, {"loudness_from_audio": True}, {"pitch_from_audio": True, "loudness_from_audio": True}):
        with pytest.raises(RuntimeError, match="the model must be on a HIP device"):
            RealtimeGraph(model, call_samples=1024, **kw)
