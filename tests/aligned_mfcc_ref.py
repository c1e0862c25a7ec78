"""The aligned streamed MFCC of ddsp_hip_stream_analysis_mfcc restated in NumPy (include/ddsp_hip.h): MFCC slot j of
call k uses the M-sample window centred in the L-sample window of stream frame k R - delay(L) + j, i.e. centred at
sample (k R - delay(L) + j) hop of the zero-preceded stream, where delay(n) = ceil((n/2) / hop) - 1.  It is built
here directly from those windows with the formulas of features_ref.py / stream_features_ref.py (left alone), and
``delayed`` gives the stream whose plain streamed MFCC (stream_features_ref.mfcc at n_fft = M) it must equal."""
import numpy as np

import features_ref as fr
import stream_features_ref as sf


def delay(n_fft, hop):
    return sf.sizes(n_fft, hop, hop)[1] - 1


def delay_samples(L, M, hop):
    """D = (delay(L) - delay(M)) hop: the samples by which the aligned MFCC lags the plain streamed one."""
    return (delay(L, hop) - delay(M, hop)) * hop


def delayed(x_all, L, M, hop):
    """x_all [..., K N] -> the same stream delayed by D samples (D zeros first), cut to the same length."""
    x_all = np.asarray(x_all)
    D = delay_samples(L, M, hop)
    pad = np.zeros(x_all.shape[:-1] + (D,), dtype=x_all.dtype)
    return np.concatenate([pad, x_all], axis=-1)[..., :x_all.shape[-1]]


def aligned_windows(x_all, L, M, hop, N, dtype=np.float64):
    """One item x_all [K N] -> [K, R, M]: the M-sample windows centred at (k R - delay(L) + j) hop, zeros before
    the stream's start."""
    x_all = np.asarray(x_all, dtype=dtype)
    K, R = len(x_all) // N, N // hop
    f = (np.arange(K)[:, None] * R - delay(L, hop) + np.arange(R)[None, :])  # [K, R] stream frames
    s = f[:, :, None] * hop - M // 2 + np.arange(M)[None, None, :]
    assert s.max() < K * N
    return np.where(s >= 0, x_all[np.clip(s, 0, K * N - 1)], dtype(0.0)).astype(dtype)


def aligned_mfcc(x_all, sample_rate, L, M, hop, N, n_mfcc=30, n_mels=128, fmin=20.0, fmax=8000.0, top_db=80.0,
                 dtype=np.float64):
    """-> [K, R, n_mfcc]: the windows above under the periodic Hann, mel dB, the causal clamp, the DCT (the
    arithmetic of stream_features_ref.mel_db / causal_clamp / mfcc)."""
    w = aligned_windows(x_all, L, M, hop, N, dtype)
    S = np.fft.rfft(w * fr.hann(M, dtype)[None, None, :], axis=-1)
    P = (np.abs(S) ** 2).astype(dtype)
    mel = P @ fr.mel_filterbank(sample_rate, M, n_mels, fmin, fmax).astype(dtype).T
    D = (dtype(10.0) * np.log10(np.maximum(dtype(1e-10), mel))).astype(dtype)
    D, _ = sf.causal_clamp(D, top_db)
    return (D @ fr.dct_matrix(n_mfcc, n_mels).astype(dtype).T).astype(dtype)
