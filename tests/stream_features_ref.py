"""The yardstick of the streaming analysis (numpy only): a restatement of the stream semantics of
include/ddsp_hip.h ("streaming analysis") by explicit ring and history bookkeeping, on top of the formulas of
features_ref.py (which it leaves alone).

Parameters: call size N = R hop, n_fft, d = ceil((n_fft / 2) / hop).  A stream is the concatenation of its calls,
zeros before its start (no reflect padding).  Frame f is the n_fft samples from f hop - n_fft / 2.  Call k receives
samples [k N, (k+1) N) and emits the frames f = k R - d + 1 + j, j < R.  Between calls an item carries
Hs = (d - 1) hop + n_fft / 2 samples in a ring of Hs + N floats, sample s at s mod (Hs + N): call k reads
[k N - Hs, k N) from the ring and the rest from its input, then writes its input over the ring's [k N, (k+1) N).
The MFCC's clamp is causal: against the running maximum of every D emitted up to and including the call.

As in features_ref.py every function takes ``dtype``: float64 is the yardstick, float32 the error baseline.
"""
import numpy as np

import features_ref as fr


def sizes(n_fft, hop, N):
    """(R, d, Hs, ring length) of a stream of N-sample calls."""
    assert N % hop == 0 and N >= hop
    d = -(-(n_fft // 2) // hop)
    Hs = (d - 1) * hop + n_fft // 2
    return N // hop, d, Hs, Hs + N


def first_frame(n_fft, hop, N, k=0):
    """The stream frame index of call k's first output."""
    R, d, _, _ = sizes(n_fft, hop, N)
    return k * R - d + 1


class Stream:
    """One item's carried history: the ring and the call counter."""

    def __init__(self, n_fft, hop, N, dtype=np.float64):
        self.n_fft, self.hop, self.N = n_fft, hop, N
        self.R, self.d, self.Hs, self.L = sizes(n_fft, hop, N)
        self.ring = np.zeros(self.L, dtype=dtype)
        self.k = 0
        self.reads = self.writes = None  # ring positions the last call read / wrote

    def windows(self, x):
        """The call's R windows [R, n_fft] of input x [N]; the call's input goes into the ring."""
        assert x.shape == (self.N,)
        kN = self.k * self.N
        rel = -self.Hs + self.hop * np.arange(self.R)[:, None] + np.arange(self.n_fft)[None, :]
        assert rel.min() == -self.Hs and rel.max() < self.N  # the oldest carried sample; never past the call
        s = kN + rel
        pos = np.mod(s, self.L)
        from_ring = self.ring[pos]
        out = np.where(rel >= 0, x[np.clip(rel, 0, self.N - 1)], np.where(s < 0, 0.0, from_ring))
        self.reads = set(pos[(rel < 0) & (s >= 0)].tolist())
        wpos = np.mod(kN + np.arange(self.N), self.L)
        self.writes = set(wpos.tolist())
        self.ring[wpos] = x
        return out.astype(self.ring.dtype)

    def advance(self):
        self.k += 1


def stream_windows(x_all, n_fft, hop, N, dtype=np.float64):
    """Every call's windows of one item x_all [K N] -> [K, R, n_fft]."""
    x_all = np.asarray(x_all, dtype=dtype)
    K = len(x_all) // N
    st = Stream(n_fft, hop, N, dtype)
    out = []
    for k in range(K):
        out.append(st.windows(x_all[k * N:(k + 1) * N]))
        st.advance()
    return np.stack(out)


def spectra(x_all, n_fft, hop, N, dtype=np.float64):
    """[K, R, n_fft/2+1] complex: the windows under the periodic Hann, unnormalised FFT (fr.stft's)."""
    w = stream_windows(x_all, n_fft, hop, N, dtype)
    return np.fft.rfft(w * fr.hann(n_fft, dtype)[None, None, :], axis=-1)


def loudness(x_all, sample_rate, hop, N, n_fft=2048, dtype=np.float64):
    """fr.loudness's arithmetic on the stream's frames -> [K, R]."""
    S = np.abs(spectra(x_all, n_fft, hop, N, dtype)).astype(dtype)
    S = np.log(S + dtype(1e-7)) + fr.a_weighting(fr.fft_frequencies(sample_rate, n_fft)).astype(dtype)
    return np.mean(S, axis=-1)


def mel_db(x_all, sample_rate, hop, N, n_fft=1024, n_mels=128, fmin=20.0, fmax=8000.0, dtype=np.float64):
    """fr.mel_db's arithmetic on the stream's frames -> [K, R, n_mels], before the clamp."""
    P = (np.abs(spectra(x_all, n_fft, hop, N, dtype)) ** 2).astype(dtype)
    M = P @ fr.mel_filterbank(sample_rate, n_fft, n_mels, fmin, fmax).astype(dtype).T
    return (dtype(10.0) * np.log10(np.maximum(dtype(1e-10), M))).astype(dtype)


def causal_clamp(D, top_db):
    """D [K, R, n_mels] -> (clamped D, the running maximum per call [K])."""
    run = np.maximum.accumulate(D.max(axis=(1, 2)))
    return np.maximum(D, (run - D.dtype.type(top_db))[:, None, None]), run


def mfcc(x_all, sample_rate, hop, N, n_mfcc=30, n_fft=1024, n_mels=128, fmin=20.0, fmax=8000.0, top_db=80.0,
         dtype=np.float64):
    """-> [K, R, n_mfcc]: mel dB, the causal clamp, the orthonormal DCT-II."""
    D, _ = causal_clamp(mel_db(x_all, sample_rate, hop, N, n_fft, n_mels, fmin, fmax, dtype), top_db)
    return (D @ fr.dct_matrix(n_mfcc, n_mels).astype(dtype).T).astype(dtype)


def ring_wraps(n_fft, hop, N, K):
    """How many times K calls go round the ring."""
    return K * N / sizes(n_fft, hop, N)[3]
