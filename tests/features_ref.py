"""The yardstick of the analysis features (numpy only): a restatement of ``ddsp/core.py:81-97``
(extract_loudness) and ``ddsp/preprocess.py:30-32`` (librosa.feature.mfcc) from their formulas, with the
conventions of librosa < 0.10 (the reference's positional ``li.load(f, sr)`` / ``mfcc(x, ...)`` calls only run
there): ``pad_mode='reflect'``, periodic Hann window, unnormalised FFT, ``power=2``, Slaney mel filterbank with
``norm='slaney'``, ``power_to_db(ref=1.0, amin=1e-10, top_db=80)``, orthonormal DCT-II.

librosa is not installed where this was written, so parity with librosa's own output has not been measured:
this restatement is what the tests pin (tests/test_features_ref.py ties its pieces to torch.stft and scipy).

Every function takes ``dtype``: float64 is the yardstick, float32 (tables rounded to fp32, numpy's
single-precision pocketfft, fp32 log and sums) is the error baseline the GPU kernels are judged against.
"""
import numpy as np


def hann(n, dtype=np.float64):
    """Periodic Hann window (scipy.signal.get_window('hann', n, fftbins=True))."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)).astype(dtype)


def frames(x, n_fft, hop):
    """Centred frames of x [T] -> [1 + T // hop, n_fft]: reflect padding by n_fft/2, frame f centred at f hop."""
    xp = np.pad(x, n_fft // 2, mode="reflect")
    n = 1 + (len(xp) - n_fft) // hop
    idx = hop * np.arange(n)[:, None] + np.arange(n_fft)[None, :]
    return xp[idx]


def stft(x, n_fft, hop, dtype=np.float64):
    """librosa.stft(x, n_fft, hop, win_length=n_fft, center=True, pad_mode='reflect'), frame-major
    [frames, n_fft/2+1] (librosa's is the transpose)."""
    x = np.asarray(x, dtype=dtype)
    return np.fft.rfft(frames(x, n_fft, hop) * hann(n_fft, dtype)[None, :], axis=-1)


def a_weighting(freqs):
    """librosa.A_weighting(freqs, min_db=-80), dB, float64."""
    f_sq = np.asarray(freqs, dtype=np.float64) ** 2
    c = np.array([12200.0, 20.6, 107.7, 737.9]) ** 2
    with np.errstate(divide="ignore"):
        w = 2.0 + 20.0 * (np.log10(c[0]) + 2 * np.log10(f_sq) - np.log10(f_sq + c[0]) - np.log10(f_sq + c[1])
                          - 0.5 * np.log10(f_sq + c[2]) - 0.5 * np.log10(f_sq + c[3]))
    return np.maximum(w, -80.0)


def fft_frequencies(sample_rate, n_fft):
    return np.linspace(0.0, sample_rate / 2.0, 1 + n_fft // 2)


def hz_to_mel(f):
    """Slaney: 200/3 Hz per mel below 1 kHz, log steps of ln(6.4)/27 above."""
    f = np.asarray(f, dtype=np.float64)
    lin = f * 3.0 / 200.0
    log = 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) / (np.log(6.4) / 27.0)
    return np.where(f >= 1000.0, log, lin)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), m * 200.0 / 3.0)


def mel_filterbank(sample_rate, n_fft, n_mels=128, fmin=20.0, fmax=8000.0):
    """librosa.filters.mel(htk=False, norm='slaney'), float64 [n_mels, n_fft/2+1]."""
    freqs = fft_frequencies(sample_rate, n_fft)
    edges = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    fb = np.zeros((n_mels, len(freqs)))
    for m in range(n_mels):
        rise = (freqs - edges[m]) / (edges[m + 1] - edges[m])
        fall = (edges[m + 2] - freqs) / (edges[m + 2] - edges[m + 1])
        fb[m] = np.maximum(0.0, np.minimum(rise, fall)) * 2.0 / (edges[m + 2] - edges[m])
    return fb


def dct_matrix(n_mfcc, n_mels):
    """Rows 0..n_mfcc-1 of the orthonormal DCT-II of n_mels points, float64."""
    t = np.empty((n_mfcc, n_mels))
    for i in range(n_mfcc):
        t[i] = np.sqrt(2.0 / n_mels) * np.cos(np.pi * i * (2 * np.arange(n_mels) + 1) / (2.0 * n_mels))
    t[0] = np.sqrt(1.0 / n_mels)
    return t


def loudness(x, sample_rate, block_size, n_fft=2048, dtype=np.float64):
    """core.py:81-97 for x [T] -> [T // block_size]: mean over bins of ln(|X| + 1e-7) + A-weighting (dB added
    to a natural log, as the reference does), last frame dropped."""
    S = np.abs(stft(x, n_fft, block_size, dtype)).astype(dtype)
    S = np.log(S + dtype(1e-7)) + a_weighting(fft_frequencies(sample_rate, n_fft)).astype(dtype)[None, :]
    return np.mean(S, axis=1)[:-1]


def mel_db(x, sample_rate, block_size, n_fft=1024, n_mels=128, fmin=20.0, fmax=8000.0, dtype=np.float64):
    """10 log10(max(1e-10, mel power spectrogram)) before the top_db clamp, [frames, n_mels]."""
    P = (np.abs(stft(x, n_fft, block_size, dtype)) ** 2).astype(dtype)
    M = P @ mel_filterbank(sample_rate, n_fft, n_mels, fmin, fmax).astype(dtype).T
    return (dtype(10.0) * np.log10(np.maximum(dtype(1e-10), M))).astype(dtype)


def mfcc(x, sample_rate, block_size, n_mfcc=30, n_fft=1024, n_mels=128, fmin=20.0, fmax=8000.0, top_db=80.0,
         dtype=np.float64):
    """preprocess.py:30-32 for x [T] -> [1 + T // block_size, n_mfcc] (the reference's ``.T`` layout)."""
    D = mel_db(x, sample_rate, block_size, n_fft, n_mels, fmin, fmax, dtype)
    D = np.maximum(D, D.max() - dtype(top_db))
    return (D @ dct_matrix(n_mfcc, n_mels).astype(dtype).T).astype(dtype)


def make_signal(sample_rate, T, B, seed=0):
    """The GPU tests' input, float32 [B, T]: per item two decaying sines (220 Hz at 0.3, 1760 Hz at 0.1, a
    linear envelope from 1 to 0.05) plus white noise of sigma 0.01 — the noise keeps every bin far above the
    fp32 FFT's own error, without it ln(|X| + 1e-7) amplifies rounding and a comparison measures nothing."""
    rng = np.random.default_rng(seed)
    t = np.arange(T) / float(sample_rate)
    env = np.linspace(1.0, 0.05, T)
    x = np.empty((B, T))
    for b in range(B):
        ph = rng.uniform(0, 2 * np.pi, 2)
        x[b] = env * (0.3 * np.sin(2 * np.pi * 220.0 * t + ph[0]) + 0.1 * np.sin(2 * np.pi * 1760.0 * t + ph[1]))
        x[b] += 0.01 * rng.standard_normal(T)
    return x.astype(np.float32)

