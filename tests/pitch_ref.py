"""The yardstick of the pitch tracker (numpy only): a restatement of the definition in include/ddsp_hip.h ("pitch"),
YIN (de Cheveigne & Kawahara 2002) with the 2^-40 floor, by direct sums.

Per frame y[0..L), W = L/2, for tau = 0 .. tau_max + 1:
    E(tau) = sum_{j<W} y[j+tau]^2,  r(tau) = sum_{j<W} y[j] y[j+tau],  d = E(0) + E(tau) - 2 r,
    d := 0 where d < 2^-40 (E(0) + E(tau)),
    d'(0) = 1, S(tau) = sum_{k=1..tau} d(k), d'(tau) = d tau / S if S > 0 else 1,
    tau* = the smallest local minimum (d'(tau) < d'(tau-1), d'(tau) <= d'(tau+1)) in [tau_min, tau_max] under the
    threshold, else the smallest index of the minimum over [tau_min, tau_max],
    s = (a - c) / (2 (a - 2b + c)) if b <= a, b <= c and a - 2b + c > 0 else 0  (a, b, c = d'(tau*-1 .. tau*+1)),
    f0 = sr / (tau* + s), confidence = 1 - min(1, b - (a - c) s / 4), period = tau*.

``dtype``: float64 is the yardstick; float32 does every operation in float32, the final division included, and
returns float32 arrays (the error baseline of the GPU gate: otherwise its error would sit below the GPU's own
output rounding).  The threshold is the float32 value the C-ABI carries, in either precision.
"""
import math

import numpy as np

import stream_features_ref as sf


def lags(sample_rate, fmin=50.0, fmax=2000.0, frame_length=2048):
    """(tau_min, tau_max): max(floor(sr / fmax), 1), min(ceil(sr / fmin), L - W - 1)."""
    L = int(frame_length)
    W = L // 2
    return max(int(math.floor(sample_rate / fmax)), 1), min(int(math.ceil(sample_rate / fmin)), L - W - 1)


def difference(y, tau_hi, dtype=np.float64):
    """(E, r, d) of one frame y [L] for tau = 0 .. tau_hi by direct sums, d after the floor."""
    y = np.asarray(y, dtype=dtype)
    W = len(y) // 2
    assert tau_hi <= len(y) - W
    win = np.lib.stride_tricks.sliding_window_view(y, W)[:tau_hi + 1]  # [tau, W]: y[tau + j]
    E = np.sum(win * win, axis=1, dtype=dtype)
    r = np.sum(win * y[None, :W], axis=1, dtype=dtype)
    tot = (E[0] + E).astype(dtype)
    d = (tot - dtype(2.0) * r).astype(dtype)
    d = np.where(d < dtype(2.0 ** -40) * tot, dtype(0.0), d).astype(dtype)
    return E, r, d


def normalise(d, dtype=np.float64):
    """d' of d [tau_hi + 1]."""
    tau = np.arange(len(d)).astype(dtype)
    d0 = d.copy()
    d0[0] = 0
    S = np.cumsum(d0, dtype=dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        dn = np.where(S > 0, (d * tau).astype(dtype) / np.where(S > 0, S, dtype(1.0)), dtype(1.0)).astype(dtype)
    dn[0] = dtype(1.0)
    return dn


def pick(dn, tau_min, tau_max, threshold):
    """tau* of d' [>= tau_max + 2]."""
    t = np.arange(tau_min, tau_max + 1)
    b = dn[t]
    cand = (b < dn[t - 1]) & (b <= dn[t + 1]) & (b < threshold)
    if cand.any():
        return int(t[np.argmax(cand)])
    return int(t[np.argmin(b)])  # the first index of the minimum


def pitch_frames(Y, sr, tau_min, tau_max, threshold=0.1, dtype=np.float64):
    """Y [F, L] -> (f0 [F], confidence [F], period [F] int32), in ``dtype``."""
    Y = np.asarray(Y)
    F, L = Y.shape
    W = L // 2
    assert 1 <= tau_min <= tau_max <= W - 1
    thr = dtype(np.float32(threshold))
    f0 = np.empty(F, dtype=dtype)
    conf = np.empty(F, dtype=dtype)
    period = np.empty(F, dtype=np.int32)
    for i in range(F):
        _, _, d = difference(Y[i], tau_max + 1, dtype)
        dn = normalise(d, dtype)
        ts = pick(dn, tau_min, tau_max, thr)
        a, b, c = dn[ts - 1], dn[ts], dn[ts + 1]
        curv = dtype(dtype(a - dtype(2.0) * b) + c)
        s = dtype(0.0)
        if b <= a and b <= c and curv > 0:
            s = dtype(dtype(dtype(0.5) * dtype(a - c)) / curv)
        f0[i] = dtype(dtype(sr) / dtype(dtype(ts) + s))
        conf[i] = dtype(dtype(1.0) - min(dtype(1.0), dtype(b - dtype(dtype(dtype(0.25) * dtype(a - c)) * s))))
        period[i] = ts
    return f0, conf, period


def offline_frames(x, frame_length, hop):
    """x [T] -> [T // hop, L]: frame f is x[reflect(f hop - L/2 + i)] (stft_frames.h's reflect indexing)."""
    x = np.asarray(x)
    T, L = len(x), int(frame_length)
    assert L // 2 < T
    idx = np.arange(T // hop)[:, None] * hop - L // 2 + np.arange(L)[None, :]
    idx = np.abs(idx)
    idx = np.where(idx >= T, 2 * (T - 1) - idx, idx)
    return x[idx]


def stream_frames(x_all, frame_length, hop, N):
    """x_all [K N] -> [K R, L]: the frames the K calls emit, in order (stream_features_ref's frame indices: call k
    emits f = k R - d + 1 + j, frame f starts at f hop - L/2, zeros before the stream)."""
    x_all = np.asarray(x_all)
    w = sf.stream_windows(x_all, frame_length, hop, N, dtype=x_all.dtype)
    return w.reshape(-1, frame_length)


def make_voiced(sr, T, B, seed, f_lo=80.0, f_hi=600.0, lead=0):
    """[B, T] float32: per item six harmonics (amplitudes 1/h, overall gain 0.2) of an f0 drawn in [f_lo, f_hi]
    that glides by a drawn +-0.25 octave with a 5.5 Hz vibrato of 0.5 %, plus white noise of sigma 0.003; the first
    ``lead`` samples zeroed."""
    rng = np.random.default_rng(seed)
    n = np.arange(T) / float(sr)
    out = np.empty((B, T), dtype=np.float32)
    for b in range(B):
        f_start = rng.uniform(f_lo, f_hi)
        glide = rng.uniform(-0.25, 0.25)
        f = f_start * 2.0 ** (glide * np.arange(T) / max(T - 1, 1)) * (1.0 + 0.005 * np.sin(2 * np.pi * 5.5 * n))
        phase = 2 * np.pi * np.cumsum(f) / sr
        y = sum(np.sin(h * phase) / h for h in range(1, 7))
        y = 0.2 * y + rng.normal(0.0, 0.003, T)
        y[:lead] = 0.0
        out[b] = y.astype(np.float32)
    return out


def steady_tone(sr, T, f, seed=0):
    """[T] float32: the six-harmonic tone of ``make_voiced`` at a steady f Hz."""
    rng = np.random.default_rng(seed)
    phase = 2 * np.pi * f * np.arange(T) / sr
    y = 0.2 * sum(np.sin(h * phase) / h for h in range(1, 7)) + rng.normal(0.0, 0.003, T)
    return y.astype(np.float32)


def restate(frames, sr, tau_min, tau_max, threshold=0.1):
    """frames [B, F, L] -> {'f064', 'conf64', 'period64', 'f032', ...}: both precisions, stacked [B, F], read-only."""
    out = {}
    for tag, dt in (("64", np.float64), ("32", np.float32)):
        res = [pitch_frames(np.asarray(fr_, dtype=dt), sr, tau_min, tau_max, threshold, dt) for fr_ in frames]
        for i, name in enumerate(("f0", "conf", "period")):
            a = np.stack([r[i] for r in res])
            a.setflags(write=False)
            out[name + tag] = a
    return out
