"""The signals of the Viterbi pitch tests and their restatements, computed once per process and read-only.

Common: sr 48000, L 2048, hop 512, T 48000 (93 frames), fmin 50, fmax 2000 (lags 24 .. 960, 256 bins at 48 per
octave), n = arange(T) / sr, one rng = default_rng(7) drawn in the order octave, bursts.
    octave  f = 196 2^(0.1 sin(2 pi 0.7 n)): a weak, fluctuating fundamental under a strong second harmonic
    bursts  f = 330 2^(-0.4 n), six harmonics, three 1400-sample bursts of noise
    clean   pitch_ref.make_voiced(48000, 48000, 4, 11)
Truth is f[frame * hop]; "interior" means frames 3 .. F - 4.
"""
import functools

import numpy as np

import pitch_ref as pr
import viterbi_ref as vr

SR, L, HOP, T = 48000, 2048, 512, 48000
FMIN, FMAX, BETA = 50.0, 2000.0, 48
F = T // HOP
INTERIOR = slice(3, F - 3)
LAMBDAS = (0.01, 0.02, 0.04)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def signals():
    """{'octave': (x [T] float32, truth [F]), 'bursts': (x, truth)}."""
    rng = np.random.default_rng(7)
    n = np.arange(T) / float(SR)
    f = 196.0 * 2.0 ** (0.1 * np.sin(2 * np.pi * 0.7 * n))
    ph = 2 * np.pi * np.cumsum(f) / SR
    a1 = 0.16 + 0.14 * np.sin(2 * np.pi * 3.1 * n)
    x = 0.3 * (a1 * np.sin(ph) + np.sin(2 * ph) + 0.3 * a1 * np.sin(3 * ph) + 0.4 * np.sin(4 * ph))
    x = x + rng.normal(0.0, 0.003, T)
    out = {"octave": (_frozen(x.astype(np.float32)), _frozen(f[np.arange(F) * HOP]))}
    f = 330.0 * 2.0 ** (-0.4 * n)
    ph = 2 * np.pi * np.cumsum(f) / SR
    x = 0.2 * sum(np.sin(h * ph) / h for h in range(1, 7)) + rng.normal(0.0, 0.003, T)
    for s in (9000, 21000, 33000):
        x[s:s + 1400] = rng.normal(0.0, 0.2, 1400)
    out["bursts"] = (_frozen(x.astype(np.float32)), _frozen(f[np.arange(F) * HOP]))
    return out


@functools.lru_cache(maxsize=None)
def audio(name):
    """[B, T'] float32, read-only: the named input of the tests."""
    if name in ("octave", "bursts"):
        return _frozen(signals()[name][0][None].copy())
    if name == "clean":
        return _frozen(pr.make_voiced(SR, T, 4, 11))
    if name == "short":  # for L 64 and L 4096
        return _frozen(pr.make_voiced(SR, 8192, 2, 5))
    if name == "silence":  # item 1 silent
        x = pr.make_voiced(SR, 8192, 2, 3)
        x[1] = 0.0
        return _frozen(x)
    raise KeyError(name)


# name -> (audio, frame_length); hop 512 throughout
SALIENCE_CASES = {"octave": ("octave", 2048), "bursts": ("bursts", 2048), "clean": ("clean", 2048),
                  "L64": ("short", 64), "L4096": ("short", 4096), "silence": ("silence", 2048)}


@functools.lru_cache(maxsize=None)
def table(frame_length=L):
    """(tau_min, tau_max, (lo, hi)) at 48 kHz, 50 .. 2000 Hz, 48 bins per octave."""
    tau_min, tau_max = pr.lags(SR, FMIN, FMAX, frame_length)
    return tau_min, tau_max, tuple(_frozen(a) for a in vr.bin_table(tau_min, tau_max, BETA))


@functools.lru_cache(maxsize=None)
def restated(case):
    """{'cost64', 'f0c64', 'lag64', 'cost32', ...}: both precisions' salience of the case, stacked [B, F, NB]."""
    name, frame_length = SALIENCE_CASES[case]
    _, tau_max, tab = table(frame_length)
    out = {}
    for tag, dt in (("64", np.float64), ("32", np.float32)):
        res = [vr.salience_frames(pr.offline_frames(x, frame_length, HOP), SR, tau_max, tab, dt) for x in audio(name)]
        for k, key in enumerate(("cost", "f0c", "lag")):
            out[key + tag] = _frozen(np.stack([r[k] for r in res]))
    return out


@functools.lru_cache(maxsize=None)
def raw_yin(name):
    """pitch_ref's fp64 YIN f0 of the named audio, [B, F]."""
    tau_min, tau_max, _ = table()
    return _frozen(np.stack([pr.pitch_frames(pr.offline_frames(x, L, HOP), SR, tau_min, tau_max)[0]
                             for x in audio(name)]))


def cents(f, truth):
    return 1200.0 * np.abs(np.log2(np.asarray(f, dtype=np.float64) / truth))
