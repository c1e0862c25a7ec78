"""The streamed Viterbi pitch tests' cases and their restatements, computed once per process and read-only: the
signals of viterbi_cases cut into calls, the stream's own frames (pitch_ref.stream_frames: zeros before the stream),
viterbi_ref's salience of them in both precisions, and the online decode of stream_viterbi_ref.

Common: sr 48000, 50 .. 2000 Hz, 48 bins per octave, calls of 1024 samples, lambda 0.02, jumps of at most 12 bins.
At hop 512 and L 2048 (d = 2) emitted frame n is stream frame n - 1, and the decision at lag D describes stream
frame f = n - D - 1; "interior" means 3 <= f <= 87 and n >= D, truth is viterbi_cases.signals()[name][1][f].
"""
import functools

import numpy as np

import pitch_ref as pr
import stream_viterbi_ref as sv
import viterbi_cases as vc
import viterbi_ref as vr

N = 1024
LAM, JUMP = 0.02, 12

# case -> (audio of viterbi_cases, calls taken from its start, frame_length, hop)
SALIENCE_CASES = {"octave": ("octave", 46, 2048, 512), "bursts": ("bursts", 46, 2048, 512),
                  "clean": ("clean", 10, 2048, 512), "silence": ("silence", 8, 2048, 512),
                  "L64": ("short", 8, 64, 512), "hop256": ("short", 8, 2048, 256)}


def _frozen(a):
    a.setflags(write=False)
    return a


def audio(case):
    """[B, K N] float32, read-only: the case's stream."""
    name, K, _, _ = SALIENCE_CASES[case]
    return vc.audio(name)[:, :K * N]


@functools.lru_cache(maxsize=None)
def frames(case):
    """[B, K R, L]: the frames the K calls emit, in order."""
    _, _, L, hop = SALIENCE_CASES[case]
    return _frozen(np.stack([pr.stream_frames(x, L, hop, N) for x in audio(case)]))


@functools.lru_cache(maxsize=None)
def restated(case):
    """{'cost64', 'f0c64', 'lag64', 'cost32', ...}: both precisions' salience of the case's emitted frames, stacked
    [B, K R, NB]."""
    _, _, L, _ = SALIENCE_CASES[case]
    _, tau_max, tab = vc.table(L)
    out = {}
    for tag, dt in (("64", np.float64), ("32", np.float32)):
        res = [vr.salience_frames(Y, vc.SR, tau_max, tab, dt) for Y in frames(case)]
        for k, key in enumerate(("cost", "f0c", "lag")):
            out[key + tag] = _frozen(np.stack([r[k] for r in res]))
    return out


@functools.lru_cache(maxsize=None)
def online(case, D):
    """(f0, confidence, path), each [K R]: the fp64 restatement's online decode of item 0 at lag D."""
    ref = restated(case)
    R = N // SALIENCE_CASES[case][3]
    return tuple(_frozen(a) for a in sv.stream(ref["cost64"][0], ref["f0c64"][0], R, LAM, JUMP, D))


@functools.lru_cache(maxsize=None)
def raw_yin(case):
    """pitch_ref's fp64 per-frame YIN f0 of item 0's emitted frames, [K R]."""
    _, _, L, _ = SALIENCE_CASES[case]
    tau_min, tau_max, _ = vc.table(L)
    return _frozen(pr.pitch_frames(frames(case)[0], vc.SR, tau_min, tau_max)[0])


def interior(name, f0, D):
    """Cents from truth of an emitted f0 track [K R] of 'octave' / 'bursts' decided at lag D (per-frame YIN: D = 0),
    over the interior frames."""
    truth = vc.signals()[name][1]
    n = np.arange(len(f0))
    f = n - D - 1
    keep = (f >= 3) & (f <= 87) & (n >= D)
    return vc.cents(np.asarray(f0)[keep], truth[f[keep]])
