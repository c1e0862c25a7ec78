"""The yardstick of the Viterbi-decoded pitch tracker (numpy only): a restatement of the definition in
include/ddsp_hip.h ("pitch_viterbi").  d' comes from pitch_ref.difference / pitch_ref.normalise.

    bins      bin(tau) = rint(beta log2(tau_max / tau)), tau in [tau_min, tau_max]; NB = bin(tau_min) + 1 <= 1024;
              lo_i / hi_i the smallest / largest tau of bin i, an empty bin its centre's nearest lag
    salience  tau^ = the smallest argmin of d' over [lo_i, hi_i]; cost = (float)min(1, d'(tau^));
              f0c = (float)(sr / (tau^ + s)) with pitch_ref's parabola; lag = tau^
    decode    delta_0 = cost(0); delta_t(j) = min_{|i - j| <= R} (delta_{t-1}(i) + lambda |i - j|) + cost(t, j), fp64,
              the smallest i among equals; the smallest argmin of the last row; backtrack

``dtype``: float64 is the yardstick; float32 does every operation of d' and the salience in float32 (the error
baseline of the GPU gate).  The decode is fp64 on fp32 costs in either case; lambda is the float32 value the C-ABI
carries.
"""
import numpy as np

import pitch_ref as pr

MAX_BINS = 1024


def bin_table(tau_min, tau_max, bins_per_octave=48):
    """(lo, hi) int32 [NB]; ValueError above 1024 bins."""
    beta = float(bins_per_octave)
    tau = np.arange(tau_min, tau_max + 1)
    bins = np.rint(beta * np.log2(float(tau_max) / tau.astype(np.float64))).astype(np.int64)
    nb = int(bins[0]) + 1
    if nb > MAX_BINS:
        raise ValueError(f"{nb} bins exceed {MAX_BINS}")
    lo = np.empty(nb, dtype=np.int32)
    hi = np.empty(nb, dtype=np.int32)
    for i in range(nb):
        members = tau[bins == i]
        if members.size:
            lo[i], hi[i] = members[0], members[-1]
        else:
            lo[i] = hi[i] = int(np.clip(np.rint(tau_max * 2.0 ** (-i / beta)), tau_min, tau_max))
    return lo, hi


def salience(dn, table, sr, dtype=np.float64):
    """d' [>= tau_max + 2] of one frame -> (cost [NB] float32, f0c [NB] float32, lag [NB] int32)."""
    lo, hi = table
    nb = len(lo)
    cost = np.empty(nb, dtype=np.float32)
    f0c = np.empty(nb, dtype=np.float32)
    lag = np.empty(nb, dtype=np.int32)
    for i in range(nb):
        ts = int(lo[i]) + int(np.argmin(dn[lo[i]:hi[i] + 1]))  # the first index of the minimum
        a, b, c = dn[ts - 1], dn[ts], dn[ts + 1]
        curv = dtype(dtype(a - dtype(2.0) * b) + c)
        s = dtype(0.0)
        if b <= a and b <= c and curv > 0:
            s = dtype(dtype(dtype(0.5) * dtype(a - c)) / curv)
        cost[i] = np.float32(min(dtype(1.0), b))
        f0c[i] = np.float32(dtype(dtype(sr) / dtype(dtype(ts) + s)))
        lag[i] = ts
    return cost, f0c, lag


def salience_frames(Y, sr, tau_max, table, dtype=np.float64):
    """Y [F, L] -> (cost, f0c, lag), each [F, NB]."""
    out = []
    for y in np.asarray(Y):
        _, _, d = pr.difference(np.asarray(y, dtype=dtype), tau_max + 1, dtype)
        out.append(salience(pr.normalise(d, dtype), table, sr, dtype))
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def viterbi(cost, lam, R, order=None):
    """cost [F, NB] float32 -> path [F] int32.  ``order``: None takes each minimum over the 2R + 1 neighbours at
    once (numpy's argmin: the first, i.e. the smallest i); 'ascending' / 'descending' run the neighbour loop from
    i = j - R up / from i = j + R down with the tie rule applied (an equal value at a smaller i wins): the same path
    by definition."""
    cost = np.asarray(cost)
    assert cost.dtype == np.float32 and cost.ndim == 2 and order in (None, "ascending", "descending")
    F, NB = cost.shape
    lam = np.float64(np.float32(lam))
    R = int(R)
    j = np.arange(NB)
    pen = lam * np.abs(np.arange(-R, R + 1)).astype(np.float64)
    delta = cost[0].astype(np.float64)
    back = np.zeros((F, NB), dtype=np.int64)
    offsets = range(R, -R - 1, -1) if order == "descending" else range(-R, R + 1)
    for t in range(1, F):
        padded = np.full(NB + 2 * R, np.inf)
        padded[R:R + NB] = delta
        if order is None:
            v = np.lib.stride_tricks.sliding_window_view(padded, 2 * R + 1) + pen[None, :]  # [j, k]: i = j + k - R
            k = np.argmin(v, axis=1)
            best, arg = v[j, k], j + k - R
        else:
            best = np.full(NB, np.inf)
            arg = np.zeros(NB, dtype=np.int64)
            for k in offsets:
                v = padded[R + k:R + k + NB] + pen[R + k]
                take = ((v <= best) if order == "descending" else (v < best)) & (j + k >= 0) & (j + k < NB)
                best = np.where(take, v, best)
                arg = np.where(take, j + k, arg)
        delta = best + cost[t].astype(np.float64)
        back[t] = arg
    path = np.empty(F, dtype=np.int32)
    path[F - 1] = int(np.argmin(delta))  # the first index of the minimum
    for t in range(F - 1, 0, -1):
        path[t - 1] = back[t, path[t]]
    return path


def decode(cost, f0c, lam=0.02, R=12):
    """cost, f0c [F, NB] float32 -> (f0 [F] float32, confidence [F] float32, path [F] int32)."""
    path = viterbi(cost, lam, R)
    t = np.arange(len(path))
    return f0c[t, path], np.float32(1.0) - cost[t, path], path
