"""The yardstick of the streamed Viterbi pitch decode (numpy only): an incremental restatement of the definition in
include/ddsp_hip.h ("pitch_viterbi_stream") — state in, one call's costs in, decisions out.

    state     delta [NB] fp64 (after the last frame seen), the back-pointers of the last D frames, their f0c and
              cost, and n, the number of frames seen
    frame n   delta_0 = cost(0); else delta_n(j) = min_{|i - j| <= J} (delta_{n-1}(i) + lambda |i - j|) + cost(n, j),
              fp64, the smallest i among equals (viterbi_ref's recursion, one frame of it)
    decision  s_n = the smallest argmin of delta_n; m = n - min(D, n); path(n) = bp_{m+1}(... bp_n(s_n));
              f0(n) = f0c(m, path(n)); confidence(n) = 1 - cost(m, path(n))

By construction path(n) == viterbi_ref.viterbi(cost[:n + 1])[m]; tests/test_stream_viterbi_ref.py checks that.
lambda is the float32 value the C-ABI carries.
"""
import numpy as np


class State:
    """A fresh stream's decode state for NB bins, jumps of at most J bins and a decision D frames back."""

    def __init__(self, NB, lam=0.02, J=12, D=0):
        self.NB, self.J, self.D = int(NB), int(J), int(D)
        self.lam = np.float64(np.float32(lam))
        self.pen = self.lam * np.abs(np.arange(-self.J, self.J + 1)).astype(np.float64)
        self.n = 0
        self.delta = None
        self.back = []   # bp_n, cost(n), f0c(n) of the last D + 1 frames, the newest last
        self.cost = []
        self.f0c = []


def _frame(st, cost, f0c):
    """One frame in: (path(n), f0(n), confidence(n))."""
    NB, J = st.NB, st.J
    j = np.arange(NB)
    if st.n == 0:
        st.delta = cost.astype(np.float64)
        arg = np.zeros(NB, dtype=np.int64)
    else:
        padded = np.full(NB + 2 * J, np.inf)
        padded[J:J + NB] = st.delta
        v = np.lib.stride_tricks.sliding_window_view(padded, 2 * J + 1) + st.pen[None, :]  # [j, k]: i = j + k - J
        k = np.argmin(v, axis=1)  # the first, i.e. the smallest i
        st.delta = v[j, k] + cost.astype(np.float64)
        arg = j + k - J
    for ring, row in ((st.back, arg), (st.cost, cost), (st.f0c, f0c)):
        ring.append(row)
        del ring[:-(st.D + 1)]
    s = int(np.argmin(st.delta))  # the first index of the minimum
    steps = min(st.D, st.n)
    for u in range(steps):
        s = int(st.back[-1 - u][s])
    st.n += 1
    return s, st.f0c[-1 - steps][s], np.float32(1.0) - st.cost[-1 - steps][s]


def call(st, cost, f0c):
    """One call: cost, f0c [R, NB] float32 -> (f0 [R] float32, confidence [R] float32, path [R] int32); st moves on."""
    cost, f0c = np.asarray(cost), np.asarray(f0c)
    assert cost.dtype == np.float32 and f0c.dtype == np.float32 and cost.shape == f0c.shape == (len(cost), st.NB)
    out = [_frame(st, c, g) for c, g in zip(cost, f0c)]
    return (np.array([o[1] for o in out], dtype=np.float32), np.array([o[2] for o in out], dtype=np.float32),
            np.array([o[0] for o in out], dtype=np.int32))


def stream(cost, f0c, R, lam=0.02, J=12, D=0):
    """cost, f0c [F, NB], F a multiple of R, cut into calls of R frames -> (f0, confidence, path), each [F]."""
    st = State(cost.shape[1], lam, J, D)
    outs = [call(st, cost[a:a + R], f0c[a:a + R]) for a in range(0, len(cost), R)]
    return tuple(np.concatenate([o[k] for o in outs]) for k in range(3))
