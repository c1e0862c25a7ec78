"""CPU side of the partitioned reverb's branch sweep (tests/test_gpu_reverb_shapes.py): fp64 references of the
convolution and its two correlations, an fp32 restatement of csrc/upols.hip's algorithm as a yardstick, a
restatement of its host-side shape arithmetic (plan), the case tables, and the per-block error measure.
tests/test_upols_ref.py checks all of it without a device."""
import math

import numpy as np
import torch

P = 2048            # partition (kP)
N = 2 * P           # transform (kN)
RING_BLK = 25       # kRingBlk: output blocks per thread of the ring MAC
RING_R = 27         # its unrolled round: kRingBlk + kRingPF - 1
STREAM_NB = 50      # kStreamNB: the one row length of the whole-row (stream) MAC
STREAM_NQ = 25      # kStreamNQ: its largest count of kernel windows
CORR_SLICES = 4     # kCorrSlices: wave slices of a correlation workgroup
CORR_GROUPS = 8     # corr_groups' cap
SR = 48000
FWD_BLOCK_TOL = 1e-6   # test_gpu_parity.py::test_reverb_partitioned_shapes' figure, per (row, block) here
GRAD_REL = 1e-5        # tests/test_gpu_grad.py's figure, per block / partition here
FALLBACK = 4.0         # x the yardstick's worst block, where the device exceeds a bound with its sums right


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------ fp64 references
def conv64(x, h):
    """y[r, t] = sum_tau h[tau] x[r, t - tau], t < T: x [rows, T], h [L] -> [rows, T] (one 2T-point FFT)"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    T = x.shape[-1]
    hp = np.zeros(T)
    hp[:min(T, h.size)] = h[:T]
    return np.fft.irfft(np.fft.rfft(x, 2 * T) * np.fft.rfft(hp, 2 * T), 2 * T)[..., :T]


def conv64_rows(x, H):
    """the same with kernel H[r] for row r"""
    return np.concatenate([conv64(x[r], H[r]) for r in range(len(x))])


def dx64(g, h):
    """dx[r, s] = sum_t g[r, t] h[t - s]: the gradient of conv64's input"""
    g = np.atleast_2d(np.asarray(g, dtype=np.float64))
    return conv64(g[:, ::-1], h)[:, ::-1]


def dh64(x, g, L):
    """dh[tau] = sum_r sum_t g[r, t] x[r, t - tau] for tau < min(L, T), zero beyond -> [L]"""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    g = np.atleast_2d(np.asarray(g, dtype=np.float64))
    T = x.shape[-1]
    c = np.fft.irfft(np.fft.rfft(g, 2 * T) * np.conj(np.fft.rfft(x, 2 * T)), 2 * T)[..., :T].sum(0)
    out = np.zeros(L)
    out[:min(L, T)] = c[:L]
    return out


# ------------------------------------------------------------------------------------------ the fp32 yardsticks
def _blocks(x, nb, second_half=False):
    """x [rows, T] -> [rows, nb, N]: block b in the first half, zeros in the other (or the reverse)"""
    rows, T = x.shape
    z = torch.zeros(rows, nb * P, dtype=x.dtype)
    z[:, :T] = x
    out = torch.zeros(rows, nb, N, dtype=x.dtype)
    (out[:, :, P:] if second_half else out[:, :, :P]).copy_(z.reshape(rows, nb, P))
    return out


def _windows(h, kc, Q):
    """h [krows, L] -> [krows, Q, N]: window q = h[(q-1)P, (q+1)P), zero outside [0, kc)"""
    krows = h.shape[0]
    hp = torch.zeros(krows, (Q + 1) * P, dtype=h.dtype)
    hp[:, P:P + kc] = h[:, :kc]
    return torch.stack([hp[:, q * P:q * P + N] for q in range(Q)], 1)


def upols32(x, h, drop=(), dtype=torch.complex64):
    """The algorithm of csrc/upols.hip's header in fp32 (torch.fft on complex64, one real row per transform):
    G_q = FFT([h_{q-1}, h_q]) / N, Z_b = FFT([x_b, 0]), Y_b = sum_q Z_{b-q} G_q in ascending q,
    y_b = the last P points of the unnormalised inverse of Y_b.  x [rows, T]; h [L] or one kernel per row
    [rows, L].  drop: (b, q) terms left out of every row's sum (the seeded fault of the discrimination tests)."""
    real = torch.float32 if dtype == torch.complex64 else torch.float64
    x = torch.tensor(np.atleast_2d(np.asarray(x))).to(real)
    h = torch.tensor(np.atleast_2d(np.asarray(h))).to(real)
    rows, T = x.shape
    nb, kc = ceil_div(T, P), min(h.shape[1], T)
    Q = ceil_div(kc, P) + 1
    G = torch.fft.fft(_windows(h, kc, Q).to(dtype) / N)          # [krows, Q, N]
    Z = torch.fft.fft(_blocks(x, nb).to(dtype))                   # [rows, nb, N]
    Y = torch.zeros_like(Z)
    for q in range(min(Q, nb)):
        term = Z[:, :nb - q] * G[:, q:q + 1]
        for (b, dq) in drop:
            if dq == q:
                term[:, b - q] = 0
        Y[:, q:] += term
    y = torch.fft.ifft(Y, norm="forward").real[:, :, P:].reshape(rows, nb * P)[:, :T]
    return y.numpy()


def corr_upols(x, g, L, dtype=torch.complex64, drop_pair=None, drop_lag=None):
    """The impulse gradient of csrc/upols.hip's backward, restated: rows packed in pairs (z = x_a + i x_b),
    dG_q = sum_pairs sum_b conj(Z_{b-q}) GZ_b with GZ_b = FFT([0, g_b]), dh_p = Re(second half of the
    unnormalised inverse of dG_p + (-1)^f dG_{p+1}) / N, cropped to min(L, T), zero beyond -> [L].
    drop_pair / drop_lag leave one pair's or one lag's contribution out."""
    real = torch.float32 if dtype == torch.complex64 else torch.float64
    x = torch.tensor(np.atleast_2d(np.asarray(x))).to(real)
    g = torch.tensor(np.atleast_2d(np.asarray(g))).to(real)
    rows, T = x.shape
    nb, kc = ceil_div(T, P), min(L, T)
    Qp = ceil_div(kc, P)
    Q = Qp + 1
    if rows % 2:
        x = torch.cat([x, torch.zeros(1, T, dtype=real)])
        g = torch.cat([g, torch.zeros(1, T, dtype=real)])
    Z = torch.fft.fft(torch.complex(_blocks(x[0::2], nb), _blocks(x[1::2], nb)).to(dtype))
    GZ = torch.fft.fft(torch.complex(_blocks(g[0::2], nb, True), _blocks(g[1::2], nb, True)).to(dtype))
    dG = torch.zeros(Q + 1, N, dtype=dtype)
    for pair in range(Z.shape[0]):
        if pair == drop_pair:
            continue
        for q in range(min(Q, nb)):
            if q != drop_lag:
                dG[q] += (Z[pair, :nb - q].conj() * GZ[pair, q:]).sum(0)
    sign = torch.tensor([1.0, -1.0], dtype=real).repeat(P)
    part = torch.fft.ifft(dG[:Qp] + sign * dG[1:Qp + 1], norm="forward").real[:, P:] / N
    out = np.zeros(L)
    out[:kc] = part.reshape(-1)[:kc].numpy()
    return out


# ------------------------------------------------------------------------------------------ shape arithmetic
def plan(rows, T, L, per_row=False):
    """csrc/upols.hip's host-side shape arithmetic (upols_apply_spectra, launch_mac, the ring kernel's chunk_base
    and pmax in both directions, upols_backward), restated.  L is the kernel's whole length."""
    nb = ceil_div(T, P)
    kc = min(L, T)
    Qp = ceil_div(max(kc, 1), P)
    Q = Qp + 1
    npairs = rows if per_row else ceil_div(rows, 2)
    p = dict(nb=nb, kc=kc, Qp=Qp, Q=Q, npairs=npairs, pairing=not per_row,
             h_stride=(ceil_div(max(L, 1), P) + 1) * N if per_row else 0,
             mac="stream" if nb == STREAM_NB and Q <= STREAM_NQ else "ring",
             tail=T - (nb - 1) * P, kc_mod=kc % P, ir_grid=max(nb, Q))
    if p["mac"] == "ring":
        chunks = ceil_div(nb, RING_BLK)
        fwd_bases = [nb - (chunks - c) * RING_BLK for c in range(chunks)]
        adj_bases = [c * RING_BLK for c in range(chunks)]
        fwd_pmax = [min(Q, b + RING_BLK) for b in fwd_bases]
        adj_pmax = [min(Q, nb - b) for b in adj_bases]
        p.update(chunks=chunks, first_base=fwd_bases[0], fwd_bases=fwd_bases, adj_bases=adj_bases,
                 fwd_pmax=fwd_pmax, adj_pmax=adj_pmax, fwd_rounds=[ceil_div(m, RING_R) for m in fwd_pmax],
                 adj_rounds=[ceil_div(m, RING_R) for m in adj_pmax])
    # the impulse-gradient correlation (paired rows always)
    cpairs = ceil_div(rows, 2)
    groups = min(ceil_div(cpairs, CORR_SLICES), CORR_GROUPS)
    PC = 13 if Q <= 13 else 25
    p.update(corr_pairs=cpairs, groups=groups, PC=PC, lag_blocks=1 if Q <= 13 else ceil_div(Q, 25),
             last_lag_block=Q - (ceil_div(Q, PC) - 1) * PC,
             slice_pairs=ceil_div(cpairs, groups * CORR_SLICES),   # slice 0 of group 0 loops over the most
             idle_slices=max(groups * CORR_SLICES - cpairs, 0))
    return p


def q_last(kc):
    """The last kernel window that holds a tap an output uses.  Window q serves taps ((q-1)P + n, qP + n] of
    output sample n of a block, so window Qp = ceil(kc / P) serves taps from (Qp-1)P + 1 on: none when
    kc % P == 1 (the window then holds tap (Qp-1)P alone, which window Qp - 1 serves for every n)."""
    return max(ceil_div(kc - 1, P), 0)


def used_taps(q, kc):
    """how many (sample, tap) products window q adds to one output block: sample n takes taps ((q-1)P + n, qP + n]"""
    n = np.arange(P)
    return int(np.clip(np.minimum(q * P + n, kc - 1) - np.maximum((q - 1) * P + n, -1), 0, P).sum())


def q_heavy(kc):
    """The last kernel window at least half full of used taps (a whole window adds P P products, or P (P + 1) / 2
    at lag 0).  It is q_last(kc) unless the kernel ends a few taps into its last partition: dropping a window of
    four taps cannot move a block by 100 x the bound, which is what the discrimination tests ask of this one."""
    q = q_last(kc)
    while q > 0 and used_taps(q, kc) < P * P // 2:
        q -= 1
    return q


def forward_drops(T, L):
    """The discrimination faults of a forward shape: for every chunk of the ring (for the stream kernel, the
    whole row) its first and last in-signal block b, each with the largest lag q that block uses (q_heavy) ->
    [(b, q, q_last)]; where q_last differs, that lighter term is dropped too and must leave the bound."""
    p = plan(3, T, L)
    nb, qh, ql = p["nb"], q_heavy(p["kc"]), q_last(p["kc"])
    bases = p["fwd_bases"] if p["mac"] == "ring" else [0]
    span = RING_BLK if p["mac"] == "ring" else nb
    out = []
    for base in bases:
        for b in sorted({max(base, 0), min(base + span, nb) - 1}):
            out.append((b, min(b, qh), min(b, ql)))
    return out


# ------------------------------------------------------------------------------------------ error measure
def block_errors(got, ref, length=None):
    """[rows, T] against [rows, T] -> [rows, nb]: rms(got - ref) over rms(ref) per block of P.  A last block
    shorter than P is measured against the rms of the row's last full block (a one-sample block has no
    meaningful rms of its own); with one block, against its own (such cases keep T >= 1024).  length: the
    part of the rows that is measured (a gradient's min(L, T) taps)."""
    got = np.atleast_2d(np.asarray(got, dtype=np.float64))
    ref = np.atleast_2d(np.asarray(ref, dtype=np.float64))
    assert got.shape == ref.shape, (got.shape, ref.shape)
    T = ref.shape[-1] if length is None else length
    got, ref = got[:, :T], ref[:, :T]
    nb = ceil_div(T, P)
    pad = nb * P - T
    d2 = np.pad((got - ref) ** 2, ((0, 0), (0, pad))).reshape(-1, nb, P).sum(-1)
    r2 = np.pad(ref ** 2, ((0, 0), (0, pad))).reshape(-1, nb, P).sum(-1)
    n = np.full(nb, float(P))
    n[-1] = P - pad
    err_rms = np.sqrt(d2 / n)
    ref_rms = np.sqrt(r2 / n)
    if pad and nb > 1:
        ref_rms[:, -1] = ref_rms[:, -2]
    assert nb > 1 or T >= 1024
    return err_rms / ref_rms


def rel(got, ref):
    return abs(float(got) - float(ref)) / abs(float(ref))


# ------------------------------------------------------------------------------------------ inputs
def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def signal(rows, T, seed=0):
    return (0.3 * _rng(1, T, seed).standard_normal((rows, T))).astype(np.float32)


def kernel(L, seed=0, krows=None):
    """0.05 randn with h[0] = 1 and no decay: every lag weighs the same in every output block"""
    h = (0.05 * _rng(2, L, seed).standard_normal((krows or 1, L))).astype(np.float32)
    h[:, 0] = 1.0
    return h if krows else h[0]


def upstream(rows, T, seed=0):
    return _rng(3, T, seed).standard_normal((rows, T)).astype(np.float32)


INITIAL_WET = 0.3
ENV_FLOOR = 0.05


def initial_decay(L):
    """Reverb's decay parameter for which the envelope exp(-softplus(-decay) t 500) is 0.0625 at t = L / SR,
    above ENV_FLOOR at the last tap: late partitions keep their weight in d_decay and d_wet"""
    sp = math.log(16.0) / (500.0 * L / SR)
    return max(-math.log(math.expm1(sp)), -2.0)  # (a few taps: any decay does)


def last_tap_envelope(decay, L):
    return math.exp(-math.log1p(math.exp(-decay)) * ((L - 1) / SR) * 500.0)


def module_params(L, seed=0):
    """(noise [L, 1] U[-1, 1), decay, wet) of modules.Reverb(L, SR, INITIAL_WET, initial_decay(L)), fp32"""
    noise = (_rng(4, L, seed).random((L, 1)) * 2 - 1).astype(np.float32)
    return noise, np.float32(initial_decay(L)), np.float32(INITIAL_WET)


def module_grads64(x, w, noise, decay, wet, L):
    """fp64 autograd through oracle/torch_ref.py's Reverb -> (out, dx, d_noise, d_decay, d_wet), numpy"""
    from oracle import torch_ref as tr
    n, d, wt = (torch.tensor(np.asarray(a)).double().requires_grad_(True) for a in (noise, decay, wet))
    xc = torch.tensor(np.asarray(x)).double().unsqueeze(-1).requires_grad_(True)
    out = tr.Reverb(n, d, wt, L, SR)(xc)
    (out * torch.tensor(np.asarray(w)).double().unsqueeze(-1)).sum().backward()
    return (out.detach().squeeze(-1).numpy(), xc.grad.squeeze(-1).numpy(), n.grad.reshape(-1).numpy(),
            float(d.grad), float(wt.grad))


# ------------------------------------------------------------------------------------------ the cases
ROWS = (1, 2, 3)

# name: (T, L, what it is there for, the plan() entries that prove it there)
FORWARD_CASES = {
    "nb1": (1500, 1500, "Q = 2; ring chunk base -24; the IR-cache grid wider than nb",
            dict(nb=1, Q=2, mac="ring", chunks=1, first_base=-24, fwd_pmax=[1], ir_grid=2)),
    "identity": (2048, 1, "one-tap kernel; Q = 2",
                 dict(nb=1, Q=2, kc=1, mac="ring", fwd_pmax=[1])),
    "tail1_2047": (2049, 2047, "one sample in the last block; kc % 2048 = 2047",
                   dict(nb=2, tail=1, Q=2, kc_mod=2047, first_base=-23, fwd_pmax=[2])),
    "tail1_2048": (2049, 2048, "one sample in the last block; kc % 2048 = 0",
                   dict(nb=2, tail=1, Q=2, kc_mod=0, fwd_pmax=[2])),
    "tail1_2049": (2049, 2049, "one sample in the last block; kc % 2048 = 1",
                   dict(nb=2, tail=1, Q=3, kc_mod=1, fwd_pmax=[2])),
    "nb25": (25 * P, 25 * P, "exactly one full chunk; Q = nb + 1",
             dict(nb=25, Q=26, chunks=1, first_base=0, fwd_pmax=[25], fwd_rounds=[1])),
    "nb26": (26 * P - 17, 30000, "two chunks, the first holding one block",
             dict(nb=26, Q=16, chunks=2, first_base=-24, fwd_pmax=[1, 16], adj_pmax=[16, 1])),
    "nb27": (27 * P, 27 * P, "pmax = 27: one round exactly",
             dict(nb=27, Q=28, chunks=2, first_base=-23, fwd_pmax=[2, 27], fwd_rounds=[1, 1])),
    "nb28": (28 * P, 28 * P, "pmax = 28: a second round with one useful step",
             dict(nb=28, Q=29, chunks=2, first_base=-22, fwd_pmax=[3, 28], fwd_rounds=[1, 2],
                  adj_pmax=[28, 3], adj_rounds=[2, 1])),
    "nb49": (49 * P - 17, 48000, "the ring below the stream shape",
             dict(nb=49, Q=25, mac="ring", chunks=2, first_base=-1, fwd_pmax=[24, 25])),
    "nb51": (51 * P - 17, 48000, "the ring above the stream shape; three chunks",
             dict(nb=51, Q=25, mac="ring", chunks=3, first_base=-24, fwd_pmax=[1, 25, 25])),
    "stream_last": (102400, 49152, "the last length the stream kernel serves",
                    dict(nb=50, Q=25, mac="stream")),
    "ring_first": (102400, 49153, "the first length the ring takes over at 50 blocks",
                   dict(nb=50, Q=26, mac="ring", chunks=2, first_base=0, fwd_pmax=[25, 26], adj_pmax=[26, 25])),
    "stream_q3": (100353, 2049, "stream kernel, Q = 3, one sample in the last block",
                  dict(nb=50, tail=1, Q=3, mac="stream")),
    "stream_q24": (100353, 47000, "stream kernel, Q = 24",
                   dict(nb=50, tail=1, Q=24, mac="stream")),
    "nb60": (60 * P - 17, 54 * P + 5, "Q = 56 > 2 R: three rounds",
             dict(nb=60, Q=56, chunks=3, first_base=-15, fwd_pmax=[10, 35, 56], fwd_rounds=[1, 2, 3],
                  adj_pmax=[56, 35, 10], adj_rounds=[3, 2, 1])),
    "long_ir": (30 * P, 250000, "IR longer than the signal (kc = T)",
                dict(nb=30, kc=30 * P, Q=31, chunks=2, first_base=-20, fwd_pmax=[5, 30], fwd_rounds=[1, 2])),
}

TRANSPOSED_CASES = ("nb1", "nb26", "nb28", "ring_first")

# core.fft_convolve (kernel length == N): 3 rows with three kernels (no pairing, h_stride = windows * kN),
# the same rows with one kernel (a pair and a lone row), 4 rows with one kernel (two pairs)
ROW_KERNEL_CASES = {
    9000: dict(nb=5, Q=6, mac="ring", chunks=1, first_base=-20, fwd_pmax=[5]),
    51 * P: dict(nb=51, Q=52, mac="ring", chunks=3, first_base=-24, fwd_pmax=[1, 26, 51], fwd_rounds=[1, 1, 2]),
}

# name: (rows, T, L, what it is there for, plan() entries)
GRAD_CASES = {}
for _name, _why, _exp in (
        ("nb1", "one block", dict(PC=13, lag_blocks=1, adj_pmax=[1])),
        ("nb26", "adjoint chunks laid from block 0: 25 blocks and one", dict(PC=25, lag_blocks=1, adj_pmax=[16, 1])),
        ("nb28", "adjoint pmax 28: two rounds; two lag blocks", dict(PC=25, lag_blocks=2, adj_rounds=[2, 1])),
        ("stream_last", "the adjoint stream kernel; one lag block of 25", dict(mac="stream", PC=25, lag_blocks=1)),
        ("ring_first", "the adjoint ring at 50 blocks; a second lag block of one lag",
         dict(mac="ring", PC=25, lag_blocks=2, last_lag_block=1)),
        ("nb60", "three adjoint rounds; three lag blocks", dict(PC=25, lag_blocks=3, adj_rounds=[3, 2, 1]))):
    for _rows in ROWS:
        _T, _L = FORWARD_CASES[_name][:2]
        GRAD_CASES[f"{_name}-r{_rows}"] = (_rows, _T, _L, _why, dict(_exp, corr_pairs=(_rows + 1) // 2, groups=1))
GRAD_CASES.update({
    "q13": (3, 14 * P, 12 * P, "Q = 13: the last shape of PC = 13", dict(nb=14, Q=13, PC=13, lag_blocks=1)),
    "q14": (3, 14 * P, 12 * P + 1, "Q = 14: the first shape of PC = 25", dict(nb=14, Q=14, PC=25, lag_blocks=1)),
    "q26": (3, 27 * P, 25 * P, "Q = 26: a second lag block of one lag",
            dict(nb=27, Q=26, PC=25, lag_blocks=2, last_lag_block=1)),
    "rows9": (9, 6000, 4097, "groups = 2: five pairs, three idle slices",
              dict(nb=3, Q=4, kc_mod=1, corr_pairs=5, groups=2, slice_pairs=1, idle_slices=3)),
    "rows17": (17, 6000, 4097, "groups = 3: nine pairs", dict(corr_pairs=9, groups=3, slice_pairs=1, idle_slices=3)),
    "rows64": (64, 6000, 4097, "groups = 8, every slice full",
               dict(corr_pairs=32, groups=8, slice_pairs=1, idle_slices=0)),
    "rows65": (65, 6000, 4097, "pair 32 in a slice's second iteration, with a lone row",
               dict(corr_pairs=33, groups=8, slice_pairs=2)),
    "rows67": (67, 6000, 4097, "34 pairs: two slices with a second iteration",
               dict(corr_pairs=34, groups=8, slice_pairs=2)),
    "past_kc": (2, 6000, 10000, "taps past kc: dimp and d_noise exactly 0 there",
                dict(nb=3, kc=6000, Q=4, corr_pairs=1, groups=1)),
})

_CACHE = {}


def forward_case(name):
    """x [3, T], h [L] and the fp64 reference of the three rows, computed once"""
    if ("f", name) not in _CACHE:
        T, L = FORWARD_CASES[name][:2]
        x, h = signal(3, T), kernel(L)
        c = dict(name=name, T=T, L=L, x=x, h=h, ref=conv64(x, h))
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE["f", name] = c
    return _CACHE["f", name]


def grad_case(name):
    """x, w [rows, T], h [L] and the fp64 dx and dimp"""
    if ("g", name) not in _CACHE:
        rows, T, L = GRAD_CASES[name][:3]
        x, w, h = signal(rows, T, 1), upstream(rows, T, 1), kernel(L, 1)
        c = dict(name=name, rows=rows, T=T, L=L, x=x, w=w, h=h, dx=dx64(w, h), dimp=dh64(x, w, L))
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE["g", name] = c
    return _CACHE["g", name]
