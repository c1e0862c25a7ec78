"""tests/upols_ref.py checked on the CPU: the fp64 references against direct sums and fp64 autograd, the fp32
restatement of csrc/upols.hip's algorithm (upols32) inside the forward bound in every block of every case, every
case proved onto the branch it is listed for through plan(), and the bounds proved to discriminate: one (block,
lag) term dropped from upols32, one pair or one lag dropped from the impulse gradient, moves the affected block or
partition by more than 100 x its bound.  The same dropped term on test_reverb_partitioned_shapes' decaying kernels
stays inside that test's whole-tensor 1e-6, which is why tests/test_gpu_reverb_shapes.py exists."""
import numpy as np
import pytest
import torch

import upols_ref as ur
from oracle import torch_ref as tr

P = ur.P


# ------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("T,L", [(1, 1), (7, 3), (5, 9), (16, 16)])
def test_conv64_against_direct_sum(T, L):
    rng = np.random.default_rng(T * 100 + L)
    x, h = rng.standard_normal((2, T)), rng.standard_normal(L)
    ref = np.stack([np.convolve(r, h)[:T] for r in x])
    np.testing.assert_allclose(ur.conv64(x, h), ref, rtol=0, atol=1e-13)
    H = rng.standard_normal((2, L))
    ref = np.stack([np.convolve(r, k)[:T] for r, k in zip(x, H)])
    np.testing.assert_allclose(ur.conv64_rows(x, H), ref, rtol=0, atol=1e-13)


@pytest.mark.parametrize("T,L", [(40, 12), (33, 33), (20, 50)])
def test_dx64_dh64_against_autograd(T, L):
    rng = np.random.default_rng(T + L)
    x, w, h = rng.standard_normal((3, T)), rng.standard_normal((3, T)), rng.standard_normal(L)
    xt = torch.tensor(x, requires_grad=True)
    ht = torch.tensor(h, requires_grad=True)
    hp = torch.nn.functional.pad(ht, (0, T - L)) if L <= T else ht[:T]
    (tr.fft_convolve(xt, hp) * torch.tensor(w)).sum().backward()
    np.testing.assert_allclose(ur.dx64(w, h), xt.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(ur.dh64(x, w, L), ht.grad.numpy(), rtol=0, atol=1e-12)
    assert np.all(ur.dh64(x, w, L)[T:] == 0)


@pytest.mark.parametrize("rows,T,L", [(1, 3000, 3000), (3, 5000, 2049), (4, 6000, 10000)])
def test_partitioned_forms_in_fp64(rows, T, L):
    """upols32 and corr_upols on complex128 are the fp64 references: the restatements are the same sums"""
    x, w, h = ur.signal(rows, T), ur.upstream(rows, T), ur.kernel(L)
    assert ur.block_errors(ur.upols32(x, h, dtype=torch.complex128), ur.conv64(x, h)).max() < 1e-13
    got, ref = ur.corr_upols(x, w, L, torch.complex128), ur.dh64(x, w, L)
    assert ur.block_errors(got, ref, min(L, T)).max() < 1e-13 and np.all(got[T:] == 0)


def test_block_errors_rules():
    ref = np.ones((1, 2 * P + 1))
    ref[0, P:2 * P] = 4.0
    got = ref.copy()
    got[0, 0] += 1.0      # block 0: rms error 1 / sqrt(P) of rms 1
    got[0, -1] += 2.0     # the one-sample last block: error 2 against the last full block's rms 4
    e = ur.block_errors(got, ref)
    np.testing.assert_allclose(e, [[1 / np.sqrt(P), 0.0, 0.5]])
    one = ur.block_errors(np.full((1, 1500), 1.5), np.full((1, 1500), 1.0))
    np.testing.assert_allclose(one, [[0.5]])


def test_envelope_floor():
    for L in sorted({c[2] for c in ur.GRAD_CASES.values()} | {c[1] for c in ur.FORWARD_CASES.values()}):
        env = ur.last_tap_envelope(float(np.float32(ur.initial_decay(L))), L)
        assert ur.ENV_FLOOR < env <= 1.0, (L, env)


# ------------------------------------------------------------------------------------------ the branches
@pytest.mark.parametrize("name", list(ur.FORWARD_CASES))
def test_forward_case_on_its_branch(name):
    T, L, _, expect = ur.FORWARD_CASES[name]
    for rows in ur.ROWS:
        p = ur.plan(rows, T, L)
        assert {k: p.get(k) for k in expect} == expect, (name, p)
        assert p["npairs"] == (rows + 1) // 2 and p["h_stride"] == 0


@pytest.mark.parametrize("n", list(ur.ROW_KERNEL_CASES))
def test_row_kernel_case_on_its_branch(n):
    expect = ur.ROW_KERNEL_CASES[n]
    p = ur.plan(3, n, n, per_row=True)
    assert {k: p.get(k) for k in expect} == expect, p
    assert p["npairs"] == 3 and not p["pairing"] and p["h_stride"] == p["Q"] * ur.N
    assert ur.plan(3, n, n)["npairs"] == 2 and ur.plan(4, n, n)["npairs"] == 2
    assert n > 4096  # past fft_convolve's direct-convolution length


@pytest.mark.parametrize("name", list(ur.GRAD_CASES))
def test_grad_case_on_its_branch(name):
    rows, T, L, _, expect = ur.GRAD_CASES[name]
    p = ur.plan(rows, T, L)
    assert {k: p.get(k) for k in expect} == expect, (name, p)


def test_the_cases_cover_the_branches():
    """every value of the host-side switches that some shape can take is taken by a case"""
    fwd = [ur.plan(3, c[0], c[1]) for c in ur.FORWARD_CASES.values()]
    grd = [ur.plan(c[0], c[1], c[2]) for c in ur.GRAD_CASES.values()]
    assert {p["mac"] for p in fwd} == {p["mac"] for p in grd} == {"ring", "stream"}
    assert {1, 2, 3} <= {p["chunks"] for p in fwd if p["mac"] == "ring"}
    assert {1, 2, 3} <= {r for p in fwd if p["mac"] == "ring" for r in p["fwd_rounds"]}
    assert {1, 2, 3} <= {r for p in grd if p["mac"] == "ring" for r in p["adj_rounds"]}
    assert {ur.RING_R, ur.RING_R + 1} <= {m for p in fwd if p["mac"] == "ring" for m in p["fwd_pmax"]}
    assert {0, 1, P - 1} <= {p["kc_mod"] for p in fwd} and {0, 1} <= {p["kc_mod"] for p in grd}
    assert {(13, 1), (25, 1), (25, 2), (25, 3)} <= {(p["PC"], p["lag_blocks"]) for p in grd}
    assert {1, 2, 3, 8} <= {p["groups"] for p in grd} and {1, 2} <= {p["slice_pairs"] for p in grd}
    assert any(p["nb"] == 50 and p["Q"] == 25 for p in fwd) and any(p["nb"] == 50 and p["Q"] == 26 for p in fwd)
    assert any(p["Q"] == p["nb"] + 1 for p in fwd)
    assert any(p["kc"] < c[1] for p, c in zip(fwd, ur.FORWARD_CASES.values()))


# ------------------------------------------------------------------------------------------ yardstick, discrimination
@pytest.mark.parametrize("name", list(ur.FORWARD_CASES))
def test_upols32_inside_the_bound_and_discriminating(name):
    c = ur.forward_case(name)
    e = ur.block_errors(ur.upols32(c["x"], c["h"]), c["ref"])
    print(f"{name}: upols32 worst block {e.max():.2e}")
    assert e.max() < ur.FWD_BLOCK_TOL, (name, e.max())
    drops = ur.forward_drops(c["T"], c["L"])
    p = ur.plan(3, c["T"], c["L"])
    assert len(drops) >= (p["chunks"] if p["mac"] == "ring" else 1)
    for b, q, ql in drops:
        assert 0 <= q <= ql <= min(b, p["Q"] - 1)
        if ql != q:  # a last window of a few taps: lighter than 100 x, and still outside the bound
            el = ur.block_errors(ur.upols32(c["x"], c["h"], drop=[(b, ql)]), c["ref"])
            print(f"{name}: term (block {b}, lag {ql}) dropped: block error {el[:, b].min():.2e}")
            assert el[:, b].min() > 10 * ur.FWD_BLOCK_TOL, (name, b, ql, el[:, b])
        ed = ur.block_errors(ur.upols32(c["x"], c["h"], drop=[(b, q)]), c["ref"])
        print(f"{name}: term (block {b}, lag {q}) dropped: block error {ed[:, b].min():.2e}")
        assert ed[:, b].min() > 100 * ur.FWD_BLOCK_TOL, (name, b, q, ed[:, b])
        others = np.delete(ed, b, axis=1)
        assert others.size == 0 or others.max() < ur.FWD_BLOCK_TOL


@pytest.mark.parametrize("n", list(ur.ROW_KERNEL_CASES))
def test_upols32_row_kernels(n):
    x, H = ur.signal(3, n, 2), ur.kernel(n, 2, krows=3)
    ref = ur.conv64_rows(x, H)
    assert ur.block_errors(ur.upols32(x, H), ref).max() < ur.FWD_BLOCK_TOL
    # every row on kernel 0 (h_stride = 0): rows 1 and 2 are wrong by their whole size
    e = ur.block_errors(ur.upols32(x, H[0]), ref)
    assert e[0].max() < ur.FWD_BLOCK_TOL and e[1:].min() > 100 * ur.FWD_BLOCK_TOL


@pytest.mark.parametrize("name", list(ur.GRAD_CASES))
def test_impulse_gradient_yardstick_and_discrimination(name):
    c = ur.grad_case(name)
    rows, T, L = c["rows"], c["T"], c["L"]
    p = ur.plan(rows, T, L)
    kc = p["kc"]
    e = ur.block_errors(ur.corr_upols(c["x"], c["w"], L), c["dimp"], kc)
    print(f"{name}: fp32 correlation worst partition {e.max():.2e}")
    assert e.max() < ur.GRAD_REL, (name, e.max())
    # the last pair (the one a slice reaches in its second iteration, where there is one)
    ed = ur.block_errors(ur.corr_upols(c["x"], c["w"], L, drop_pair=p["corr_pairs"] - 1), c["dimp"], kc)
    assert ed.min() > 100 * ur.GRAD_REL, (name, "pair", ed.min())
    # the last lag with a tap in it: partitions q - 1 (its first half) and q (its second)
    q = min(ur.q_last(kc), p["nb"] - 1)
    ed = ur.block_errors(ur.corr_upols(c["x"], c["w"], L, drop_lag=q), c["dimp"], kc)
    assert ed[0, max(q - 1, 0)] > 100 * ur.GRAD_REL, (name, "lag", q, ed)


# ------------------------------------------------------------------------------------------ the measured hole
@pytest.mark.parametrize("nb_blocks,L", [(50, 96000), (120, 250000)])
def test_decaying_kernel_hides_a_dropped_term(nb_blocks, L):
    """test_gpu_parity.py::test_reverb_partitioned_shapes' inputs, with the last block's last lag dropped from
    the sum: inside that test's whole-tensor bound."""
    T = nb_blocks * P - 17
    rng = np.random.default_rng(L + T)
    x = (rng.standard_normal((3, T, 1)) * 0.3).astype(np.float32)[..., 0]
    h = (rng.standard_normal(L) * np.exp(-np.arange(L) / 8000.0)).astype(np.float32)
    h[0] = 1.0
    ref = ur.conv64(x, h)
    b = nb_blocks - 1
    drop = (b, min(b, ur.q_heavy(min(L, T))))
    scale = np.sqrt(np.mean(ref ** 2))
    for d in ((), (drop,)):
        got = ur.upols32(x, h, drop=d)
        whole = np.sqrt(np.mean((got - ref) ** 2)) / scale
        worst = ur.block_errors(got, ref).max()
        print(f"({nb_blocks}, {L}) dropped {d}: whole tensor {whole:.3e}, worst block {worst:.3e}")
        assert whole < 1e-6
    # the same term on a kernel of constant variance
    hf = ur.kernel(L)
    e = ur.block_errors(ur.upols32(x, hf, drop=(drop,)), ur.conv64(x, hf))
    assert e[:, b].min() > 100 * ur.FWD_BLOCK_TOL
