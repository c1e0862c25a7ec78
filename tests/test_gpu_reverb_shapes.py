"""The partitioned reverb (csrc/upols.hip; entry points in csrc/reverb.hip) at every branch its shape arithmetic
takes, against the fp64 references of tests/upols_ref.py, checked PER BLOCK: rms(got - ref) over rms(ref) of every
(row, block of 2048 samples) <= 1e-6 for the forward (test_gpu_parity.py::test_reverb_partitioned_shapes' figure,
there applied to the whole tensor), <= GRAD_REL = 1e-5 (tests/test_gpu_grad.py's) for dx per block, for dimp and
d_noise per partition of 2048 taps, and for d_decay and d_wet relative to the fp64 value.  A last block shorter
than 2048 is measured against the rms of the row's last full block; a lone block against its own.

Inputs: x = 0.3 randn, upstream gradient randn, kernel h = 0.05 randn with h[0] = 1 and NO decay.  The older
reverb tests use kernels decaying as exp(-t / 8000) and one figure per tensor: a (block, lag) term dropped from the
MAC's sum then stays inside their bound (tests/test_upols_ref.py::test_decaying_kernel_hides_a_dropped_term), while
here the same term moves its block by 6e-2 to 1 (test_upols32_inside_the_bound_and_discriminating).  The module
route uses modules.Reverb(L, 48000, initial_wet=0.3) with the decay that leaves the envelope at 1/16 at the last tap.
Every output, spectrum and workspace is allocated over NaNs (poison), and no NaN may remain.  tests/test_upols_ref.py
proves every case onto the branch listed here through upols_ref.plan, the restatement of the host-side arithmetic.

Q = ceil(min(L, T) / 2048) + 1 kernel windows; the whole-row MAC (upols_mac_stream_kernel) runs iff nb == 50 and
Q <= 25, else the ring MAC (upols_mac_ring_kernel) in chunks of 25 blocks laid from the signal's end (forward) or from
block 0 (adjoint), pmax = min(Q, lags that stay in the signal) steps per chunk in unrolled rounds of 27.

Forward, core.reverb_spectrum + core.reverb_apply and modules.Reverb (the cached-IR launch upols_forward_ir_kernel,
against the fp64 convolution with the module's own impulse); rows 1, 2 and 3 as batches of their own:
  case          nb  T             L                   reaches
  nb1            1  1500          1500                Q = 2; ring chunk base -24; the IR-cache grid wider than nb
  identity       1  2048          1                   one-tap kernel; Q = 2
  tail1_*        2  2049          2047 / 2048 / 2049  one sample in the last block; kc % 2048 = 2047, 0, 1
  nb25          25  25 * 2048     T                   exactly one full chunk; Q = nb + 1
  nb26          26  26 * 2048-17  30000               two chunks, the first holding one block (pmax 1)
  nb27, nb28    27, 28  nb * 2048 T                   pmax 27 and 28: one round exactly, a second with one useful step
  nb49, nb51    49, 51  nb * 2048-17  48000           the ring on either side of the stream shape; 51: three chunks
  stream_last   50  102400        49152               the last length of the stream kernel (Q = 25)
  ring_first    50  102400        49153               the first of the ring at 50 blocks (Q = 26)
  stream_q3/q24 50  100353        2049 / 47000        stream kernel, Q = 3 and 24, one sample in the last block
  nb60          60  60 * 2048-17  54 * 2048 + 5       Q = 56 > 2 * 27: three rounds
  long_ir       30  30 * 2048     250000              IR longer than the signal (kc = T)
test_stream_and_ring_agree: stream_last's taps with a zero appended run on the ring and agree with the stream
kernel's output per block within the bound.
Per-row kernels (core.fft_convolve, N = 9000 and 51 * 2048): 3 rows with three different kernels (no pairing,
h_stride = windows * 4096), the same rows with one kernel (a pair and a lone row), 4 rows with one kernel (two pairs).
Transposed (ddsp_hip_reverb_apply_transposed, reverse = true): nb1, nb26, nb28, ring_first against dx64.

Backward, grad.reverb_backward (dx and dimp; from the forward's kept spectra and recomputed from x, bit-equal) and
modules.Reverb under autograd (dx, d_noise, d_decay, d_wet from upols_corr_finish_impulse_kernel):
  rows               shape                         reaches
  1, 2, 3            nb1, nb26, nb28, stream_last, adjoint ring chunks laid from block 0 (25 + 1 blocks; pmax 28 and 56:
                     ring_first, nb60              two and three rounds); the adjoint stream kernel; correlation
                                                   PC = 13, and PC = 25 with 1, 2 and 3 lag blocks
  3                  nb 14, L = 12 * 2048, + 1     Q = 13 (PC = 13) and Q = 14 (PC = 25)
  3                  nb 27, L = 25 * 2048          Q = 26: a second lag block of one lag
  9, 17, 64, 65, 67  T = 6000, L = 4097            groups = 2, 3, 8, 8, 8 of four wave slices: idle slices; every slice
                                                   full; pair 32 in a slice's second iteration with a lone row; 34 pairs
  2                  T = 6000, L = 10000           taps past kc: dimp and d_noise exactly 0 there; d_noise[0] == 0

Largest per-block error measured on an MI355X (a record; the assertions are the constants), beside the fp32
restatements' (upols_ref.upols32 and corr_upols, torch.fft on one host's CPU; tests/test_upols_ref.py prints them):
  forward, reverb_apply   whole blocks 1.7e-7 (identity) to 3.5e-7 (nb60); the one-sample last blocks 5.1e-7
                          (tail1_2047), 5.5e-7 (tail1_2048), 4.1e-7 (stream_q3), 5.3e-7 (stream_q24)
                          upols32: 2.0e-7 to 2.4e-7
  forward, modules.Reverb 1.7e-7 to 3.8e-7 (nb60)      fft_convolve 2.7e-7 to 3.4e-7      ring against stream 2.2e-7
  transposed              2.3e-7 to 3.2e-7
  dx                      2.2e-7 to 3.5e-7; through the module 2.2e-7 to 3.9e-7 (nb60)
  dimp                    2.4e-7 to 3.5e-7, 5.6e-7 in ring_first's one-tap last partition; corr_upols: 1.7e-7 to 3.7e-7
  d_noise                 2.2e-7 to 3.7e-7, 5.3e-7 in nb28's last partition (envelope 1/16)
  d_decay, d_wet          1.1e-7 to 1.9e-6; 3.5e-6 (nb26, 2 rows), 4.6e-6 (rows64)
No case needed the fallback bound (4 x the yardstick's worst block).  The whole file takes 5.4 s on the device.

Seeded faults, each built once into a copy of the library (a term dropped or misdirected inside the allocated
buffers, no address moved) and run against this file and against the older reverb tests (test_gpu_parity.py,
test_gpu_mac_wide.py, test_gpu_grad.py, test_gpu_autograd_boundary.py: the 92 tests on the reverb and fft_convolve):
  ring MAC: pmax one lower                          32 of these 95 fail (nb1, identity, nb26, nb28, nb51, N = 51 * 2048:
                                                    every chunk with pmax 1 or 28) | older: 17, all at T = 2048 (pmax 1)
  ring MAC: gload's `q < Q` as `q < Q - 1`          29 fail (tail1_2047/2048, nb26, nb49, nb51, nb60, q13, q26; nb60's
                                                    last window holds five taps) | older: 7
  h_stride forced to 0                              2 fail (both N, the three-kernel call) | older: 3, of which
                                                    test_fft_convolve_large only since it has three distinct kernels
  correlation's pair loop stopped after one pass    4 fail (rows65, rows67, both routes) | older: none
  correlation's grid capped at one group            10 fail (rows 9 to 67, both routes) | older: none

Branches no case reaches, and why:
  pmax one lower where pmax - 1 needs as many rounds of 27 (nb27, nb60): the rounds run whole, the outputs are the
    same bits; only pmax = 1 and 28 can tell.
  the last kernel window when kc % 2048 == 1 (tail1_2049, stream_q3, ring_first, the rows cases): window Qp then
    holds tap (Qp - 1) 2048 alone, which no output sample takes from it (upols_ref.q_last); dropping it changes
    nothing that a reference could see.
  grid_fits' limits (65535 chunks, pairs or windows: 3.3e9 samples or 131070 rows) and corr groups = 4 to 7
    (25 to 56 rows: the code of groups = 2, 3 and 8 with other counts).
  batch == 0 (memsets, no kernel of upols.hip); the IR cache's validation-only launch (tests/test_gpu_reverb_ir.py).
"""
import math

import numpy as np
import pytest
import torch

import upols_ref as ur

pytestmark = pytest.mark.gpu

P = ur.P


@pytest.fixture(scope="module")
def dd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ddsp_pytorch_amd
    ddsp_pytorch_amd._lib.load()
    return ddsp_pytorch_amd


def poison(*sizes):
    """The kernels write into torch.empty buffers: leave NaNs in the allocator's free blocks of these sizes (a
    shape of floats, or a count of workspace bytes), so that a block, partition or tap a kernel skips does not come
    back holding an earlier run's correct value."""
    for s in sizes:
        if isinstance(s, int):
            torch.full((max(s, 4) // 4,), math.nan, dtype=torch.float32, device="cuda")
        else:
            torch.full(tuple(s), math.nan, dtype=torch.float32, device="cuda")


def cu(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()


def rows_of(t):
    """[B, T, 1] on the device -> [B, T] numpy, with no NaN left in it"""
    a = t.detach().squeeze(-1).cpu().numpy()
    assert not np.isnan(a).any(), "a sample the kernels did not write"
    return a


def check_blocks(got, ref, tol, what, length=None):
    e = ur.block_errors(got, ref, length)
    r, b = np.unravel_index(np.argmax(e), e.shape)
    print(f"{what}: worst block {e.max():.2e} (row {r}, block {b} of {e.shape[1]})")
    assert e.max() <= tol, (what, float(e.max()), int(r), int(b))
    return float(e.max())


def spectrum(dd, h, T):
    poison((dd.core.reverb_spectrum_floats(T, len(h)),))
    spec = dd.core.reverb_spectrum(cu(h), T)
    assert not torch.isnan(spec).any()
    return spec


def apply(dd, x, spec, L):
    """core.reverb_apply of x [rows, T] -> [rows, T] on NaN-poisoned output and workspace"""
    from ddsp_pytorch_amd import _lib
    rows, T = x.shape
    poison((rows, T, 1), int(_lib.query("reverb_workspace_size", rows, T, L)))
    with torch.no_grad():
        return rows_of(dd.core.reverb_apply(cu(x[..., None]), spec, L))


def reverb_module(dd, L, seed=0):
    noise, decay, wet = ur.module_params(L, seed)
    assert ur.last_tap_envelope(float(decay), L) > ur.ENV_FLOOR
    rv = dd.modules.Reverb(L, ur.SR, initial_wet=float(wet), initial_decay=float(decay))
    with torch.no_grad():
        rv.noise.copy_(torch.from_numpy(noise))
    return rv.cuda(), (noise, decay, wet)


# ------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("name", list(ur.FORWARD_CASES))
def test_forward_apply(dd, name):
    """core.reverb_spectrum + core.reverb_apply: rows 1, 2 and 3 as batches of their own, one reference"""
    c = ur.forward_case(name)
    spec = spectrum(dd, c["h"], c["T"])
    for rows in ur.ROWS:
        check_blocks(apply(dd, c["x"][:rows], spec, c["L"]), c["ref"][:rows], ur.FWD_BLOCK_TOL,
                     f"forward {name} rows={rows}")


@pytest.mark.parametrize("name", list(ur.FORWARD_CASES))
def test_forward_module(dd, name):
    """modules.Reverb (upols_forward_ir_kernel: the transforms with the IR cache's validation in one launch) with
    the module's own impulse: the first call builds every window of the cache, the later ones find it valid"""
    from ddsp_pytorch_amd import _lib
    c = ur.forward_case(name)
    T, L = c["T"], c["L"]
    rv, _ = reverb_module(dd, L)
    with torch.no_grad():
        imp = rv.build_impulse().reshape(-1).cpu().numpy()
    assert imp[0] == 1.0 and not np.isnan(imp).any()
    ref = ur.conv64(c["x"], imp)
    for rows in ur.ROWS:
        poison((rows, T, 1), int(_lib.query("reverb_workspace_size", rows, T, L)))
        with torch.no_grad():
            out = rows_of(rv(cu(c["x"][:rows, :, None])))
        check_blocks(out, ref[:rows], ur.FWD_BLOCK_TOL, f"module {name} rows={rows}")


def test_stream_and_ring_agree(dd):
    """50 blocks: the 49152-tap kernel on the stream kernel, and the same taps with a zero appended (49153: the
    ring), per block within the bound of each other"""
    c = ur.forward_case("stream_last")
    T, L = c["T"], c["L"]
    assert ur.plan(3, T, L)["mac"] == "stream" and ur.plan(3, T, L + 1)["mac"] == "ring"
    a = apply(dd, c["x"], spectrum(dd, c["h"], T), L)
    b = apply(dd, c["x"], spectrum(dd, np.append(c["h"], np.float32(0)), T), L + 1)
    check_blocks(b, a, ur.FWD_BLOCK_TOL, "ring against stream")
    check_blocks(b, c["ref"], ur.FWD_BLOCK_TOL, "ring with a zero last tap")


@pytest.mark.parametrize("n", list(ur.ROW_KERNEL_CASES))
def test_fft_convolve_row_kernels(dd, n):
    """core.fft_convolve: three rows with three different kernels (no pairing, a kernel stride), the same rows with
    one kernel (a pair and a lone row), four rows with one kernel (two pairs)"""
    from ddsp_pytorch_amd import _lib
    x, x4, H = ur.signal(3, n, 2), ur.signal(4, n, 3), ur.kernel(n, 2, krows=3)
    assert not np.array_equal(H[0], H[1]) and not np.array_equal(H[1], H[2])
    for xs, ks, ref, what in ((x, H, ur.conv64_rows(x, H), "three kernels"),
                              (x, H[:1], ur.conv64(x, H[0]), "one kernel"),
                              (x4, H[:1], ur.conv64(x4, H[0]), "four rows, one kernel")):
        poison((len(xs), n), int(_lib.query("fft_convolve_workspace_size", len(xs), len(ks), n)))
        with torch.no_grad():
            out = dd.core.fft_convolve(cu(xs), cu(ks)).cpu().numpy()
        assert not np.isnan(out).any()
        check_blocks(out, ref, ur.FWD_BLOCK_TOL, f"fft_convolve N={n} {what}")


@pytest.mark.parametrize("name", ur.TRANSPOSED_CASES)
def test_transposed(dd, name):
    """ddsp_hip_reverb_apply_transposed (reverse = true in the forward and inverse transforms) against dx64"""
    from ddsp_pytorch_amd import _lib, core
    c = ur.forward_case(name)
    T, L = c["T"], c["L"]
    w = ur.upstream(3, T)
    ref = ur.dx64(w, c["h"])
    spec = spectrum(dd, c["h"], T)
    for rows in ur.ROWS:
        wg = cu(w[:rows, :, None])
        nbytes = int(_lib.query("reverb_workspace_size", rows, T, L))
        poison((rows, T, 1), nbytes)
        dx = torch.empty(rows, T, 1, dtype=torch.float32, device="cuda")
        ws = core._workspace(nbytes, wg.device)
        _lib.call("reverb_apply_transposed", _lib.ptr(wg), _lib.ptr(spec), _lib.ptr(dx), rows, T, L, _lib.ptr(ws),
                  ws.numel(), _lib.stream_of(wg))
        check_blocks(rows_of(dx), ref[:rows], ur.GRAD_REL, f"transposed {name} rows={rows}")


# ------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("name", list(ur.GRAD_CASES))
def test_backward_dimp_route(dd, name):
    """grad.reverb_backward: dx and dimp, from the forward's kept input spectra and recomputed from x (bit-equal)"""
    from ddsp_pytorch_amd import _lib, core, grad
    c = ur.grad_case(name)
    rows, T, L = c["rows"], c["T"], c["L"]
    kc = min(L, T)
    x, w = cu(c["x"][..., None]), cu(c["w"][..., None])
    spec = spectrum(dd, c["h"], T)
    poison((rows, T, 1), int(_lib.query("reverb_workspace_size", rows, T, L)))
    with torch.no_grad():
        _, ws = core._reverb_apply_launch(x, spec, L)
    res = []
    for xs, kept in ((None, ws), (x, None)):
        poison((rows, T, 1), (L,), int(_lib.query("reverb_backward_workspace_size", rows, T, L, int(kept is not None))))
        res.append(grad.reverb_backward(xs, kept, spec, w, L, True, True))
    (dx1, di1), (dx2, di2) = res
    dx, dimp = rows_of(dx1), di1.cpu().numpy()
    assert not np.isnan(dimp).any(), "a tap the kernels did not write"
    assert torch.equal(dx1, dx2) and torch.equal(di1, di2)
    assert np.all(dimp[kc:] == 0)
    check_blocks(dx, c["dx"], ur.GRAD_REL, f"dx {name}")
    check_blocks(dimp, c["dimp"], ur.GRAD_REL, f"dimp {name}", kc)


@pytest.mark.parametrize("name", list(ur.GRAD_CASES))
def test_backward_module_route(dd, name):
    """modules.Reverb under autograd: dx, and d_noise / d_decay / d_wet from upols_corr_finish_impulse_kernel,
    against fp64 autograd through oracle/torch_ref.py's Reverb"""
    from ddsp_pytorch_amd import _lib
    c = ur.grad_case(name)
    rows, T, L = c["rows"], c["T"], c["L"]
    kc = min(L, T)
    rv, (noise, decay, wet) = reverb_module(dd, L, 1)
    _, dx_ref, dn_ref, dd_ref, dw_ref = ur.module_grads64(c["x"], c["w"], noise, decay, wet, L)
    xg = cu(c["x"][..., None]).requires_grad_(True)
    poison((rows, T, 1), int(_lib.query("reverb_workspace_size", rows, T, L)))
    out = rv(xg)
    poison((rows, T, 1), (L, 1), (1,), (1,), int(_lib.query("reverb_backward_workspace_size", rows, T, L, 1)))
    (out * cu(c["w"][..., None])).sum().backward()
    dn = rv.noise.grad.reshape(-1).cpu().numpy()
    assert not np.isnan(dn).any(), "a tap the kernels did not write"
    assert dn[0] == 0 and np.all(dn[kc:] == 0)
    check_blocks(rows_of(xg.grad), dx_ref, ur.GRAD_REL, f"module dx {name}")
    check_blocks(dn, dn_ref, ur.GRAD_REL, f"d_noise {name}", kc)
    ed, ew = ur.rel(rv.decay.grad, dd_ref), ur.rel(rv.wet.grad, dw_ref)
    print(f"module {name}: d_decay {ed:.2e}, d_wet {ew:.2e}")
    assert ed <= ur.GRAD_REL and ew <= ur.GRAD_REL, (name, ed, ew)
