"""The Viterbi pitch tracker on the CPU: the yardstick (tests/viterbi_ref.py) is pinned to ground, the inputs are shown
to discriminate (raw YIN jumps octaves on them, the decoded track does not), the fp32 restatement — the GPU gate's
error baseline — is tied to the fp64 one, and the new entry points' boundary is checked without a device.

Measured with the restatement (the asserts are the conditions, not these figures): octave: raw YIN more than 50
cents off on 58 of 87 interior frames, decoded at most 6.2 cents off at lambda 0.02; bursts: raw off on 7, decoded at
most 29.3 cents; clean: decoded within 10.2 cents of raw YIN; fp32 against fp64: no lag and no path frame differs,
cost error <= 1.4e-6.
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import viterbi_cases as vc
import viterbi_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ddsp_hip_pitch_salience", "ddsp_hip_pitch_viterbi", "ddsp_hip_pitch_viterbi_workspace_bytes",
       "ddsp_hip_pitch_viterbi_chunk_frames")
EINVAL, EWS, ERANGE = 1, 4, 5


def _decoded(case, lam):
    r = vc.restated(case)
    return np.stack([vr.decode(c, g, lam, 12)[0] for c, g in zip(r["cost64"], r["f0c64"])])


@pytest.mark.parametrize("name,raw_off_at_least", [("octave", (vc.F - 6 + 1) // 2), ("bursts", 5)])
def test_inputs_discriminate_and_the_decode_holds(name, raw_off_at_least):
    truth = vc.signals()[name][1]
    raw = vc.cents(vc.raw_yin(name)[0], truth)[vc.INTERIOR]
    n_raw = int((raw > 50.0).sum())
    print(f"{name}: raw YIN more than 50 cents off on {n_raw} of {raw.size} interior frames")
    assert n_raw >= raw_off_at_least
    for lam in vc.LAMBDAS:
        dec = vc.cents(_decoded(name, lam)[0], truth)[vc.INTERIOR]
        print(f"{name}: lambda {lam}: decoded max {dec.max():.1f} cents")
        assert (dec <= 50.0).all(), (name, lam, float(dec.max()))


def test_clean_input_stays_within_one_bin_of_raw_yin():
    dev = vc.cents(_decoded("clean", 0.02), vc.raw_yin("clean"))
    print(f"clean: decoded within {dev.max():.1f} cents of raw YIN")
    assert dev.shape == (4, vc.F) and (dev <= 25.0).all()


@pytest.mark.parametrize("case", ["octave", "bursts", "clean"])
def test_fp32_restatement_is_a_usable_baseline(case):
    r = vc.restated(case)
    B, F, NB = r["lag64"].shape
    n_lag = int((r["lag32"] != r["lag64"]).sum())
    same = r["lag32"] == r["lag64"]
    err = np.abs(r["cost32"].astype(np.float64) - r["cost64"])[same]
    print(f"{case}: fp32 lag differs in {n_lag} of {B * F * NB} entries; cost error max {err.max():.2e}")
    assert ((r["lag32"] != r["lag64"]).sum(axis=(1, 2)) <= F * NB // 50).all()
    assert np.isfinite(r["cost32"]).all() and np.isfinite(r["f0c32"]).all()
    # the quantity the GPU gate scales must be an fp32 rounding error, not a disagreement: d' <= a few units, and
    # fp32 sums of W = 1024 terms are off by at most ~1024 * 2^-24 = 6e-5 relative
    assert err.max() < 1e-4
    for lam in vc.LAMBDAS:
        for b in range(B):
            p32 = vr.viterbi(r["cost32"][b], lam, 12)
            p64 = vr.viterbi(r["cost64"][b], lam, 12)
            assert int((p32 != p64).sum()) <= F // 50, (case, lam, b)


def test_decode_tie_rule_is_order_independent():
    rng = np.random.default_rng(3)
    cost = (rng.integers(0, 5, size=(40, 33)) / 4.0).astype(np.float32)
    up = vr.viterbi(cost, 0.25, 3, order="ascending")
    down = vr.viterbi(cost, 0.25, 3, order="descending")
    assert up.dtype == np.int32 and np.array_equal(up, down) and np.array_equal(up, vr.viterbi(cost, 0.25, 3))
    assert len(set(up.tolist())) > 1  # the path moves: the ties are exercised, not avoided
    flat = np.ones((40, 33), dtype=np.float32)
    for order in (None, "ascending", "descending"):
        assert not vr.viterbi(flat, 0.25, 3, order=order).any()
    # the same with R >= NB and on unquantised costs
    wide = rng.uniform(0.0, 1.0, size=(12, 5)).astype(np.float32)
    for order in ("ascending", "descending"):
        assert np.array_equal(vr.viterbi(wide, 0.02, 12, order=order), vr.viterbi(wide, 0.02, 12))
    # a single frame: the smallest argmin; R = 0: the path cannot move
    assert vr.viterbi(cost[:1], 0.25, 3)[0] == int(np.argmin(cost[0]))
    stay = vr.viterbi(cost, 0.25, 0)
    assert (stay == stay[0]).all() and stay[0] == int(np.argmin(cost.astype(np.float64).sum(0)))


@pytest.mark.parametrize("sr,nb,filled,most", [(48000, 256, 28, 14), (16000, None, None, None)])
def test_bin_table(sr, nb, filled, most):
    import pitch_ref as pr
    from ddsp_pytorch_amd import core
    tau_min, tau_max = pr.lags(sr, 50.0, 2000.0, 2048)
    lo, hi = vr.bin_table(tau_min, tau_max, 48)
    tau = np.arange(tau_min, tau_max + 1)
    bins = np.rint(48 * np.log2(tau_max / tau)).astype(int)
    NB = len(lo)
    assert NB == bins[0] + 1 and bins[-1] == 0 and lo[0] <= tau_max == hi[0] and lo[-1] == tau_min
    empty = np.setdiff1d(np.arange(NB), bins)
    assert (lo <= hi).all() and lo.min() >= tau_min and hi.max() <= tau_max
    assert (lo[empty] == hi[empty]).all()
    assert (np.diff(lo) <= 0).all() and (np.diff(hi) <= 0).all()  # higher bins, shorter lags
    for i in np.setdiff1d(np.arange(NB), empty):
        assert (bins[(tau >= lo[i]) & (tau <= hi[i])] == i).all() and (hi[i] - lo[i] + 1) == (bins == i).sum()
    if nb is not None:
        assert (tau_min, tau_max) == (24, 960)
        assert NB == nb and len(empty) == filled and int((hi - lo + 1).max()) <= most
    # the host layer builds the same integers
    got = core.pitch_bins(sr, 50.0, 2000.0, 2048, 48)
    assert got[:2] == (tau_min, tau_max) and got[2] == lo.tolist() and got[3] == hi.tolist()
    assert all(isinstance(v, int) for v in got[2] + got[3])


def test_more_than_1024_bins_raise():
    from ddsp_pytorch_amd import core
    with pytest.raises(ValueError):
        vr.bin_table(24, 960, 200)
    with pytest.raises(RuntimeError, match="1024"):
        core.pitch_bins(48000, 50.0, 2000.0, 2048, 200)
    assert len(vr.bin_table(24, 960, 192)[0]) == 1023


@pytest.fixture(scope="module")
def lib():
    from ddsp_pytorch_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", ROOT, "-j4"], check=True)
    return _lib.load()


def test_entry_points_are_declared_exported_and_bound(lib):
    from ddsp_pytorch_amd import _lib
    header = open(os.path.join(ROOT, "include", "ddsp_hip.h")).read()
    declared = set(re.findall(r"\b(ddsp_hip_\w+)\s*\(", header))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                        check=True).stdout
    for name in NEW:
        assert name in declared, name
        assert re.search(rf"\b{name}\b", nm), name
        assert name in _lib.SIGNATURES, name
    section = header[header.index("pitch_viterbi:"):]
    assert "rint(beta log2(tau_max / tau))" in section and "the smallest i attaining" in section


def test_entry_points_reject_bad_arguments_without_launching(lib):
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(256)  # p: never dereferenced
    big = 1 << 40

    def sal(x=p, lo=p, hi=p, cost=p, f0c=p, lag=null, f0=null, conf=null, period=null, B=1, T=4096, L=2048, hop=512,
            tmin=24, tmax=960, nb=256, sr=48000.0, thr=0.1):
        return lib.ddsp_hip_pitch_salience(x, lo, hi, cost, f0c, lag, f0, conf, period, B, T, L, hop, tmin, tmax, nb,
                                           sr, thr, null)

    def vit(cost=p, f0c=p, f0=p, conf=p, path=p, ws=p, nbytes=big, B=1, F=8, nb=256, R=12, lam=0.02):
        return lib.ddsp_hip_pitch_viterbi(cost, f0c, f0, conf, path, ws, nbytes, B, F, nb, R, lam, null)

    for name in ("x", "lo", "hi", "cost", "f0c"):
        assert sal(**{name: null}) == EINVAL, name
    assert sal(B=-1) == EINVAL and sal(hop=0) == EINVAL and sal(L=0) == EINVAL and sal(T=0) == EINVAL
    assert sal(nb=0) == EINVAL and sal(nb=-4) == EINVAL and sal(nb=1025) == ERANGE
    assert sal(tmin=0) == EINVAL and sal(tmax=1024) == EINVAL and sal(sr=float("nan")) == EINVAL
    assert sal(L=8192, tmin=1, tmax=2) == ERANGE and sal(B=65536) == ERANGE
    assert sal(T=1024) == EINVAL                                    # reflect padding needs T > L/2
    assert sal(conf=p) == EINVAL and sal(period=p) == EINVAL       # the raw outputs come with f0
    assert sal(B=0, x=null, lo=null, hi=null, cost=null, f0c=null) == 0

    for name in ("cost", "f0c", "f0", "path", "ws"):
        assert vit(**{name: null}) == EINVAL, name
    assert vit(B=-1) == EINVAL and vit(F=-1) == EINVAL and vit(nb=0) == EINVAL and vit(R=-1) == EINVAL
    assert vit(lam=-0.5) == EINVAL and vit(lam=float("nan")) == EINVAL and vit(lam=float("inf")) == EINVAL
    assert vit(nb=1025) == ERANGE and vit(R=128) == ERANGE
    assert vit(B=0, cost=null, ws=null) == 0 and vit(F=0, cost=null, ws=null) == 0
    need = lib.ddsp_hip_pitch_viterbi_workspace_bytes(3, 93, 256)
    assert need == 3 * 93 * 256
    assert vit(B=3, F=93, nbytes=need - 1) == EWS and vit(nbytes=0) == EWS
    assert lib.ddsp_hip_pitch_viterbi_workspace_bytes(-1, 93, 256) == 0
    assert lib.ddsp_hip_pitch_viterbi_workspace_bytes(1, 93, 1025) == 0
    chunk = lib.ddsp_hip_pitch_viterbi_chunk_frames
    assert [chunk(n) for n in (0, 1, 64, 65, 256, 1024, 1025)] == [0, 512, 512, 504, 128, 32, 0]
    assert all(chunk(n) * n <= 32768 for n in range(1, 1025))


def test_host_layer_signatures_and_refusals():
    import ddsp_pytorch_amd as dd
    core = dd.core
    for name in ("pitch_bins", "pitch_salience", "viterbi_path", "track_pitch"):
        assert name in core.__all__
    x = torch.zeros(2, 4096)
    with pytest.raises(RuntimeError, match="HIP device"):
        core.pitch_salience(x, 48000, 512)
    with pytest.raises(RuntimeError, match="HIP device"):
        core.track_pitch(x, 48000, 512)
    with pytest.raises(RuntimeError, match="HIP device"):
        core.viterbi_path(torch.zeros(1, 4, 8), torch.zeros(1, 4, 8))
    with pytest.raises(RuntimeError, match="HIP device"):
        dd.features.analyze(x, None, 48000, 512, viterbi=True)

    def defaults(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items()
                if v.default is not inspect.Parameter.empty}

    assert defaults(core.pitch_bins) == dict(bins_per_octave=48)
    assert list(inspect.signature(core.pitch_bins).parameters)[:4] == ["sample_rate", "fmin", "fmax", "frame_length"]
    want = dict(fmin=50.0, fmax=2000.0, frame_length=2048, bins_per_octave=48, return_lag=False)
    got = defaults(core.pitch_salience)
    assert {k: got[k] for k in want} == want
    assert defaults(core.viterbi_path) == dict(transition=0.02, max_jump=12)
    assert defaults(core.track_pitch) == dict(fmin=50.0, fmax=2000.0, frame_length=2048, bins_per_octave=48,
                                              transition=0.02, max_jump=12, return_confidence=False,
                                              return_path=False)
    for fn in (core.pitch_salience, core.track_pitch):
        assert list(inspect.signature(fn).parameters)[:3] == ["signal", "sample_rate", "block_size"]
    sig = inspect.signature(dd.features.analyze)
    assert list(sig.parameters)[-1] == "viterbi" and sig.parameters["viterbi"].default is False
    # extract_pitch keeps its signature, and install() still does not rebind it
    assert list(inspect.signature(core.extract_pitch).parameters) == [
        "signal", "sample_rate", "block_size", "fmin", "fmax", "frame_length", "threshold", "return_confidence",
        "return_period"]
    import importlib
    inst = importlib.import_module("ddsp_pytorch_amd.install")
    assert "extract_pitch" not in inst.FUNCTIONS + inst.LOSS_FUNCTIONS
    assert "track_pitch" not in inst.FUNCTIONS + inst.LOSS_FUNCTIONS
