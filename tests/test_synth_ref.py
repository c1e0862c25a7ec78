"""tests/synth_ref.py tied to the reference and to the kernels' shape arithmetic.  No GPU.

1. The fp64 references reproduce the goldens the reference itself wrote (g2_controls, g3_noise, g1_harmonic_small)
   within the goldens' own fp32 error: per frame within the reference side's share of each bound, and within the
   whole-tensor figures tests/test_oracle.py already holds the numpy oracle to.
2. On every case of tests/test_gpu_synth_shapes.py the reference side uses no more than its share of the bound the
   kernels are held to: the sequential fp32 model of the oscillator bank <= (HARM_FRAME_TOL - 3.4e-7) / 2, the
   fp32 torch oracle's filtered noise <= NOISE_FRAME_TOL / 4 (per frame, against the condition scale), and the
   constants are what their derivation says and within their caps.
3. Each case reaches the branch it is listed for: the kernels' shape arithmetic restated in synth_ref (frame_shape,
   frame_plan, shared_rev_frame, the fast test against kFastArgLimit, the two module kernels' dispatch) and
   asserted on.

Measured on one host (the oracle's figures depend on its FFT library: another host gave 2.6e-7 and 7.1e-7 where
this one gave 3.0e-7 and 7.3e-7; largest per-frame error against the scale): sequential model 8.11e-7 (Hcap; 5.4e-7 transition, 5.1e-7
N9, 4.4e-7 config, <= 2e-7 at H <= 17; in ascending k 3.4e-6 on transition, see test_summation_order); fp32 oracle
noise 3.0e-7 (transition; 9e-8 config, 1.2e-7 N6) and 7.3e-7 on N5b; fallback cases: model <= 1.5e-7, oracle
<= 2.3e-7.
"""
import numpy as np
import pytest

import synth_ref as sr
from conftest import load_golden, rms

ALL_FUSED = sr.all_fused_names()


# ------------------------------------------------------------------------------------------ 1. goldens
def test_golden_controls_and_harmonic():
    g = load_golden("g2_controls")
    bs = int(g["block_size"])
    amp, A = sr.harmonic_controls64(g["f0"], g["param"])
    np.testing.assert_allclose(g["amplitudes"], amp, rtol=2e-6)
    np.testing.assert_allclose(g["distribution_after_forward"], A, rtol=4e-6, atol=1e-12)
    ref, _ = sr.oscillator_ref(g["f0"], A, bs, model=False)
    e = sr.frame_err(g["out"], ref, np.abs(A).sum(-1))
    print(f"g2_controls: golden against the fp64 reference, per frame {e.max():.2e}")
    assert e.max() <= sr.HARM_MODEL_SHARE
    assert rms(g["out"].reshape(ref.shape), ref) < 1e-6


def test_golden_harmonic_small():
    g = load_golden("g1_harmonic_small")
    bs = int(g["block_size"])
    A = g["amp_frames"].astype(np.float64)
    ref, _ = sr.oscillator_ref(g["f0_frames"], A, bs, model=False)
    e = sr.frame_err(g["out"], ref, np.abs(A).sum(-1))
    print(f"g1_harmonic_small: golden against the fp64 reference, per frame {e.max():.2e}")
    assert e.max() <= sr.HARM_MODEL_SHARE
    assert rms(g["out"].reshape(ref.shape), ref) < 2e-7


def test_golden_noise():
    g = load_golden("g3_noise")
    bs = int(g["block_size"])
    nz, h, m = sr.noise_ref(g["mags"], g["noise_in"], bs)
    np.testing.assert_allclose(g["magnitudes"], m, rtol=2e-6)
    np.testing.assert_allclose(g["impulse"], h, atol=2e-7)
    e = sr.frame_err(g["out"], nz, np.abs(h).sum(-1))
    print(f"g3_noise: golden against the fp64 reference, per frame {e.max():.2e}")
    assert e.max() <= sr.NOISE_FRAME_TOL / 4
    assert rms(g["out"].reshape(nz.shape), nz) < 1e-7
    # the same taps from the golden's own scaled magnitudes, and the odd-length designs
    h2 = sr.impulse_response64(g["magnitudes"], bs)
    assert np.abs(h2 - g["impulse"]).max() <= 2e-7
    for target in (40, 20):
        np.testing.assert_allclose(g[f"ir_odd_{target}"], sr.impulse_response64(g["amp_odd"], target), atol=1e-6)


# ------------------------------------------------------------------------------------------ 2. the bounds
def test_constants_follow_their_derivation():
    raw = sr.SINE_TERM + 2 * sr.HARM_MODEL_MAX
    digit = 10.0 ** np.floor(np.log10(raw))
    assert np.isclose(sr.HARM_FRAME_TOL, np.ceil(raw / digit) * digit)  # rounded up to one significant digit
    assert sr.HARM_FRAME_TOL <= sr.HARM_FRAME_CAP == 3e-6
    assert sr.HARM_MODEL_MAX <= sr.HARM_MODEL_SHARE
    assert sr.NOISE_FRAME_TOL == 4 * sr.NOISE_ORACLE_MAX <= sr.NOISE_FRAME_CAP == 1.5e-6
    for name, own in sr.NOISE_OWN_ORACLE.items():
        assert 4 * own > sr.NOISE_FRAME_CAP, name  # only a case the cap cannot hold has a bound of its own


def model_err(c):
    return sr.frame_err(c["harm_model"], c["harm_ref"], c["harm_scale"])


@pytest.mark.parametrize("name", [n for n in ALL_FUSED if not n.endswith("/philox")])
def test_model_share(name):
    """The sequential fp32 model (the kernels' order: descending k) within its share of HARM_FRAME_TOL, per frame"""
    e = model_err(sr.fused_case(name))
    print(f"{name}: sequential model per frame {e.max():.2e} (median {np.median(e):.2e}), share "
          f"{sr.HARM_MODEL_SHARE:.2e}")
    assert e.max() <= sr.HARM_MODEL_SHARE, (name, float(e.max()))


def test_model_max_is_the_measured_figure():
    """HARM_MODEL_MAX, from which HARM_FRAME_TOL is derived, is the largest figure of test_model_share and
    test_fallback_shares to three digits, not a rounded-up one"""
    cases = [sr.fused_case(n) for n in ALL_FUSED if not n.endswith("/philox")]
    cases += [sr.fallback_case(n) for n in sr.FALLBACK_CASES]
    worst = max(float(model_err(c).max()) for c in cases)
    print(f"sequential model, largest per-frame error over all cases: {worst:.4e}")
    assert abs(worst - sr.HARM_MODEL_MAX) <= 0.005 * sr.HARM_MODEL_MAX


def test_summation_order():
    """Why the kernels sum from the highest harmonic down.  On "transition" one audible harmonic carries 0.9 of the
    scale and 1023 masked ones follow it in ascending k, each added to a sum of that size and rounded at its ulp:
    the ascending model is 3.4e-6 in the worst frame and past its share in more than half of them, which is what
    the device measured (3.35e-6) while its kernels summed that way.  Descending, the same case is 5.4e-7."""
    c = sr.fused_case("transition")
    _, up = sr.oscillator_ref(c["f0"], c["A"], c["bs"], descending=False)
    e_up = sr.frame_err(up, c["harm_ref"], c["harm_scale"])
    e_down = model_err(c)
    print(f"transition: ascending {e_up.max():.2e} (median {np.median(e_up):.2e}), descending {e_down.max():.2e}")
    assert e_up.max() > sr.HARM_FRAME_TOL and np.median(e_up) > sr.HARM_MODEL_SHARE
    assert e_down.max() <= sr.HARM_MODEL_SHARE and e_down.max() < e_up.max() / 4


@pytest.mark.parametrize("name", ALL_FUSED)
def test_noise_oracle_share(name):
    c = sr.fused_case(name)
    e = sr.frame_err(sr.oracle32_noise(c["mags"], c["noise"], c["bs"]), c["noise_ref"], c["noise_scale"])
    print(f"{name}: fp32 oracle noise per frame {e.max():.2e}, share {sr.noise_oracle_share(name):.2e}")
    assert e.max() <= sr.noise_oracle_share(name), (name, float(e.max()))
    assert sr.noise_tol(name) <= sr.NOISE_FRAME_CAP or name.partition("/")[0] in sr.NOISE_OWN_ORACLE


@pytest.mark.parametrize("name", sorted(sr.FALLBACK_CASES))
def test_fallback_shares(name):
    c = sr.fallback_case(name)
    e = model_err(c)
    assert e.max() <= sr.HARM_MODEL_SHARE, (name, float(e.max()))
    for (kind, raw), (nz, scale) in c["noise_refs"].items():
        x = c["noise"] if kind == "inject" else c["philox"]
        o = sr.oracle32_noise(c["mags"] if raw else c["scaled"], x, c["bs"], sr.BIAS if raw else None)
        en = sr.frame_err(o, nz, scale)
        print(f"{name} {kind} raw={raw}: model {e.max():.2e}, fp32 oracle noise {en.max():.2e}")
        assert en.max() <= sr.NOISE_ORACLE_MAX, (name, kind, raw, float(en.max()))


def test_metric_sees_one_sample():
    """One sample of one quiet frame off by 1e-4 of that frame's scale: far inside the suite's absolute
    whole-tensor bounds (rms < 1e-7 on the noise, < 1e-6 on the sum), 78 times NOISE_FRAME_TOL per frame."""
    c = sr.fused_case("config")
    got = c["noise_ref"].copy()
    b, f = np.unravel_index(np.argmin(c["noise_scale"]), c["noise_scale"].shape)
    got[b, f, 511] += 1e-4 * c["noise_scale"][b, f]
    assert rms(got, c["noise_ref"]) < 1e-9
    e = sr.frame_err(got, c["noise_ref"], c["noise_scale"])
    assert (b, f) == np.unravel_index(np.argmax(e), e.shape)
    assert abs(e[b, f] - 1e-4) < 1e-12 and e.sum() == e[b, f]
    assert e.max() > 75 * sr.NOISE_FRAME_TOL
    # in the sum the same fault is 0.09 of the signal's bound (the harmonic scale dominates it): the parts are
    # checked on their own for that reason
    assert sr.signal_err(c["harm_ref"] + got, c).max() < 1


def test_metric_zero_scale_and_nan():
    ref = np.ones((1, 3, 4))
    scale = np.array([[1.0, 0.0, 1.0]])
    ref[0, 1] = 0
    got = ref.copy()
    assert sr.frame_err(got, ref, scale).tolist() == [[0.0, 0.0, 0.0]]
    got[0, 1, 2] = 1e-30
    got[0, 2, 0] = np.nan
    assert sr.frame_err(got, ref, scale).tolist() == [[0.0, np.inf, np.inf]]
    assert sr.control_err(np.array([1.0, np.nan]), np.array([1.0, 2.0]), "amplitudes") == np.inf


# ------------------------------------------------------------------------------------------ 3. the branches
def shape_of(name):
    c = sr.fused_case(name)
    return c, sr.frame_shape(c["NB"], c["bs"]), sr.frame_plan(c["B"], c["F"], c["H"], c["NB"], c["bs"])


@pytest.mark.parametrize("name", ALL_FUSED)
def test_launch_forms(name):
    """batch form: unsplit, 512 <= B F <= 1024 and no prefix; "/prefix": F > FRAME_PREFIX_MIN_FRAMES; the SPLIT
    slice launches G > 1 thread groups; only the shapes with nt = 256 have no SPLIT form"""
    c, _, plan = shape_of(name)
    assert sr.in_envelope(c["H"], c["NB"], c["bs"], c["B"])
    assert plan["G"] == 1 and 512 <= c["B"] * c["F"] <= 1024
    assert plan["prefix"] == name.endswith("/prefix") == (c["F"] > sr.FRAME_PREFIX_MIN_FRAMES)
    sl = sr.split_slice(name)
    if sl is None:
        assert plan["prefix"] or plan["nt"] == 256
    else:
        items, frames = sl
        assert 1 <= items <= c["B"] and 1 <= frames <= c["F"]
        sp = sr.frame_plan(items, frames, c["H"], c["NB"], c["bs"])
        assert sp["G"] == 256 // plan["nt"] > 1 and sp["NT"] == 256 and not sp["prefix"]


# name -> (two_run, dpp_tail, nt, irfft in the batch form); the SPLIT form has NT = 256 and, at 65 bands, "pair"
NOISE_BRANCHES = {
    "config": (True, True, 128, "pair"),
    "N2": (True, True, 64, "general"),
    "N2b": (True, True, 128, "pair"),
    "N3a": (True, True, 64, "general"),
    "N3b": (True, False, 64, "general"),
    "N4": (True, False, 64, "general"),
    "N5a": (False, False, 64, "general"),
    "N5b": (False, False, 64, "general"),
    "N6": (True, False, 64, "general"),
    "N6b": (False, False, 64, "general"),
    "N7": (False, False, 64, "general"),
    "N8": (True, False, 64, "general"),
    "N9": (True, False, 256, "general"),
    "N10": (False, False, 256, "general"),
}


@pytest.mark.parametrize("name", sorted(NOISE_BRANCHES))
def test_noise_branches(name):
    two_run, dpp, nt, irfft = NOISE_BRANCHES[name]
    c, fs, plan = shape_of(name)
    assert (fs["two_run"], fs["dpp_tail"], plan["nt"], plan["irfft"]) == (two_run, dpp, nt, irfft)
    sl = sr.split_slice(name)
    assert (sl is None) == (nt == 256)
    if sl:  # 256 threads build the frame: at 65 bands by the lane-pair irfft whatever the block
        sp = sr.frame_plan(*sl, c["H"], c["NB"], c["bs"])
        assert sp["NT"] == 256 > plan["NT"] and sp["irfft"] == ("pair" if c["NB"] == 65 else "general")
    # the FIR's two runs stay inside the frame and its padding
    assert 0 < fs["lo_end"] <= fs["tail_start"] <= c["bs"] and fs["lo_end"] % 4 == 0 and fs["pad"] >= fs["lo_end"] + 4
    if fs["dpp_tail"]:
        assert fs["tail_start"] - 63 >= fs["lo_end"]  # the 63 zeroed taps below tail_start do not reach the first run


def test_noise_branch_edges():
    bs, n = (lambda name: sr.fused_case(name)["bs"]), (lambda name: sr.frame_shape(sr.fused_case(name)["NB"], 4)["n"])
    # N3: 192 is the smallest block that takes the DPP triangle at 65 bands, 188 the first below it
    assert sr.frame_shape(65, 192)["dpp_tail"] and not any(sr.frame_shape(65, b)["dpp_tail"] for b in range(4, 192, 4))
    assert bs("N3b") == 188 and sr.frame_shape(65, 188)["two_run"]
    # N2 / N2b: 256 is the largest block on irfft_tap at 65 bands, 260 the smallest on the lane-pair irfft
    assert (bs("N2"), bs("N2b")) == (256, 260)
    fs = sr.frame_shape(65, bs("N4"))  # N4: the two runs meet
    assert fs["two_run"] and fs["tail_start"] == fs["lo_end"] == fs["half"]
    assert bs("N5a") < n("N5a") <= 2 * bs("N5a") and n("N5b") > 2 * bs("N5b")
    c6 = sr.fused_case("N6")
    assert sr.frame_shape(18, 64)["half"] == 17 and 4096 % n("N6") != 0 and c6["H"] % 4 == 1
    fs = sr.frame_shape(18, bs("N6b"))  # N6b: bs >= n and still one run (the second would overlap the first)
    assert bs("N6b") >= fs["n"] and not fs["two_run"] and bs("N6b") - fs["half"] < sr.roundup4(fs["half"])
    c7 = sr.fused_case("N7")  # the envelope's floor
    assert (c7["H"], sr.roundup4(c7["H"]), c7["bs"] // 4, n("N7")) == (1, 4, 1, 2)
    assert not sr.in_envelope(1, 2, 0) and not sr.in_envelope(0, 2, 4) and not sr.in_envelope(1, 1, 4)
    assert n("N8") == bs("N8") and n("N9") == bs("N9") == 1024
    c10 = sr.fused_case("N10")
    assert c10["NB"] == 1025 and not sr.in_envelope(4, 1026, 1024) and n("N10") > bs("N10")
    assert sr.fused_case("Hcap")["H"] == 1024 and not sr.in_envelope(1025, 9, 64)
    assert not sr.in_envelope(8, 65, 1028) and not sr.in_envelope(8, 65, 441)


def test_oscillator_loops():
    """which of the three sine loops each harmonic case's frames take"""
    def lp(name):
        c = sr.fused_case(name)
        assert sr.shared_rev_margin(c["f0"], c["H"]).min() > 1e-3, name  # no frame sits on the guard
        return c, sr.loops(c["f0"], c["H"], c["bs"])

    for name in ("config", "N2", "N6", "N7", "H12", "Hcap", "config/prefix", "N6/prefix"):
        c, l = lp(name)
        assert l["shared"].all() and not l["persample"].any() and not l["general"].any(), name
    c, _ = lp("H12")
    assert sr.roundup4(c["H"]) == 12 and (12 // 4) % 2 == 1  # three trips of the four-harmonic loop
    c, _ = lp("Hcap")
    assert (c["f0"] * np.float32(1024) < 24000).all()  # every one of the 1024 harmonics audible
    for name in ("persample", "persample/prefix"):
        c, l = lp(name)
        assert l["persample"].all() and not l["shared"].any() and not l["general"].any(), name
        audible = (c["f0"] * np.arange(1, c["H"] + 1, dtype=np.float32) < 24000).sum(-1)
        assert 3000 <= c["f0"].min() and c["f0"].max() <= 9000 and audible.min() >= 2 and audible.max() <= 7
    c, l = lp("nyquist")  # both throughput loops in one launch
    assert l["shared"].any() and l["persample"].any() and not l["general"].any()


@pytest.mark.parametrize("name,shared", [("transition", False), ("transition_shared", True)])
def test_transition_frames(name, shared):
    """frames entirely fast, exactly one frame with fast and general quads side by side, then frames on the general
    loop with sin_slow; the SPLIT slice of "transition" holds all three kinds"""
    c = sr.fused_case(name)
    assert (sr.shared_rev_frame(c["f0"], c["H"]) == shared).all()
    fq = sr.fast_quads(c["f0"], c["H"], c["bs"])[0]  # [F, quads]
    mixed = np.flatnonzero(fq.any(-1) & ~fq.all(-1))
    assert len(mixed) == 1
    x = int(mixed[0])
    assert fq[:x].all() and not fq[x + 1:].any() and 0 < x < c["F"] - 1
    q = int(np.flatnonzero(~fq[x])[0])
    assert fq[x, :q].all() and not fq[x, q:].any() and 0 < q < fq.shape[1]
    # past the limit the arguments themselves exceed it: sin_slow runs
    w = sr.frame_phase(c["f0"], c["bs"])
    assert np.abs(w[0, -1] * np.float32(c["H"])).max() >= sr.FAST_ARG_LIMIT
    sl = sr.split_slice(name)
    if name == "transition":
        assert x == 46 and sl == (1, 128)
    else:
        assert sl is None  # nt = 256


def test_nyquist_case():
    c = sr.fused_case("nyquist")
    f0 = c["f0"][0, :, 0]
    k = np.arange(1, c["H"] + 1, dtype=np.float32)
    half = np.float32(sr.SR / 2)
    n_set = 2 + 3 * (len(sr.NYQUIST_EXACT) + 1) + 1
    assert (c["f0"][:, :n_set] == c["f0"][:1, :n_set]).all()  # every item has the same set frames, then its own
    assert (f0[:2] == 0).all() and (c["harm_ref"][:, :2] == 0).all()  # the phase has not moved: exactly silent
    for i, v in enumerate(sr.NYQUIST_EXACT):
        lo, at, hi = f0[2 + 3 * i:5 + 3 * i]
        assert lo < at == np.float32(v) < hi
        hit = np.flatnonzero(at * k == half)
        assert len(hit) == 1  # a product exactly equal to sr / 2: masked by `<`
        j = hit[0]
        assert lo * k[j] < half and not at * k[j] < half and not hi * k[j] < half
        # the coefficient of that harmonic drops by the mask's 1e-4 between the two neighbouring frames
        A = c["A"][0, 2 + 3 * i:5 + 3 * i, j] / c["amplitudes"][0, 2 + 3 * i:5 + 3 * i, 0]
        assert A[1] < 1e-3 * A[0] * 10 or A[0] > 100 * A[1]
    i0 = 2 + 3 * len(sr.NYQUIST_EXACT)
    assert (f0[i0:i0 + 3] * k[0] >= half).all() and f0[i0 + 1] == sr.NYQUIST_ALL_MASKED  # every harmonic masked
    assert f0[i0 + 3] == 0 and np.abs(c["harm_ref"][:, i0 + 3]).max() > 0  # silent pitch, standing phase


def test_philox_cases_share_their_base():
    for base in sr.PHILOX_CASES:
        c, b = sr.fused_case(base + "/philox"), sr.fused_case(base)
        assert c["param"] is b["param"] and c["harm_ref"] is b["harm_ref"]
        assert not np.array_equal(c["noise"], b["noise"]) and np.abs(c["noise"]).max() < 1
        assert c["noise"].shape == (c["B"], c["F"], c["bs"])


# name -> harmonic (SPT, nt, passes); noise (layout, vec4_load, vec4_store, table128, fir_passes)
FALLBACK_BRANCHES = {
    "F441": ((4, 128, 1), ("two-run", False, False, True, 1)),
    "F30": ((2, 64, 1), ("cropped", False, False, False, 1)),
    "F6": ((2, 64, 1), ("two-run", False, False, False, 1)),
    "F1": ((2, 64, 1), ("cropped", False, False, True, 1)),
    "F2048": ((4, 256, 2), ("two-run", True, True, False, 4)),
    "F255": ((2, 128, 1), ("two-run", False, False, False, 1)),
    "F256": ((4, 64, 1), ("two-run", True, True, True, 1)),
    "F36": ((2, 64, 1), ("two-run", True, False, False, 1)),
    "F35": ((2, 64, 1), ("overlap", False, False, False, 1)),
    "F128": ((2, 64, 1), ("two-run", True, True, False, 1)),
    "F129": ((2, 64, 2), ("two-run", False, False, False, 1)),
    "F130": ((2, 128, 1), ("two-run", False, False, False, 1)),
    "F1028": ((4, 256, 2), ("two-run", True, False, True, 3)),
    "Fslow": ((4, 128, 1), ("two-run", False, False, False, 1)),
}


@pytest.mark.parametrize("name", sorted(sr.FALLBACK_CASES))
def test_fallback_branches(name):
    H, NB, bs = sr.FALLBACK_CASES[name]
    harm, noise = FALLBACK_BRANCHES[name]
    assert sr.harmonic_fallback_plan(bs) == harm
    p = sr.noise_fallback_plan(NB, bs)
    assert (p["layout"], p["vec4_load"], p["vec4_store"], p["table128"], p["fir_passes"]) == noise
    assert not sr.in_envelope(H, NB, bs) or name in ("F256", "F36", "F128")  # these three the fused kernel takes too
    B, F, _ = sr.fallback_shape(name)
    assert (B * F) % 4 != 0  # the last noise workgroup has idle waves


def test_fallback_general_loop():
    """Fslow reaches harmonic_frames_kernel's general loop (a thread whose SPT samples, t, t + nt, ... past the
    block included, are not all below kFastArgLimit): frames 0-5 wholly on the fast loop, frames 6-12 wholly on the
    general loop, frame 6 with samples either side of the limit (the loop's choice between sin_reduced and
    sin_slow per term)"""
    c = sr.fallback_case("Fslow")
    spt, nt, passes = sr.harmonic_fallback_plan(c["bs"])
    assert passes == 1
    H4 = np.float32(sr.roundup4(c["H"]))
    w = sr.frame_phase(c["f0"], c["bs"])[0]  # [F, bs]
    inc = sr.no.phase_increment(c["f0"][0, :, 0], sr.SR).astype(np.float64)
    start = np.concatenate([[0.0], np.cumsum(inc * c["bs"])[:-1]])
    wp = (start[:, None] + np.arange(1, nt * spt + 1)[None, :] * inc[:, None]).astype(np.float32)
    assert np.array_equal(wp[:, :c["bs"]], w)  # the kernel's formula, extended to the samples past the block
    thread_fast = (np.abs(wp) * H4 < sr.FAST_ARG_LIMIT).reshape(c["F"], spt, nt).all(1)
    assert thread_fast[:6].all() and not thread_fast[6:].any()
    fast = np.abs(w) * H4 < sr.FAST_ARG_LIMIT
    assert fast[6].any() and not fast[6].all() and not fast[7:].any()
    assert (np.abs(w[-1]) * np.float32(c["H"])).max() >= sr.FAST_ARG_LIMIT


def test_fallback_boundaries():
    """the cases sit either side of each boundary of launch_frames"""
    plan = sr.harmonic_fallback_plan
    assert plan(255)[0] == 2 and plan(256)[0] == 4  # SPT
    assert plan(128)[2] == 1 and plan(129)[2] == 2  # SPT = 2 at 64 threads: a second pass of one sample
    assert plan(129)[1] == 64 and plan(130)[1] == 128  # SPT = 2: a second wave
    assert plan(1024)[2] == 1 and plan(1028)[2] == 2  # SPT = 4 at 256 threads: a second pass
    for bs in (255, 256, 128, 129, 130, 1028):
        assert any(v[2] == bs for v in sr.FALLBACK_CASES.values())
