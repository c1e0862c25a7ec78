"""tests/pitch_ref.py, the yardstick of the pitch tracker, tied to independent ground on the CPU: known
frequencies, an FFT correlation, the frames the rules decide by themselves, and the absence of near-ties on the
inputs of the GPU tests."""
import math

import numpy as np
import pytest

import pitch_cases as pc
import pitch_ref as pr

TONES = (110.0, 220.5, 440.0, 987.77, 1500.0)


@pytest.mark.parametrize("sr,hop,T", [(48000, 512, 8192), (16000, 160, 4000)])
def test_steady_tones_come_out_within_ten_cents(sr, hop, T):
    """The issue's prototype measured <= 7.6 cents with edge frames included; more than 10 on frames whose window
    lies inside the signal means the restatement departs from the definition."""
    L = 2048
    tmin, tmax = pr.lags(sr, 50.0, 2000.0, L)
    worst = 0.0
    for f in TONES:
        x = pr.steady_tone(sr, T, f, seed=int(f))
        Y = pr.offline_frames(x, L, hop)
        start = np.arange(len(Y)) * hop - L // 2
        inside = (start >= 0) & (start + L <= T)
        assert inside.sum() >= 4
        f0, conf, _ = pr.pitch_frames(Y[inside], sr, tmin, tmax, 0.1, np.float64)
        cents = np.abs(1200.0 * np.log2(f0 / f))
        print(f"sr {sr} tone {f}: worst {cents.max():.2f} cents, confidence >= {conf.min():.3f}")
        worst = max(worst, cents.max())
        assert conf.min() > 0.8
    assert worst <= 10.0, worst


def test_difference_function_matches_an_fft_correlation():
    from scipy import signal
    x = pr.make_voiced(48000, 6144, 1, seed=5)[0].astype(np.float64)
    for L in (256, 2048):
        W = L // 2
        y = x[1000:1000 + L]
        E, r, d = pr.difference(y, W, np.float64)
        full = signal.fftconvolve(y, y[:W][::-1])  # full[W - 1 + tau] = sum_j y[j] y[j + tau]
        r_fft = full[W - 1:W - 1 + W + 1]
        c = np.concatenate([[0.0], np.cumsum(y * y)])
        E_scan = c[np.arange(W + 1) + W] - c[np.arange(W + 1)]
        d_fft = E_scan[0] + E_scan - 2.0 * r_fft
        tot = E[0] + E
        assert (np.abs(d_fft - (tot - 2.0 * r)) <= 1e-10 * tot).all()
        assert (np.abs(np.where(d_fft < 2.0 ** -40 * tot, 0.0, d_fft) - d) <= 1e-10 * tot).all()


def test_frames_the_rules_decide():
    sr, L = 48000, 2048
    W = L // 2
    tmin, tmax = pr.lags(sr, 50.0, 2000.0, L)
    assert (tmin, tmax) == (24, 960)
    for dt in (np.float64, np.float32):
        # silence: d = 0, S = 0, d' = 1 everywhere -> tau_min, sr / tau_min, confidence 0
        f0, conf, per = pr.pitch_frames(np.zeros((1, L)), sr, tmin, tmax, 0.1, dt)
        assert per[0] == tmin and f0[0] == dt(sr) / dt(tmin) and conf[0] == 0.0
        assert f0.dtype == dt and conf.dtype == dt and per.dtype == np.int32
        # the first W samples zero: r = 0, d = E(tau) non-decreasing, d' >= 1 where S > 0 -> tau_min again
        y = np.zeros(L)
        y[W + 300:] = pr.steady_tone(sr, L, 440.0)[W + 300:]
        E, r, d = pr.difference(y, tmax + 1, dt)
        assert E[0] == 0.0 and not r.any() and np.array_equal(d, E) and d[300] == 0.0 and d[302] > 0.0
        f0, conf, per = pr.pitch_frames(y[None], sr, tmin, tmax, 0.1, dt)
        assert per[0] == tmin and f0[0] == dt(sr) / dt(tmin) and conf[0] == 0.0
        # an exactly periodic square wave of integer period: d(tau0) = 0 exactly, so b = d'(tau0) = 0 is the first
        # dip under the threshold; the parabola through (a, 0, c) shifts by s = (a - c) / (2 (a + c)), and
        # confidence = 1 + (a - c) s / 4 >= 1 (the rules cap the subtracted term from above only)
        tau0 = 100
        sq = np.where((np.arange(L) % tau0) < tau0 // 2, 0.25, -0.25)
        _, _, d = pr.difference(sq, tmax + 1, dt)
        assert d[tau0] == 0.0 and d[2 * tau0] == 0.0 and d[tau0 - 1] > 0.0
        dn = pr.normalise(d, dt)
        a, c = float(dn[tau0 - 1]), float(dn[tau0 + 1])
        assert dn[tau0] == 0.0 and a > 0.0 and c > 0.0
        shift = 0.5 * (a - c) / (a + c)
        f0, conf, per = pr.pitch_frames(sq[None], sr, tmin, tmax, 0.1, dt)
        assert per[0] == tau0 and abs(shift) < 0.5
        assert abs(f0[0] / (sr / (tau0 + shift)) - 1.0) < 1e-6
        assert abs(conf[0] - (1.0 + 0.25 * (a - c) * shift)) < 1e-6 and conf[0] >= 1.0
    # the floor: a difference of 1e-16 E, as a transform would return, is taken for the zero it stands for
    E = 3.0
    assert (np.array([1e-16 * E]) < 2.0 ** -40 * 2 * E).all()


def _no_near_ties(ref, what):
    diff = int((ref["period32"] != ref["period64"]).sum())
    rel = np.abs(ref["f032"].astype(np.float64) / ref["f064"] - 1.0)
    print(f"{what}: {ref['period64'].size} frames, {diff} period differences, fp32 f0 rel max {rel.max():.2e}, "
          f"conf abs max {np.abs(ref['conf32'] - ref['conf64']).max():.2e}")
    assert diff == 0, what


def test_the_gpu_tests_inputs_have_no_near_ties():
    for case in pc.OFFLINE:
        _no_near_ties(pc.offline_case(*case)[2], f"offline {case}")
    for L in pc.SIZES:
        _no_near_ties(pc.size_case(L)[2], f"frame_length {L}")
    for case in pc.STREAM:
        x, _, ref = pc.stream_case(*case)
        _no_near_ties(ref, f"stream {case}")
        sr, hop, N, B, L, K = case
        d = -(-(L // 2) // hop)
        # the frames before the stream (f < 0) are silent frames
        assert (ref["period64"][:, :d - 1] == pr.lags(sr, 50.0, 2000.0, L)[0]).all()
        assert not ref["conf64"][:, :d - 1].any()


def test_every_size_case_keeps_its_period_in_range():
    for L in pc.SIZES:
        hop, T, fmin, f_lo, f_hi = pc.size_params(L)
        assert math.isclose(pc.SIZES_SR / f_hi, 4.0) and math.isclose(pc.SIZES_SR / f_lo, L // 4)
        tmin, tmax = pc.size_case(L)[1]
        assert 1 <= tmin <= tmax <= L // 2 - 1


def test_host_lags_are_the_formulas():
    """tau_min = max(floor(sr / fmax), 1), tau_max = min(ceil(sr / fmin), L - W - 1) for the defaults (50 Hz,
    2000 Hz, L 2048), written out."""
    from ddsp_pytorch_amd import core
    want = {48000: (24, 960), 16000: (8, 320), 44100: (22, 882)}
    for sr, lag in want.items():
        assert core.pitch_lags(sr, 50.0, 2000.0, 2048) == lag
        assert pr.lags(sr, 50.0, 2000.0, 2048) == lag
    assert core.pitch_lags(48000, 20.0, 2000.0, 2048) == (24, 1023)   # capped at L - W - 1
    assert core.pitch_lags(48000, 50.0, 96000.0, 2048) == (1, 960)    # floored at 1
    with pytest.raises(RuntimeError, match="no lag"):
        core.pitch_lags(16000, 50.0, 100.0, 64)                        # floor(160) > 31
