"""The pitch gradient's yardstick (tests/f0_grad_ref.py) tied to the oracle on the CPU: the closed form is what the
reference's autograd computes, and the bound the device is held to is one the reference's own fp32 autograd meets
with room to spare.

* With nothing rounded to fp32, the closed form equals the fp64 autograd of oracle/torch_ref.py's
  harmonic_controls + harmonic_forward within 1e-7 relative L2 on every case (the two differ by the order of their
  fp64 sums and by the cancellation in cos at large arguments; measured 1e-16 to 9e-10, and 3.2e-8 on "slow",
  whose arguments reach 1.2e7 rad).
* The fp32 oracle's autograd, the reference by itself, stays within a quarter of the per-frame bound
  (FRAME_TOL / 4 = 5e-7 of the frame's condition scale) of the closed form with the reference's fp32 rounding
  points, and within GRAD_REL / 4 of it as a whole tensor, on every case: the bound leaves the kernels three
  quarters of itself.
"""
import pytest
import torch

import f0_grad_ref as fr
import vjp_ref as vr

FP64_REL = 1e-7


def test_cases_are_the_issue_table():
    assert set(fr.CASES) >= {"c8", "m16", "b4", "odd", "h1", "high", "nyq", "sub", "f441", "f1", "slow", "long"}
    assert fr.CASES["scan_below"] == (4, 4, 2, fr.SCAN_CHUNK - 1, "low")
    assert fr.CASES["scan_above"] == (4, 4, 2, fr.SCAN_CHUNK + 1, "low")
    assert fr.CASES["long"][3] > 512 and fr.CASES["odd"][1] % 4 == 0 and fr.CASES["odd"][0] % 4
    assert fr.FRAME_TOL == 2e-6 and fr.FRAME_CAP == 3e-6 and fr.GRAD_REL == 1e-5


@pytest.mark.parametrize("name", sorted(fr.CASES))
def test_closed_form_is_the_fp64_autograd(name):
    c = fr.case(name)
    want = fr.oracle_f0_grad(c["f0"], c["param"], c["g"], c["bs"], torch.float64)
    got, _ = fr.params_ref(c["f0"], c["param"], c["g"], c["bs"], points="fp64")
    e = vr.relerr(got, want)
    print(f"{name}: closed form vs fp64 autograd {e:.2e}")
    assert e <= FP64_REL, (name, e)


@pytest.mark.parametrize("name", sorted(fr.CASES))
def test_fp32_oracle_meets_a_quarter_of_the_bound(name):
    c = fr.case(name)
    got = fr.oracle_f0_grad(c["f0"], c["param"], c["g"], c["bs"], torch.float32)
    e = float(fr.frame_err(got, c["grad_params"], c["scale_params"]).max())
    w = vr.relerr(got, c["grad_params"])
    print(f"{name}: fp32 oracle per frame {e:.2e}, whole {w:.2e}")
    assert e <= fr.FRAME_TOL / 4, (name, e)
    assert w <= fr.GRAD_REL / 4, (name, w)


def test_zero_scale_frames_are_exact():
    """b4's last frames have a zero upstream gradient and nothing after them: scale and gradient exactly zero, and
    the metric reads inf for anything else there"""
    c = fr.case("b4")
    tail = fr.ZERO_TAIL["b4"]
    assert (c["scale_params"][:, -tail:] == 0).all() and (c["grad_params"][:, -tail:] == 0).all()
    assert (c["scale_params"][:, :-tail] > 0).all()
    bad = c["grad_params"].clone()
    bad[0, -1] = 1e-30
    assert float(fr.frame_err(c["grad_params"], c["grad_params"], c["scale_params"]).max()) == 0.0
    assert float(fr.frame_err(bad, c["grad_params"], c["scale_params"]).max()) == float("inf")


def test_frame_route_reference_is_close_to_the_param_route():
    """the frame route's A is the param route's rounded to fp32 controls: the two references agree to fp32 rounding"""
    for name in ("c8", "nyq"):
        c = fr.case(name)
        assert vr.relerr(c["grad_frames"], c["grad_params"]) <= 1e-6
