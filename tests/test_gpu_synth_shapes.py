"""The forward synthesis kernels (csrc/synth_frame.hip: synth_frame_kernel / frame_synth; outside its envelope
csrc/synth.hip: harmonic_frames_kernel and csrc/noise.hip: filtered_noise_kernel) at every branch their shape
arithmetic takes, against the fp64 references of tests/synth_ref.py, checked PER FRAME: max_j |got - ref| of each
frame against the frame's condition scale (sum_k |A_k| for the harmonic part, sum_m |h_m| for the filtered noise,
both for the signal) <= HARM_FRAME_TOL = 2e-6, NOISE_FRAME_TOL = 1.28e-6 and their scale-weighted mean plus an ulp
for the signal; the three controls within the tolerances of test_synth_frames_controls_output.  The whole-tensor
absolute bounds of the other forward tests (rms < 1e-6, < 1e-7 on the noise) are relative bounds of 1e-4 to 1e-3
on the noise part at the model's bias of -5, and do not see one wrong frame, tap or sample; these do.
tests/test_synth_ref.py derives the two constants from the reference side's own error on every case and proves
each case onto the branch listed here.  Every launch runs on a NaN-poisoned allocator with parts=True,
controls=True, so a band or frame a kernel skips does not come back holding an earlier run's value.

Sample rate 48000, raw controls randn, noise U[-1, 1), bias -5, pitch 50 Hz - 1 kHz per frame unless said.

Every fused case runs in up to three launch shapes (frame_plan):
  batch   512 <= B F <= 1024, F <= 512: the 4-samples-per-thread kernels (what config 2 and bench.py run);
  SPLIT   the first items (or, for one item, frames) of the same inputs with B' F' < 512: G = 256 / nt thread groups
          per frame, one sample per thread.  Every output must equal the batch form's bit for bit; nt = 256 has none;
  PREFIX  B = 1, F = 520 > FRAME_PREFIX_MIN_FRAMES (inputs of their own): frame_phase_prefix, then the PREFIX kernels.

  case (H, NB, bs), B x F        what it reaches (n = 2 (NB - 1) taps; nt threads per frame)
  config (100, 65, 512) 2x256    lane-pair irfft (n == 128, NT >= 128), two-run FIR, DPP tap triangle, nt = 128; the
                                 O(f) phase prefix over two passes of 128 threads; also PREFIX, Philox, strides
  N2 (64, 65, 256)               batch NT = 64: general irfft_tap at n = 128 (tap 32 by irfft128_tap32), DPP tail;
                                 SPLIT NT = 256 takes the lane-pair irfft and agrees bit for bit.  It did not: the
                                 two paths summed tap 32 in different orders, and N2, N3a, N3b, N4 and N5a differed
                                 between the forms in 24 to 161 of 448 frames (the finding that added irfft128_tap32)
  N2b (8, 65, 260)               the smallest block on the lane-pair irfft in the batch form (nt = 128, 65 of its
                                 threads with samples)
  N3a (8, 65, 192)               the DPP tail's smallest block (bs - 127 = 65 >= lo_end = 64)
  N3b (8, 65, 188)               the first block below it: two-run, general tail loop
  N4 (8, 65, 128)                n == bs: two runs that meet (tail_start == lo_end == n/2), general tail
  N5a (8, 65, 64)                bs < n <= 2 bs: one run, cropped taps (also Philox)
  N5b (8, 65, 8)                 n > 2 bs: the tap index wraps (ir_at_half's q % target); noise bound of its own,
                                 3.1e-6 (synth_ref.NOISE_OWN_ORACLE: the fp32 oracle is 7.3e-7 there; also Philox,
                                 two quads per frame)
  N6 (17, 18, 64)                n/2 = 17 odd: n = 34 (cospi table, modular irfft_tap), padded tables; H % 4 = 1
                                 (also PREFIX, Philox)
  N6b (17, 18, 36)               bs >= n and still one run: bs - n/2 = 19 < roundup4(n/2) = 20
  N7 (1, 2, 4)                   the envelope's floor: H4 = 4 with three padded harmonics, empty cosine loop, one
                                 quad, one run
  N8 (4, 33, 64)                 n == bs at n = 64
  N9 (128, 513, 1024)            n == bs at the block cap; nt = 256, no SPLIT form
  N10 (4, 1025, 1024)            the band cap, n = 2048 > bs; nt = 256
  Hcap (1024, 9, 64)             the harmonic cap, pitch 12-23 Hz: all 1024 harmonics audible, shared-count loop
  H12 (12, 9, 64)                H4 = 12: three trips (odd) of the four-harmonics-per-iteration shared loop
  persample (100, 9, 64)         pitch log-uniform 3-9 kHz: every frame past the shared-count guard (1.8 kHz at
                                 H = 100) on the per-sample loop osc_bank4; 2 to 7 audible harmonics, 93+ masked
                                 (also PREFIX)
  transition (1024, 9, 64) 1x512 constant 20 kHz: |omega| H4 crosses 8e6 in frame 46: frames 0-45 on osc_bank4,
                                 frame 46 with fast and general quads side by side, frames 47+ on the general loop
                                 with sin_slow.  SPLIT: the first 128 frames, bit for bit.  One audible harmonic and
                                 1023 masked ones: 3.35e-6 while the loops summed in ascending k (the finding that
                                 turned the coefficient table round; test_synth_ref.py::test_summation_order)
  transition_shared (8, 9, 1024) constant 21 kHz, 1x512: the same crossing (frame 355) from the shared-count loop;
                                 nt = 256
  nyquist (48, 9, 64)            pitches 500, 1000, 2000, 12000, 8000, 4800, 1500, 960: f0 k == sr/2 exactly for one
                                 k (masked by `<`), each with the fp32 value below and above it; 30000 (every
                                 harmonic masked); f0 = 0 from the start (exactly silent) and after the phase moved;
                                 shared and per-sample frames in one launch
  strides                        config: param and mags as column slices of wider buffers (ldp = H + 8,
                                 ldm = NB + 5, bases 12 and 8 bytes into their rows), bit-equal to the contiguous call
  */philox                       config, N5a, N5b, N6: noise=None with a pinned (seed, offset 2^32 + 5) through core._synth_frames_launch;
                                 the reference filters oracle/philox.py's samples

Template instantiations: RNG x SPLIT x PREFIX all with CTRL = true (the launches here); CTRL = false is tied to them
by test_synth_frames_controls_output's bit equality.  Not here: CARRY (synth_stream_kernel), which
tests/test_gpu_stream.py ties to these kernels by chunked against one-shot equality.  Unreachable: PREFIX with SPLIT
(synth_frames_launch never splits a launch that reads a prefix); frame_plan's LDS guard (cannot bind under the
caps: 45,104 bytes at most); the shared-count loop's crossing of kFastArgLimit in the SPLIT form (the guard
2 H4 inc / 2 pi < 7.5 puts the crossing past sample 340,000, and a SPLIT launch has at most 511 frames of 512).

The two module kernels, the route core.synth_signal takes outside the envelope: core.harmonic_synth_params, then
core.filtered_noise(..., add=harmonic, raw_bias=), B x F = 2 x 5 (the last noise workgroup has idle waves), each
with raw (bias -5) and pre-scaled magnitudes, injected and Philox noise (filtered_noise_kernel<RNG, RAW>: all four):
  case (H, NB, bs)      harmonic_frames_kernel<SPT, RAW=1>, nt, passes | filtered_noise_kernel: layout,
                        (bs & 3) == 0 float4 noise loads, (bs & 7) == 0 float4 stores, n == 128 table, FIR passes
  F441 (17, 65, 441)    <4> 128, 1 | two-run, scalar loads, scalar stores, table, 1  (the bs of 44.1 kHz models)
  F30 (5, 33, 30)       <2> 64, 1  | cropped (n > bs: every tap in the windowed loop), scalar, scalar, irfft_tap, 1
  F6 (3, 2, 6)          <2> 64, 1  | two-run at NB = 2 (empty cosine loop), scalar, scalar, irfft_tap, 1
  F1 (3, 65, 1)         <2> 64, 1  | cropped at bs = 1, scalar, scalar, table, 1
  F2048 (8, 33, 2048)   <4> 256, 2 | two-run, float4, float4, irfft_tap, 4 passes of 512 outputs
  F255 (8, 33, 255)     <2> 128, 1 | two-run, scalar, scalar: below the SPT boundary
  F256 (8, 65, 256)     <4> 64, 1  | two-run, float4, float4, table: above the SPT boundary
  F36 (4, 9, 36)        <2> 64, 1  | two-run, float4 loads, scalar stores
  F35 (4, 18, 35)       <2> 64, 1  | overlap (bs >= n but tail_start < lo_end: every tap in the windowed loop)
  F128 / F129 / F130    <2> 64, 1 / 64, 2 (a second pass of one sample) / 128, 1 | two-run
  F1028 (4, 65, 1028)   <4> 256, 2 (a second pass of four samples) | two-run, float4 loads, scalar stores, table, 3
  Fslow (1024, 9, 441)  <4> 128, 1, one item of 13 frames at a constant 20 kHz: frames 0-5 on the fast loop, 6-12 on
                        the general loop (k from H4 - H, past the table's padding), frame 6 with sin_reduced and
                        sin_slow terms side by side | two-run, scalar, scalar, irfft_tap, 1
Not on this route: harmonic_frames_kernel<SPT, RAW=0> (core.harmonic_synth_frames; tests/test_gpu_parity.py).

Largest per-frame error measured on an MI355X (a record; the assertions are the constants), beside the reference
side's on the CPU (tests/test_synth_ref.py):
  harmonic, fused    device 7.7e-7 (Hcap; 6.3e-7 transition, 5.7e-7 config)   sequential fp32 model 8.1e-7 (Hcap)
  noise, fused       device 2.2e-7 (N7; 1.5e-7 config), 7.1e-7 N5b            fp32 oracle 3.0e-7 (transition), 7.3e-7 N5b
  signal             device 0.25 of its bound; controls 0.32 of theirs
  module kernels     device harmonic 3.0e-7 (Fslow), noise 1.7e-7 (F6)        model 1.5e-7, oracle 2.3e-7
The CPU figures are one host's (the oracle's depend on its FFT library).  The whole file takes 5 s on the device.

Seeded faults, each built once into a copy of the library and run against this file:
  the DC band's factor flipped in irfft_tap                       75 tests fail (15 of the 77 older forward tests too)
  frame_shape's tail_start one lower                              4 fail (of the 77 older forward tests: none)
  shared_rev_frame always true (every frame on the shared count)  4 fail: transition 1.7e-5, nyquist 3.2e-6, both forms
  `<=` for `<` in the Nyquist mask                                2 fail: nyquist, both forms
The guards are wider than the arithmetic needs, and two milder faults stay inside the bounds: kSharedRevLimit 8 -> 24
(persample's frames on the shared count: 5.0e-7), and the `fast` test dropped from the shared-count branch
(transition_shared: its arguments stay below 1.2e7, and rev_count's shifter counts revolutions exactly to 2.6e7).
For those, which loop a frame takes is asserted on the CPU restatement only (tests/test_synth_ref.py).
"""
import math

import numpy as np
import pytest
import torch

import synth_ref as sr

pytestmark = pytest.mark.gpu

FRAME_KEYS = ("f0", "param", "mags", "noise", "harm_ref", "noise_ref", "A", "amplitudes", "magnitudes", "harm_scale",
              "noise_scale")
OUTPUTS = ("signal", "harmonic", "noise", "amplitudes", "harmonic_distribution", "magnitudes")


@pytest.fixture(scope="module")
def dd():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ddsp_pytorch_amd
    ddsp_pytorch_amd._lib.load()
    return ddsp_pytorch_amd


def poison(*shapes):
    """The kernels write into torch.empty buffers: leave NaNs in the allocator's free blocks of these sizes, so
    that a frame or a sample the kernel skips does not come back holding an earlier run's correct value."""
    for s in shapes:
        torch.full(s, math.nan, dtype=torch.float32, device="cuda")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def wide(t, ld, at):
    """t [B, F, C] as a column slice, from column `at`, of a NaN buffer with rows of ld floats"""
    buf = torch.full(t.shape[:2] + (ld,), math.nan, dtype=torch.float32, device="cuda")
    v = buf[..., at:at + t.shape[-1]]
    v.copy_(t)
    assert not v.is_contiguous() and v.stride(1) == ld
    return v


def view(c, B, F):
    """the case's first B items and F frames"""
    v = dict(c)
    v.update({k: c[k][:B, :F] for k in FRAME_KEYS}, B=B, F=F)
    return v


def launch(dd, c, strided=False):
    B, F, H, NB, bs = (c[k] for k in ("B", "F", "H", "NB", "bs"))
    f0, param, mags = cu(c["f0"]), cu(c["param"]), cu(c["mags"])
    if strided:
        param, mags = wide(param, H + 8, 3), wide(mags, NB + 5, 2)
    poison((B, F * bs, 1), (B, F * bs, 1), (B, F * bs, 1), (B * F * (1 + H + NB),))
    with torch.no_grad():
        if c.get("variant") == "philox":
            sig, harm, nz, ctrl = dd.core._synth_frames_launch(f0, param, mags, bs, sr.SR, sr.BIAS, None, True,
                                                               sr.PHILOX_SEED, sr.PHILOX_OFFSET, True)
        else:
            sig, harm, nz, ctrl = dd.core.synth_frames(f0, param, mags, bs, sr.SR, bias=sr.BIAS, noise=cu(c["noise"]),
                                                       parts=True, controls=True)
    return dict(signal=sig, harmonic=harm, noise=nz, **ctrl)


def check(c, out, what):
    eh = float(sr.frame_err(out["harmonic"], c["harm_ref"], c["harm_scale"]).max())
    en = float(sr.frame_err(out["noise"], c["noise_ref"], c["noise_scale"]).max())
    es = float(sr.signal_err(out["signal"], c).max())
    ec = {k: sr.control_err(out[k], c[r], k) for k, r in (("amplitudes", "amplitudes"), ("harmonic_distribution", "A"),
                                                          ("magnitudes", "magnitudes"))}
    print(f"{what}: per frame harmonic {eh:.2e}, noise {en:.2e}, signal {es:.2f} of its bound; controls "
          + ", ".join(f"{k} {v:.2f}" for k, v in ec.items()) + " of theirs")
    assert torch.equal(out["harmonic"] + out["noise"], out["signal"]), what
    assert en <= sr.noise_tol(c["name"]), (what, "noise", en)
    assert es <= 1.0, (what, "signal", es)
    assert all(v <= 1.0 for v in ec.values()), (what, ec)
    assert eh <= sr.HARM_FRAME_TOL, (what, "harmonic", eh)


_BATCH = {}


def batch_form(dd, name):
    """the batch (or PREFIX) launch of a case, run once and kept for the SPLIT and strides comparisons"""
    if name not in _BATCH:
        _BATCH[name] = launch(dd, sr.fused_case(name))
    return _BATCH[name]


# ------------------------------------------------------------------------------------------ the fused kernels
@pytest.mark.parametrize("name", sr.all_fused_names())
def test_batch_form(dd, name):
    c = sr.fused_case(name)
    assert dd.core.synth_frames_in_envelope(c["H"], c["NB"], c["bs"], c["B"])
    check(c, batch_form(dd, name), f"{name} {'PREFIX' if name.endswith('/prefix') else 'batch'}")


@pytest.mark.parametrize("name", [n for n in sr.all_fused_names() if sr.split_slice(n)])
def test_split_form(dd, name):
    """the SPLIT kernels on a slice of the case: within the bounds, and bit for bit the batch form's outputs"""
    items, frames = sr.split_slice(name)
    c = view(sr.fused_case(name), items, frames)
    out = launch(dd, c)
    full = batch_form(dd, name)
    bs = c["bs"]
    for k in OUTPUTS:
        ref = full[k][:items, :frames * bs] if k in ("signal", "harmonic", "noise") else full[k][:items, :frames]
        same = torch.equal(out[k], ref)
        if not same:
            bad = (out[k] != ref).reshape(items, frames, -1).any(-1).nonzero()
            print(f"{name} SPLIT {k}: {len(bad)} frames differ from the batch form, first (item, frame) {bad[0].tolist()}")
        assert same, (name, k)
    check(c, out, f"{name} SPLIT {items}x{frames}")


def test_transition_crossing_frame(dd):
    """the frame whose quads take two different loops is the same bit for bit in both launch shapes; prints its
    error beside its two neighbours' (test_batch_form and test_split_form assert the bound on every frame)"""
    c = sr.fused_case("transition")
    x = 46
    fq = sr.fast_quads(c["f0"], c["H"], c["bs"])[0, x]
    assert fq.any() and not fq.all()
    full = batch_form(dd, "transition")["harmonic"].reshape(1, c["F"], c["bs"])
    part = launch(dd, view(c, 1, 128))["harmonic"].reshape(1, 128, c["bs"])
    assert torch.equal(full[:, x], part[:, x])
    e = sr.frame_err(full[:, x - 1:x + 2], c["harm_ref"][:, x - 1:x + 2], c["harm_scale"][:, x - 1:x + 2])
    print(f"transition frames {x - 1}..{x + 1} (fast, crossing, general): {e[0].tolist()}")


def test_strided_rows(dd):
    c = sr.fused_case("config")
    out, full = launch(dd, c, strided=True), batch_form(dd, "config")
    for k in OUTPUTS:
        assert torch.equal(out[k], full[k]), k


def test_exactly_silent_frames(dd):
    """nyquist frames 0-1 (f0 = 0 from the start): the harmonic part is exactly zero, the signal is the noise"""
    out = batch_form(dd, "nyquist")
    c = sr.fused_case("nyquist")
    n = 2 * c["bs"]
    assert (out["harmonic"][:, :n] == 0).all() and torch.equal(out["signal"][:, :n], out["noise"][:, :n])


# ------------------------------------------------------------------------------------------ the module kernels
@pytest.mark.parametrize("kind", ["inject", "philox"])
@pytest.mark.parametrize("raw", [True, False], ids=["raw", "scaled"])
@pytest.mark.parametrize("name", sorted(sr.FALLBACK_CASES))
def test_module_kernels(dd, name, raw, kind):
    c = dict(sr.fallback_case(name))
    B, F, bs = c["B"], c["F"], c["bs"]
    c["noise_ref"], c["noise_scale"] = c["noise_refs"][kind, raw]
    f0, param = cu(c["f0"]), cu(c["param"])
    mags = cu(c["mags"] if raw else c["scaled"])
    bias = sr.BIAS if raw else None
    poison((B, F * bs, 1), (B, F * bs, 1), (B, F * bs, 1))
    with torch.no_grad():
        harm = dd.core.harmonic_synth_params(f0, param, bs, sr.SR)
        if kind == "inject":
            sig, nz = dd.core.filtered_noise(mags, bs, noise=cu(c["noise"]), add=harm, return_noise=True, raw_bias=bias)
        else:
            sig, nz = dd.core._filtered_noise_launch(mags, bs, None, harm, True, bias, sr.PHILOX_SEED, sr.PHILOX_OFFSET)
    eh = float(sr.frame_err(harm, c["harm_ref"], c["harm_scale"]).max())
    en = float(sr.frame_err(nz, c["noise_ref"], c["noise_scale"]).max())
    es = float(sr.signal_err(sig, c).max())
    print(f"{name} {'raw' if raw else 'scaled'} {kind}: per frame harmonic {eh:.2e}, noise {en:.2e}, signal {es:.2f} "
          "of its bound")
    assert torch.equal(harm + nz, sig)
    assert eh <= sr.HARM_FRAME_TOL, (name, "harmonic", eh)
    assert en <= sr.NOISE_FRAME_TOL, (name, "noise", en)
    assert es <= 1.0, (name, "signal", es)


def test_synth_signal_takes_the_module_kernels(dd):
    """core.synth_signal outside the envelope is that route: bit for bit the two calls above"""
    c = sr.fallback_case("F441")
    f0, param, mags, noise = (cu(c[k]) for k in ("f0", "param", "mags", "noise"))
    assert not dd.core.synth_frames_in_envelope(c["H"], c["NB"], c["bs"], c["B"])
    with torch.no_grad():
        sig = dd.core.synth_signal(f0, param, mags, c["bs"], sr.SR, bias=sr.BIAS, noise=noise)
        harm = dd.core.harmonic_synth_params(f0, param, c["bs"], sr.SR)
        two = dd.core.filtered_noise(mags, c["bs"], noise=noise, add=harm, raw_bias=sr.BIAS)
    assert torch.equal(sig, two)
