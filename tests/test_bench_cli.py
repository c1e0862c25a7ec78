"""bench.py's command line: a plain run prints the headline line alone and does only what it needs,
--full adds the rest, --dump-outputs DIR writes the last timed step's audio (repeatable: the
device-noise stream is rewound after the warmup, so timed step k draws Philox offset k)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}


def _parse(argv, monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_full_and_dump_are_off_by_default(monkeypatch):
    a = _parse(["--gpus", "1", "--steps", "7", "--warmup", "3"], monkeypatch)
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    a = _parse(["--full", "--dump-outputs", "d"], monkeypatch)
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    import bench
    x = torch.arange(2 * 50, dtype=torch.float64).reshape(2, 50, 1)
    bench.dump_outputs(x, str(tmp_path / "a"))
    a = np.load(tmp_path / "a" / "signal.npy")
    assert a.dtype == np.float32 and a.shape == (2, 50, 1) and np.array_equal(a, x.numpy())
    # above the size cap: a fixed sample (the same elements on every call), within the cap
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4 * 30)
    bench.dump_outputs(x, str(tmp_path / "b"))
    bench.dump_outputs(x, str(tmp_path / "c"))
    b, c = np.load(tmp_path / "b" / "signal.npy"), np.load(tmp_path / "c" / "signal.npy")
    assert b.dtype == np.float32 and b.shape == (30,) and b.nbytes <= 4 * 30
    assert np.array_equal(b, c) and np.all(np.diff(b) >= 0) and set(b) <= set(x.flatten().tolist())


@pytest.mark.gpu
def test_plain_run_headline_and_dump(tmp_path):
    """One small plain run: the headline keys and nothing of --full's, --steps timed steps, and the
    dumped audio equal bit for bit to the same path driven in this process for --steps calls."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    B, F, H, NB, bs, sr, L, steps = 3, 9, 100, 65, 512, 48000, 4800, 3
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "2", "--settle", "0",
           "--batch", str(B), "--frames", str(F), "--reverb-length", str(L), "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=100)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert HEADLINE <= set(line) and line["steps"] == steps and line["ms_per_step"] > 0
    assert line["unit"] == "samples/s" and line["higher_is_better"] is True and line["dtype"] == "fp32"
    # value = samples per step / step time; ms_per_step is printed rounded to 1e-4 ms
    rel = 0.5e-4 / line["ms_per_step"] + 1e-6
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / (B * F * bs) - 1) <= 1.01 * rel / (1 - rel)
    assert not {"roofline", "kernel_ms", "cpu_baseline", "train_step", "realtime", "pipelined"} & set(line)
    assert sorted(os.listdir(tmp_path)) == ["signal.npy"]
    got = np.load(tmp_path / "signal.npy")
    assert got.dtype == np.float32 and got.shape == (B, F * bs, 1)

    from ddsp_pytorch_amd import core
    from ddsp_pytorch_amd.synth import SynthPath, make_inputs
    inp = make_inputs(B, F, H, NB, bs, seed=0, device="cuda", with_noise=False)
    syn = SynthPath(bs, sr, reverb_length=L, noise_mode="device").cuda()
    core.set_noise_seed(1234)
    for _ in range(steps):
        out = syn(inp["f0"], inp["param"], inp["mags"], None)
    assert np.array_equal(got, out.cpu().numpy())
