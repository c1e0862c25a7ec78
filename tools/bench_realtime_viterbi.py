"""Per-call latency of the audio-in RealtimeGraph (``loudness_from_audio`` + ``pitch_from_audio``) with the per-frame
pitch and with ``pitch_viterbi`` at lag 0 and lag 4, on the same device in one run, alternating: ``--rounds`` rounds of
``--calls`` calls each, A B C A B C ..., so that clock and thermal drift fall on all alike.  A call is what a realtime
host pays: pinned host buffers in, one graph replay, audio out, one synchronisation; it has to stay inside its own
audio, call_samples / sample_rate (21.3 ms).  Then the launches on their own, each ``--launches`` times back to back
between two device events (the same call again and again, which the stream entry points allow before the advance):
the graph's existing analysis launch (``core.stream_analysis``), the loudness alone, and the two launches
``pitch_viterbi`` adds, the salience and the carried decode at lags 0, 4 and 64.  Prints one JSON line per figure.
The realtime size: hidden 512, 64 harmonics, 65 bands, block 256, calls of 1024 samples at 48 kHz.  Needs a HIP
device."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddsp_pytorch_amd as dd  # noqa: E402
from ddsp_pytorch_amd import core  # noqa: E402
from ddsp_pytorch_amd.realtime import RealtimeGraph  # noqa: E402

SR, BS, N = 48000, 256, 1024


def launches_us(fn, n):
    """Microseconds per launch of fn(), n launches back to back between two device events (after 20 to warm up)."""
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=2000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_realtime_viterbi: needs a HIP device")
    variants = (("pitch_from_audio", {}), ("pitch_viterbi lag 0", {"pitch_viterbi": True, "pitch_lag": 0}),
                ("pitch_viterbi lag 4", {"pitch_viterbi": True, "pitch_lag": 4}))
    graphs = {}
    for name, kw in variants:
        torch.manual_seed(0)
        model = dd.DDSPDecoder(512, 64, 65, SR, BS, False).eval().cuda()
        graphs[name] = RealtimeGraph(model, N, mean_loudness=-6.5, std_loudness=1.75, loudness_from_audio=True,
                                     pitch_from_audio=True, **kw)
    t = torch.arange(N * 64) / SR  # a voiced stream: a 220 Hz tone with a strong second harmonic, 64 calls long
    stream = (0.1 * torch.sin(2 * np.pi * 220.0 * t) + 0.3 * torch.sin(2 * np.pi * 440.0 * t)).reshape(64, 1, N, 1)
    times = {name: [] for name in graphs}
    for rt in graphs.values():  # warm-up
        for k in range(50):
            rt(stream[k % 64])
    for _ in range(args.rounds):
        for name, rt in graphs.items():
            for k in range(args.calls):
                t0 = time.perf_counter()
                rt(stream[k % 64])
                times[name].append(time.perf_counter() - t0)
    budget_us = 1e6 * N / SR
    for name, ts in times.items():
        us = 1e6 * np.asarray(ts)
        print(json.dumps({"variant": name, "calls": len(ts), "p50_us": round(float(np.percentile(us, 50)), 1),
                          "p99_us": round(float(np.percentile(us, 99)), 1), "mean_us": round(float(us.mean()), 1),
                          "max_us": round(float(us.max()), 1), "budget_us": round(budget_us, 1)}), flush=True)

    # the launches on their own
    x = stream[3].reshape(1, N).cuda()
    n_bins = core.stream_pitch_bin_count(SR)
    ring = core.FeatureStreamState(1, "cuda", N, 2048, BS)
    ring_p = core.FeatureStreamState(1, "cuda", N, 2048, BS)
    cost, f0c = core.stream_pitch_salience(x, SR, BS, ring_p)
    rows = [("stream_analysis (loudness + per-frame pitch)", lambda: core.stream_analysis(x, SR, BS, ring)),
            ("stream_loudness", lambda: core.stream_loudness(x, SR, BS, ring)),
            ("stream_pitch_salience", lambda: core.stream_pitch_salience(x, SR, BS, ring_p))]
    for lag in (0, 4, 64):
        st = core.ViterbiStreamState(1, "cuda", N // BS, n_bins, lag)
        st.counter.fill_(1000)  # past the start: every walk at its full length
        rows.append((f"stream_viterbi_path lag {lag}", lambda st=st: core.stream_viterbi_path(cost, f0c, st)))
    for name, fn in rows:
        print(json.dumps({"launch": name, "n_bins": n_bins, "frames_per_call": N // BS,
                          "us_per_launch": round(launches_us(fn, args.launches), 2)}), flush=True)


if __name__ == "__main__":
    main()
