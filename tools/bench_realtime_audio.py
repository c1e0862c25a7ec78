"""Per-call latency of RealtimeGraph with pitch and loudness inputs, with ``loudness_from_audio`` (the streamed
loudness computed inside the captured graph) and with ``pitch_from_audio`` on top of it (the audio alone in: the
loudness and the YIN pitch from one launch), on the same device, alternating: ``--rounds`` rounds of ``--calls``
calls each, A B C A B C ..., so that clock and thermal drift fall on all alike.  A call is what a realtime host
pays: pinned host buffers in, one graph replay, audio out, one synchronisation.  A fourth variant is the
z-conditioned ``DDSPAutoencoder`` of the same sizes from audio alone (the loudness, the MFCC and the pitch from one
launch, the encoder with its carried state, the decoder with z).  Prints one JSON line per variant
with p50 / p99 / mean in microseconds over all its rounds.  Config 3's shape: hidden 512, 64 harmonics, 65 bands,
block 256, calls of 1024 samples at 48 kHz.  Needs a HIP device."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddsp_pytorch_amd as dd  # noqa: E402
from ddsp_pytorch_amd.realtime import RealtimeGraph  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--continuous", action="store_true", help="continuous=True, reverb=True on every variant")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_realtime_audio: needs a HIP device")
    N = 1024
    graphs = {}
    for name, kw in (("loudness input", {}), ("loudness_from_audio", {"loudness_from_audio": True}),
                     ("pitch_from_audio", {"loudness_from_audio": True, "pitch_from_audio": True}),
                     ("autoencoder pitch_from_audio", {"loudness_from_audio": True, "pitch_from_audio": True})):
        torch.manual_seed(0)
        cls = dd.DDSPAutoencoder if name.startswith("autoencoder") else dd.DDSPDecoder
        model = cls(512, 64, 65, 48000, 256, False).eval().cuda()
        graphs[name] = RealtimeGraph(model, N, mean_loudness=-6.5, std_loudness=1.75, continuous=args.continuous,
                                     reverb=args.continuous, **kw)
    g = torch.Generator().manual_seed(1)
    pitch = 80.0 * 10.0 ** torch.rand(1, N, 1, generator=g)
    audio = 0.1 * torch.randn(1, N, 1, generator=g)
    inputs = {"loudness input": (pitch, torch.randn(1, N, 1, generator=g) - 6.0),
              "loudness_from_audio": (pitch, audio), "pitch_from_audio": (audio,),
              "autoencoder pitch_from_audio": (audio,)}
    times = {name: [] for name in graphs}
    for name, rt in graphs.items():  # warm-up
        for _ in range(50):
            rt(*inputs[name])
    for _ in range(args.rounds):
        for name, rt in graphs.items():
            for _ in range(args.calls):
                t0 = time.perf_counter()
                rt(*inputs[name])
                times[name].append(time.perf_counter() - t0)
    for name, ts in times.items():
        us = 1e6 * np.asarray(ts)
        print(json.dumps({"variant": name, "continuous": args.continuous, "calls": len(ts),
                          "p50_us": round(float(np.percentile(us, 50)), 1),
                          "p99_us": round(float(np.percentile(us, 99)), 1), "mean_us": round(float(us.mean()), 1)}),
              flush=True)


if __name__ == "__main__":
    main()
