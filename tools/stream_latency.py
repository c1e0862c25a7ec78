"""Config 3 (batch 1, block_size 256, 64 harmonics, 65 bands, 1024-sample calls): per-call latency of the seamless
realtime stream beside the stateless route, in one process on one device.

    python tools/stream_latency.py [--calls 2000] [--only default|continuous|reverb]

Three RealtimeGraph variants, interleaved call by call so that clock and host drift hit them alike: the default
(stateless), continuous=True (phase carry; the advance launch replaces the counter advance, no launch added) and
continuous=True, reverb=True (plus ddsp_hip_stream_reverb, N = 1024, L = 48000: 47 partitions).  Per variant: p50 /
p99 of host pitch/loudness in -> host audio out, and the device time per replay.  Prints one JSON line.
--only runs a single variant for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/stream_latency.py
--only reverb)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = {"default": {}, "continuous": {"continuous": True}, "reverb": {"continuous": True, "reverb": True}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--only", choices=sorted(VARIANTS), default=None)
    args = ap.parse_args()
    import ddsp_pytorch_amd as dd
    from ddsp_pytorch_amd.realtime import RealtimeGraph
    names = [args.only] if args.only else list(VARIANTS)
    graphs = {}
    for name in names:
        torch.manual_seed(0)
        m = dd.DDSPDecoder(512, 64, 65, 48000, 256, False).eval().cuda()  # its reverb: 48000 taps
        graphs[name] = RealtimeGraph(m, 1024, **VARIANTS[name])
    loud = torch.zeros(1, 1024, 1)
    lat = {name: [] for name in names}
    with torch.no_grad():
        for i in range(args.calls + 50):
            p = torch.full((1, 1024, 1), 220.0 * 2 ** ((i // 20) % 12 / 12))
            for name in names:
                t0 = time.perf_counter()
                y = graphs[name](p, loud)
                dt = (time.perf_counter() - t0) * 1e3
                if i >= 50:
                    lat[name].append(dt)
            assert torch.isfinite(y).all()
        res = {"config": "config 3: batch 1, block_size 256, n_harmonic 64, n_bands 65, 1024-sample calls, "
                         "reverb 48000 taps", "calls": args.calls, "budget_ms": 1024 / 48.0}
        pd, ld = p.cuda(), loud.cuda()
        for name in names:
            rt = graphs[name]
            for _ in range(20):
                rt(pd, ld)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                rt(pd, ld)
            e1.record()
            torch.cuda.synchronize()
            v = sorted(lat[name])
            res[name] = {"p50_ms": v[len(v) // 2], "p99_ms": v[int(0.99 * len(v))], "max_ms": v[-1],
                         "device_ms_per_replay": e0.elapsed_time(e1) / 200}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
