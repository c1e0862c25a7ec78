"""Times the analysis front end (core.extract_loudness, core.mfcc, features.analyze: csrc/features.hip) on the
GPU, beside what a user would write today on the same GPU: torch.stft plus the same tables as dense ATen ops.

Shapes: the training shape of the reference's config.yaml (16 items x 192,000 samples, block 512, 48 kHz) and
config 2's (64 x 102,400).  Each figure is the median over `--windows` event-timed windows of `--reps` calls,
after a warm-up of every timed callable.  Beside each time: the bytes the algorithm needs (x read once, the
features written, and for the MFCC the D workspace written and read back) and the rate they make.  Prints one
JSON line per (shape, leg); DESIGN.md 3f records a run.  Needs a HIP device: there is no CPU path.

``--leg stream`` times the streaming analysis (core.stream_loudness, core.stream_mfcc) at the realtime shape (one
item, calls of 1024 samples, block 256, 48 kHz), each leg captured in a HIP graph and replayed: the stream
kernels, beside the route open without them — the offline kernels over a rolling window of Hs + N samples (the
history a call's frames need plus the call), the window's shift included.  DESIGN.md 3g records a run.

``--leg pitch`` times the pitch tracker (core.extract_pitch: csrc/pitch.hip) at the two offline shapes beside the
same definition (include/ddsp_hip.h, "pitch") composed from torch.fft and ATen ops in fp64 — what a user would
write today; the package had no pitch path before — and core.stream_pitch at the realtime shape, captured in a HIP
graph.  DESIGN.md 3f-pitch records a run.

``--leg viterbi`` times the Viterbi-decoded tracker (core.pitch_salience, core.viterbi_path, core.track_pitch:
csrc/pitch_viterbi.hip) at the two offline shapes beside core.extract_pitch alone and beside the same definition
(include/ddsp_hip.h, "pitch_viterbi") composed from torch.fft / ATen ops in fp64 with a per-frame torch loop for the
recursion, and the decode alone on a minute of audio.  DESIGN.md 3f-viterbi records a run.

``--leg aligned`` times core.stream_analysis_mfcc (the streamed loudness, MFCC and pitch in one launch over one state,
on one time axis) against core.stream_analysis + core.stream_mfcc as two launches on two states, and against
core.stream_analysis alone, the same way.

``--leg fused`` times core.stream_analysis (the streamed loudness and pitch in one launch over one state) against
core.stream_loudness + core.stream_pitch (two launches, two states) at the realtime shape, each captured in a HIP
graph, the legs' windows alternating.  DESIGN.md 3f-fused records a run.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ddsp_pytorch_amd as dd  # noqa: E402
from ddsp_pytorch_amd import core  # noqa: E402

SHAPES = [("train 16x192000", 16, 192000, 512, 48000), ("config2 64x102400", 64, 102400, 512, 48000)]


def torch_loudness(x, w, n_fft, hop):
    """core.py:81-97 as torch ops: a full complex spectrogram and its log go through memory."""
    S = torch.stft(x, n_fft, hop, n_fft, torch.hann_window(n_fft, device=x.device), center=True, pad_mode="reflect",
                   return_complex=True).abs()
    return (torch.log(S + 1e-7) + w[None, :, None]).mean(1)[..., :-1]


def torch_mfcc(x, fb, dct, n_fft, hop, top_db=80.0):
    """preprocess.py:30-32 as torch ops with the dense filterbank and DCT as matmuls."""
    P = torch.stft(x, n_fft, hop, n_fft, torch.hann_window(n_fft, device=x.device), center=True, pad_mode="reflect",
                   return_complex=True).abs() ** 2
    D = 10.0 * torch.log10(torch.clamp(fb @ P, min=1e-10))
    D = torch.maximum(D, D.amax(dim=(1, 2), keepdim=True) - top_db)
    return (dct @ D).transpose(1, 2)


def torch_dprime(x, hop, L, tau_max):
    """d' [B, F, tau_max + 2] of include/ddsp_hip.h "pitch" as torch ops in fp64: the frames, their transforms, d and
    d' all go through memory."""
    W, F = L // 2, x.shape[1] // hop
    xp = torch.nn.functional.pad(x[:, None], (W, W), mode="reflect")[:, 0]
    Y = xp.unfold(1, L, hop)[:, :F].double()
    r = torch.fft.irfft(torch.fft.rfft(Y[..., :W], n=L).conj() * torch.fft.rfft(Y, n=L), n=L)[..., :tau_max + 2]
    c = torch.nn.functional.pad(torch.cumsum(Y * Y, -1), (1, 0))
    E = c[..., W:W + tau_max + 2] - c[..., :tau_max + 2]
    tot = E[..., :1] + E
    d = tot - 2.0 * r
    d = torch.where(d < 2.0 ** -40 * tot, torch.zeros_like(d), d)
    d[..., 0] = 0.0
    S = torch.cumsum(d, -1)
    tau = torch.arange(tau_max + 2, device=x.device, dtype=torch.float64)
    dn = torch.where(S > 0, d * tau / torch.where(S > 0, S, torch.ones_like(S)), torch.ones_like(S))
    dn[..., 0] = 1.0
    return dn


def torch_pitch(x, sr, hop, L, tau_min, tau_max, threshold=0.1):
    """include/ddsp_hip.h "pitch" as torch ops in fp64 (the candidates too go through memory).
    -> (f0 [B, F] fp32, period [B, F])."""
    dn = torch_dprime(x, hop, L, tau_max)
    b, a, cn = dn[..., tau_min:tau_max + 1], dn[..., tau_min - 1:tau_max], dn[..., tau_min + 1:tau_max + 2]
    cand = (b < a) & (b <= cn) & (b < float(torch.tensor(threshold, dtype=torch.float32)))
    first = (torch.cumsum(cand, -1) == 0).sum(-1)
    ts = torch.where(cand.any(-1), first, b.argmin(-1)) + tau_min
    a, b, cn = (dn.gather(-1, (ts + o)[..., None])[..., 0] for o in (-1, 0, 1))
    curv = a - 2.0 * b + cn
    ok = (b <= a) & (b <= cn) & (curv > 0)
    s = torch.where(ok, 0.5 * (a - cn) / torch.where(ok, curv, torch.ones_like(curv)), torch.zeros_like(curv))
    return (sr / (ts + s)).float(), ts


def pitch_leg(dev, reps, windows):
    L, fmin, fmax = 2048, 50.0, 2000.0
    for name, B, T, hop, sr in SHAPES:
        g = torch.Generator().manual_seed(B + T)
        t = torch.arange(T) / sr
        f = 110.0 * 2.0 ** (torch.arange(B)[:, None] / 8.0) * (1.0 + 0.005 * torch.sin(2 * torch.pi * 5.5 * t))[None, :]
        phase = 2 * torch.pi * torch.cumsum(f.double(), 1) / sr
        x = 0.2 * sum(torch.sin(h * phase) / h for h in range(1, 7)).float() + 0.003 * torch.randn(B, T, generator=g)
        x = x.to(dev)
        F = T // hop
        tau_min, tau_max = core.pitch_lags(sr, fmin, fmax, L)
        nbytes = 4 * (B * T + 3 * B * F)
        f_hip, _, p_hip = core.extract_pitch(x, sr, hop, return_confidence=True, return_period=True)
        f_t, p_t = torch_pitch(x, sr, hop, L, tau_min, tau_max)
        same = p_hip == p_t
        rel = float(((f_hip - f_t).abs() / f_t)[same].max())
        print(json.dumps({"shape": name, "frames": B * F, "periods_that_differ": int((~same).sum()),
                          "max_rel_diff_f0": rel}), flush=True)
        legs = [
            ("pitch hip", lambda: core.extract_pitch(x, sr, hop, return_confidence=True, return_period=True), nbytes),
            ("pitch torch.fft (fp64)", lambda: torch_pitch(x, sr, hop, L, tau_min, tau_max), None),
        ]
        for leg, fn, nb in legs:
            med, lo, hi = timed(fn, reps if nb is not None else max(reps // 20, 5), windows)
            row = {"shape": name, "leg": leg, "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
            if nb is not None:
                row["algorithmic_bytes"] = nb
                row["GB_per_s"] = round(nb / (med * 1e-3) / 1e9, 1)
            print(json.dumps(row), flush=True)
    sr, hop, N = 48000, 256, 1024
    x = 0.1 * torch.randn(1, N, device=dev)
    st = core.FeatureStreamState(1, dev, N, L, hop)

    def stream_and_advance():
        out = core.stream_pitch(x, sr, hop, st, return_confidence=True, return_period=True)
        core.stream_advance(st)
        return out

    for leg, fn, launches in (("stream pitch", lambda: core.stream_pitch(x, sr, hop, st, return_confidence=True,
                                                                       return_period=True), 1),
                              ("stream pitch + advance", stream_and_advance, 2)):
        med, lo, hi = timed(graphed(fn), reps, windows)
        print(json.dumps({"shape": "stream 1x1024 block 256", "leg": leg, "graph_nodes": launches,
                          "us": round(1e3 * med, 2), "us_min": round(1e3 * lo, 2), "us_max": round(1e3 * hi, 2)}),
              flush=True)


def torch_salience(dn, sr, lo, hi):
    """include/ddsp_hip.h "pitch_viterbi", the salience, as torch ops in fp64: dn [B, F, tau_max + 2], lo / hi [NB]
    (long) -> (cost, f0c) fp32 [B, F, NB]."""
    span = int((hi - lo).max()) + 1
    idx = lo[:, None] + torch.arange(span, device=dn.device)[None, :]  # [NB, span]
    inside = idx <= hi[:, None]
    idx = torch.minimum(idx, hi[:, None])
    v = dn[..., idx]                                                    # [B, F, NB, span]
    v = torch.where(inside, v, torch.full_like(v, float("inf")))
    ts = lo + v.argmin(-1)                                              # the first index of the minimum
    a, b, cn = (dn.gather(-1, ts + o) for o in (-1, 0, 1))
    curv = a - 2.0 * b + cn
    ok = (b <= a) & (b <= cn) & (curv > 0)
    s = torch.where(ok, 0.5 * (a - cn) / torch.where(ok, curv, torch.ones_like(curv)), torch.zeros_like(curv))
    return b.clamp(max=1.0).float(), (sr / (ts + s)).float()


def torch_viterbi(cost, f0c, lam, R):
    """The decode as torch ops in fp64 with a per-frame loop for the recursion and another for the backtrack: what
    a user would write today.  -> (f0, confidence, path) [B, F]."""
    B, F, NB = cost.shape
    lam = float(torch.tensor(lam, dtype=torch.float32))
    pen = lam * torch.arange(-R, R + 1, device=cost.device).abs().double()
    c = cost.double()
    delta = c[:, 0]
    back = torch.zeros(B, F, NB, dtype=torch.long, device=cost.device)
    j = torch.arange(NB, device=cost.device)
    for t in range(1, F):
        padded = torch.nn.functional.pad(delta, (R, R), value=float("inf"))
        v = padded.unfold(1, 2 * R + 1, 1) + pen                        # [B, NB, 2R + 1]: i = j + k - R
        best, k = v.min(-1)                                             # (ties: the first, as argmin)
        back[:, t] = j + k - R
        delta = best + c[:, t]
    path = torch.empty(B, F, dtype=torch.long, device=cost.device)
    path[:, F - 1] = delta.argmin(-1)
    for t in range(F - 1, 0, -1):
        path[:, t - 1] = back[:, t].gather(-1, path[:, t:t + 1])[:, 0]
    g = path[..., None]
    return f0c.gather(-1, g)[..., 0], 1.0 - cost.gather(-1, g)[..., 0], path.int()


def viterbi_leg(dev, reps, windows):
    """core.pitch_salience, core.viterbi_path and their sum (core.track_pitch) at the two offline shapes, beside
    core.extract_pitch alone and beside the same definition composed from torch.fft / ATen ops in fp64 with a
    per-frame loop; then the decode alone on one item of 5625 frames (a minute of audio at block 512)."""
    L, fmin, fmax, beta, lam, R = 2048, 50.0, 2000.0, 48, 0.02, 12
    for name, B, T, hop, sr in SHAPES:
        g = torch.Generator().manual_seed(B + T)
        t = torch.arange(T) / sr
        f = 110.0 * 2.0 ** (torch.arange(B)[:, None] / 8.0) * (1.0 + 0.005 * torch.sin(2 * torch.pi * 5.5 * t))[None, :]
        phase = 2 * torch.pi * torch.cumsum(f.double(), 1) / sr
        x = 0.2 * sum(torch.sin(h * phase) / h for h in range(1, 7)).float() + 0.003 * torch.randn(B, T, generator=g)
        x = x.to(dev)
        tau_min, tau_max, lo, hi = core.pitch_bins(sr, fmin, fmax, L, beta)
        lo_d, hi_d = (torch.tensor(a, device=dev) for a in (lo, hi))
        cost, f0c = core.pitch_salience(x, sr, hop)

        def torch_track():
            return torch_viterbi(*torch_salience(torch_dprime(x, hop, L, tau_max), sr, lo_d, hi_d), lam, R)

        p_hip = core.track_pitch(x, sr, hop, return_path=True)[1]
        p_t = torch_track()[2]
        print(json.dumps({"shape": name, "frames": B * (T // hop), "bins": len(lo),
                          "path_frames_that_differ": int((p_hip != p_t).sum())}), flush=True)
        legs = [
            ("salience hip", lambda: core.pitch_salience(x, sr, hop), reps),
            ("decode hip", lambda: core.viterbi_path(cost, f0c, lam, R), reps),
            ("track_pitch hip (salience + decode)", lambda: core.track_pitch(x, sr, hop), reps),
            ("pitch hip (extract_pitch alone)", lambda: core.extract_pitch(x, sr, hop), reps),
            ("track_pitch torch.fft + per-frame loop (fp64)", torch_track, 2),
        ]
        for leg, fn, n in legs:
            med, lo_ms, hi_ms = timed(fn, n, windows)
            print(json.dumps({"shape": name, "leg": leg, "reps": n, "ms": round(med, 4), "ms_min": round(lo_ms, 4),
                              "ms_max": round(hi_ms, 4)}), flush=True)
    F, NB = 5625, 256
    g = torch.Generator().manual_seed(F)
    cost = torch.rand(1, F, NB, generator=g).to(dev)
    f0c = (50.0 + 1950.0 * torch.rand(1, F, NB, generator=g)).to(dev)
    med, lo_ms, hi_ms = timed(lambda: core.viterbi_path(cost, f0c, lam, R), max(reps // 10, 5), windows)
    print(json.dumps({"shape": f"decode 1x{F}x{NB}", "leg": "decode hip", "ms": round(med, 4),
                      "ms_min": round(lo_ms, 4), "ms_max": round(hi_ms, 4),
                      "us_per_frame": round(1e3 * med / F, 3)}), flush=True)


def timed(fn, reps, windows):
    """Median milliseconds per call over `windows` event-timed windows of `reps` calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return statistics.median(ms), min(ms), max(ms)


def graphed(fn):
    """fn captured in a HIP graph after a warm-up on a side stream -> the replay callable."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    g.keep = keep  # the outputs live as long as the graph
    return g.replay


def stream_leg(dev, reps, windows):
    """One item, calls of 1024 samples, block 256, 48 kHz; microseconds per replayed call."""
    sr, hop, N = 48000, 256, 1024
    x = 0.1 * torch.randn(1, N, device=dev)
    sl = core.FeatureStreamState(1, dev, N, 2048, hop)
    sm = core.FeatureStreamState(1, dev, N, 1024, hop, counter=sl.counter)
    hs_l = core.stream_feature_delay(2048, hop) * hop + 1024
    hs_m = core.stream_feature_delay(1024, hop) * hop + 512
    win_l = torch.zeros(1, hs_l + N, device=dev)
    win_m = torch.zeros(1, hs_m + N, device=dev)

    def roll(win):  # the window moves on by one call: two small copies
        win[:, :-N].copy_(win[:, N:].clone())
        win[:, -N:].copy_(x)

    def rolling_loudness():
        roll(win_l)
        return core.extract_loudness(win_l, sr, hop)

    def rolling_mfcc():
        roll(win_m)
        return core.mfcc(win_m, sr, hop)

    def stream_both():
        out = core.stream_loudness(x, sr, hop, sl), core.stream_mfcc(x, sr, hop, sm)
        core.stream_advance(sl)
        return out

    legs = [
        ("stream loudness", lambda: core.stream_loudness(x, sr, hop, sl), 1),
        ("stream mfcc", lambda: core.stream_mfcc(x, sr, hop, sm), 1),
        ("stream both + advance", stream_both, 3),
        ("advance alone", lambda: core.stream_advance(sl), 1),
        ("rolling-window loudness (offline kernel)", rolling_loudness, 4),
        ("rolling-window mfcc (offline kernels)", rolling_mfcc, 5),
        ("rolling-window both", lambda: (rolling_loudness(), rolling_mfcc()), 9),
    ]
    for leg, fn, launches in legs:
        med, lo, hi = timed(graphed(fn), reps, windows)
        print(json.dumps({"shape": "stream 1x1024 block 256", "leg": leg, "graph_nodes": launches,
                          "us": round(1e3 * med, 2), "us_min": round(1e3 * lo, 2), "us_max": round(1e3 * hi, 2)}),
              flush=True)


def fused_leg(dev, reps, windows):
    """The fused launch (core.stream_analysis, one state) against the route without it (core.stream_loudness +
    core.stream_pitch, two launches on two states), each captured in a HIP graph; the legs' windows alternate, so
    that a drift of the box lands on all of them alike."""
    sr, hop, N, L = 48000, 256, 1024, 2048
    x = 0.1 * torch.randn(1, N, device=dev)
    sf = core.FeatureStreamState(1, dev, N, L, hop)
    sl = core.FeatureStreamState(1, dev, N, L, hop, counter=sf.counter)
    sp = core.FeatureStreamState(1, dev, N, L, hop, counter=sf.counter)
    kw = dict(return_confidence=True, return_period=True)
    legs = [
        ("stream loudness + stream pitch (two launches, two states)",
         graphed(lambda: (core.stream_loudness(x, sr, hop, sl, n_fft=L), core.stream_pitch(x, sr, hop, sp, **kw))), 2),
        ("stream analysis (one launch, one state)", graphed(lambda: core.stream_analysis(x, sr, hop, sf, **kw)), 1),
        ("stream pitch", graphed(lambda: core.stream_pitch(x, sr, hop, sp, **kw)), 1),
        ("stream loudness", graphed(lambda: core.stream_loudness(x, sr, hop, sl, n_fft=L)), 1),
    ]
    ms = [[] for _ in legs]
    for _ in range(windows):
        for i, (_, fn, _) in enumerate(legs):
            ms[i].append(timed(fn, reps, 1)[0])
    for (leg, _, launches), m in zip(legs, ms):
        print(json.dumps({"shape": "stream 1x1024 block 256 L 2048", "leg": leg, "graph_nodes": launches,
                          "us": round(1e3 * statistics.median(m), 2), "us_min": round(1e3 * min(m), 2),
                          "us_max": round(1e3 * max(m), 2), "windows_us": [round(1e3 * v, 2) for v in m]}),
              flush=True)


def aligned_leg(dev, reps, windows):
    """The three-feature launch (core.stream_analysis_mfcc: loudness, MFCC and pitch over one state, on one time
    axis) against the route without it for the same features (core.stream_analysis + core.stream_mfcc, two launches
    on two states) and against core.stream_analysis alone, each captured in a HIP graph; the legs' windows alternate
    as fused_leg's do."""
    sr, hop, N, L, M = 48000, 256, 1024, 2048, 1024
    x = 0.1 * torch.randn(1, N, device=dev)
    sa = core.FeatureStreamState(1, dev, N, L, hop)
    sf = core.FeatureStreamState(1, dev, N, L, hop, counter=sa.counter)
    sm = core.FeatureStreamState(1, dev, N, M, hop, counter=sa.counter)
    kw = dict(return_confidence=True, return_period=True)
    legs = [
        ("stream analysis + stream mfcc (two launches, two states)",
         graphed(lambda: (core.stream_analysis(x, sr, hop, sf, **kw), core.stream_mfcc(x, sr, hop, sm, n_fft=M))), 2),
        ("stream analysis mfcc (one launch, one state)",
         graphed(lambda: core.stream_analysis_mfcc(x, sr, hop, sa, mfcc_n_fft=M, **kw)), 1),
        ("stream analysis mfcc, pitch=False", graphed(lambda: core.stream_analysis_mfcc(x, sr, hop, sa, pitch=False)), 1),
        ("stream analysis alone", graphed(lambda: core.stream_analysis(x, sr, hop, sf, **kw)), 1),
        ("stream mfcc alone", graphed(lambda: core.stream_mfcc(x, sr, hop, sm, n_fft=M)), 1),
    ]
    ms = [[] for _ in legs]
    for _ in range(windows):
        for i, (_, fn, _) in enumerate(legs):
            ms[i].append(timed(fn, reps, 1)[0])
    for (leg, _, launches), m in zip(legs, ms):
        print(json.dumps({"shape": "stream 1x1024 block 256 L 2048 M 1024", "leg": leg, "graph_nodes": launches,
                          "us": round(1e3 * statistics.median(m), 2), "us_min": round(1e3 * min(m), 2),
                          "us_max": round(1e3 * max(m), 2), "windows_us": [round(1e3 * v, 2) for v in m]}),
              flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--leg", choices=("offline", "stream", "pitch", "viterbi", "fused", "aligned", "all"), default="all",
                    help="all: offline and stream (the pitch, viterbi, fused and aligned legs run on request)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_features: needs a HIP device (there is no CPU path)")
    dev = torch.device("cuda", 0)
    if args.leg == "fused":
        fused_leg(dev, args.reps, args.windows)
        return
    if args.leg == "aligned":
        aligned_leg(dev, args.reps, args.windows)
        return
    if args.leg == "pitch":
        pitch_leg(dev, args.reps, args.windows)
        return
    if args.leg == "viterbi":
        viterbi_leg(dev, args.reps, args.windows)
        return
    if args.leg in ("stream", "all"):
        stream_leg(dev, args.reps, args.windows)
    if args.leg == "stream":
        return
    for name, B, T, hop, sr in SHAPES:
        g = torch.Generator().manual_seed(B + T)
        t = torch.arange(T) / sr
        x = (0.3 * torch.sin(2 * torch.pi * 220.0 * t) + 0.1 * torch.sin(2 * torch.pi * 1760.0 * t))[None, :] \
            * torch.linspace(1.0, 0.05, T)[None, :] + 0.01 * torch.randn(B, T, generator=g)
        x = x.to(dev)
        F = T // hop
        pitch = torch.full((B, F, 1), 220.0, device=dev)
        w = torch.from_numpy(core.a_weighting_table(sr, 2048)).float().to(dev)
        fb = torch.from_numpy(core.mel_filterbank_table(sr, 1024, 128, 20.0, 8000.0)).float().to(dev)
        dct = torch.from_numpy(core.dct_table(30, 128)).float().to(dev)
        n_w = int(core.mfcc_tables(sr, 30, 1024, 128, 20.0, 8000.0, dev)[2].numel())
        loud_bytes = 4 * (B * T + B * F + 1025)
        mfcc_bytes = 4 * (B * T + 2 * B * (F + 1) * 128 + B * (F + 1) * 30 + n_w + 30 * 128)
        legs = [
            ("loudness hip", lambda: core.extract_loudness(x, sr, hop), loud_bytes),
            ("loudness torch.stft", lambda: torch_loudness(x, w, 2048, hop), None),
            ("mfcc hip", lambda: core.mfcc(x, sr, hop), mfcc_bytes),
            ("mfcc torch.stft", lambda: torch_mfcc(x, fb, dct, 1024, hop), None),
            ("analyze hip", lambda: dd.features.analyze(x, pitch, sr, hop), loud_bytes + mfcc_bytes),
            ("analyze torch.stft", lambda: (torch_loudness(x, w, 2048, hop), torch_mfcc(x, fb, dct, 1024, hop)), None),
        ]
        # the two routes compute the same features (fp32 FFTs of different structure)
        dl = float((core.extract_loudness(x, sr, hop) - torch_loudness(x, w, 2048, hop)).abs().max())
        dm = float((core.mfcc(x, sr, hop) - torch_mfcc(x, fb, dct, 1024, hop)).abs().max())
        print(json.dumps({"shape": name, "max_abs_diff_loudness": dl, "max_abs_diff_mfcc": dm}), flush=True)
        for leg, fn, nbytes in legs:
            med, lo, hi = timed(fn, args.reps, args.windows)
            row = {"shape": name, "leg": leg, "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
            if nbytes is not None:
                row["algorithmic_bytes"] = nbytes
                row["GB_per_s"] = round(nbytes / (med * 1e-3) / 1e9, 1)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
