"""Digests of the reverb's output and gradients (seeded input) for the library DDSP_HIP_LIB points at: same-box
bit-identity check of a kernel variant against the shipped library (tools/ab_build.sh / tools/ab_src.sh /
tools/ab_commit.sh builds).  The forward at config 2 (two calls: the IR built, then cached); the backward
(dx, d_noise, d_decay, d_wet through grad.reverb_backward_params) at config 2, the whole-row stream MACs, and at
(B, T, L) = (3, 20000, 9000), the ring MACs.

    DDSP_HIP_LIB=build/ab_<name>.so python tools/exp_lib_digest.py [B]
"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddsp_pytorch_amd import core, grad  # noqa: E402
from ddsp_pytorch_amd.synth import SynthPath  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
dev = torch.device("cuda", 0)


def digest(*tensors):
    return hashlib.sha256(b"".join(t.detach().cpu().numpy().tobytes() for t in tensors)).hexdigest()[:16]


def backward_digests(rv, b, T):
    """dx, d_noise, d_decay, d_wet of the reverb module rv for a seeded (x, g) of b rows of T samples."""
    gen = torch.Generator().manual_seed(b * T + rv.length)
    x = (torch.randn(b, T, 1, generator=gen) * 0.3).to(dev)
    g = torch.randn(b, T, 1, generator=gen).to(dev)
    noise, decay, wet = (p.detach() for p in (rv.noise, rv.decay, rv.wet))
    with torch.no_grad():
        spec = core.reverb_impulse_spectrum(noise, decay, wet, rv.sample_rate, T)
        _, ws = core._reverb_apply_launch(x, spec, rv.length)
    out = grad.reverb_backward_params(ws, spec, g, noise, decay, wet, rv.length, rv.sample_rate, True)
    torch.cuda.synchronize()
    return {k: digest(t) for k, t in zip(("dx", "d_noise", "d_decay", "d_wet"), out)}


torch.manual_seed(0)
syn = SynthPath(512, 48000, reverb_length=48000).to(dev)
x = torch.randn(B, 200 * 512, 1, device=dev)
with torch.no_grad():
    y = syn.reverb(x)
    y2 = syn.reverb(x * 0.5)  # a second call on the cached IR spectrum
torch.cuda.synchronize()
res = {"lib": os.environ.get("DDSP_HIP_LIB", "in-tree"), "B": B, "digest": digest(y, y2),
       "rms": float(y.pow(2).mean().sqrt()), "finite": bool(torch.isfinite(y).all()),
       "bwd_config2": backward_digests(syn.reverb, B, 200 * 512)}
torch.manual_seed(0)
small = SynthPath(512, 48000, reverb_length=9000).to(dev)
res["bwd_3_20000_9000"] = backward_digests(small.reverb, 3, 20000)
print(json.dumps(res))
