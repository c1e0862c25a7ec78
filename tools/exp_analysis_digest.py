"""Digests of what the analysis entry points compute (loudness, MFCC, YIN pitch, salience, the Viterbi decodes, offline
and streamed, separate and fused) for the library DDSP_HIP_LIB points at: same-box bit-identity check of a variant of
the analysis kernels against the shipped library (tools/ab_commit.sh builds).  Seeded input at small shapes: a batch of
3, frame lengths 64, 2048 and 4096 (16 too for the loudness and the MFCC), a hop that leaves an odd frame count (the
lone last frame of a pair and the lanes past the last frame both run); every streamed entry point runs three calls from
a fresh state (call 0, the partly filled ring, the wrapped ring); the decodes run with 1, 65 and 1024 bins, max_jump 0
and 12, lag 0 and 4.  One JSON line; two libraries that compute the same print the same "digests".

    DDSP_HIP_LIB=build/ab_<name>.so python tools/exp_analysis_digest.py
"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddsp_pytorch_amd import core  # noqa: E402

dev = torch.device("cuda", 0)
SR, HOP, B, CALLS = 16000, 96, 3, 3
N = 5 * HOP  # samples per streamed call: five frames
MELS = {16: (4, 4), 64: (16, 16), 2048: (256, 256), 4096: (128, 30)}  # n_fft -> (n_mels, n_mfcc)


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if isinstance(t, (tuple, list)):
            h.update(digest(*t).encode())
        else:
            h.update(t.detach().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def audio(seed, n):
    gen = torch.Generator().manual_seed(seed)
    t = torch.arange(n) / SR
    tone = torch.sin(2 * torch.pi * (180.0 + 40.0 * torch.arange(B)[:, None]) * t[None])
    return (0.5 * tone + 0.1 * torch.randn(B, n, generator=gen)).to(dev)


def streamed(fn, L, seed):
    """The digests of CALLS calls of fn(x, state) from a fresh FeatureStreamState of frame length L."""
    state = core.FeatureStreamState(B, dev, N, L, HOP)
    x = audio(seed, CALLS * N)
    out = []
    for k in range(CALLS):
        out.append(fn(x[:, k * N:(k + 1) * N].contiguous(), state))
        core.stream_advance(state)
    return digest(*out)


res = {}
for L in (16, 64, 2048, 4096):
    T = 25 * HOP + 7 + L // 2
    T += HOP * (1 - (T // HOP) % 2)  # 25 or more frames, an odd count
    x = audio(L, T)
    n_mels, n_mfcc = MELS[L]
    mkw = dict(n_mfcc=n_mfcc, n_fft=L, n_mels=n_mels, fmin=20.0, fmax=8000.0)
    res[f"loudness/{L}"] = digest(core.extract_loudness(x, SR, HOP, n_fft=L))
    res[f"mfcc/{L}"] = digest(core.mfcc(x, SR, HOP, return_db=True, **mkw))
    res[f"stream_loudness/{L}"] = streamed(lambda c, s: core.stream_loudness(c, SR, HOP, s, n_fft=L), L, L + 1)
    res[f"stream_mfcc/{L}"] = streamed(lambda c, s: core.stream_mfcc(c, SR, HOP, s, **mkw), L, L + 2)
    if L < 64:
        continue
    pkw = dict(frame_length=L, return_confidence=True, return_period=True)
    res[f"pitch/{L}"] = digest(core.extract_pitch(x, SR, HOP, **pkw))
    res[f"stream_pitch/{L}"] = streamed(lambda c, s: core.stream_pitch(c, SR, HOP, s, **pkw), L, L + 3)
    res[f"stream_analysis/{L}"] = streamed(lambda c, s: core.stream_analysis(c, SR, HOP, s, **pkw), L, L + 4)
    skw = dict(frame_length=L, return_lag=True, return_raw=True)
    res[f"pitch_salience/{L}"] = digest(core.pitch_salience(x, SR, HOP, **skw))
    res[f"pitch_salience_plain/{L}"] = digest(core.pitch_salience(x, SR, HOP, frame_length=L))
    res[f"stream_pitch_salience/{L}"] = streamed(lambda c, s: core.stream_pitch_salience(c, SR, HOP, s, **skw), L, L + 5)
    if L > 2048:
        continue
    for M in (L, L // 2):
        m_mels, m_mfcc = MELS.get(M, (32, 13))
        akw = dict(frame_length=L, mfcc_n_fft=M, n_mfcc=m_mfcc, n_mels=m_mels)
        res[f"stream_analysis_mfcc/{L}/{M}"] = streamed(
            lambda c, s: core.stream_analysis_mfcc(c, SR, HOP, s, return_confidence=True, return_period=True, **akw),
            L, L + M)
        res[f"stream_analysis_mfcc_nopitch/{L}/{M}"] = streamed(
            lambda c, s: core.stream_analysis_mfcc(c, SR, HOP, s, pitch=False, **akw), L, L + M + 1)

for NB in (1, 65, 1024):
    gen = torch.Generator().manual_seed(NB)
    F = 2 * core._lib.query("pitch_viterbi_chunk_frames", NB) + 3 if NB == 1024 else 37  # more than one chunk
    cost = torch.rand(B, F, NB, generator=gen).mul(8).round().div(8).to(dev)  # ties: the smallest index wins
    f0c = (100.0 + 400.0 * torch.rand(B, F, NB, generator=gen)).to(dev)
    for J in (0, 12):
        res[f"pitch_viterbi/{NB}/{J}"] = digest(core.viterbi_path(cost, f0c, transition=0.02, max_jump=J))
        for D in (0, 4):
            state = core.ViterbiStreamState(B, dev, 5, NB, lag=D)
            out = []
            for k in range(CALLS):
                sl = slice(5 * k, 5 * k + 5)
                out.append(core.stream_viterbi_path(cost[:, sl].contiguous(), f0c[:, sl].contiguous(), state,
                                                    transition=0.02, max_jump=J))
                core.stream_advance(state)
            res[f"stream_pitch_viterbi/{NB}/{J}/{D}"] = digest(*out)

torch.cuda.synchronize()
print(json.dumps({"lib": os.environ.get("DDSP_HIP_LIB", "in-tree"),
                  "all": hashlib.sha256("".join(res.values()).encode()).hexdigest()[:16], "digests": res}))
