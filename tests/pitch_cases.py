"""The inputs of the GPU pitch tests (test_gpu_pitch.py, test_gpu_stream_pitch.py) and their restatements, built
once and shared: test_pitch_ref.py checks on the CPU that none of them has a near-tie (the fp32 restatement picks
the fp64 one's period on every frame), so a period that differs on the GPU is the GPU's."""
import functools

import numpy as np

import pitch_ref as pr

L_DEFAULT = 2048

# (sample rate, block, T, B, kind).  kind: "plain"; "one_d" (passed as a 1-D tensor); "onset" (1500 leading zeros);
# "zeros" (item 0 silent beside a voiced one)
OFFLINE = [
    (48000, 512, 4096, 2, "plain"),
    (48000, 64, 2048, 3, "plain"),
    (16000, 160, 2080, 1, "plain"),   # hop not a power of two
    (44100, 256, 2304, 2, "plain"),
    (48000, 512, 2660, 1, "plain"),   # T % hop != 0
    (48000, 512, 4096, 1, "one_d"),
    (48000, 256, 4096, 1, "onset"),
    (48000, 512, 4096, 2, "zeros"),
]

# every transform size: frame_length at 16 kHz, hop L/4 + 1, T = 3 L + 37, B = 2
SIZES = [64, 128, 256, 512, 1024, 4096]
SIZES_SR, SIZES_B = 16000, 2

# (sample rate, hop, N, B, frame_length, K calls)
STREAM = [
    (48000, 256, 1024, 1, 2048, 6),  # the ring of 2816 floats wraps twice
    (48000, 512, 512, 2, 2048, 5),   # R = 1
    (16000, 160, 480, 3, 1024, 6),   # R odd, hop not a power of two, L/2 not a multiple of hop
]


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def offline_case(sr, block, T, B, kind):
    """-> (x [B, T] float32, (tau_min, tau_max), restatement dict), read-only."""
    seed = {"plain": 0, "one_d": 1, "onset": 2, "zeros": 3}[kind] * 100003 + T + block
    x = pr.make_voiced(sr, T, B, seed, lead=1500 if kind == "onset" else 0)
    if kind == "zeros":
        x[0] = 0.0
    tmin, tmax = pr.lags(sr, 50.0, 2000.0, L_DEFAULT)
    frames = [pr.offline_frames(x[b], L_DEFAULT, block) for b in range(B)]
    return _frozen(x), (tmin, tmax), pr.restate(frames, sr, tmin, tmax)


def size_params(L):
    """(hop, T, fmin, f_lo, f_hi) of the every-transform-size case: the period lies between 4 and W/2."""
    W = L // 2
    return L // 4 + 1, 3 * L + 37, SIZES_SR / (W - 1) + 1, SIZES_SR / (W / 2), SIZES_SR / 4.0


@functools.lru_cache(maxsize=None)
def size_case(L):
    hop, T, fmin, f_lo, f_hi = size_params(L)
    x = pr.make_voiced(SIZES_SR, T, SIZES_B, seed=L, f_lo=f_lo, f_hi=f_hi)
    tmin, tmax = pr.lags(SIZES_SR, fmin, 2000.0, L)
    frames = [pr.offline_frames(x[b], L, hop) for b in range(SIZES_B)]
    return _frozen(x), (tmin, tmax), pr.restate(frames, SIZES_SR, tmin, tmax)


@functools.lru_cache(maxsize=None)
def stream_case(sr, hop, N, B, L, K):
    """-> (x [B, K N], (tau_min, tau_max), restatement dict of [B, K R] arrays)."""
    x = pr.make_voiced(sr, K * N, B, seed=N + hop + L)
    tmin, tmax = pr.lags(sr, 50.0, 2000.0, L)
    frames = [pr.stream_frames(x[b], L, hop, N) for b in range(B)]
    return _frozen(x), (tmin, tmax), pr.restate(frames, sr, tmin, tmax)
