"""fp64 numpy models of the realtime stream (ddsp_hip_stream_*), written from its definition: the references of
tests/test_gpu_stream.py, themselves checked against oracle/numpy_oracle.py by tests/test_stream_host.py."""
import numpy as np

from oracle import numpy_oracle as no

f32 = np.float32
TWO_PI = 2.0 * np.pi


def wrap_2pi(x):
    """x modulo 2 pi in fp64, into [0, 2 pi)."""
    x = np.asarray(x, dtype=np.float64)
    return x - TWO_PI * np.floor(x / TWO_PI)


def harmonic_stream(amps, f0, block_size, sample_rate, frames_per_call, wrap, carry0=None, exact=False):
    """The harmonic part of a stream of calls of `frames_per_call` frames: frame f of call k starts from
    S = carry[b] + sum_{g<f} bs inc_g (fp64), omega = fl32(S + (j + 1) inc), out = sum_k A_k sin(fl32(omega k));
    after a call carry[b] += sum_g bs inc_g, with `wrap` reduced modulo 2 pi (the initial carry too).
    amps [B,F,H] (harmonic_distribution * amplitudes), f0 [B,F,1] -> (audio [B, F*bs], final carry [B],
    largest omega).  `exact`: no fp32 rounding of omega or its products (the ideal oscillator)."""
    amps = np.asarray(amps, dtype=f32).astype(np.float64)
    B, F, H = amps.shape
    bs, R = int(block_size), int(frames_per_call)
    assert F % R == 0
    inc = no.phase_increment(f0, sample_rate)[..., 0].astype(np.float64)  # [B,F]
    carry = np.zeros(B) if carry0 is None else np.asarray(carry0, dtype=np.float64).copy()
    kk = np.arange(1, H + 1, dtype=f32)
    j1 = np.arange(1, bs + 1, dtype=np.float64)
    out = np.empty((B, F * bs))
    wmax = 0.0
    for k in range(F // R):
        c = wrap_2pi(carry) if wrap else carry
        pre = np.zeros(B)
        for f in range(R):
            g = k * R + f
            w = (c + pre)[:, None] + j1[None, :] * inc[:, g, None]  # [B,bs] fp64
            wmax = max(wmax, float(np.abs(w).max()))
            if exact:
                arg = w[..., None] * kk.astype(np.float64)
            else:
                arg = (w.astype(f32)[..., None] * kk).astype(f32).astype(np.float64)
            out[:, g * bs:(g + 1) * bs] = (np.sin(arg) * amps[:, g, None, :]).sum(-1)
            pre = pre + bs * inc[:, g]
        carry = c + pre
        if wrap:
            carry = wrap_2pi(carry)
    return out, carry, wmax


def reverb_stream(x, h, call_samples):
    """The streamed reverb's algorithm in fp64: overlap-save with the call as the partition and a ring of the last
    P = ceil(L / N) input-window spectra, slot = call index mod P.  x [B, K*N], h [L] -> y [B, K*N]."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    N, L = int(call_samples), h.shape[0]
    B, T = x.shape
    assert T % N == 0
    P = (L + N - 1) // N
    hp = np.zeros(P * N)
    hp[:L] = h
    G = np.fft.rfft(hp.reshape(P, N), 2 * N, axis=-1)  # FFT([h_p, 0]), bins 0..N
    ring = np.zeros((B, P, N + 1), dtype=np.complex128)
    hist = np.zeros((B, N))
    y = np.empty_like(x)
    for k in range(T // N):
        xk = x[:, k * N:(k + 1) * N]
        slot = k % P
        ring[:, slot] = np.fft.rfft(np.concatenate([hist, xk], axis=-1), axis=-1)
        Y = np.zeros((B, N + 1), dtype=np.complex128)
        for p in range(P):
            Y += ring[:, (slot - p) % P] * G[p]
        y[:, k * N:(k + 1) * N] = np.fft.irfft(Y, 2 * N, axis=-1)[:, N:]
        hist = xk
    return y
