"""The analysis front end: raw audio on the device -> the batch ``DDSPAutoencoder.forward`` consumes.

The reference computes ``batch['loudness']`` and ``batch['mfcc']`` on the host, file by file, with librosa
(``ddsp/core.py:81-97``, ``ddsp/preprocess.py:28-32``) and stores them; ``ddsp/data.py:22-32`` hands them to the
model as [frames, 1], [frames, 1] and [frames, 30].  ``analyze`` produces the same dict from audio that is
already on the HIP device (``core.extract_loudness``, ``core.mfcc``: csrc/features.hip).  Pitch (the reference's
CREPE network, ``extract_pitch``) is not computed here: ``f0`` stays an input.
"""
import torch

from . import core

__all__ = ["analyze"]


def analyze(signal, pitch, sample_rate, block_size, mean_loudness=None, std_loudness=None):
    """signal [T] or [B, T] (HIP, fp32) and pitch (F = T // block_size values per item, [B, F] or [B, F, 1]) ->
    ``{'pitch': [B, F, 1], 'loudness': [B, F, 1], 'mfcc': [B, F, 30]}``, the shapes of ``ddsp/data.py:22-32``
    (the MFCC's last frame is dropped there, ``data.py:25``; the loudness's inside ``extract_loudness``).
    With ``mean_loudness`` and ``std_loudness`` the loudness is normalised as ``train.py:87`` does,
    ``(l - mean) / std``.  No autograd, no host synchronisation after the first call (see ``core.mfcc``)."""
    if (mean_loudness is None) != (std_loudness is None):
        raise ValueError("analyze: mean_loudness and std_loudness go together")
    x = signal.unsqueeze(0) if signal.dim() == 1 else signal
    loudness = core.extract_loudness(x, sample_rate, block_size)
    B, F = loudness.shape
    if mean_loudness is not None:
        loudness = (loudness - mean_loudness) / std_loudness
    mfcc = core.mfcc(x, sample_rate, block_size)[:, :F]
    pitch = torch.as_tensor(pitch, dtype=torch.float32, device=x.device)
    if pitch.numel() != B * F:
        raise RuntimeError(f"analyze: pitch must hold {B} x {F} values (T // block_size per item), got "
                           f"{tuple(pitch.shape)}")
    return {"pitch": pitch.reshape(B, F, 1), "loudness": loudness.unsqueeze(-1), "mfcc": mfcc}
