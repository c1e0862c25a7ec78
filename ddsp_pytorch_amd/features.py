"""The analysis front end: raw audio on the device -> the batch ``DDSPAutoencoder.forward`` consumes.

The reference computes ``batch['loudness']`` and ``batch['mfcc']`` on the host, file by file, with librosa
(``ddsp/core.py:81-97``, ``ddsp/preprocess.py:28-32``) and stores them; ``ddsp/data.py:22-32`` hands them to the
model as [frames, 1], [frames, 1] and [frames, 30].  ``analyze`` produces the same dict from audio that is
already on the HIP device (``core.extract_loudness``, ``core.mfcc``: csrc/features.hip).  The reference's pitch
is the CREPE network (``extract_pitch``), whose weights are not part of this package: a pitch track from elsewhere
can be passed in as before, and without one ``analyze`` computes f0 on the device with the YIN estimator
(``core.extract_pitch``: csrc/pitch.hip) — a classical tracker, not CREPE.

``StreamAnalyzer`` is the same front end for a realtime stream: audio comes in call by call and each call returns
the frames it completes (``core.stream_loudness``, ``core.stream_mfcc`` and, on request, ``core.stream_pitch``;
``aligned=True``: all of them from one launch on one time axis, ``core.stream_analysis_mfcc``; ``viterbi=True``: the
pitch from the streamed Viterbi decode, ``core.stream_track_pitch``), the history carried on the device.
"""
import torch

from . import core

__all__ = ["analyze", "StreamAnalyzer"]


def analyze(signal, pitch=None, sample_rate=None, block_size=None, mean_loudness=None, std_loudness=None, fmin=50.0,
            fmax=2000.0, viterbi=False):
    """signal [T] or [B, T] (HIP, fp32) and pitch (F = T // block_size values per item, [B, F] or [B, F, 1]) ->
    ``{'pitch': [B, F, 1], 'loudness': [B, F, 1], 'mfcc': [B, F, 30]}``, the shapes of ``ddsp/data.py:22-32``
    (the MFCC's last frame is dropped there, ``data.py:25``; the loudness's inside ``extract_loudness``).
    ``pitch=None``: f0 is computed from the audio (``core.extract_pitch`` over ``fmin`` .. ``fmax`` Hz, YIN; with
    ``viterbi=True`` ``core.track_pitch``, the Viterbi decode over the same frames' d', which keeps the track from
    jumping octaves the way the reference's ``crepe.predict(..., viterbi=True)`` does).
    ``sample_rate`` and ``block_size`` are required.  With ``mean_loudness`` and ``std_loudness`` the loudness is
    normalised as ``train.py:87`` does, ``(l - mean) / std``.  No autograd, no host synchronisation after the first
    call (see ``core.mfcc``)."""
    if sample_rate is None or block_size is None:
        raise TypeError("analyze: sample_rate and block_size are required")
    if (mean_loudness is None) != (std_loudness is None):
        raise ValueError("analyze: mean_loudness and std_loudness go together")
    x = signal.unsqueeze(0) if signal.dim() == 1 else signal
    loudness = core.extract_loudness(x, sample_rate, block_size)
    B, F = loudness.shape
    if mean_loudness is not None:
        loudness = (loudness - mean_loudness) / std_loudness
    mfcc = core.mfcc(x, sample_rate, block_size)[:, :F]
    if pitch is None:
        track = core.track_pitch if viterbi else core.extract_pitch
        pitch = track(x, sample_rate, block_size, fmin=fmin, fmax=fmax)
    pitch = torch.as_tensor(pitch, dtype=torch.float32, device=x.device)
    if pitch.numel() != B * F:
        raise RuntimeError(f"analyze: pitch must hold {B} x {F} values (T // block_size per item), got "
                           f"{tuple(pitch.shape)}")
    return {"pitch": pitch.reshape(B, F, 1), "loudness": loudness.unsqueeze(-1), "mfcc": mfcc}


class StreamAnalyzer:
    """Loudness and MFCC of a stream, call by call: ``analyzer(audio)`` takes the stream's next ``call_samples``
    samples, audio [B, N] or [B, N, 1] on the device, and returns ``{'loudness': [B, R, 1], 'mfcc': [B, R, 30]}``
    for the R = N // block_size frames the call completes, then advances the stream (one launch per feature and one
    for the advance).  ``pitch=True`` adds ``'pitch'`` and ``'confidence'`` ([B, R, 1] each: ``core.stream_pitch``
    over ``fmin`` .. ``fmax`` Hz with frames of 2048 samples, a third state on the shared counter).  The frames are
    the stream's own (zeros before its start, no reflect padding); call k holds frames
    ``k R + first_frame[name] + j`` of the offline alignment (frame f centred at sample f * block_size), so each
    feature lags by ``delay_frames[name]`` frames (loudness: n_fft 2048, MFCC: n_fft 1024 as in ``analyze``; pitch:
    2048, so it lags exactly as the loudness does).  ``fused=True`` (needs ``pitch=True``): the loudness and the
    pitch come from ONE launch over ONE state (``core.stream_analysis``; ``pitch_state is loudness_state``), the
    same bits with one launch and one ring less.  ``aligned=True`` (with or without ``pitch``): every feature comes
    from ONE launch over ONE state (``core.stream_analysis_mfcc``; ``mfcc_state is loudness_state``, and
    ``pitch_state`` too), the MFCC window centred in the loudness's, so that ``delay_frames['mfcc'] ==
    delay_frames['loudness']`` — what a model that consumes all three per frame needs.  The MFCC's top_db clamp is
    causal (``core.stream_mfcc``).
    ``viterbi=True`` (needs ``pitch=True``): ``'pitch'`` and ``'confidence'`` come from the streamed Viterbi decode
    (``core.stream_track_pitch``: the salience of the call's frames, then the carried decode with its decision
    ``pitch_lag`` frames back; ``pitch_transition`` per bin moved, at most ``pitch_max_jump`` bins a frame), which
    removes the octave jumps the per-frame pick makes under a strong second harmonic — at ``pitch_lag=0`` with no
    added latency; ``delay_frames['pitch']`` grows by ``pitch_lag``.  In this first cut the decode does not ride in
    the fused kernels, which are untouched: the loudness (``aligned=True``: the loudness and the MFCC, from
    ``core.stream_analysis_mfcc(pitch=False)``) comes from its existing launch, and the pitch from the two new
    launches over a pitch ring of its own (``pitch_state``) and the decode state (``viterbi_state``), on the shared
    counter.  ``fused=True`` is the loudness and the per-frame pick in one launch and is refused with ``viterbi``.
    ``mean_loudness`` / ``std_loudness`` as in ``analyze``.  After one warm-up call (the tables) nothing
    synchronises with the host: a call can be captured in a HIP graph over a static input buffer.  ``counter``: a
    stream counter to share (e.g. a ``core.StreamState``'s), with ``advance=False`` when that stream's own advance
    ends the call."""

    N_FFT = {"loudness": 2048, "mfcc": 1024, "pitch": 2048}

    def __init__(self, sample_rate, block_size, call_samples, batch=1, device="cuda", mean_loudness=None,
                 std_loudness=None, counter=None, advance=True, pitch=False, fmin=50.0, fmax=2000.0, fused=False,
                 aligned=False, viterbi=False, pitch_lag=0, pitch_transition=0.02, pitch_max_jump=12):
        if (mean_loudness is None) != (std_loudness is None):
            raise ValueError("StreamAnalyzer: mean_loudness and std_loudness go together")
        if fused and not pitch:
            raise ValueError("StreamAnalyzer: fused=True is the loudness and the pitch in one launch; it needs "
                             "pitch=True")
        if viterbi and not pitch:
            raise ValueError("StreamAnalyzer: viterbi=True decodes the pitch; it needs pitch=True")
        if viterbi and fused:
            raise ValueError("StreamAnalyzer: fused=True is the loudness and the per-frame pitch in one launch; "
                             "viterbi=True takes the pitch from the salience and the decode instead")
        self.sample_rate, self.block_size, self.call_samples = float(sample_rate), int(block_size), int(call_samples)
        self.mean_loudness, self.std_loudness = mean_loudness, std_loudness
        self.advance = bool(advance)
        self.loudness_state = core.FeatureStreamState(batch, device, call_samples, self.N_FFT["loudness"], block_size,
                                                      counter=counter)
        self.counter = self.loudness_state.counter
        self.aligned = bool(aligned)
        if self.aligned:  # one ring for every feature, the MFCC's window centred in the loudness's
            self.mfcc_state = self.loudness_state
        else:
            self.mfcc_state = core.FeatureStreamState(batch, device, call_samples, self.N_FFT["mfcc"], block_size,
                                                      counter=self.counter)
        self.delay_frames = {"loudness": self.loudness_state.delay_frames, "mfcc": self.mfcc_state.delay_frames}
        self.pitch, self.fmin, self.fmax = bool(pitch), float(fmin), float(fmax)
        self.viterbi, self.pitch_lag = bool(viterbi), int(pitch_lag)
        self.pitch_transition, self.pitch_max_jump = float(pitch_transition), int(pitch_max_jump)
        self.fused = bool(fused) or (self.aligned and self.pitch and not self.viterbi)
        self.pitch_state = self.viterbi_state = None
        if self.viterbi:  # a pitch ring of its own and the decode state, both on the shared counter
            n_bins = core.stream_pitch_bin_count(sample_rate, fmin, fmax, self.N_FFT["pitch"])
            self.pitch_state = core.FeatureStreamState(batch, device, call_samples, self.N_FFT["pitch"], block_size,
                                                       counter=self.counter)
            self.viterbi_state = core.ViterbiStreamState(batch, device, self.pitch_state.frames, n_bins,
                                                         self.pitch_lag, counter=self.counter)
            self.delay_frames["pitch"] = self.pitch_state.delay_frames + self.pitch_lag
        elif self.pitch:
            core.pitch_lags(sample_rate, fmin, fmax, self.N_FFT["pitch"])  # a bad range is refused here
            if self.fused:  # one ring for both: the same frames of the same samples
                if self.N_FFT["pitch"] != self.N_FFT["loudness"]:
                    raise RuntimeError("StreamAnalyzer: fused=True and aligned=True need one frame length for "
                                       "loudness and pitch")
                self.pitch_state = self.loudness_state
            else:
                self.pitch_state = core.FeatureStreamState(batch, device, call_samples, self.N_FFT["pitch"],
                                                           block_size, counter=self.counter)
            self.delay_frames["pitch"] = self.pitch_state.delay_frames
        self.first_frame = {k: -v for k, v in self.delay_frames.items()}

    def reset(self):
        self.loudness_state.reset()
        if self.mfcc_state is not self.loudness_state:
            self.mfcc_state.reset()
        if self.pitch_state is not None and self.pitch_state is not self.loudness_state:
            self.pitch_state.reset()
        if self.viterbi_state is not None:
            self.viterbi_state.reset()

    @torch.no_grad()
    def __call__(self, audio):
        f0 = conf = mfcc = None
        if self.aligned:
            got = core.stream_analysis_mfcc(audio, self.sample_rate, self.block_size, self.loudness_state,
                                            pitch=self.fused, fmin=self.fmin, fmax=self.fmax,
                                            frame_length=self.N_FFT["loudness"], return_confidence=self.fused,
                                            mfcc_n_fft=self.N_FFT["mfcc"])
            loudness, mfcc = got[:2]
            if self.fused:
                f0, conf = got[2:]
        elif self.fused:
            loudness, f0, conf = core.stream_analysis(audio, self.sample_rate, self.block_size, self.loudness_state,
                                                      fmin=self.fmin, fmax=self.fmax,
                                                      frame_length=self.N_FFT["loudness"], return_confidence=True)
        else:
            loudness = core.stream_loudness(audio, self.sample_rate, self.block_size, self.loudness_state,
                                            n_fft=self.N_FFT["loudness"])
        if self.mean_loudness is not None:
            loudness = (loudness - self.mean_loudness) / self.std_loudness
        if mfcc is None:
            mfcc = core.stream_mfcc(audio, self.sample_rate, self.block_size, self.mfcc_state,
                                    n_fft=self.N_FFT["mfcc"])
        out = {"loudness": loudness.unsqueeze(-1), "mfcc": mfcc}
        if self.pitch:
            if self.viterbi:
                f0, conf = core.stream_track_pitch(audio, self.sample_rate, self.block_size, self.pitch_state,
                                                   self.viterbi_state, fmin=self.fmin, fmax=self.fmax,
                                                   frame_length=self.N_FFT["pitch"],
                                                   transition=self.pitch_transition, max_jump=self.pitch_max_jump,
                                                   return_confidence=True)
            elif not self.fused:
                f0, conf = core.stream_pitch(audio, self.sample_rate, self.block_size, self.pitch_state,
                                             fmin=self.fmin, fmax=self.fmax, frame_length=self.N_FFT["pitch"],
                                             return_confidence=True)
            out["pitch"], out["confidence"] = f0.unsqueeze(-1), conf.unsqueeze(-1)
        if self.advance:
            core.stream_advance(self.loudness_state)
        return out
