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
pitch from the streamed Viterbi decode, ``core.stream_track_pitch``), the history carried on the device.  Which
launches run over which rings is ``stream_analysis_route``'s table; ``StreamAnalysisPlan`` holds the states and runs
it, for ``StreamAnalyzer`` and ``realtime.RealtimeGraph`` alike.
"""
from collections import namedtuple

import torch

from . import core

__all__ = ["analyze", "StreamAnalyzer", "StreamAnalysisPlan", "stream_analysis_route"]


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


N_FFT = {"loudness": 2048, "mfcc": 1024, "pitch": 2048}  # the streamed features' frame lengths, ``analyze``'s

StreamRoute = namedtuple("StreamRoute", "mfcc pitch calls rings decode")


def stream_analysis_route(mfcc, pitch):
    """Which ``core`` calls one call of a stream makes, over which rings (pure: no device, no state).  ``mfcc``:
    None, "own" (``stream_mfcc`` over a ring of the MFCC's frame length) or "aligned" (in the loudness's launch, on its
    time axis).  ``pitch``: None, "own" (``stream_pitch`` over a ring of its own), "fused" (the per-frame pick in the
    loudness's launch) or "viterbi" (the salience over a ring of its own, then the carried decode).  -> StreamRoute:
    ``calls``, the ``core.stream_*`` functions in launch order (the advance not counted); ``rings``, a (feature, ring)
    pair per feature — "main" is the loudness's ring, "mfcc" and "pitch" rings of their own; ``decode``, whether a
    ``ViterbiStreamState`` exists.  The table (calls without their ``stream_`` prefix; ``analysis_mfcc`` computes the
    pitch exactly when the pitch reads "main", i.e. under "fused"):

        mfcc     pitch    calls                                            rings
        None     None     loudness                                         main
        None     own      loudness, pitch                                  main, pitch
        None     fused    analysis                                         main
        None     viterbi  pitch_salience, viterbi_path, loudness           main, pitch
        own      None     loudness, mfcc                                   main, mfcc
        own      own      loudness, mfcc, pitch                            main, mfcc, pitch
        own      fused    analysis, mfcc                                   main, mfcc
        own      viterbi  pitch_salience, viterbi_path, loudness, mfcc     main, mfcc, pitch
        aligned  None     analysis_mfcc(pitch=False)                       main
        aligned  fused    analysis_mfcc(pitch=True)                        main
        aligned  viterbi  pitch_salience, viterbi_path, analysis_mfcc(pitch=False)  main, pitch

    ("aligned", "own") is refused: the aligned launch takes the per-frame pick along."""
    if mfcc not in (None, "own", "aligned") or pitch not in (None, "own", "fused", "viterbi"):
        raise ValueError(f"stream_analysis_route: no such route, mfcc={mfcc!r}, pitch={pitch!r}")
    if mfcc == "aligned" and pitch == "own":
        raise ValueError("stream_analysis_route: mfcc='aligned' computes the per-frame pitch in its own launch "
                         "(pitch='fused'), not in a launch beside it")
    main = "stream_analysis_mfcc" if mfcc == "aligned" else "stream_analysis" if pitch == "fused" else "stream_loudness"
    calls = ("stream_pitch_salience", "stream_viterbi_path") if pitch == "viterbi" else ()
    calls += (main,) + (("stream_mfcc",) if mfcc == "own" else ()) + (("stream_pitch",) if pitch == "own" else ())
    rings = (("loudness", "main"),)
    if mfcc:
        rings += (("mfcc", "main" if mfcc == "aligned" else "mfcc"),)
    if pitch:
        rings += (("pitch", "main" if pitch == "fused" else "pitch"),)
    return StreamRoute(mfcc, pitch, calls, rings, pitch == "viterbi")


class StreamAnalysisPlan:
    """One route of ``stream_analysis_route`` made runnable: ``states``, the ``core.FeatureStreamState`` each feature
    reads (one object per ring: features on "main" share the loudness's), and ``viterbi_state``, the
    ``core.ViterbiStreamState``, all on one ``counter`` (``counter``: one to share); ``delay_frames`` per feature (the
    pitch's with ``pitch_lag``).  ``n_fft``: the frame lengths by feature (``N_FFT``).  Refused at construction: what
    the states refuse, a pitch range without a lag (``core.pitch_lags``), and a pitch in the loudness's launch at
    another frame length.  ``run(audio)`` makes the route's calls on one call of the stream, audio [B, N] or
    [B, N, 1], and returns the raw (loudness, mfcc, f0, confidence), None for a feature the route lacks: no
    normalisation, no advance, no host synchronisation after the first call (capturable in a HIP graph)."""

    def __init__(self, route, sample_rate, block_size, call_samples, batch, device, counter=None, n_fft=None,
                 n_mfcc=30, fmin=50.0, fmax=2000.0, threshold=0.1, pitch_lag=0, pitch_transition=0.02,
                 pitch_max_jump=12):
        self.route, self.n_fft = route, dict(N_FFT if n_fft is None else n_fft)
        self.sample_rate, self.block_size, self.n_mfcc = float(sample_rate), int(block_size), int(n_mfcc)
        self.pitch_lag = int(pitch_lag)
        # keywords of the pitch calls, of the per-frame pick among them, and of the decode
        self.pitch_args = dict(fmin=float(fmin), fmax=float(fmax), frame_length=self.n_fft["pitch"])
        self.pick_args = dict(self.pitch_args, threshold=float(threshold), return_confidence=True)
        self.decode_args = dict(transition=float(pitch_transition), max_jump=int(pitch_max_jump))
        if route.pitch:
            core.pitch_lags(sample_rate, fmin, fmax, self.n_fft["pitch"])  # a bad range is refused here
            if route.pitch == "fused" and self.n_fft["pitch"] != self.n_fft["loudness"]:
                raise RuntimeError("StreamAnalysisPlan: pitch='fused' needs one frame length for loudness and pitch")
        self.counter, self.states, rings = counter, {}, {}
        for feature, ring in route.rings:  # "main", the loudness's, comes first: its counter is everyone's
            if ring not in rings:
                rings[ring] = core.FeatureStreamState(batch, device, call_samples, self.n_fft[feature], block_size,
                                                      counter=self.counter)
                self.counter = rings[ring].counter
            self.states[feature] = rings[ring]
        self.delay_frames = {feature: s.delay_frames for feature, s in self.states.items()}
        self.viterbi_state = None
        if route.decode:
            n_bins = core.stream_pitch_bin_count(sample_rate, fmin, fmax, self.n_fft["pitch"])
            self.viterbi_state = core.ViterbiStreamState(batch, device, self.states["pitch"].frames, n_bins,
                                                         self.pitch_lag, counter=self.counter)
            self.delay_frames["pitch"] += self.pitch_lag

    def reset(self):
        for s in list(self.states.values()) + [self.viterbi_state] * self.route.decode:
            s.reset()

    def run(self, audio):
        sr, bs, n_fft = self.sample_rate, self.block_size, self.n_fft
        loudness = mfcc = f0 = conf = None
        for call in self.route.calls:
            if call == "stream_pitch_salience":
                cost, f0c = core.stream_pitch_salience(audio, sr, bs, self.states["pitch"], **self.pitch_args)
            elif call == "stream_viterbi_path":
                f0, conf, _ = core.stream_viterbi_path(cost, f0c, self.viterbi_state, **self.decode_args)
            elif call == "stream_loudness":
                loudness = core.stream_loudness(audio, sr, bs, self.states["loudness"], n_fft=n_fft["loudness"])
            elif call == "stream_mfcc":
                mfcc = core.stream_mfcc(audio, sr, bs, self.states["mfcc"], n_mfcc=self.n_mfcc, n_fft=n_fft["mfcc"])
            elif call == "stream_pitch":
                f0, conf = core.stream_pitch(audio, sr, bs, self.states["pitch"], **self.pick_args)
            elif call == "stream_analysis":
                loudness, f0, conf = core.stream_analysis(audio, sr, bs, self.states["loudness"], **self.pick_args)
            elif self.route.pitch == "fused":
                loudness, mfcc, f0, conf = core.stream_analysis_mfcc(
                    audio, sr, bs, self.states["loudness"], n_mfcc=self.n_mfcc, mfcc_n_fft=n_fft["mfcc"],
                    **self.pick_args)
            else:
                loudness, mfcc = core.stream_analysis_mfcc(
                    audio, sr, bs, self.states["loudness"], pitch=False, frame_length=n_fft["loudness"],
                    n_mfcc=self.n_mfcc, mfcc_n_fft=n_fft["mfcc"])
        return loudness, mfcc, f0, conf


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
    added latency; ``delay_frames['pitch']`` grows by ``pitch_lag``.  ``fused=True`` is the loudness and the
    per-frame pick in one launch and is refused with ``viterbi``.  Which launches a call makes over which rings is
    ``stream_analysis_route``'s table, for ``route_for``'s (mfcc, pitch); ``plan`` holds the states and runs it.
    ``mean_loudness`` / ``std_loudness`` as in ``analyze``.  After one warm-up call (the tables) nothing
    synchronises with the host: a call can be captured in a HIP graph over a static input buffer.  ``counter``: a
    stream counter to share (e.g. a ``core.StreamState``'s), with ``advance=False`` when that stream's own advance
    ends the call."""

    N_FFT = N_FFT

    @staticmethod
    def route_for(pitch=False, fused=False, aligned=False, viterbi=False):
        """The flags -> ``stream_analysis_route``'s (mfcc, pitch); a combination the constructor refuses raises here."""
        if fused and not pitch:
            raise ValueError("StreamAnalyzer: fused=True is the loudness and the pitch in one launch; it needs "
                             "pitch=True")
        if viterbi and not pitch:
            raise ValueError("StreamAnalyzer: viterbi=True decodes the pitch; it needs pitch=True")
        if viterbi and fused:
            raise ValueError("StreamAnalyzer: fused=True is the loudness and the per-frame pitch in one launch; "
                             "viterbi=True takes the pitch from the salience and the decode instead")
        how = None if not pitch else "viterbi" if viterbi else "fused" if fused or aligned else "own"
        return "aligned" if aligned else "own", how

    def __init__(self, sample_rate, block_size, call_samples, batch=1, device="cuda", mean_loudness=None,
                 std_loudness=None, counter=None, advance=True, pitch=False, fmin=50.0, fmax=2000.0, fused=False,
                 aligned=False, viterbi=False, pitch_lag=0, pitch_transition=0.02, pitch_max_jump=12):
        if (mean_loudness is None) != (std_loudness is None):
            raise ValueError("StreamAnalyzer: mean_loudness and std_loudness go together")
        route = stream_analysis_route(*self.route_for(pitch, fused, aligned, viterbi))
        self.sample_rate, self.block_size, self.call_samples = float(sample_rate), int(block_size), int(call_samples)
        self.mean_loudness, self.std_loudness = mean_loudness, std_loudness
        self.advance = bool(advance)
        self.plan = StreamAnalysisPlan(route, sample_rate, block_size, call_samples, batch, device, counter=counter,
                                       n_fft=self.N_FFT, fmin=fmin, fmax=fmax, pitch_lag=pitch_lag,
                                       pitch_transition=pitch_transition, pitch_max_jump=pitch_max_jump)
        self.pitch, self.aligned, self.viterbi = bool(pitch), bool(aligned), bool(viterbi)
        self.fused = route.pitch == "fused"
        self.counter, self.delay_frames = self.plan.counter, self.plan.delay_frames
        self.loudness_state, self.mfcc_state = self.plan.states["loudness"], self.plan.states["mfcc"]
        self.pitch_state, self.viterbi_state = self.plan.states.get("pitch"), self.plan.viterbi_state
        self.first_frame = {k: -v for k, v in self.delay_frames.items()}

    def reset(self):
        self.plan.reset()

    @torch.no_grad()
    def __call__(self, audio):
        loudness, mfcc, f0, conf = self.plan.run(audio)
        if self.mean_loudness is not None:
            loudness = (loudness - self.mean_loudness) / self.std_loudness
        out = {"loudness": loudness.unsqueeze(-1), "mfcc": mfcc}
        if self.pitch:
            out["pitch"], out["confidence"] = f0.unsqueeze(-1), conf.unsqueeze(-1)
        if self.advance:
            core.stream_advance(self.loudness_state)
        return out
