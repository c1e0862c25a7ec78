"""ddsp_pytorch_amd — MI355X (gfx950) backend for the DDSP harmonic-plus-noise synthesis path.

Drop-in for hugofloresgarcia/ddsp_pytorch's synthesis hot path:

* function level — ``ddsp_pytorch_amd.core``: scale_function, remove_above_nyquist,
  upsample, harmonic_synth, amp_to_impulse_response, fft_convolve (ddsp/core.py);
* module level — ``ddsp_pytorch_amd.modules``: HarmonicSynth, FilteredNoise, Reverb
  (ddsp/models/modules.py), fused kernels;
* ``install(ddsp)`` rebinds both inside an imported reference package;
* analysis — ``core.extract_loudness``, ``core.mfcc`` and ``features.analyze``: the loudness and MFCC
  features the models consume, from raw audio on the device (ddsp/core.py:81-97, ddsp/preprocess.py:28-32);
  ``features.StreamAnalyzer`` / ``core.stream_loudness`` / ``core.stream_mfcc``: the same per call of a stream;
  ``core.extract_pitch`` / ``core.stream_pitch``: f0 from the audio by the YIN estimator (the reference's
  ``extract_pitch`` is the CREPE network, which this package does not carry), so ``analyze(signal, None, ...)``
  runs from audio alone; ``core.track_pitch`` (``analyze(..., viterbi=True)``): the same d' decoded over time by a
  Viterbi path, offline, as the reference's ``crepe.predict(..., viterbi=True)`` decodes its salience;
  ``core.stream_track_pitch`` / ``StreamAnalyzer(viterbi=True)`` / ``RealtimeGraph(pitch_viterbi=True)``: the same
  decode per call of a stream, its forward recursion carried on the device and its decision taken at a fixed lag;
  ``core.stream_analysis``: the streamed loudness and pitch in one launch over one state,
  which ``realtime.RealtimeGraph(loudness_from_audio=True, pitch_from_audio=True)`` runs per call (audio in,
  audio out); ``core.stream_analysis_mfcc`` / ``StreamAnalyzer(aligned=True)``: the streamed loudness, MFCC and pitch
  of the same frames in one launch on one time axis, which ``RealtimeGraph`` runs for a ``DDSPAutoencoder`` (the
  encoder's GRU state carried between calls): realtime timbre transfer from audio alone;
* ``DDSPDecoder`` and ``DDSPAutoencoder`` — the reference's two models (same state_dicts) running
  on these kernels.

All compute goes through the C-ABI library (include/ddsp_hip.h, lib/libddsp_hip.so);
nothing falls back to CPU.
"""
from . import core
from .core import (amp_to_impulse_response, fft_convolve, harmonic_synth, remove_above_nyquist,
                   scale_function, upsample)
from .decoder import DDSPDecoder
from .encoder import DDSPAutoencoder
from . import features
from .features import StreamAnalysisPlan, StreamAnalyzer, analyze, stream_analysis_route
from .install import install
from .modules import FilteredNoise, HarmonicSynth, Reverb
from . import synth  # noqa: E402  (SynthPath, make_inputs: the bench's and the tests' synthesis-path driver)

__version__ = "0.1.0"
