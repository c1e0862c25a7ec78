"""Realtime streaming on a captured HIP graph (BASELINE.json config 3).

The reference's realtime host, the `ddsp~` Pd external, calls the exported model once per
1024-sample buffer from a worker thread (`realtime/ddsp_tilde/ddsp_model.cpp:32-52`,
`ddsp_tilde.cpp:67-98`): pitch and loudness at audio rate in, audio out, the GRU state carried
between calls in `cache_gru` (`decoder.py:56-60`), no reverb (`export.py:37-40`).  At batch 1
and 4 frames per call that forward is ~25 short launches (MLPs, LayerNorms, the GRU steps, the
synthesis), so its latency is launch-bound, not compute-bound.

`RealtimeGraph` captures one call — loudness normalisation, decimation by block_size, the
control network with the cached GRU state, the fused synthesis kernel — into a HIP graph
(`torch.cuda.CUDAGraph` is hipGraph on ROCm) over static device buffers, and replays it per
call: one graph launch plus the two host<->device copies.  With `fused=True` (default) the
control network runs on `ddsp_hip_dense_rows` (csrc/dense.hip): each Linear one launch with the
previous block's LayerNorm + LeakyReLU, the first K=1 Linear, the loudness normalisation and
the concatenations folded into its input — 7 launches + the GRU steps + the synthesis instead
of ~30 torch kernels.  The on-device noise takes its
Philox offset from a device counter the graph advances (`ddsp_hip_synth_frames_counter`), so
every replay draws fresh noise; call k equals the eager model run with noise offset k.

By default the synthesis is stateless across calls, as the reference's: every oscillator restarts at
phase zero at each call boundary and there is no reverb.  ``continuous=True`` makes the stream
seamless: the graph holds the streamed synthesis (`ddsp_hip_stream_synth_frames`), whose phase prefix
continues from a per-stream carry in device memory, and the advance launch that replaces the counter
advance also moves the carry (``wrap``: modulo 2 pi, so omega keeps its fp32 resolution for ever) —
the same number of launches.  ``reverb=True`` adds the streamed reverb (`ddsp_hip_stream_reverb`, one
more launch) with the model's reverb parameters and the impulse response at its full length, so K
calls of N samples are the K N samples the offline model renders.

``loudness_from_audio=True`` makes the input side seamless too: the second input of a call is the stream's
audio, and the graph computes the loudness from it (`ddsp_hip_stream_loudness`, one more launch: the reference's
`extract_loudness`, core.py:81-97, with the history a 2048-sample window needs carried on the device) before
the normalisation and the control network.  ``pitch_from_audio=True`` on top of it makes the audio the only input:
that launch becomes `ddsp_hip_stream_analysis`, which computes the loudness and the YIN f0 of the same frames side by
side over the same ring, and the f0 drives the control network and the synthesis — audio in, audio out.

A ``DDSPAutoencoder`` (the reference's z-conditioned model, ``ddsp/models/encoder.py``) runs the same way, from audio
alone: the analysis launch becomes `ddsp_hip_stream_analysis_mfcc`, which adds the streamed MFCC of the same frames
(its 1024-sample window centred in the loudness's 2048, so z, f0 and loudness of one frame describe one instant),
the MFCC encoder runs with its GRU state carried from call to call in ``encoder_state``, and z joins the decoder
GRU's input through ``z_mlp``.
"""
from collections import namedtuple

import torch

from . import core
from .decoder import gru_decoder_forward
from .features import StreamAnalysisPlan, stream_analysis_route

_Linear = namedtuple("_Linear", "weight bias in_features out_features")


class RealtimeGraph:
    """Graph-replayed realtime forward of a `DDSPDecoder` (the ScriptDDSP realtime model of
    export.py:23-40: `forward(pitch[1,N,1], loudness[1,N,1]) -> audio[1,N,1]`) or, from audio, of a
    `DDSPAutoencoder` (last paragraph).

    The model's `decoder.cache_gru` is the stream state (updated in place by every call, as in
    decoder.py:56-60); `reset()` zeroes it and rewinds the noise counter.  The returned tensor
    is a static buffer overwritten by the next call (the host copies it out, as `ddsp~` does
    with memcpy).

    ``continuous=True``: the oscillator phase carries over from call to call (``wrap``, default True
    then: the carry is kept modulo 2 pi).  ``reverb=True`` (needs ``continuous`` and a power-of-two
    ``call_samples`` in [64, 2048]): the model's reverb runs in the stream with its full impulse
    response, built at construction (`refresh()` rebuilds it after the parameters change).  The
    stream's device state is `self.stream` (core.StreamState); `reset()` zeroes it too.

    ``loudness_from_audio=True``: ``__call__(pitch, audio)`` — the second input is the call's audio [1, N, 1],
    and the graph runs `core.stream_loudness` (n_fft 2048, hop = block_size) on it in place of a loudness input.
    A frame's window is complete only `loudness_delay_samples` (= (ceil(1024 / block_size) - 1) block_size: 768 at
    block 256) after its centre, so the loudness that drives a call's frames is that much older than the call's
    samples.  The pitch is NOT delayed to match: pitch trackers bring a latency of their own, and aligning the
    two is the caller's.  The analysis shares the stream's call counter (with ``continuous`` the `StreamState`'s),
    its state is `self.analysis` (core.FeatureStreamState), and `reset()` zeroes it too.

    ``pitch_from_audio=True`` (needs ``loudness_from_audio=True``; with or without ``continuous`` / ``reverb``):
    ``__call__(audio)`` — the call's audio [1, N, 1] is the only input (a host call copies N floats in, not 2 N),
    and the graph runs `core.stream_analysis` on it: the loudness and the YIN f0 (``pitch_fmin`` .. ``pitch_fmax``
    Hz, ``pitch_threshold``) of the same 2048-sample frames in one launch over the one analysis state, so the graph
    holds as many launches as with ``loudness_from_audio`` alone.  The per-frame f0 drives the control network and
    the synthesis; it lags as the loudness does (`pitch_delay_samples == loudness_delay_samples`).  `self.f0` and
    `self.confidence` are static [1, R] device buffers holding the last call's values, for the host to monitor or
    gate on.  Nothing holds or smooths f0: an unvoiced or silent frame carries YIN's value as it is (a silent frame
    gives sample_rate / tau_min with confidence 0), and the instrument is then as quiet as its loudness says.

    ``pitch_viterbi=True`` (needs ``pitch_from_audio=True``; decoder or autoencoder, with or without ``continuous`` /
    ``reverb``): the graph's f0 is the streamed Viterbi decode's (`core.stream_track_pitch`: ``pitch_transition`` per
    bin moved, at most ``pitch_max_jump`` bins a frame, the decision ``pitch_lag`` frames back), so an octave jump of
    the per-frame pick under a strong second harmonic no longer passes through the control network and the
    oscillator bank as a one-frame yodel.  The salience runs over a pitch ring of its own, `self.pitch_ring`, the
    carried decode over `self.viterbi`, and they give `self.f0` and `self.confidence` (1 - d' along the path).
    `pitch_delay_samples == loudness_delay_samples + pitch_lag * block_size`; the loudness is NOT delayed to match
    (the stance above for an external pitch), and ``pitch_lag=0``, the default, adds no latency.  `reset()` gives a
    fresh decode.  Which launches the analysis makes over which rings, for any of these options, is
    `features.stream_analysis_route`'s table at `route_for`'s (mfcc, pitch); `self.plan`
    (features.StreamAnalysisPlan) holds the states and runs it.

    A ``DDSPAutoencoder`` (recognised by ``model.decoder.add_z`` and ``model.encoder``) needs
    ``loudness_from_audio=True``: its encoder's MFCC can only come from audio.  With ``pitch_from_audio=True``
    ``__call__(audio)`` is audio in, audio out; without it ``__call__(pitch, audio)``; ``continuous`` / ``reverb`` as for
    the decoder.  The graph runs `core.stream_analysis_mfcc` on the one analysis state (the loudness, the MFCC and,
    from audio, the pitch in one launch; `mfcc_delay_samples == loudness_delay_samples`), then the encoder — ``norm``,
    the GRU with a carried state, ``proj`` — and the decoder with z.  ``encoder_state`` [1, 1, hidden] is the encoder
    GRU's state between calls: a buffer of this object (the model's state_dict stays the reference's), zero at the
    start and after `reset()`.  ``z`` is a static [1, R, 16] device buffer with the last call's values.
    ``fused=True`` runs all of it on `ddsp_hip_dense_rows` and the GRU step kernels (the encoder's GRU always on the
    step kernels, the decoder's by ``gru_route``): 3 dense launches and R encoder steps more than the decoder's graph —
    the encoder GRU's input projection (with ``norm`` folded in as a LayerNorm without activation), ``proj``, and
    ``z_mlp``'s first Linear; ``z_mlp``'s other two blocks ride in ``f0_mlp``'s and ``loudness_mlp``'s launches as a
    third problem, and the decoder GRU's input projection takes three segments (K = 3 hidden, up to 1536).
    ``fused=False`` replays the package's eager kernels (``model.encoder.norm``, `core.gru` with the carried state,
    ``model.encoder.proj``, `gru_decoder_forward` with z).  The capture stays on one stream: the encoder chain is not
    forked beside the f0 / loudness MLPs."""

    def __init__(self, model, call_samples=1024, mean_loudness=0.0, std_loudness=1.0,
                 seed=0x5EEDDD5B, device=None, warmup=3, fused=True, gru_route="steps",
                 continuous=False, reverb=False, wrap=None, loudness_from_audio=False, pitch_from_audio=False,
                 pitch_fmin=50.0, pitch_fmax=2000.0, pitch_threshold=0.1, pitch_viterbi=False, pitch_lag=0,
                 pitch_transition=0.02, pitch_max_jump=12):
        device = torch.device(device) if device is not None else next(model.parameters()).device
        if device.type != "cuda":
            raise RuntimeError("RealtimeGraph: the model must be on a HIP device")
        bs = int(model.block_size)
        N = int(call_samples)
        if N % bs:
            raise RuntimeError(f"RealtimeGraph: call_samples {N} must be a multiple of block_size {bs}")
        if not core.synth_frames_in_envelope(model.harmonic_proj.out_features - 1,
                                             model.noise_proj.out_features, bs, 1):
            raise RuntimeError("RealtimeGraph: model shape outside the fused synthesis kernel's envelope")
        self.autoencoder = bool(getattr(model.decoder, "add_z", False)) and hasattr(model, "encoder")
        if self.autoencoder and not loudness_from_audio:
            raise RuntimeError("RealtimeGraph: a DDSPAutoencoder needs loudness_from_audio=True (its encoder's MFCC can "
                               "only come from audio)")
        self.model = model
        self.device = device
        self.block_size = bs
        self.call_samples = N
        self.sample_rate = float(model.sample_rate)
        self.mean_loudness = float(mean_loudness)
        self.std_loudness = float(std_loudness)
        self.seed = int(seed)
        self.bias = float(model.noise_synth.initial_bias)
        # pitch and loudness share one buffer: one host->device copy per call
        self._inp = torch.zeros(2, N, 1, device=device)
        self.pitch, self.loudness = self._inp[0:1], self._inp[1:2]
        self.counter = torch.zeros(1, dtype=torch.int64, device=device)
        self.continuous = bool(continuous)
        self.reverb = bool(reverb)
        self.wrap = self.continuous if wrap is None else bool(wrap)
        self.stream = None
        if self.reverb and not self.continuous:
            raise RuntimeError("RealtimeGraph: reverb=True needs continuous=True (the streamed reverb)")
        if self.wrap and not self.continuous:
            raise RuntimeError("RealtimeGraph: wrap applies to the phase carry of continuous=True")
        if self.continuous:
            L = int(model.reverb.length) if self.reverb else 0
            self.stream = core.StreamState(1, device, N, L)  # raises on a call size the reverb cannot take
            self.counter = self.stream.counter
            if self.reverb:
                self._spec = torch.empty(int(core._lib.query("stream_spectrum_floats", N, L)), device=device)
                self.refresh()
        self.loudness_from_audio, self.pitch_from_audio = bool(loudness_from_audio), bool(pitch_from_audio)
        self.pitch_viterbi = bool(pitch_viterbi)
        if self.pitch_from_audio and not self.loudness_from_audio:
            raise RuntimeError("RealtimeGraph: pitch_from_audio=True needs loudness_from_audio=True (one launch "
                               "computes both from the same frames of the same ring)")
        route = self.route_for(self.autoencoder, self.pitch_from_audio, self.pitch_viterbi)
        self.plan = self.analysis = self.pitch_ring = self.viterbi = None
        self.f0 = self.confidence = self.z = self.mfcc = self.encoder_state = None
        delay = {}
        if self.loudness_from_audio:  # raises on a call size, a block or a pitch range the analysis cannot take
            self.plan = StreamAnalysisPlan(
                stream_analysis_route(*route), self.sample_rate, bs, N, 1, device, counter=self.counter,
                n_mfcc=model.encoder.gru.input_size if self.autoencoder else 30, fmin=pitch_fmin, fmax=pitch_fmax,
                threshold=pitch_threshold, pitch_lag=pitch_lag, pitch_transition=pitch_transition,
                pitch_max_jump=pitch_max_jump)
            delay = self.plan.delay_frames
            self.analysis, self.viterbi = self.plan.states["loudness"], self.plan.viterbi_state
            if self.pitch_viterbi:  # the salience's ring; the per-frame pick reads the analysis's
                self.pitch_ring = self.plan.states["pitch"]
        self.loudness_delay_samples, self.pitch_delay_samples, self.mfcc_delay_samples = (
            delay.get(k, 0) * bs for k in ("loudness", "pitch", "mfcc"))
        if self.autoencoder:  # the encoder GRU's carried state is this object's: the model's state_dict stays as it is
            self.encoder_state = torch.zeros(1, 1, model.encoder.gru.hidden_size, device=device)
        self._inp_h = torch.zeros(2, N, 1).pin_memory()
        self._out_h = torch.zeros(1, N, 1).pin_memory()
        self.fused = bool(fused)
        if gru_route not in ("steps", "persistent"):
            raise ValueError("RealtimeGraph: gru_route must be 'steps' or 'persistent'")
        self.gru_route = gru_route  # the route requested; gru_route_taken: the one the graph holds
        self.gru_route_taken = None
        if self.fused:
            self._setup_fused()
        self.graph = torch.cuda.CUDAGraph()
        cache0 = model.decoder.cache_gru.detach().clone()
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.no_grad(), torch.cuda.stream(side):
            for _ in range(max(1, int(warmup))):  # library handles / workspaces before capture
                self._forward()
        torch.cuda.current_stream(device).wait_stream(side)
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.out = self._forward()
        torch.cuda.synchronize(device)
        self.reset()  # the warm-up and the capture ran the stream
        model.decoder.cache_gru.copy_(cache0)

    def refresh(self):
        """Rebuild the streamed reverb's IR spectra from the model's reverb parameters (in place: the
        captured graph reads the same buffer)."""
        if not self.reverb:
            raise RuntimeError("RealtimeGraph.refresh: the stream has no reverb")
        rv = self.model.reverb
        with torch.no_grad():
            imp = core.reverb_build_impulse(rv.noise.detach(), rv.decay.detach(), rv.wet.detach(), rv.sample_rate)
            self._spec.copy_(core.stream_spectrum(imp, self.call_samples))

    def _synthesis(self, f0, param, mags):
        """The call's synthesis: stateless (the counter-keyed fused kernel), or the stream's."""
        bs = self.block_size
        if not self.continuous:
            return core.synth_frames_counter(f0, param, mags, bs, self.sample_rate, self.counter, self.seed,
                                             bias=self.bias)
        out = core.stream_synth_frames(f0, param, mags, bs, self.sample_rate, self.stream, self.seed,
                                       bias=self.bias, wrap=self.wrap)
        if self.reverb:
            out = core.stream_reverb(out, self._spec, self.stream)
        core.stream_advance(self.stream, f0, bs, self.sample_rate, wrap=self.wrap)
        return out

    def _control_frames(self):
        """The call's pitch and loudness, one value per frame: (pitch, its stride, loudness, its stride) — the
        inputs decimated by block_size; with ``loudness_from_audio`` the loudness is the streamed analysis of the
        audio in the loudness buffer (stride 1); with ``pitch_from_audio`` both come from that audio, and the call's
        f0 and confidence stay in ``self.f0`` / ``self.confidence`` (the MFCC in ``self.mfcc``): ``self.plan``'s run."""
        if not self.loudness_from_audio:
            return self.pitch, self.block_size, self.loudness, self.block_size
        loud, self.mfcc, self.f0, self.confidence = self.plan.run(self.loudness)
        if not self.pitch_from_audio:
            return self.pitch, self.block_size, loud, 1
        return self.f0, 1, loud, 1

    @staticmethod
    def route_for(autoencoder=False, pitch_from_audio=False, pitch_viterbi=False):
        """The flags -> ``features.stream_analysis_route``'s (mfcc, pitch) of the graph's analysis."""
        if pitch_viterbi and not pitch_from_audio:
            raise RuntimeError("RealtimeGraph: pitch_viterbi=True decodes the pitch computed from the audio; it "
                               "needs pitch_from_audio=True")
        pitch = None if not pitch_from_audio else "viterbi" if pitch_viterbi else "fused"
        return "aligned" if autoencoder else None, pitch

    def _setup_fused(self):
        m, dev = self.model, self.device
        d = m.decoder
        if not core.gru_supported(d.gru):
            raise RuntimeError("RealtimeGraph(fused=True): GRU shape outside the step kernel's")
        for seq in (d.f0_mlp, d.loudness_mlp, d.out_mlp) + ((d.z_mlp,) if self.autoencoder else ()):
            if len(seq) != 9 or any(seq[i].negative_slope != 0.01 for i in (2, 5, 8)):
                raise RuntimeError("RealtimeGraph(fused=True): mlp(.., .., 3) blocks of core.py:122-129 expected")
        R = self.call_samples // self.block_size
        if R > 8:
            raise RuntimeError("RealtimeGraph(fused=True): at most 8 frames per call")
        Hd = d.gru.hidden_size
        z = lambda n: torch.zeros(R, n, device=dev)
        self._buf = {"y2f": z(Hd), "y2l": z(Hd), "y3f": z(Hd), "y3l": z(Hd), "xp": z(3 * Hd),
                     "gru": z(Hd), "y4": z(Hd), "y5": z(Hd), "y6": z(Hd),
                     "param": z(m.harmonic_proj.out_features), "mags": z(m.noise_proj.out_features),
                     "f0": z(1), "loud": z(1), "h_last": z(Hd)[:1]}
        if self.autoencoder:
            e = m.encoder
            if not core.gru_supported(e.gru):
                raise RuntimeError("RealtimeGraph(fused=True): the encoder's GRU shape is outside the step kernel's")
            He = e.gru.hidden_size
            self._buf.update({"xpe": z(3 * He), "gru_e": z(He), "z": z(e.proj.out_features), "y1z": z(Hd),
                              "y2z": z(Hd), "y3z": z(Hd)})
            self.z = self._buf["z"].view(1, R, -1)
        # the persistent recurrence's sync words (ddsp_hip_gru_forward_persistent), zeroed by the call itself
        self._gru_ws = torch.zeros(int(core._lib.query("gru_persistent_workspace_size")), dtype=torch.uint8,
                                   device=dev)

    def _forward_fused(self):
        """The same forward on ddsp_hip_dense_rows: decoder.py:43-68 + the projections
        (decoder.py:107-114) in 7 launches, the GRU on its step kernels (``gru_route="steps"``: R launches)
        or as one persistent launch (``"persistent"``: zeroing + persistent + rescue-check launches), then
        the synthesis."""
        m, d, bs, b = self.model, self.model.decoder, self.block_size, self._buf
        R, dev = self.call_samples // bs, self.device
        di = core.dense_input
        inv = 1.0 / self.std_loudness
        f0m, lm, om = d.f0_mlp, d.loudness_mlp, d.out_mlp
        pitch, pitch_ld, loud, loud_ld = self._control_frames()
        l2z, l3z, xpz = [], [], []
        if self.autoencoder:
            # the encoder (encoder.py:22-26) with a carried state: the GRU's input projection of norm(mfcc) (a
            # LayerNorm without activation), the recurrence on the step kernels writing h_T over the state, proj
            # -> z; then z_mlp's first Linear.  Its second and third blocks ride in f0_mlp's and loudness_mlp's
            # launches and its output is the third block of columns of the decoder GRU's input (decoder.py:31-49):
            # 3 launches + R steps more than the decoder alone
            e, zm = m.encoder, d.z_mlp
            ge = e.gru
            w_ie = _Linear(ge.weight_ih_l0, ge.bias_ih_l0, ge.input_size, 3 * ge.hidden_size)
            core.dense_rows([([di(self.mfcc.view(R, -1), norm=e.norm, activation=False)], w_ie, b["xpe"])], R, dev)
            core.gru_recurrence(b["xpe"].view(1, R, -1), ge.weight_hh_l0, ge.bias_hh_l0, self.encoder_state,
                                b["gru_e"].view(1, R, -1), self.encoder_state, persistent=False)
            core.dense_rows([([di(b["gru_e"])], e.proj, b["z"])], R, dev)
            core.dense_rows([([di(b["z"])], zm[0], b["y1z"])], R, dev)
            l2z = [([di(b["y1z"], norm=zm[1])], zm[3], b["y2z"])]
            l3z = [([di(b["y2z"], norm=zm[4])], zm[6], b["y3z"])]
            xpz = [di(b["y3z"], norm=zm[7])]
        core.dense_rows([  # mlp layers 1-2 (core.py:122-129), f0 and loudness
            ([di(pitch, ld=pitch_ld, first=f0m[0], norm=f0m[1], x_copy=b["f0"])], f0m[3], b["y2f"]),
            ([di(loud, ld=loud_ld, scale=inv, shift=-self.mean_loudness * inv, first=lm[0], norm=lm[1],
                 x_copy=b["loud"])], lm[3], b["y2l"])] + l2z, R, dev)
        core.dense_rows([([di(b["y2f"], norm=f0m[4])], f0m[6], b["y3f"]),
                         ([di(b["y2l"], norm=lm[4])], lm[6], b["y3l"])] + l3z, R, dev)
        # GRU input projection of cat([f0_mlp(f0), loudness_mlp(loudness)[, z_mlp(z)]]) (decoder.py:49)
        g = d.gru
        w_ih = _Linear(g.weight_ih_l0, g.bias_ih_l0, g.input_size, 3 * g.hidden_size)
        core.dense_rows([([di(b["y3f"], norm=f0m[7]), di(b["y3l"], norm=lm[7])] + xpz, w_ih, b["xp"])], R, dev)
        # the state in place: the step kernels write h_T over h0; the persistent launch, whose rescue re-reads h0,
        # into a buffer of its own, copied over the state after it.  The workspace is this object's: the graph holds it
        cache = d.cache_gru
        self.gru_route_taken = core.gru_recurrence(
            b["xp"].view(1, R, -1), g.weight_hh_l0, g.bias_hh_l0, cache, b["gru"].view(1, R, -1), b["h_last"],
            ws=self._gru_ws, persistent=self.gru_route == "persistent", h_last_steps=cache)
        if self.gru_route_taken == "persistent":
            cache.view(1, -1).copy_(b["h_last"])
        # out_mlp(cat([gru_out, f0, loudness])) (decoder.py:68), then the projections
        core.dense_rows([([di(b["gru"]), di(b["f0"]), di(b["loud"])], om[0], b["y4"])], R, dev)
        core.dense_rows([([di(b["y4"], norm=om[1])], om[3], b["y5"])], R, dev)
        core.dense_rows([([di(b["y5"], norm=om[4])], om[6], b["y6"])], R, dev)
        core.dense_rows([([di(b["y6"], norm=om[7])], m.harmonic_proj, b["param"]),
                         ([di(b["y6"], norm=om[7])], m.noise_proj, b["mags"])], R, dev)
        return self._synthesis(b["f0"].view(1, R, 1), b["param"].view(1, R, -1), b["mags"].view(1, R, -1))

    def _forward(self):
        """export.py:33-40 realtime ScriptDDSP.forward with the model's synthesis fused."""
        if self.fused:
            return self._forward_fused()
        m, bs = self.model, self.block_size
        pitch, pitch_ld, loud, loud_ld = self._control_frames()
        pitch = pitch.view(1, -1, 1)[:, ::pitch_ld]
        loudness = (loud.view(1, -1, 1)[:, ::loud_ld] - self.mean_loudness) / self.std_loudness
        z = None
        if self.autoencoder:  # encoder.py:22-26 with the GRU state carried in self.encoder_state
            e = m.encoder
            x, h = core.gru(e.norm(self.mfcc), e.gru, self.encoder_state)
            self.encoder_state.copy_(h)
            z = self.z = e.proj(x)
        hidden = gru_decoder_forward(m.decoder, pitch, loudness, z, realtime=True)
        param = m.harmonic_proj(hidden)
        mags = m.noise_proj(hidden)
        return self._synthesis(pitch.contiguous(), param, mags)

    def reset(self):
        self.model.decoder.cache_gru.zero_()
        if self.encoder_state is not None:
            self.encoder_state.zero_()
        self.counter.zero_()
        if self.stream is not None:
            self.stream.reset()
        if self.plan is not None:
            self.plan.reset()

    @torch.no_grad()
    def __call__(self, pitch, loudness=None):
        """pitch, loudness [1, N, 1] on the host (returns a host tensor) or on the device (returns
        the device output buffer).  With ``loudness_from_audio`` the second input is the call's audio; with
        ``pitch_from_audio`` the call's audio is the only input."""
        if self.pitch_from_audio:
            return self._call_audio(pitch, loudness)
        if loudness is None:
            raise RuntimeError("RealtimeGraph: two inputs expected, pitch and loudness (one, the audio, only with "
                               "pitch_from_audio=True)")
        if tuple(pitch.shape) != (1, self.call_samples, 1) or tuple(loudness.shape) != tuple(pitch.shape):
            raise RuntimeError(f"RealtimeGraph: pitch and loudness must be [1, {self.call_samples}, 1]")
        stream = torch.cuda.current_stream(self.device)
        if pitch.is_cuda:
            self.pitch.copy_(pitch)
            self.loudness.copy_(loudness)
            self.graph.replay()
            return self.out
        self._inp_h[0:1].copy_(pitch)
        self._inp_h[1:2].copy_(loudness)
        self._inp.copy_(self._inp_h, non_blocking=True)
        self.graph.replay()
        self._out_h.copy_(self.out, non_blocking=True)
        stream.synchronize()
        return self._out_h

    def _call_audio(self, audio, extra):
        """``pitch_from_audio``: the call's audio [1, N, 1] in (N floats, not 2 N), audio out."""
        if extra is not None:
            raise RuntimeError("RealtimeGraph(pitch_from_audio=True) takes one input, the call's audio; the pitch "
                               "is computed from it")
        if tuple(audio.shape) != (1, self.call_samples, 1):
            raise RuntimeError(f"RealtimeGraph: audio must be [1, {self.call_samples}, 1]")
        if audio.is_cuda:
            self.loudness.copy_(audio)
            self.graph.replay()
            return self.out
        stream = torch.cuda.current_stream(self.device)
        self._inp_h[1:2].copy_(audio)
        self.loudness.copy_(self._inp_h[1:2], non_blocking=True)
        self.graph.replay()
        self._out_h.copy_(self.out, non_blocking=True)
        stream.synchronize()
        return self._out_h
