"""features.stream_analysis_route: which core calls one call of a stream makes over which rings, and how
StreamAnalyzer's and RealtimeGraph's flags map onto it — plain host logic, checked without a device."""
import itertools

import pytest

from ddsp_pytorch_amd.features import StreamAnalyzer, stream_analysis_route
from ddsp_pytorch_amd.realtime import RealtimeGraph

SAL, VIT = "stream_pitch_salience", "stream_viterbi_path"
LOUD, MFCC, PITCH = "stream_loudness", "stream_mfcc", "stream_pitch"
AN, ANM = "stream_analysis", "stream_analysis_mfcc"

# (mfcc, pitch) -> (calls in order, the ring each feature reads, decode state); stream_analysis_mfcc runs with
# pitch=True exactly when the pitch reads "main"
TABLE = {
    (None, None): ((LOUD,), {"loudness": "main"}, False),
    (None, "own"): ((LOUD, PITCH), {"loudness": "main", "pitch": "pitch"}, False),
    (None, "fused"): ((AN,), {"loudness": "main", "pitch": "main"}, False),
    (None, "viterbi"): ((SAL, VIT, LOUD), {"loudness": "main", "pitch": "pitch"}, True),
    ("own", None): ((LOUD, MFCC), {"loudness": "main", "mfcc": "mfcc"}, False),
    ("own", "own"): ((LOUD, MFCC, PITCH), {"loudness": "main", "mfcc": "mfcc", "pitch": "pitch"}, False),
    ("own", "fused"): ((AN, MFCC), {"loudness": "main", "mfcc": "mfcc", "pitch": "main"}, False),
    ("own", "viterbi"): ((SAL, VIT, LOUD, MFCC), {"loudness": "main", "mfcc": "mfcc", "pitch": "pitch"}, True),
    ("aligned", None): ((ANM,), {"loudness": "main", "mfcc": "main"}, False),
    ("aligned", "fused"): ((ANM,), {"loudness": "main", "mfcc": "main", "pitch": "main"}, False),
    ("aligned", "viterbi"): ((SAL, VIT, ANM), {"loudness": "main", "mfcc": "main", "pitch": "pitch"}, True),
}
# the distinct rings of the issue's table, per route
RINGS = {
    (None, None): {"main"}, (None, "own"): {"main", "pitch"}, (None, "fused"): {"main"},
    (None, "viterbi"): {"main", "pitch"}, ("own", None): {"main", "mfcc"}, ("own", "own"): {"main", "mfcc", "pitch"},
    ("own", "fused"): {"main", "mfcc"}, ("own", "viterbi"): {"main", "mfcc", "pitch"}, ("aligned", None): {"main"},
    ("aligned", "fused"): {"main"}, ("aligned", "viterbi"): {"main", "pitch"},
}


@pytest.mark.parametrize("mfcc,pitch", list(TABLE))
def test_route_table(mfcc, pitch):
    calls, rings, decode = TABLE[(mfcc, pitch)]
    route = stream_analysis_route(mfcc, pitch)
    assert (route.mfcc, route.pitch) == (mfcc, pitch)
    assert route.calls == calls
    assert dict(route.rings) == rings and len(route.rings) == len(rings)
    assert set(dict(route.rings).values()) == RINGS[(mfcc, pitch)]
    assert route.decode is decode
    with pytest.raises((AttributeError, TypeError)):  # immutable
        route.calls = ()
    with pytest.raises(TypeError):
        route.rings[0] = ("loudness", "pitch")


def test_route_refusals():
    assert len(TABLE) == 11 and len(RINGS) == 11
    with pytest.raises(ValueError, match="aligned"):
        stream_analysis_route("aligned", "own")
    for mfcc, pitch in (("fused", None), (None, "aligned"), (True, None), (None, True)):
        with pytest.raises(ValueError, match="no such route"):
            stream_analysis_route(mfcc, pitch)


def test_stream_analyzer_flags_to_route():
    accepted = {}
    for pitch, fused, aligned, viterbi in itertools.product((False, True), repeat=4):
        flags = dict(pitch=pitch, fused=fused, aligned=aligned, viterbi=viterbi)
        if (fused or viterbi) and not pitch:
            with pytest.raises(ValueError, match="needs pitch=True"):
                StreamAnalyzer.route_for(**flags)
        elif fused and viterbi:
            with pytest.raises(ValueError, match="viterbi=True takes the pitch"):
                StreamAnalyzer.route_for(**flags)
        else:
            accepted[(pitch, fused, aligned, viterbi)] = StreamAnalyzer.route_for(**flags)
    assert accepted == {
        (False, False, False, False): ("own", None),
        (False, False, True, False): ("aligned", None),
        (True, False, False, False): ("own", "own"),
        (True, False, False, True): ("own", "viterbi"),
        (True, False, True, False): ("aligned", "fused"),
        (True, False, True, True): ("aligned", "viterbi"),
        (True, True, False, False): ("own", "fused"),
        (True, True, True, False): ("aligned", "fused"),
    }
    for pair in accepted.values():  # every one of them is a route of the table
        assert pair in TABLE
    assert StreamAnalyzer.route_for() == ("own", None)


def test_realtime_graph_flags_to_route():
    got = {}
    for autoencoder, pitch_from_audio, pitch_viterbi in itertools.product((False, True), repeat=3):
        if pitch_viterbi and not pitch_from_audio:
            with pytest.raises(RuntimeError, match="needs pitch_from_audio=True"):
                RealtimeGraph.route_for(autoencoder, pitch_from_audio, pitch_viterbi)
        else:
            got[(autoencoder, pitch_from_audio, pitch_viterbi)] = RealtimeGraph.route_for(
                autoencoder, pitch_from_audio, pitch_viterbi)
    assert got == {
        (False, False, False): (None, None),
        (False, True, False): (None, "fused"),
        (False, True, True): (None, "viterbi"),
        (True, False, False): ("aligned", None),
        (True, True, False): ("aligned", "fused"),
        (True, True, True): ("aligned", "viterbi"),
    }
    for pair in got.values():
        assert pair in TABLE
