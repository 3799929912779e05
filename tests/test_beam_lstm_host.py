"""CPU: the beam search's host loop with an rnnt_amd.LSTMPredictor (rnnt_amd/stream.py HostBeamLoop; DESIGN.md §4h "LSTM") in float64
against tests/beam_oracle.beam_search over the same modules (tests/beam_lstm_oracle.py): identical lists, scores within 1e-9.  The host
loop and the oracle share the modules' float64 arithmetic, so the lists are equal whatever the gap; the premises that keep the test
honest — two lengths, an entry of 3 labels — are asserted."""
import pytest
import torch

from tests import beam_lstm_oracle as bo
from tests import context_oracle as co
from tests import lstm_decode_cases as dc
from tests import lstm_predictor_cases as lc


def _lens(mel):
    return torch.tensor([mel.shape[-1]])


def _search(model, mel, **kw):
    out = model.beam_search(mel, _lens(mel), return_nbest=True, **kw)
    assert model.last_beam_path == "host"
    return out


# with and without text_ln, a blank other than V - 1
CONFIGS = [(name, beam) for name in ("wiring", "wiring_text", "blank_5") for beam in (2, 4, 16)]


@pytest.mark.parametrize("name,beam", CONFIGS, ids=[f"{n}-{b}" for n, b in CONFIGS])
def test_host_loop_gives_the_oracle_lists(name, beam):
    T, seed = bo.SEEDS[(name, beam)]
    want = bo.checked(name, T, seed, beam)
    model, mel = bo.model_of(name), bo.mel_of(name, T, seed)
    assert model.last_beam_path in (None, "host")
    got = _search(model, mel, beam_size=beam)
    bo.assert_matches(got, want, (name, beam), score_tol=1e-9)
    assert model.beam_search(mel, _lens(mel), beam_size=beam) == want[0][0]


@pytest.mark.parametrize("key", list(bo.CAPS), ids=[f"{k[0]}-beam{k[1]}-ml{k[2]}-m{k[3]}" for k in bo.CAPS])
def test_host_loop_under_the_caps(key):
    name, beam, ml, m = key
    T, seed = bo.CAPS[key]
    want = bo.checked(name, T, seed, beam, ml, m)
    got = _search(bo.model_of(name), bo.mel_of(name, T, seed), beam_size=beam, max_length=ml, max_symbols_per_frame=m)
    bo.assert_matches(got, want, key, score_tol=1e-9)
    assert max(len(y) for y, _ in got) <= ml - 1


@pytest.mark.parametrize("name", ["wiring", "wiring_text", "blank_5"])
def test_beam_1_is_the_greedy_decode(name):
    model = bo.model_of(name)
    mel = lc.decode_frames() if name == "wiring" else dc.case_frames(dc.BY_NAME[name])
    o = dc.greedy_oracle(model, mel, 200)
    assert o.gap > dc.MARGIN and len(o.tokens) >= 4
    assert model.beam_search(mel, _lens(mel), beam_size=1) == o.tokens == model.greedy_decode(mel, _lens(mel))
    want, _, _ = bo.beam_oracle.beam_search(bo.Model(model, mel), 1, 200)
    bo.assert_matches(_search(model, mel, beam_size=1), want, name, score_tol=1e-9)


def test_beam_search_many_is_beam_search_per_entry():
    model = bo.model_of("wiring")
    mels = [bo.mel_of("wiring", T, seed) for T, seed in ((6, 22), (1, 3), (10, 80), (3, 5))]
    assert model.beam_search_many([]) == []
    for kw in (dict(beam_size=4), dict(beam_size=20, max_length=4), dict(beam_size=3, max_symbols_per_frame=2)):
        many = model.beam_search_many(mels, return_nbest=True, batch=3, **kw)
        assert model.last_beam_path == "host"
        assert many == [_search(model, mel, **kw) for mel in mels]  # tokens and Python floats
        assert model.beam_search_many(mels, **kw) == [nb[0][0] for nb in many]
    with pytest.raises(ValueError):
        model.beam_search_many(mels, batch=33)  # the LSTM search's limit, not the ConvPredictor search's 64
    with pytest.raises(ValueError):
        model.beam_search_many(mels, batch=0)
    with pytest.raises(ValueError):
        model.beam_search(mels[0], _lens(mels[0]), beam_size=0)


@pytest.mark.parametrize("chunks", [[1] * 10, [3, 0, 1, 4, 2], [0, 10, 0], [7, 3]], ids=["ones", "uneven", "all_at_once", "two"])
def test_stream_equals_the_search_of_the_frames_so_far(chunks):
    """Any chunking: after every push the stream shows beam_search of the frames pushed so far (tokens and Python floats).  A push that
    ends on capped labels prunes the cache to the carried beam; the next push finds every parent's state there."""
    model = bo.model_of("wiring")
    mel = bo.mel_of("wiring", 10, 80)
    assert sum(chunks) == mel.shape[-1]
    for kw in (dict(beam_size=4), dict(beam_size=4, max_symbols_per_frame=1), dict(beam_size=16, max_length=4)):
        stream = model.beam_stream(**kw)
        at = 0
        for k in chunks:
            stream.push_encoded(mel[..., at:at + k])
            at += k
            want = _search(model, mel[..., :at], **kw) if at else [([], 0.0)]
            assert stream.nbest == want and stream.frames == at, (kw, at)
            assert stream.last_path in (None, "host")
        assert stream.last_path == "host"
        # every text vector and state the loop keeps belongs to the carried beam
        loop = stream._group._loops[0]
        assert set(loop._feats) == {tuple(y) for y, _ in stream.nbest}
    group = model.beam_streams(2, beam_size=4)
    group.push_encoded([mel[..., :4], None])
    group.push_encoded([mel[..., 4:], mel[..., :6]])
    assert group.nbest[0] == _search(model, mel, beam_size=4) and group.nbest[1] == _search(model, mel[..., :6], beam_size=4)
    assert group.last_path == "host"


def test_capped_labels_are_carried_over_a_push():
    """max_symbols_per_frame = 1: every kept label is capped, so each frame's beam holds hypotheses that have not taken their step."""
    model = bo.model_of("wiring")
    mel = bo.mel_of("wiring", 6, 22)
    want = _search(model, mel, beam_size=4, max_symbols_per_frame=1)
    assert max(len(y) for y, _ in want) >= 3
    stream = model.beam_stream(beam_size=4, max_symbols_per_frame=1)
    for t in range(mel.shape[-1]):
        stream.push_encoded(mel[..., t:t + 1])
    assert stream.nbest == want


def test_context_graph_runs_the_host_loop_and_matches_its_oracle():
    """tests/context_oracle.beam_search takes the same model object as beam_oracle's: the biased search against its own oracle, and the
    graphs that cannot change a search against the plain one."""
    from rnnt_amd import ContextGraph
    model = bo.model_of("wiring")
    T, seed = bo.SEEDS[("wiring", 4)]
    mel = bo.mel_of("wiring", T, seed)
    plain = bo.checked("wiring", T, seed, 4)
    for g in (None, ContextGraph([], 2.0), ContextGraph([(1, 2)], 0.0)):
        bo.assert_matches(_search(model, mel, beam_size=4, context=g), plain, "inactive graph", score_tol=1e-9)
    phrases = [tuple(plain[-1][0][:2]), (3, 1, 4)]  # the first labels of the WORST entry of the plain list, and a phrase off the beam
    assert len(phrases[0]) == 2
    want = co.beam_search(bo.Model(model, mel), 4, 200, graph=co.Trie(phrases, 1.5))
    g = ContextGraph(phrases, 1.5)
    got = _search(model, mel, beam_size=4, context=g)
    bo.assert_matches(got, want.nbest, "context", score_tol=1e-9)
    assert want.events["touched"] > 0 and [y for y, _ in got] != [y for y, _ in plain]
    assert model.beam_search_many([mel], beam_size=4, context=g, return_nbest=True) == [got]
    stream = model.beam_stream(beam_size=4, context=g)
    stream.push_encoded(mel[..., :2])
    stream.push_encoded(mel[..., 2:])
    assert stream.nbest == got


def test_other_stateful_predictors_are_still_refused():
    import rnnt_amd
    from tests.stream_models import LSTMLikePredictor, PassThroughEncoder
    model = bo.model_of("wiring")
    other = rnnt_amd.RNNTModel(LSTMLikePredictor(16, 32, 16, seed=3), PassThroughEncoder(), model.joint).eval()
    mel = bo.mel_of("wiring", 3, 1)
    for call in (lambda: other.beam_search(mel, _lens(mel)), lambda: other.beam_search_many([mel]), other.beam_stream,
                 lambda: other.beam_streams(2)):
        with pytest.raises(NotImplementedError, match="stateful"):
            call()
