"""CPU: contextual biasing in the host loop (rnnt_amd/stream.py HostBeamLoop; DESIGN.md §4h "Context") — beam_search(context=g) held to the
float64 oracle (tests/context_oracle.py) on the configurations the device is held to, a beam_stream(context=g) in any chunking against
the offline search, and the arguments a model method refuses."""
import numpy as np
import pytest
import torch

from rnnt_amd import ContextGraph
from tests import context_oracle as co
from tests.helpers import load_decode_case
from tests.stream_models import cpu_model, partitions

_cases = {}


def _case(golden_dir, name):
    if name not in _cases:
        c = load_decode_case(golden_dir, name)
        _cases[name] = (c, cpu_model(c["spec"], c["pred_sd"], c["joint_sd"]), torch.from_numpy(np.ascontiguousarray(c["frames"].T))[None])
    return _cases[name]


def _search(model, mel, **kw):
    return model.beam_search(mel, torch.tensor([mel.shape[-1]]), return_nbest=True, **kw)


@pytest.mark.parametrize("name,ml,key,score,beams", co.CONFIGS, ids=[f"{c[2]}-{c[3]}" for c in co.CONFIGS])
def test_host_loop_matches_the_oracle(golden_dir, name, ml, key, score, beams):
    """The bar of tests/test_beam_oracle.py: identical finalised lists, scores within 1e-4 * max(1, |score|), where the oracle's gap is
    above GAP.  The host loop takes a per-slot top-`beam` of the BIASED row: the `outside` candidates (raw rank >= beam) are its test."""
    c, model, mel = _case(golden_dir, name)
    g = ContextGraph(co.PHRASES[key], score)
    for beam in beams:
        want = co.result(golden_dir, name, ml, key, score, beam)
        print(f"{name} {key} score {score} beam {beam}: gap {want.gap:.3e} {want.events}")
        assert want.gap > co.GAP, (name, key, score, beam, want.gap)
        got = _search(model, mel, beam_size=beam, max_length=ml, context=g)
        assert [y for y, _ in got] == [y for y, _ in want.nbest], (name, key, score, beam)
        for (_, gs), (_, ws) in zip(got, want.nbest):
            assert abs(gs - ws) <= 1e-4 * max(1.0, abs(ws)), (name, beam, gs, ws)
        assert model.beam_search(mel, torch.tensor([mel.shape[-1]]), beam_size=beam, max_length=ml, context=g) == want.nbest[0][0]
        assert got[0][0] != _search(model, mel, beam_size=beam, max_length=ml)[0][0]  # the graph changed the best hypothesis


def test_a_graph_that_cannot_act_is_the_plain_search_exactly(golden_dir):
    for name, ml in (("decode_small", 60), ("decode_cap", 37)):
        c, model, mel = _case(golden_dir, name)
        for beam in (1, 4, 20):
            plain = _search(model, mel, beam_size=beam, max_length=ml)
            for g in (None, ContextGraph([], 2.0), ContextGraph(co.PHRASES[name], 0.0)):
                assert _search(model, mel, beam_size=beam, max_length=ml, context=g) == plain  # tokens and Python floats
    # beam 1 without a graph is still the reference's greedy decode; with one it is not
    c, model, mel = _case(golden_dir, "decode_small")
    g = ContextGraph(co.PHRASES["decode_small"], 1.5)
    assert _search(model, mel, beam_size=1, max_length=60)[0][0] == c["tokens"][60]
    assert _search(model, mel, beam_size=1, max_length=60, context=g)[0][0] != c["tokens"][60]


@pytest.mark.parametrize("name,ml,score,beam", [("decode_small", 60, 1.5, 4), ("decode_cap", 37, 3.0, 2), ("decode_cap", 37, 1.5, 20)])
def test_any_chunking_of_a_stream_equals_the_offline_search(golden_dir, name, ml, score, beam):
    """The carried beam is internal, `nbest` / `tokens` / `stable` are finalised views: after every push — empty ones included — the stream
    shows beam_search(context=g) of the frames so far."""
    c, model, mel = _case(golden_dir, name)
    g = ContextGraph(co.PHRASES[name], score)
    T = mel.shape[-1]
    offline = {0: [([], 0.0)]}

    def want(k):
        if k not in offline:
            offline[k] = _search(model, mel[..., :k], beam_size=beam, max_length=ml, context=g)
        return offline[k]

    assert model.beam_stream(beam_size=beam, max_length=ml, context=g).nbest == [([], 0.0)]
    parts = partitions(T, seed=3)
    assert any(0 in sizes for sizes in parts.values())  # empty pushes are part of the test
    for pname in ("7", "all", "random"):
        s = model.beam_stream(beam_size=beam, max_length=ml, context=g)
        t = 0
        for k in parts[pname]:
            best = s.push_encoded(mel[..., t:t + k])
            t += k
            assert s.nbest == want(t), (name, pname, t)  # the same lists, the same Python floats
            assert best == s.tokens == want(t)[0][0] and s.frames == t
            assert all(y[:len(s.stable)] == s.stable for y, _ in s.nbest)
            if t:
                assert s.last_path == "host"
        assert t == T
    grp = model.beam_streams(2, beam_size=beam, max_length=ml, context=g)
    grp.push_encoded([mel[..., :9], None])
    grp.push_encoded([mel[..., 9:20], mel[..., :5]])
    assert grp.nbest == [want(20), want(5)]
    grp.reset(0)
    grp.push_encoded([mel[..., :5], None])
    assert grp.nbest == [want(5), want(5)]


def test_model_methods_refuse_bad_graphs(golden_dir):
    c, model, mel = _case(golden_dir, "decode_small")
    V = c["spec"]["V"]
    lens = torch.tensor([mel.shape[-1]])
    for bad in (ContextGraph([(1, V)], 1.0), ContextGraph([(V - 1, 2)], 1.0), ContextGraph([(V + 5,)], 0.0)):  # outside / blank / inactive too
        with pytest.raises(ValueError):
            model.beam_search(mel, lens, context=bad)
        with pytest.raises(ValueError):
            model.beam_search_many([mel], context=bad)
        with pytest.raises(ValueError):
            model.beam_stream(context=bad)
        with pytest.raises(ValueError):
            model.beam_streams(2, context=bad)
    with pytest.raises(TypeError):
        model.beam_search(mel, lens, context=[(1, 2)])
    g = ContextGraph(co.PHRASES["decode_small"], 1.5)
    many = model.beam_search_many([mel, mel[..., :20]], beam_size=3, max_length=60, return_nbest=True, context=g)
    assert many == [_search(model, m, beam_size=3, max_length=60, context=g) for m in (mel, mel[..., :20])]
