"""-m gpu: contextual biasing on the device (rnnt_engine_beam_decode_ctx / _batch_ctx; DESIGN.md §4h "Context") against (1) the float64
oracle of the biased search (tests/context_oracle.py), at the bar of tests/test_beam_gpu.py and only where the oracle's gap is above GAP,
(2) the plain search, exactly, wherever the graph cannot act, (3) itself: batched against single, run against run."""
import numpy as np
import pytest
import torch

import rnnt_amd
from rnnt_amd import ContextGraph
from tests import context_oracle as co
from tests.helpers import load_decode_case
from tests.test_beam_batch_gpu import utterances
from tests.test_beam_gpu import _lens, _mel
from tests.test_decode_gpu import build_model

pytestmark = pytest.mark.gpu

_cases = {}


def _case(golden_dir, name):
    if name not in _cases:
        c = load_decode_case(golden_dir, name)
        _cases[name] = (c, build_model(c["spec"], c["pred_sd"], c["joint_sd"]))
    return _cases[name]


def _search(model, mel, **kw):
    return model.beam_search(mel, _lens(mel), return_nbest=True, **kw)


@pytest.mark.parametrize("name,ml,key,score,beams", co.CONFIGS, ids=[f"{c[2]}-{c[3]}" for c in co.CONFIGS])
def test_device_matches_the_oracle(golden_dir, name, ml, key, score, beams):
    """Identical finalised token lists, scores within 1e-4 * max(1, |score|), where the oracle's gap is above GAP (asserted).  beam 1 is
    among the beams: with a graph it is NOT the greedy decode any more, it is the oracle's beam 1."""
    c, model = _case(golden_dir, name)
    mel = _mel(c["frames"])
    g = ContextGraph(co.PHRASES[key], score)
    for beam in beams:
        want = co.result(golden_dir, name, ml, key, score, beam)
        print(f"{name} {key} score {score} beam {beam}: oracle gap {want.gap:.3e} pruned {want.pruned} {want.events}")
        assert want.gap > co.GAP, (name, key, score, beam, want.gap)
        assert model._beam_device_ok(mel.permute(0, 2, 1), beam, ml, g)
        got = _search(model, mel, beam_size=beam, max_length=ml, context=g)
        assert [y for y, _ in got] == [y for y, _ in want.nbest], (name, key, score, beam)
        for (_, gs), (_, ws) in zip(got, want.nbest):
            assert abs(gs - ws) <= 1e-4 * max(1.0, abs(ws)), (name, key, score, beam, gs, ws)
        assert model.beam_search(mel, _lens(mel), beam_size=beam, max_length=ml, context=g) == want.nbest[0][0]
        assert got[0][0] != _search(model, mel, beam_size=beam, max_length=ml)[0][0]  # the best hypothesis is not the unbiased one


def test_the_configurations_exercise_every_event(golden_dir):
    """Summed over the configurations above (the oracle's results are shared with them): kept label candidates from OUTSIDE the raw
    top-`beam` of their row, with a cancelled bonus, landed through a fail link, and banked."""
    total = dict.fromkeys(co.EVENTS, 0)
    for name, ml, key, score, beams in co.CONFIGS:
        for beam in beams:
            for k, v in co.result(golden_dir, name, ml, key, score, beam).events.items():
                if k in total:
                    total[k] += v
    print(total)
    assert all(v > 0 for v in total.values()), total


def test_beam1_with_a_graph_is_the_oracles_beam1_not_the_greedy_decode(golden_dir):
    c, model = _case(golden_dir, "decode_small")
    mel = _mel(c["frames"])
    g = ContextGraph(co.PHRASES["decode_small"], 1.5)
    want = co.result(golden_dir, "decode_small", 60, "decode_small", 1.5, 1)
    assert want.gap > co.GAP
    got = model.beam_search(mel, _lens(mel), beam_size=1, max_length=60, context=g)
    assert got == want.nbest[0][0] and got != c["tokens"][60]
    assert model.beam_search(mel, _lens(mel), beam_size=1, max_length=60) == c["tokens"][60]  # without one it still is


@pytest.mark.parametrize("name,ml", [("decode_small", 60), ("decode_cap", 37)])
def test_a_graph_that_cannot_act_is_the_plain_search_exactly(golden_dir, name, ml):
    c, model = _case(golden_dir, name)
    utts = utterances(c["frames"])
    mel, mels = _mel(c["frames"]), [_mel(u) for u in utts[:5]]
    for beam in (1, 4, 16):
        plain = _search(model, mel, beam_size=beam, max_length=ml)
        plain_many = model.beam_search_many(mels, beam_size=beam, max_length=ml, return_nbest=True)
        for g in (None, ContextGraph([], 2.0), ContextGraph(co.PHRASES[name], 0.0)):
            assert _search(model, mel, beam_size=beam, max_length=ml, context=g) == plain, (name, beam)  # tokens and float64 scores
            assert model.beam_search_many(mels, beam_size=beam, max_length=ml, return_nbest=True, context=g) == plain_many, (name, beam)


def _raw(model, mel, beam, ml, tables):
    """engine.beam_decode as RNNTModel._beam_search_device calls it, with the graph's tables given directly: [(tokens, INTERNAL score)]"""
    frames = mel[0].T.float().contiguous()
    p = model.predictor
    state, tokens, scores = rnnt_amd.engine.beam_decode(
        frames, p._params(), (float(p.input_layer_norm.eps), float(p.output_layer_norm.eps)), None, None, model.joint.joint_ln.weight,
        model.joint.joint_ln.bias, model.joint.blank_idx, ml, beam, context=tables)
    st, toks, sc = state.tolist(), tokens.tolist(), scores.tolist()
    assert st[3] == 1 and 1 <= st[2] <= beam
    return [(toks[j][1:1 + st[8 + j]], sc[j]) for j in range(st[2])]


@pytest.mark.parametrize("name,ml", [("decode_small", 60), ("decode_cap", 37)])
def test_graphs_that_never_match_give_the_plain_result_through_the_context_kernels(golden_dir, name, ml):
    """A 1-node graph (RNNTModel would not even take the context path for it: the engine is called directly) and a graph whose only phrase
    never matches — per the oracle no kept candidate ever has a delta — run k_beam_reduce / k_beam_select in their context form and must
    return the plain search's lists and scores, exactly."""
    c, model = _case(golden_dir, name)
    assert not hasattr(model.joint, "text_ln") and not hasattr(model.joint, "audio_ln")
    mel = _mel(c["frames"])
    dev = mel.device
    never = ContextGraph([(24, 24)], 1.5)
    for beam in (4, 16):
        plain = _search(model, mel, beam_size=beam, max_length=ml)
        assert _raw(model, mel, beam, ml, None) == plain
        assert _raw(model, mel, beam, ml, ContextGraph([], 1.5).device_tables(dev)) == plain, (name, beam)
        om = co.result(golden_dir, name, ml, None, 0.0, beam)  # (the Model of the case)
        r = co.beam_search(co._models[name], beam, ml, graph=co.Trie([(24, 24)], 1.5))
        assert r.events["touched"] == 0 and r.gap > co.GAP and r.nbest == om.nbest
        assert never.active and _raw(model, mel, beam, ml, never.device_tables(dev)) == plain, (name, beam)
        assert _search(model, mel, beam_size=beam, max_length=ml, context=never) == plain


@pytest.mark.parametrize("beam", [4, 16])
@pytest.mark.parametrize("name,ml,score", [("decode_small", 60, 1.5), ("decode_cap", 37, 3.0)])
def test_batch_equals_the_single_search_exactly(golden_dir, name, ml, score, beam):
    """The 12 windows of tests/test_beam_batch_gpu.utterances (1-frame utterances among them), ONE graph for the batch: every entry is
    beam_search(context=g) of that utterance — tokens and float64 scores with == — whatever the batch size and the order."""
    c, model = _case(golden_dir, name)
    mels = [_mel(u) for u in utterances(c["frames"])]
    assert min(m.shape[-1] for m in mels) == 1
    g = ContextGraph(co.PHRASES[name], score)
    kw = dict(beam_size=beam, max_length=ml, return_nbest=True, context=g)
    single = [_search(model, m, beam_size=beam, max_length=ml, context=g) for m in mels]
    plain = model.beam_search_many(mels, beam_size=beam, max_length=ml, return_nbest=True)
    assert sum(a != b for a, b in zip(single, plain)) >= 3  # the graph acts on these utterances
    assert model.beam_search_many(mels, **kw) == single
    assert model.beam_search_many(mels, batch=5, **kw) == single  # 5 + 5 + 2
    assert model.beam_search_many(mels, batch=1, **kw) == single
    order = [7, 0, 11, 3, 3, 9, 0, 4]
    assert model.beam_search_many([mels[i] for i in order], **kw) == [single[i] for i in order]
    assert model.beam_search_many(mels[::-1], batch=7, **kw) == single[::-1]
    assert model.beam_search_many(mels, beam_size=beam, max_length=ml, context=g) == [s[0][0] for s in single]


def test_nan_workspace_and_repeat_runs_are_bit_identical(golden_dir):
    c, model = _case(golden_dir, "decode_small_proj")
    mel = _mel(c["frames"])
    mels = [_mel(u) for u in utterances(c["frames"])]
    g = ContextGraph(co.PHRASES["decode_small_proj"], 3.0)
    kw = dict(beam_size=8, max_length=60, context=g)
    many = lambda: model.beam_search_many(mels, return_nbest=True, **kw)  # noqa: E731
    a, am = _search(model, mel, **kw), many()
    assert _search(model, mel, **kw) == a and many() == am  # tokens and float64 scores, exactly
    assert a != _search(model, mel, beam_size=8, max_length=60)  # (the graph acts here)
    dev = torch.device("cuda", torch.cuda.current_device())
    for fn, want in ((lambda: _search(model, mel, **kw), a), (many, am)):
        ws = rnnt_amd.engine.workspace(dev, 1)  # the stream's cached scratch buffer the call will reuse
        ws.fill_(255)  # every float / double in it is a NaN, every node and counter garbage
        torch.cuda.synchronize()
        assert fn() == want


def test_malformed_tables_stay_in_bounds_and_terminate(golden_dir):
    """The tables are device memory the C layer cannot check: node indices out of range, fail links that loop, child ranges beyond the
    arrays, unsorted children, absurd depths.  The result may be wrong; the search must end, with at most `beam` entries of in-range
    labels (every index is clamped, the fail walk and the bisection are counted loops)."""
    c, model = _case(golden_dir, "decode_small")
    mel = _mel(c["frames"])
    V = c["spec"]["V"]
    good = ContextGraph(co.PHRASES["decode_small"], 1.5).tables()
    n, nc = good["n_nodes"], good["n_children"]
    rng = np.random.default_rng(5)
    bad = dict(good)
    bad["fail_link"] = np.arange(n, dtype=np.int32)                                   # every fail link a self-loop
    bad["fail_link"][1::3] = rng.integers(-10 ** 6, 10 ** 6, len(bad["fail_link"][1::3]))
    bad["child_node"] = rng.integers(-10 ** 6, 10 ** 6, nc).astype(np.int32)
    bad["child_off"] = rng.integers(-100, 10 ** 6, n + 1).astype(np.int32)
    bad["child_tok"] = rng.integers(-5, V + 5, nc).astype(np.int32)                    # unsorted, out of the vocabulary, the blank
    bad["depth"] = rng.integers(-10 ** 6, 10 ** 6, n).astype(np.int32)
    bad["terminal"] = rng.integers(0, 2, n).astype(np.int32)
    tables = {k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in bad.items()}
    for beam in (4, 16):
        got = _raw(model, mel, beam, 60, tables)  # asserts done and 1 <= n <= beam
        assert all(0 <= k < V - 1 for y, _ in got for k in y) and all(len(y) <= 59 for y, _ in got)
        assert all(np.isfinite(s) for _, s in got)


def test_graphs_beyond_the_device_envelope_take_the_host_loop(golden_dir):
    c, model = _case(golden_dir, "decode_small")
    mel = _mel(c["frames"][:6])
    g = ContextGraph(co.PHRASES["decode_small"], 1.5)
    assert model._beam_device_ok(mel.permute(0, 2, 1), 4, 60, g)
    dev = _search(model, mel, beam_size=4, max_length=60, context=g)
    real = g.children
    g.children = real + [{}] * (65537 - len(real))  # (n_nodes is what the envelope looks at; the extra nodes are unreachable)
    assert g.n_nodes > rnnt_amd.engine.BEAM_CONTEXT_MAX_NODES and not model._beam_device_ok(mel.permute(0, 2, 1), 4, 60, g)
    host = _search(model, mel, beam_size=4, max_length=60, context=g)
    g.children = real
    assert [y for y, _ in host] == [y for y, _ in dev]
    for (_, a), (_, b) in zip(host, dev):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b))
