"""CPU: the contextual-biasing definition (DESIGN.md §4h "Context") — rnnt_amd.ContextGraph's unit cases, its agreement with the
independent restatement in tests/context_oracle.py, and that oracle itself: without a graph it is tests/beam_oracle.beam_search, and the
configurations the host loop and the device are held to have the gaps and the events they are chosen for."""
import math

import numpy as np
import pytest

import rnnt_amd
from rnnt_amd import ContextGraph
from tests import beam_oracle, context_oracle as co
from tests.helpers import load_decode_case


@pytest.mark.parametrize("name,ml,beams", [("decode_small", 60, (1, 4)), ("decode_cap", 37, (2, 16))])
def test_without_a_graph_the_oracle_is_the_plain_oracle(golden_dir, name, ml, beams):
    c = load_decode_case(golden_dir, name)
    om = beam_oracle.Model(c["frames"], c["pred_sd"], c["joint_sd"])
    for beam in beams:
        want, pruned, gap = beam_oracle.beam_search(om, beam, ml)
        got = co.beam_search(om, beam, ml)
        assert got.nbest == want and got.internal == want and got.pruned == pruned and got.gap == gap  # float for float
        assert not any(got.events.values())
        # a graph that cannot act is the same search: no phrase, or score 0
        for g in (co.Trie([], 2.0), co.Trie(co.PHRASES[name], 0.0)):
            r = co.beam_search(om, beam, ml, graph=g)
            assert r.nbest == want and r.pruned == pruned


def test_the_configurations_have_their_gaps_and_events(golden_dir):
    total = dict.fromkeys(co.EVENTS, 0)
    for name, ml, key, score, beams in co.CONFIGS:
        if name == "decode_ref_widths":
            continue  # (the slowest oracle: asserted where it is needed, tests/test_beam_context_host.py and the GPU test)
        for beam in beams:
            r = co.result(golden_dir, name, ml, key, score, beam)
            print(f"{name} {key} score {score} beam {beam}: gap {r.gap:.3e} pruned {r.pruned} {r.events}")
            assert r.gap > co.GAP, (name, key, score, beam, r.gap)
            assert len(r.nbest) == len(r.internal) <= beam
            assert sorted(map(tuple, (y for y, _ in r.nbest))) == sorted(map(tuple, (y for y, _ in r.internal)))
            for k in total:
                total[k] += r.events[k]
    assert all(v > 0 for v in total.values()), total
    # the fixture that leans hardest on labels OUTSIDE the raw top-`beam` of their row
    assert co.result(golden_dir, "decode_cap", 37, "decode_cap", 3.0, 2).events["outside"] >= 5


def test_long_list_shape():
    g = ContextGraph(co.PHRASES["decode_wide_vocab+600"], 1.5)
    assert len(g.children[0]) == 605 and g.n_nodes == 1228
    t = co.Trie(co.PHRASES["decode_wide_vocab+600"], 1.5)
    assert len(t.kids[0]) == 605 and len(t.kids) == 1228


def test_fail_links_of_overlapping_phrases():
    g = ContextGraph([(1, 2, 3), (2, 3, 4), (3, 5)], 1.0)
    node = lambda *p: g.walk(p)  # noqa: E731  (no phrase completes along these paths)
    assert g.fail[node(1)] == 0 and g.fail[node(1, 2)] == node(2) and g.fail[node(2, 3)] == node(3)
    assert g.depth[node(1, 2)] == 2 and g.bonus(node(1, 2)) == 2.0
    # 1 2 then 3 completes (1, 2, 3): banked, back at the root — the suffix (2, 3) is not carried
    n, d = g.step(node(1, 2), 3)
    assert (n, d) == (0, 1.0)
    # 2 3 then 5: no child at (2, 3), its fail (3) has 5: lands on the terminal (3, 5): delta = 2 - 2
    n, d = g.step(node(2, 3), 5)
    assert (n, d) == (0, 0.0)
    # 1 2 then 9: nothing matches, the partial bonus is taken back
    assert g.step(node(1, 2), 9) == (0, -2.0)
    # 1 then 1: the match restarts at depth 1
    assert g.step(node(1), 1) == (node(1), 0.0)
    assert g.exceptions(node(1, 2)) == {3, 1, 2}  # children of (1, 2), of its fail (2), of the root


def test_a_phrase_extending_another_contributes_nothing_beyond_it():
    g = ContextGraph([(7, 8, 9, 10), (7, 8), (5,)], 2.0)
    assert g.n_nodes == 4  # root, (7), (7, 8) terminal, (5) terminal: the tail 9 10 is unreachable
    assert g.step(g.walk((7,)), 8) == (0, 2.0)
    assert g.walk((7, 8, 9)) == 0 and g.step(0, 9) == (0, 0.0)
    assert g.step(0, 5) == (0, 2.0)  # a one-token phrase banks at once
    same = ContextGraph([(7, 8), (5,)], 2.0)
    assert (same.children, same.fail, same.terminal, same.depth) == (g.children, g.fail, g.terminal, g.depth)


def test_duplicates_are_dropped_and_bad_arguments_raise():
    g = ContextGraph([[1, 2], (1, 2), np.array([1, 2]), [3]], 0.5)
    assert g.phrases == [(3,), (1, 2)] and g.n_nodes == 4
    assert ContextGraph([], 1.0).n_nodes == 1 and not ContextGraph([], 1.0).active and not ContextGraph([(1,)], 0.0).active
    assert ContextGraph([list(range(64))], 1.0).n_nodes == 65
    for phrases, score in (([[]], 1.0), ([(1,), ()], 1.0), ([(1,)], -0.5), ([(1,)], math.inf), ([(1,)], math.nan), ([(1,)], "x"),
                           ([list(range(65))], 1.0), ([(-1,)], 1.0), ([(1.5,)], 1.0)):
        with pytest.raises(ValueError):
            ContextGraph(phrases, score)
    g.check(10, 9)
    with pytest.raises(ValueError, match="blank"):
        g.check(10, 3)
    with pytest.raises(ValueError, match="vocabulary"):
        g.check(3, 2)


def _random_graph(rng, vocab, n, score):
    return [tuple(int(k) for k in rng.integers(0, vocab, rng.integers(1, 6))) for _ in range(n)], score


@pytest.mark.parametrize("seed", range(4))
def test_the_graph_is_the_oracles_trie_and_deltas_telescope(seed):
    """rnnt_amd.ContextGraph against the independent Trie of tests/context_oracle.py (fail links by definition there), and along any
    sequence: sum of deltas - bonus(final node) = score * (tokens of the banked phrases); delta >= -bonus(n), equal exactly at the root."""
    rng = np.random.default_rng(seed)
    vocab = 4 + seed  # small: overlaps, repeats and extensions are the rule
    phrases, score = _random_graph(rng, vocab, 12, 1.5)
    g, t = ContextGraph(phrases, score), co.Trie(phrases, score)
    assert g.n_nodes == len(t.kids)
    to_t = {0: 0}  # node numbering may differ: map by path
    for n in range(g.n_nodes):
        for k, c in g.children[n].items():
            to_t[c] = t.kids[to_t[n]][k]
            assert g.terminal[c] == t.term[to_t[c]] and g.depth[c] == t.depth[to_t[c]]
    assert all(to_t[g.fail[n]] == t.fail[to_t[n]] for n in range(g.n_nodes))
    for _ in range(50):
        seq = rng.integers(0, vocab, 30)
        n, total, banked = 0, 0.0, 0
        for k in seq:
            k = int(k)
            nn, d = g.step(n, k)
            tn, td, _, tbank = t.step(to_t[n], k)
            assert to_t[nn] == tn and d == td
            assert d >= -g.bonus(n) and (d == -g.bonus(n)) == (g._land(n, k) == 0)
            if tbank:
                banked += g.depth[g._land(n, k)]
            total += d
            n = nn
        assert n == g.walk(seq.tolist())
        assert total - g.bonus(n) == score * banked  # (score 1.5: every term exact)
        assert g.finalise([(seq.tolist(), total)]) == [(seq.tolist(), score * banked)]
    row = g.delta_row(n, vocab)
    assert [row[k] for k in range(vocab)] == [g.step(n, k)[1] for k in range(vocab)]


def test_tables_are_the_flat_form_of_the_graph():
    g = ContextGraph(co.PHRASES["decode_cap"], 1.5)
    t = g.tables()
    assert t["n_nodes"] == g.n_nodes and t["n_children"] == g.n_nodes - 1 and t["score"] == 1.5
    assert all(t[k].dtype == np.int32 for k in ("child_off", "child_tok", "child_node", "fail_link", "depth", "terminal"))
    assert t["child_off"][0] == 0 and t["child_off"][-1] == t["n_children"] and len(t["child_off"]) == g.n_nodes + 1
    for n in range(g.n_nodes):
        a, b = t["child_off"][n], t["child_off"][n + 1]
        toks = t["child_tok"][a:b].tolist()
        assert toks == sorted(g.children[n]) and [g.children[n][k] for k in toks] == t["child_node"][a:b].tolist()
    assert t["fail_link"].tolist() == g.fail and t["depth"].max() <= 64
    empty = ContextGraph([], 1.0).tables()
    assert empty["n_nodes"] == 1 and empty["n_children"] == 0 and len(empty["child_tok"]) == 1  # never a zero-length array
    assert rnnt_amd.context.MAX_DEVICE_NODES == rnnt_amd.engine.BEAM_CONTEXT_MAX_NODES == 65536
