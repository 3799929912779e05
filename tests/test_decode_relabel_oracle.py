"""CPU: the premises of tests/test_decode_blank_gpu.py, on the float64 oracles alone (no device; the engine only for size queries).

(1) Relabelling commutes with the oracles: the greedy oracle and the beam oracle run on a case relabelled to `blank`
(tests/decode_relabel.py) give the MAPPED results of the oracle at V - 1 — token lists exactly, scores within 1e-12, the same gap — so a
device path that is right at V - 1 and wrong at `blank` cannot hide behind the reference.  (2) Every configuration the device tests run
has the gap, the margin, the ids and the tie share it was chosen for."""
import numpy as np
import pytest

from oracle import decode_oracle
from tests import beam_oracle
from tests import decode_relabel as dr
from tests.helpers import DECODE_CASES, load_decode_case


def _greedy(c, ml, **kw):
    return decode_oracle.greedy_decode(c["frames"], c["pred_sd"], c["joint_sd"], max_length=ml, blank=c["blank"],
                                       window=7 if c["spec"]["E"] > 64 else None, **kw)


def test_the_blanks_cover_every_quad_position_and_a_chunk_of_another_wave():
    assert sorted(b % 4 for b in dr.BLANKS["decode_small"]) == [0, 1, 2, 3]  # once in each position of k_beam_reduce's float4
    assert {b % 4 for b in dr.BLANKS["decode_small"]} == {0 % 4, 5 % 4, 15 % 4, 30 % 4} == {0, 1, 3, 2}
    for name, blanks in dr.BLANKS.items():
        V = DECODE_CASES[name]["V"]
        assert all(0 <= b < V - 1 for b in blanks), name  # V - 1 stays with the existing tests
    assert dr.WIDE_BLANK % 4 == 1 and (dr.WIDE_BLANK // 256) % 16 == 3 and dr.WIDE_BLANK < DECODE_CASES["decode_wide_vocab"]["V"] - 1
    assert dr.WIDE_BLANK + 4096 >= DECODE_CASES["decode_wide_vocab"]["V"]  # (one trip per wave there: wave 3 meets the blank on its only one)
    assert dr.BEYOND_MOVED_BLANK >= 4096 and dr.BEYOND_MOVED_BLANK % 4 == 1  # the second trip of wave 0, quad position 1


@pytest.mark.parametrize("name", list(dr.BLANKS))
def test_the_oracles_commute_with_the_relabelling(golden_dir, name):
    base = dr.case_at(golden_dir, name)
    ml = dr.BEAM_ML[name]
    for blank in dr.BLANKS[name]:
        c = dr.case_at(golden_dir, name, blank)
        nmap = c["new_of_old"]
        assert c["blank"] == blank and nmap[base["blank"]] == blank and sorted(nmap) == list(range(len(nmap)))
        labels = np.delete(nmap, base["blank"])
        assert (np.diff(labels) > 0).all()  # the order among the labels is kept
        for gml, stored in base["tokens"].items():
            want0, m0 = _greedy(base, gml)
            want, m = _greedy(c, gml)
            assert want0 == stored and want == dr.map_tokens(stored, nmap) == c["tokens"][gml], (name, blank, gml)
            assert blank not in want and np.abs(m - m0).max() <= 1e-12 and m.min() > dr.MARGIN, (name, blank, gml, m.min())
        for beam in dr.SMALL_BEAMS:
            nb0, pruned0, gap0 = dr.beam_at(golden_dir, name, None, beam, ml)
            nb, pruned, gap = dr.beam_at(golden_dir, name, blank, beam, ml)
            assert [y for y, _ in nb] == [y for y, _ in dr.map_nbest(nb0, nmap)], (name, blank, beam)
            err = max(abs(s - s0) for (_, s), (_, s0) in zip(nb, nb0))
            print(f"{name} blank {blank} beam {beam}: oracle gap {gap:.3e} (at V - 1: {gap0:.3e}), scores differ by {err:.1e}")
            assert err <= 1e-12 and pruned == pruned0 and abs(gap - gap0) <= 1e-12, (name, blank, beam, err, gap, gap0)
            assert gap > dr.GAP, (name, blank, beam, gap)
        if name in dr.CONTEXT:
            assert dr.CONTEXT[name][0] == ml
            for beam in dr.CONTEXT_BEAMS:
                r, phrases, score = dr.context_at(golden_dir, name, blank, beam)
                if beam not in dr.context_beams(name, blank):
                    assert r.gap <= dr.GAP  # left out on the oracle alone
                    continue
                plain = dr.beam_at(golden_dir, name, blank, beam, ml)[0]
                print(f"{name} blank {blank} beam {beam} context: oracle gap {r.gap:.3e} {r.events}")
                assert r.gap > dr.GAP and r.events["touched"] > 0, (name, blank, beam, r.gap)
                assert not any(blank in ph for ph in phrases) and r.nbest[0][0] != plain[0][0]  # the graph acts
                assert {k for k in (blank - 1, blank + 1) if k >= 0} == set(phrases[-1])  # the blank's neighbours are a phrase


def test_the_wide_vocabulary_and_the_reference_widths(golden_dir):
    for name, blank, mls in (("decode_wide_vocab", dr.WIDE_BLANK, (60, 9)), ("decode_ref_widths_proj", dr.REF_WIDTHS_BLANK, (25,))):
        base, c = dr.case_at(golden_dir, name), dr.case_at(golden_dir, name, blank)
        for gml in mls:
            want, m = _greedy(c, gml)
            assert want == dr.map_tokens(base["tokens"][gml], c["new_of_old"]) and m.min() > dr.MARGIN and len(want) > 3, (name, gml)
        nb, _, gap = dr.beam_at(golden_dir, name, blank, 4, max(mls))
        print(f"{name} blank {blank} beam 4 max_length {max(mls)}: oracle gap {gap:.3e}")
        assert gap > dr.GAP and len(nb[0][0]) > 3, (name, gap)


@pytest.mark.parametrize("name,ml,beams", dr.ODD_BEAMS)
def test_the_widths_that_are_no_power_of_two_have_their_gap(golden_dir, name, ml, beams):
    assert all(b & (b - 1) for b in beams) and ml == dr.BEAM_ML[name]
    for beam in beams:
        nb, pruned, gap = dr.beam_at(golden_dir, name, None, beam, ml)
        print(f"{name} beam {beam}: oracle gap {gap:.3e}, {len(nb)} entries")
        assert gap > dr.GAP and pruned > 0, (name, beam, gap)
    mname, mml, mblank, mbeams = dr.ODD_BEAMS_MOVED
    if name == mname:
        for beam in mbeams:
            assert beam in beams and dr.beam_at(golden_dir, name, mblank, beam, mml)[2] > dr.GAP


@pytest.mark.parametrize("V,blank", [(4100, None), (4100, dr.BEYOND_MOVED_BLANK), (8196, None)])
def test_beyond_one_pass_of_the_reduction(V, blank):
    """What the seeded cases past V = 4096 were picked for: the greedy decode emits labels from wave 0's later trips with a clear
    margin, and every n-best list holds ids of wave 0's first trip (< 256) AND of each later one — the list carried into the next chunk
    is merged with live entries there."""
    c = dr.beyond_one_pass_case(V, blank)
    nmap = c["new_of_old"]
    assert c["blank"] == (V - 1 if blank is None else blank) and V % 4 == 0 and V > 4096
    trips = [(lo, min(lo + 256, V)) for lo in range(0, V, 4096)]  # wave 0's chunks
    assert len(trips) == (2 if V == 4100 else 3) and trips[-1][1] - trips[-1][0] == 4
    if blank is not None:
        assert trips[1][0] <= blank < trips[1][1]
    want, m = decode_oracle.greedy_decode(c["frames"], c["pred_sd"], c["joint_sd"], max_length=c["ml"], blank=c["blank"])
    print(f"V {V} blank {c['blank']}: greedy {want}, smallest margin {m.min():.3e}")
    assert len(want) >= 3 and any(k >= 4096 for k in want) and m.min() > dr.MARGIN
    om = dr.oracle_model(c["frames"], c["pred_sd"], c["joint_sd"], c["blank"])
    for beam in c["beams"]:
        nb, _, gap = dr.oracle_search(om, beam, c["ml"])
        ids = {k for y, _ in nb for k in y}
        print(f"V {V} blank {c['blank']} beam {beam}: oracle gap {gap:.3e}, ids {sorted(ids)}")
        assert gap > dr.GAP, (V, beam, gap)
        for lo, hi in trips:
            assert any(lo <= k < hi for k in ids), (V, beam, lo, sorted(ids))
        assert c["blank"] not in ids
    if blank is not None:  # the relabelled case is the mapped case
        c0 = dr.beyond_one_pass_case(V)
        want0, _ = decode_oracle.greedy_decode(c0["frames"], c0["pred_sd"], c0["joint_sd"], max_length=c["ml"])
        assert want == dr.map_tokens(want0, nmap)
    for u in dr.beyond_windows(c["frames"], c["windows"])[1:]:
        om = dr.oracle_model(u, c["pred_sd"], c["joint_sd"], c["blank"])
        for beam in c["beams"]:
            assert dr.oracle_search(om, beam, c["ml"])[2] > dr.GAP, (V, len(u), beam)


def test_exact_ties(golden_dir):
    """The tied pair is the maximum at a quarter to three quarters of the decisions, every decision's margin to the best logit OUTSIDE the
    pair is clear, and who wins the tie changes what is decoded."""
    case = load_decode_case(golden_dir, "decode_small")
    lists = {}
    for variant, cfg in dr.TIES.items():
        r = dr.tied_case(case, variant)
        a, b = r["pair"]
        assert a < b and (r["blank"] in (a, b)) == (variant != "two_labels")
        assert not r["joint_sd"]["joint_ln.weight"][[a, b]].any() and r["joint_sd"]["joint_ln.bias"][a] == r["joint_sd"]["joint_ln.bias"][b]
        want, m, share = dr.tied_greedy(r, 60)
        print(f"{variant}: {len(want)} labels, {len(m)} decisions, pair on top at {share:.2f}, margin to the rest {m.min():.3e}")
        assert 0.25 <= share <= 0.75 and m.min() > dr.MARGIN and len(want) > 3, (variant, share, m.min())
        assert b not in want  # the higher index never wins: it is the blank, or a label that is tied with a lower index wherever it leads
        lists[variant] = want
        # beam 1 of the search: k_beam_reduce's label list takes the lower id at equal values, k_beam_select a finished (blank) candidate
        # before a label at equal SCORES — so a tie between the blank and a label ends the frame whichever index is lower, and beam 1 is
        # the greedy decode in `blank_first` and `two_labels` but not in `label_first`
        nb, _, _ = beam_oracle.beam_search(dr.oracle_model(r["frames"], r["pred_sd"], r["joint_sd"], r["blank"]), 1, 60)
        assert (nb[0][0] == want) == (variant != "label_first"), variant
    assert lists["blank_first"] != lists["label_first"]
    assert 5 in lists["label_first"] and 20 not in lists["blank_first"]


def test_the_decode_tables_take_a_vocabulary_the_persistent_loop_refuses():
    """beam_search_many and beam_stream bring the model's tables (rnnt_engine_greedy_decode_build_tables) to searches that take any number
    of symbols; only the persistent greedy loop stops at 4096.  The tables' size query used to apply that loop's limit, so both raised at
    V = 4100 where beam_search ran.  (Size queries: no device work.)"""
    import ctypes

    import rnnt_amd
    eng = rnnt_amd.engine
    for V in dr.BEYOND:
        s = dr.BEYOND[V]["spec"]
        sizes = (V, s["E"], s["O"], s["H"], V, False)
        n = ctypes.c_size_t(0)
        assert eng.lib().rnnt_engine_greedy_decode_tables_bytes(V, s["E"], s["O"], s["H"], 0, ctypes.byref(n)) == 0
        assert n.value >= 4 * (3 * V * s["E"] + V * s["E"])  # the three tap tables and the normalised embedding
        assert not eng.greedy_decode_persistent_supported(12, *sizes)
        assert eng.beam_decode_supported(*sizes, 60, 16) and eng.beam_decode_batch_supported(*sizes, 60, 16, 3)
        assert eng.beam_stream_supported(*sizes, 60, 16)
