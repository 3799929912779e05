"""-m gpu: the decode and beam kernels where the existing device suites never put them — the blank anywhere but V - 1 (every position
of k_beam_reduce's float4 quad, a chunk of another wave), beam widths that are no power of two, a vocabulary past one 4096-entry pass
of k_beam_reduce's waves, and exact ties.  Every device path reads model.joint.blank_idx: greedy_decode on each of its paths,
greedy_decode_many, the greedy stream, beam_search, beam_search_many, beam_stream and the context forms.

The references are the float64 oracles (oracle/decode_oracle.py, tests/beam_oracle.py, tests/context_oracle.py) run AT the moved blank;
tests/test_decode_relabel_oracle.py shows on the CPU that they give the mapped results of the oracle at V - 1 and that every
configuration here has the gap it needs (asserted again below, never assumed).  The bars are the existing ones: identical token lists
where the oracle's gap is above 1e-3, scores within 1e-4 * max(1, |score|), batch and stream equal to the single search exactly.
Each configuration prints its oracle gap and worst score error (profiles/decode_blank_parity.txt is one such run)."""
import numpy as np
import pytest
import torch

from oracle import decode_oracle
from tests import beam_oracle
from tests import decode_relabel as dr
from tests.helpers import load_decode_case
from tests.stream_models import partitions
from tests.test_beam_batch_gpu import utterances
from tests.test_beam_gpu import _lens, _mel
from tests.test_beam_stream_gpu import Offline, _feed
from tests.test_decode_gpu import all_paths
from tests.test_stream_gpu import _stream

pytestmark = pytest.mark.gpu

_models = {}


def _model(golden_dir, name, blank):
    """(relabelled case, engine model told its blank), built once per module."""
    if (name, blank) not in _models:
        c = dr.case_at(golden_dir, name, blank)
        _models[name, blank] = (c, dr.build_relabelled(c["spec"], c["pred_sd"], c["joint_sd"], c["blank"]))
    return _models[name, blank]


def _check_nbest(got, want, tag):
    """Identical token lists, scores within the project's bar; -> the worst score error relative to that bar's max(1, |score|)."""
    assert [y for y, _ in got] == [y for y, _ in want], tag
    worst = 0.0
    for (_, gs), (_, ws) in zip(got, want):
        assert abs(gs - ws) <= 1e-4 * max(1.0, abs(ws)), (tag, gs, ws)
        worst = max(worst, abs(gs - ws) / max(1.0, abs(ws)))
    return worst


def _greedy_streams(model, frames, ml, want, tag, persistent=(True, False)):
    """model.greedy_stream on its device paths, pushed in chunks of 1, 7 and T frames: the concatenated labels are `want`."""
    frames_ct = torch.from_numpy(np.ascontiguousarray(frames.T)).cuda()
    T = frames_ct.shape[1]
    for p in persistent:
        for sizes in ([1] * T, partitions(T)["7"], [T]):
            _, got, _ = _stream(model, frames_ct, sizes, ml, p)  # (asserts the path every push took)
            assert got == want, (tag, ml, p, sizes[0])


def _tok0(model, frames, blank, ml, beam=4):
    """Word 0 of the token buffers the ABI entries return is the blank the caller named."""
    import rnnt_amd
    eng = rnnt_amd.engine
    fr = model._decode_frames(_mel(frames).permute(0, 2, 1))
    bundle = model._decode_bundle()
    assert bundle[-1] == blank
    state, toks = eng.greedy_decode_loop(fr, *bundle, ml)
    assert toks[:1].tolist() == [blank] and state.tolist()[eng.DECODE_NTOK] >= 1
    if eng.greedy_decode_persistent_supported(fr.shape[0], *model._decode_sizes()):
        state, toks = eng.greedy_decode_persistent(fr, *bundle, ml)
        both = state._with_tokens.tolist()
        assert both[eng.DECODE_CODE] == 0 and both[eng.DECODE_STATE_WORDS] == blank
    state, tokens, _ = eng.beam_decode(fr, *bundle, ml, beam)
    st, tk = state.tolist(), tokens.tolist()
    assert st[3] == 1 and st[2] >= 1 and all(tk[j][0] == blank for j in range(st[2])), (st, [r[0] for r in tk])


def _beam_paths(model, frames, beam, ml, want, gap, tag, windows, every_push=None):
    """beam_search against the oracle's `want`; beam_search_many over `windows` (the first one is `frames`) equal to the single search
    exactly; beam_stream pushed frame by frame equal to it too (`every_push`: chunks after each of which the stream equals the offline
    search of the prefix).  Each on the device."""
    assert gap > dr.GAP, (tag, gap)
    mel = _mel(frames)
    assert model._beam_device_ok(mel.permute(0, 2, 1), beam, ml), tag
    model.last_beam_path = None
    got = model.beam_search(mel, _lens(mel), beam_size=beam, max_length=ml, return_nbest=True)
    assert model.last_beam_path == "device", tag
    worst = _check_nbest(got, want, tag)
    print(f"{tag} beam {beam} max_length {ml}: oracle gap {gap:.3e}, worst score error {worst:.3e}, {len(got)} entries")
    assert model.beam_search(mel, _lens(mel), beam_size=beam, max_length=ml) == want[0][0], tag
    mels = [_mel(u) for u in windows]
    assert all(model._beam_device_ok(m.permute(0, 2, 1), beam, ml) for m in mels) and model._beam_batch_ok(len(mels), beam, ml), tag
    many = model.beam_search_many(mels, beam_size=beam, max_length=ml, return_nbest=True)
    assert model.last_beam_path == "device" and many[0] == got, tag  # tokens and float64 scores, exactly
    for i, m in enumerate(mels[1:], 1):
        assert many[i] == model.beam_search(m, _lens(m), beam_size=beam, max_length=ml, return_nbest=True), (tag, beam, i)
    frames_ct = mel[0]
    T = frames_ct.shape[1]
    s = model.beam_stream(beam_size=beam, max_length=ml)
    if every_push is None:
        for t in range(T):
            s.push_encoded(frames_ct[None, :, t:t + 1])
    else:
        _feed(s, frames_ct, every_push, Offline(model, frames_ct, beam_size=beam, max_length=ml), tag)
    assert s.last_path == "device" and s.frames == T and s.nbest == got, tag
    return got


def _context_paths(golden_dir, model, name, blank, frames):
    """One configuration of tests/context_oracle.CONFIGS, its phrases mapped and a phrase of the blank's neighbours added, against the
    context oracle at that blank: beam_search and beam_search_many (ONE graph for the 12 windows)."""
    from rnnt_amd import ContextGraph
    ml = dr.CONTEXT[name][0]
    mel = _mel(frames)
    mels = [_mel(u) for u in utterances(frames)]
    for beam in dr.context_beams(name, blank):
        want, phrases, score = dr.context_at(golden_dir, name, blank, beam)
        assert want.gap > dr.GAP and want.events["touched"] > 0, (name, blank, beam, want.gap)
        g = ContextGraph(phrases, score)
        assert model._beam_device_ok(mel.permute(0, 2, 1), beam, ml, g)
        got = model.beam_search(mel, _lens(mel), beam_size=beam, max_length=ml, return_nbest=True, context=g)
        assert model.last_beam_path == "device"
        worst = _check_nbest(got, want.nbest, (name, blank, beam, "context"))
        print(f"{name} blank {blank} beam {beam} context (score {score}, {len(phrases)} phrases): oracle gap {want.gap:.3e}, "
              f"worst score error {worst:.3e}")
        many = model.beam_search_many(mels, beam_size=beam, max_length=ml, return_nbest=True, context=g)
        assert model.last_beam_path == "device" and many[0] == got
        for i in (1, 4, 7):  # a window from the start, the 1-frame one, a reversed one
            assert many[i] == model.beam_search(mels[i], _lens(mels[i]), beam_size=beam, max_length=ml, return_nbest=True, context=g), i


SMALL = [(name, blank) for name, blanks in dr.BLANKS.items() for blank in blanks]


@pytest.mark.parametrize("name,blank", SMALL)
def test_greedy_paths_at_a_moved_blank(golden_dir, name, blank):
    c, model = _model(golden_dir, name, blank)
    assert model.joint.blank_idx == blank != c["spec"]["V"] - 1
    mel = _mel(c["frames"])
    paths = set()
    for ml, want in c["tokens"].items():
        assert blank not in want and len(want) > 3
        paths |= all_paths(model, mel, _lens(mel), ml, want, (name, blank))
        _greedy_streams(model, c["frames"], ml, want, (name, blank))
    assert "persistent" in paths  # as for the case at V - 1 (tests/test_decode_gpu.py)
    _tok0(model, c["frames"], blank, max(c["tokens"]))


@pytest.mark.parametrize("name,blank", SMALL)
def test_beam_paths_at_a_moved_blank(golden_dir, name, blank):
    c, model = _model(golden_dir, name, blank)
    ml = dr.BEAM_ML[name]
    windows = utterances(c["frames"])
    for beam in dr.SMALL_BEAMS:
        want, _, gap = dr.beam_at(golden_dir, name, blank, beam, ml)
        got = _beam_paths(model, c["frames"], beam, ml, want, gap, f"{name} blank {blank}", windows)
        if beam == 1 and ml in c["tokens"]:
            assert got[0][0] == c["tokens"][ml]  # beam 1 is the reference's greedy decode, mapped
    if name in dr.CONTEXT:
        _context_paths(golden_dir, model, name, blank, c["frames"])


def test_the_wide_vocabulary_with_the_blank_in_another_waves_chunk(golden_dir):
    name, blank = "decode_wide_vocab", dr.WIDE_BLANK
    c, model = _model(golden_dir, name, blank)
    mel = _mel(c["frames"])
    paths = set()
    for ml, want in c["tokens"].items():
        paths |= all_paths(model, mel, _lens(mel), ml, want, (name, blank))
        _greedy_streams(model, c["frames"], ml, want, (name, blank))
    assert "persistent" in paths
    _tok0(model, c["frames"], blank, 60)
    want, _, gap = dr.beam_at(golden_dir, name, blank, 4, 60)
    _beam_paths(model, c["frames"], 4, 60, want, gap, f"{name} blank {blank}", utterances(c["frames"]))


def test_the_reference_widths_with_the_blank_first(golden_dir):
    name, blank, ml = "decode_ref_widths_proj", dr.REF_WIDTHS_BLANK, 25
    c, model = _model(golden_dir, name, blank)
    mel = _mel(c["frames"])
    want = c["tokens"][ml]
    assert "persistent" in all_paths(model, mel, _lens(mel), ml, want, (name, blank))
    _greedy_streams(model, c["frames"], ml, want, (name, blank))
    _tok0(model, c["frames"], blank, ml)
    nbest, _, gap = dr.beam_at(golden_dir, name, blank, 4, ml)
    _beam_paths(model, c["frames"], 4, ml, nbest, gap, f"{name} blank {blank}", utterances(c["frames"])[:4])  # (4 windows, as at V - 1)


ODD = [(name, ml, beam, None) for name, ml, beams in dr.ODD_BEAMS for beam in beams] + \
      [(dr.ODD_BEAMS_MOVED[0], dr.ODD_BEAMS_MOVED[1], beam, dr.ODD_BEAMS_MOVED[2]) for beam in dr.ODD_BEAMS_MOVED[3]]


@pytest.mark.parametrize("name,ml,beam,blank", ODD)
def test_beam_widths_that_are_no_power_of_two(golden_dir, name, ml, beam, blank):
    """k_beam_reduce and k_beam_select keep entry q in lane q and loop q < beam: widths 3 .. 15 that the device suites never ran.  The
    stream equals the offline search after EVERY push (7 frames each)."""
    assert beam & (beam - 1)
    c, model = _model(golden_dir, name, blank)
    want, _, gap = dr.beam_at(golden_dir, name, blank, beam, ml)
    tag = f"{name} blank {c['blank']}"
    got = _beam_paths(model, c["frames"], beam, ml, want, gap, tag, utterances(c["frames"]), every_push=partitions(c["frames"].shape[0])["7"])
    assert len(got) == beam  # the whole list is live: an entry past `beam` or a missing one would show


@pytest.mark.parametrize("V,blank", [(4100, None), (4100, dr.BEYOND_MOVED_BLANK), (8196, None)])
def test_a_vocabulary_beyond_one_pass_of_the_reduction(V, blank):
    """V > 4096: wave 0 of k_beam_reduce makes a second (V = 8196: a third) trip with its running list carried along, guarded by v < V;
    the oracle's lists hold ids of every trip (tests/test_decode_relabel_oracle.py)."""
    import rnnt_amd
    c = dr.beyond_one_pass_case(V, blank)
    model = dr.build_relabelled(c["spec"], c["pred_sd"], c["joint_sd"], c["blank"])
    mel = _mel(c["frames"])
    want, margins = decode_oracle.greedy_decode(c["frames"], c["pred_sd"], c["joint_sd"], max_length=c["ml"], blank=c["blank"])
    assert margins.min() > dr.MARGIN and any(k >= 4096 for k in want)
    paths = all_paths(model, mel, _lens(mel), c["ml"], want, (V, blank))
    assert ("persistent" in paths) == rnnt_amd.engine.greedy_decode_persistent_supported(mel.shape[-1], *model._decode_sizes())
    _greedy_streams(model, c["frames"], c["ml"], want, (V, blank), persistent=(False,) + ((True,) if "persistent" in paths else ()))
    _tok0(model, c["frames"], c["blank"], c["ml"])
    windows = dr.beyond_windows(c["frames"], c["windows"])
    om = dr.oracle_model(c["frames"], c["pred_sd"], c["joint_sd"], c["blank"])
    for beam in c["beams"]:
        nbest, _, gap = dr.oracle_search(om, beam, c["ml"])
        ids = {k for y, _ in nbest for k in y}
        assert any(k < 256 for k in ids) and any(k >= 4096 for k in ids)
        _beam_paths(model, c["frames"], beam, c["ml"], nbest, gap, f"V {V} blank {c['blank']}", windows)
        mels = [_mel(u) for u in windows]
        many = model.beam_search_many(mels, beam_size=beam, max_length=c["ml"], return_nbest=True)
        for i, u in enumerate(windows[1:], 1):  # the shorter windows against the oracle too
            w, _, g = dr.oracle_search(dr.oracle_model(u, c["pred_sd"], c["joint_sd"], c["blank"]), beam, c["ml"])
            assert g > dr.GAP
            _check_nbest(many[i], w, (V, blank, beam, i))


@pytest.mark.parametrize("variant", list(dr.TIES))
def test_exact_ties_go_to_the_first_index(golden_dir, variant):
    """Two classes with EXACTLY equal logits on every path (zero weight rows, one bias), the pair on top at 40 - 66 % of the decisions: the
    lower index wins in k_argmax_scan, in its lane and wave merges, in the persistent loop and in k_beam_reduce's label list
    (beam_before) — the blank ends the frame where it is the lower one, the label is emitted (up to the cap) where it is.  beam 1 of the
    SEARCH is held to its own oracle: k_beam_select puts a finished (blank) candidate before a label at equal scores (DESIGN.md §4h
    "Ties: finished first"), so there a blank / label tie ends the frame whichever index is lower."""
    r = dr.tied_case(load_decode_case(golden_dir, "decode_small"), variant)
    want, margins, share = dr.tied_greedy(r, 60)
    assert 0.25 <= share <= 0.75 and margins.min() > dr.MARGIN and len(want) > 3
    model = dr.build_relabelled(r["spec"], r["pred_sd"], r["joint_sd"], r["blank"])
    mel = _mel(r["frames"])
    assert "persistent" in all_paths(model, mel, _lens(mel), 60, want, variant)
    _greedy_streams(model, r["frames"], 60, want, variant)
    nbest, _, _ = beam_oracle.beam_search(dr.oracle_model(r["frames"], r["pred_sd"], r["joint_sd"], r["blank"]), 1, 60)
    assert (nbest[0][0] == want) == (variant != "label_first")
    assert model._beam_device_ok(mel.permute(0, 2, 1), 1, 60)
    got = model.beam_search(mel, _lens(mel), beam_size=1, max_length=60, return_nbest=True)
    worst = _check_nbest(got, nbest, variant)
    print(f"ties {variant}: pair {r['pair']} on top at {share:.2f} of {len(margins)} decisions, margin to the rest {margins.min():.3e}, "
          f"{len(want)} labels; beam 1 worst score error {worst:.3e}")
    other = {"blank_first": "label_first", "label_first": "blank_first"}.get(variant)
    if other:  # who wins the tie changes what is decoded
        ro = dr.tied_case(load_decode_case(golden_dir, "decode_small"), other)
        assert dr.tied_greedy(ro, 60)[0] != want
