"""-m gpu: RNNTModel.beam_search_many (rnnt_engine_beam_decode_batch, DESIGN.md §4h "Batched") — N utterances advanced in lockstep —
against (1) beam_search of each utterance alone, exactly (token lists and float64 scores with ==), (2) the float64 oracle of the
search (tests/beam_oracle.py) and (3) the reference's greedy token lists (beam 1).  The utterances of a case are windows of its stored
frames, forward and time-reversed: 12 per case, lengths 1 .. T."""
import numpy as np
import pytest
import torch

from tests import beam_oracle
from tests.helpers import load_decode_case
from tests.test_beam_gpu import _lens, _mel
from tests.test_decode_gpu import build_model

pytestmark = pytest.mark.gpu

GAP = 1e-3  # smallest oracle score gap at a keep / drop boundary for which identical n-best lists are demanded


def windows(T):
    return [(0, T), (0, 8 * T // 15), (T // 4, T), (T // 7, T // 7 + max(2, T // 4)), (T - 1, T), (T // 2, T // 2 + 3)]


def utterances(frames):
    """The 12 frame arrays of a case: every window forward, then every window time-reversed."""
    w = [frames[a:b] for a, b in windows(frames.shape[0])]
    assert all(len(x) >= 1 for x in w)
    return [x.copy() for x in w] + [x[::-1].copy() for x in w]  # (copies: a reversed view has a negative stride)


def _case(golden_dir, name):
    c = load_decode_case(golden_dir, name)
    model = build_model(c["spec"], c["pred_sd"], c["joint_sd"])
    return c, model, utterances(c["frames"])


def _single(model, mel, **kw):
    return model.beam_search(mel, _lens(mel), return_nbest=True, **kw)


@pytest.mark.parametrize("beam", [1, 4, 8, 16])
@pytest.mark.parametrize("name,ml", [("decode_small", 60), ("decode_small_proj", 60), ("decode_cap", 37)])
def test_batch_equals_the_single_search_exactly(golden_dir, name, ml, beam):
    c, model, utts = _case(golden_dir, name)
    mels = [_mel(u) for u in utts]
    assert sorted(m.shape[-1] for m in mels)[0] == 1 and max(m.shape[-1] for m in mels) == c["frames"].shape[0]
    assert all(model._beam_device_ok(m.permute(0, 2, 1), beam, ml) for m in mels)
    got = model.beam_search_many(mels, beam_size=beam, max_length=ml, return_nbest=True)
    assert len(got) == len(mels)
    for i, mel in enumerate(mels):
        assert got[i] == _single(model, mel, beam_size=beam, max_length=ml), (name, beam, i)  # tokens and float64 scores, exactly
    best = model.beam_search_many(mels, beam_size=beam, max_length=ml)
    assert best == [g[0][0] for g in got]


def test_batch_equals_the_single_search_at_the_reference_widths(golden_dir):
    c, model, utts = _case(golden_dir, "decode_ref_widths")
    mels = [_mel(u) for u in utts[:4]]
    got = model.beam_search_many(mels, beam_size=4, max_length=200, return_nbest=True)
    for i, mel in enumerate(mels):
        assert model._beam_device_ok(mel.permute(0, 2, 1), 4, 200)
        assert got[i] == _single(model, mel, beam_size=4, max_length=200), i


@pytest.mark.parametrize("name", ["decode_small", "decode_small_proj"])
def test_batch_matches_the_oracle(golden_dir, name):
    c, model, utts = _case(golden_dir, name)
    mels = [_mel(u) for u in utts]
    for beam in (4, 8):
        got = model.beam_search_many(mels, beam_size=beam, max_length=60, return_nbest=True)
        for i, u in enumerate(utts):
            want, _, gap = beam_oracle.beam_search(beam_oracle.Model(u, c["pred_sd"], c["joint_sd"]), beam, 60)
            print(f"{name} beam {beam} utterance {i} (T={len(u)}): oracle gap {gap:.3e}")
            assert gap > GAP, (name, beam, i, gap)
            assert [g[0] for g in got[i]] == [w[0] for w in want], (name, beam, i)
            for (_, gs), (_, ws) in zip(got[i], want):
                assert abs(gs - ws) <= 1e-4 * max(1.0, abs(ws)), (name, beam, i, gs, ws)


@pytest.mark.parametrize("name", ["decode_small", "decode_small_proj", "decode_cap"])
def test_beam1_is_the_reference_greedy_decode(golden_dir, name):
    c, model, utts = _case(golden_dir, name)
    mels = [_mel(u) for u in utts]
    for ml, want in c["tokens"].items():
        assert model.beam_search_many(mels, beam_size=1, max_length=ml)[0] == want, (name, ml)  # entry 0: (0, T) forward


def test_results_do_not_depend_on_batch_mates_position_or_batch_size(golden_dir):
    c, model, utts = _case(golden_dir, "decode_small_proj")
    mels = [_mel(u) for u in utts]
    kw = dict(beam_size=4, max_length=60, return_nbest=True)
    full = model.beam_search_many(mels, batch=12, **kw)
    assert model.beam_search_many(mels, batch=5, **kw) == full  # 5 + 5 + 2
    assert model.beam_search_many(mels, batch=1, **kw) == full
    assert model.beam_search_many(mels, **kw) == full           # the default batch
    order = [7, 0, 11, 3, 3, 9, 0]                              # other neighbours, other positions, repeats
    assert model.beam_search_many([mels[i] for i in order], **kw) == [full[i] for i in order]
    assert model.beam_search_many([mels[2], mels[2]], **kw) == [full[2], full[2]]
    assert model.beam_search_many(mels[::-1], **kw) == full[::-1]


def test_poisoned_workspace_and_repeat_runs_are_bit_identical(golden_dir):
    import rnnt_amd
    c, model, utts = _case(golden_dir, "decode_small_proj")
    mels = [_mel(u) for u in utts]
    kw = dict(beam_size=8, max_length=60, return_nbest=True)
    a = model.beam_search_many(mels, **kw)
    assert model.beam_search_many(mels, **kw) == a  # tokens and float64 scores, exactly
    dev = torch.device("cuda", torch.cuda.current_device())
    ws = rnnt_amd.engine.workspace(dev, 1)  # the stream's cached scratch buffer the call will reuse
    ws.fill_(255)  # every float / double in it is a NaN, every counter and status garbage
    torch.cuda.synchronize()
    assert model.beam_search_many(mels, **kw) == a


def test_edges(golden_dir):
    import rnnt_amd
    c, model, utts = _case(golden_dir, "decode_small")
    mels = [_mel(u) for u in utts]
    assert model.beam_search_many([], beam_size=4, max_length=60) == []
    one = model.beam_search_many(mels[:1], beam_size=4, max_length=60, return_nbest=True)  # N = 1
    assert one == [_single(model, mels[0], beam_size=4, max_length=60)]
    s = c["spec"]
    sizes = (s["V"], s["E"], s["O"], s["H"], s["V"], False, 60, 4)
    assert rnnt_amd.engine.beam_decode_batch_supported(*sizes, 64)
    assert not rnnt_amd.engine.beam_decode_batch_supported(*sizes, 65)
    assert not rnnt_amd.engine.beam_decode_batch_supported(*sizes, 0)
    many = (mels * 6)[:64]  # N = 64 in one batch
    got = model.beam_search_many(many, beam_size=4, max_length=60, return_nbest=True, batch=64)
    full = model.beam_search_many(mels, beam_size=4, max_length=60, return_nbest=True)
    assert got == (full * 6)[:64]
    with pytest.raises(ValueError):
        model.beam_search_many(mels, batch=65)


def test_blank_always_wins_gives_empty_for_every_utterance(golden_dir):
    c = load_decode_case(golden_dir, "decode_small")
    joint = dict(c["joint_sd"])
    joint["joint_ln.bias"] = joint["joint_ln.bias"].copy()
    joint["joint_ln.bias"][-1] += 1000.0
    model = build_model(c["spec"], c["pred_sd"], joint)
    mels = [_mel(u) for u in utterances(c["frames"])]
    assert model.beam_search_many(mels, beam_size=4, max_length=60) == [[] for _ in mels]
