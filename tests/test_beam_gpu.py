"""-m gpu: RNNTModel.beam_search on the device (rnnt_engine_beam_decode) against (1) the reference's greedy token lists
(tests/golden/decode_*.npz: beam 1 is the reference's greedy decode), (2) the float64 oracle of the search (tests/beam_oracle.py) and
(3) the transducer likelihood (oracle/brute_force.py) where nothing is pruned."""
import itertools

import numpy as np
import pytest
import torch

from oracle.brute_force import nll_bruteforce
from tests import beam_oracle
from tests.helpers import DECODE_CASES, decode_case_arrays, load_decode_case
from tests.test_decode_gpu import build_model

pytestmark = pytest.mark.gpu

GAP = 1e-3  # smallest oracle score gap at a keep / drop boundary for which identical n-best lists are demanded


def _mel(frames):
    return torch.from_numpy(np.ascontiguousarray(frames.T))[None].cuda()  # (1, C, T): PassThroughEncoder's output


def _lens(mel):
    return torch.tensor([mel.shape[-1]], device="cuda")


@pytest.mark.parametrize("name", list(DECODE_CASES))
def test_beam1_is_the_reference_greedy_decode(golden_dir, name):
    c = load_decode_case(golden_dir, name)
    model = build_model(c["spec"], c["pred_sd"], c["joint_sd"])
    mel = _mel(c["frames"])
    for ml, want in c["tokens"].items():
        assert model._beam_device_ok(mel.permute(0, 2, 1), 1, ml), name
        assert model.beam_search(mel, _lens(mel), beam_size=1, max_length=ml) == want, (name, ml)


# (case, max_length, beams): every entry's oracle gap is above GAP (checked below, not assumed)
ORACLE_CONFIGS = [("decode_small", 60, (2, 4, 8, 16)), ("decode_small_proj", 60, (2, 4, 8)), ("decode_small_proj", 9, (16,)),
                  ("decode_cap", 37, (2, 4, 8, 16)), ("decode_wide_vocab", 60, (2, 4, 8, 16)), ("decode_ref_widths", 200, (2, 4, 8))]


@pytest.mark.parametrize("name,ml,beams", ORACLE_CONFIGS)
def test_beams_match_the_oracle(golden_dir, name, ml, beams):
    c = load_decode_case(golden_dir, name)
    model = build_model(c["spec"], c["pred_sd"], c["joint_sd"])
    om = beam_oracle.Model(c["frames"], c["pred_sd"], c["joint_sd"])
    mel = _mel(c["frames"])
    for beam in beams:
        want, pruned, gap = beam_oracle.beam_search(om, beam, ml)
        assert gap > GAP, (name, beam, ml, gap)
        assert model._beam_device_ok(mel.permute(0, 2, 1), beam, ml)
        got = model.beam_search(mel, _lens(mel), beam_size=beam, max_length=ml, return_nbest=True)
        assert [g[0] for g in got] == [w[0] for w in want], (name, beam, ml)
        for (_, gs), (_, ws) in zip(got, want):
            assert abs(gs - ws) <= 1e-4 * max(1.0, abs(ws)), (name, beam, ml, gs, ws)
        assert model.beam_search(mel, _lens(mel), beam_size=beam, max_length=ml) == want[0][0]


def test_beam1_one_symbol_per_frame_is_greedy_loop(golden_dir):
    import rnnt_amd
    for name in ("decode_small", "decode_cap"):
        c = load_decode_case(golden_dir, name)
        model = build_model(c["spec"], c["pred_sd"], c["joint_sd"])
        mel = _mel(c["frames"])
        frames = mel[0].T.contiguous()
        p = model.predictor
        ml = max(c["tokens"])
        state, toks = rnnt_amd.engine.greedy_decode_loop(frames, p._params(), 1e-5, None, None, model.joint.joint_ln.weight,
                                                         model.joint.joint_ln.bias, model.joint.blank_idx, ml, max_per_frame=1)
        n = int(state[2])
        want = toks[1:1 + n].tolist()
        assert len(want) > 3
        assert model.beam_search(mel, _lens(mel), beam_size=1, max_length=ml, max_symbols_per_frame=1) == want


TINY = dict(V=4, E=8, O=8, H=8, fa=-1, ft=-1, T=3, max_lengths=(2,), w_scale=1.0, store=False)


@pytest.mark.parametrize("T,ml,m", [(3, 2, 2), (1, 3, 3), (2, 2, 3)])
def test_unpruned_scores_are_transducer_likelihoods(T, ml, m):
    """Nothing pruned and m >= max_length (every alignment ends each frame with a blank): every sequence of <= max_length - 1
    labels survives, with score log P(y | x) = -(RNN-T loss of y)."""
    spec = dict(TINY, T=T)
    frames, pred_sd, joint_sd = decode_case_arrays(spec, 77 + T, 0.0)
    om = beam_oracle.Model(frames, pred_sd, joint_sd)
    _, pruned, _ = beam_oracle.beam_search(om, 16, ml, m)
    assert pruned == 0
    model = build_model(spec, pred_sd, joint_sd)
    mel = _mel(frames)
    assert model._beam_device_ok(mel.permute(0, 2, 1), 16, ml)
    got = model.beam_search(mel, _lens(mel), beam_size=16, max_length=ml, max_symbols_per_frame=m, return_nbest=True)
    seqs = [list(y) for n in range(ml) for y in itertools.product(range(spec["V"] - 1), repeat=n)]
    assert sorted(g[0] for g in got) == sorted(seqs)
    for y, s in got:
        want = -nll_bruteforce(beam_oracle.lattice_logits(om, y), y, T, len(y), om.blank)
        assert abs(s - want) <= 1e-5, (y, s, want)


def test_blank_always_wins_gives_empty(golden_dir):
    c = load_decode_case(golden_dir, "decode_small")
    joint = dict(c["joint_sd"])
    joint["joint_ln.bias"] = joint["joint_ln.bias"].copy()
    joint["joint_ln.bias"][-1] += 1000.0
    model = build_model(c["spec"], c["pred_sd"], joint)
    mel = _mel(c["frames"])
    assert model.beam_search(mel, _lens(mel), beam_size=4, max_length=60) == []


def test_nan_workspace_and_repeat_runs_are_bit_identical(golden_dir):
    import rnnt_amd
    c = load_decode_case(golden_dir, "decode_small_proj")
    model = build_model(c["spec"], c["pred_sd"], c["joint_sd"])
    mel = _mel(c["frames"])
    a = model.beam_search(mel, _lens(mel), beam_size=8, max_length=60, return_nbest=True)
    b = model.beam_search(mel, _lens(mel), beam_size=8, max_length=60, return_nbest=True)
    assert a == b  # tokens and float64 scores, exactly
    dev = torch.device("cuda", torch.cuda.current_device())
    ws = rnnt_amd.engine.workspace(dev, 1)  # the stream's cached scratch buffer the call will reuse
    ws.fill_(255)  # every float / double in it is a NaN
    torch.cuda.synchronize()
    assert model.beam_search(mel, _lens(mel), beam_size=8, max_length=60, return_nbest=True) == a
