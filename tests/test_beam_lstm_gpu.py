"""-m gpu: beam search of LSTMPredictor models on the device (rnnt_engine_beam_decode_lstm, rnnt_amd/csrc/beam.hip + lstm.hip; DESIGN.md
§4h "LSTM") against the float64 oracle of tests/beam_lstm_oracle.py.

n-best lists are compared for EQUALITY under the premise — asserted at the head of each test (bo.checked) — that the oracle's smallest
keep / drop gap exceeds bo.GAP and that the list holds entries of two lengths, one of 3 or more labels; scores are held to the oracle
within 1e-4 max(1, |score|).  An utterance's tokens, state words and float64 scores in a batch are compared for bit equality with its
search alone.  With RNNT_BEAM_LSTM_PARITY_OUT=<file> set the score errors of every oracle comparison are appended to that file
(profiles/beam_lstm_parity.txt is such a run)."""
import copy
import functools
import itertools
import os

import numpy as np
import pytest
import torch

from oracle.brute_force import nll_bruteforce
from tests import beam_lstm_oracle as bo
from tests import lstm_decode_cases as dc

pytestmark = pytest.mark.gpu


def on_device(model64):
    return copy.deepcopy(model64).float().cuda().eval()


@functools.lru_cache(maxsize=None)
def device_model(name):
    return on_device(bo.model_of(name))


def _lens(mel):
    return torch.tensor([mel.shape[-1]]).cuda()


def search(model, mel64, **kw):
    mel = mel64.float().cuda()
    out = model.beam_search(mel, _lens(mel), return_nbest=True, **kw)
    assert model.last_beam_path == "lstm_device" and model.predictor.last_backend == "engine"
    return out


def record(tag, got, want):
    """Each returned score against the float64 score of the same sequence: worst absolute and relative error."""
    errs = [abs(gs - ws) for (_, gs), (_, ws) in zip(got, want)]
    rels = [e / max(1.0, abs(ws)) for e, (_, ws) in zip(errs, want)]
    line = f"{tag:44s} entries {len(got):2d}  worst |err| {max(errs):.3e}  worst rel {max(rels):.3e}  bar {bo.SCORE_TOL:.0e}"
    print(line)
    path = os.environ.get("RNNT_BEAM_LSTM_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def raw(model, mels64, beam, max_length=200, m=10):
    """engine.beam_decode_lstm of the mels on the device model: per utterance (state words, [token row of each entry], float64 scores)."""
    from rnnt_amd import engine
    frames = [model._decode_frames(model.encoder(mel.float().cuda()).permute(0, 2, 1)) for mel in mels64]
    tl = getattr(model.joint, "text_ln", None)
    state, tokens, scores = engine.beam_decode_lstm(
        frames, model.predictor._decode_bundle(), tl.weight if tl is not None else None, tl.bias if tl is not None else None,
        model.joint.joint_ln.weight, model.joint.joint_ln.bias, model.joint.blank_idx, max_length, beam, max_per_frame=m)
    torch.cuda.synchronize()
    st, tk, sc = state.cpu().numpy(), tokens.cpu().numpy(), scores.cpu().numpy()
    assert (st[:, 3] == 1).all(), st
    out = []
    for u in range(len(mels64)):
        n = st[u, 2]
        out.append((st[u].copy(), [tk[u, j, :1 + st[u, 8 + j]].copy() for j in range(n)], sc[u, :n].copy()))
    return out


def same_bits(a, b):
    return (np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
            and a[2].tobytes() == b[2].tobytes())


# ---- beam 1 is the device greedy decode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.GOLDENS)
def test_beam_1_gives_the_reference_modules_token_lists(name):
    fx = dc.load_golden(name)
    assert float(fx["gap"]) > dc.MARGIN
    model64, mel = dc.golden_model(fx)
    model = on_device(model64)
    got = search(model, mel, beam_size=1, max_length=int(fx["max_length"]))
    assert got[0][0] == fx["tokens"].tolist() and len(got) == 1


@pytest.mark.parametrize("case", dc.WIDTHS + dc.CONTROL, ids=[c.name for c in dc.WIDTHS + dc.CONTROL])
def test_beam_1_is_greedy_decode(case):
    model = device_model(case.name)
    mel = dc.case_frames(case).float().cuda()
    o = dc.greedy_oracle(bo.model_of(case.name), dc.case_frames(case), case.max_length)
    assert o.gap > dc.MARGIN
    want = model.greedy_decode(mel, _lens(mel), max_length=case.max_length)
    assert want == o.tokens and model.last_decode_path == "lstm_loop"
    assert model.beam_search(mel, _lens(mel), beam_size=1, max_length=case.max_length) == want
    assert model.last_beam_path == "lstm_device"


# ---- the oracle's lists and scores at the smallest shapes where the kernels can go wrong -----------------------------------------------
NAMES = ("wiring_text", "hd36_e20", "hd256", "hd260", "l3_noln", "blank_5")
CONFIGS = [(name, beam) for name in NAMES for beam in (2, 4, 16)]


@pytest.mark.parametrize("name,beam", CONFIGS, ids=[f"{n}-{b}" for n, b in CONFIGS])
def test_lists_and_scores_match_the_oracle(name, beam):
    T, seed = bo.SEEDS[(name, beam)]
    want = bo.checked(name, T, seed, beam)
    assert T <= 10
    got = search(device_model(name), bo.mel_of(name, T, seed), beam_size=beam)
    record(f"{name} beam {beam}", got, want)
    bo.assert_matches(got, want, (name, beam))


@pytest.mark.parametrize("key", list(bo.CAPS), ids=[f"{k[0]}-beam{k[1]}-ml{k[2]}-m{k[3]}" for k in bo.CAPS])
def test_caps_on_length_and_labels_per_frame(key):
    name, beam, ml, m = key
    T, seed = bo.CAPS[key]
    want = bo.checked(name, T, seed, beam, ml, m)
    got = search(device_model(name), bo.mel_of(name, T, seed), beam_size=beam, max_length=ml, max_symbols_per_frame=m)
    record(f"{name} beam {beam} max_length {ml} m {m}", got, want)
    bo.assert_matches(got, want, key)


# ---- nothing pruned: every sequence survives with its transducer likelihood ------------------------------------------------------------
TINY = dc._case("v4", None, V=4, O=8, E=8, Hd=8, L=2, seed=5)


@pytest.mark.parametrize("T,ml,m", [(3, 2, 2), (1, 3, 3), (2, 2, 3)])
def test_unpruned_scores_are_transducer_likelihoods(T, ml, m):
    """m >= max_length: every alignment ends each frame with a blank, so every sequence of <= max_length - 1 labels survives with score
    log P(y | x).  Sibling labels continue ONE parent state and merged hypotheses keep either: a wrong row shows here."""
    assert m >= ml
    model64 = dc.build_model(TINY)
    mel = dc.frames_of(TINY.H, T, 77 + T)
    om = bo.Model(model64, mel)
    _, pruned, _ = bo.beam_oracle.beam_search(om, 16, ml, m)
    assert pruned == 0
    got = search(on_device(model64), mel, beam_size=16, max_length=ml, max_symbols_per_frame=m)
    seqs = [list(y) for n in range(ml) for y in itertools.product(range(TINY.V - 1), repeat=n)]
    assert sorted(g[0] for g in got) == sorted(seqs)
    for y, s in got:
        want = -nll_bruteforce(bo.lattice_logits(om, y), y, T, len(y), om.blank)
        assert abs(s - want) <= 1e-5, (y, s, want)


# ---- a batch equals its utterances alone, bit for bit ----------------------------------------------------------------------------------
BATCH_BEAM = 4


@pytest.fixture(scope="module")
def batch():
    """The device model, the 33 mels (ragged, T = 1 next to the longest) and each utterance searched ALONE (computed once, never changed)."""
    model = device_model("wiring")
    mels = dc.batch_mels()
    alone = [raw(model, [mel], BATCH_BEAM)[0] for mel in mels]
    assert len({len(a[1][0]) for a in alone}) >= 4 and max(len(a[1][0]) for a in alone) >= 4  # best entries of several lengths
    return model, mels, alone


@pytest.mark.parametrize("n_utt", [1, 2, 3, 31, 32])  # half a row tile, one tile, a tile and a half, the limit
def test_batch_equals_alone_bitwise(batch, n_utt):
    model, mels, alone = batch
    for first in (0, 7):  # two positions of every utterance: the other half of a tile, another tile
        idx = [(first + k) % len(mels) for k in range(n_utt)]
        got = raw(model, [mels[i] for i in idx], BATCH_BEAM)
        for pos, i in enumerate(idx):
            assert same_bits(got[pos], alone[i]), (n_utt, first, pos, i)
    if n_utt >= 2:
        assert {dc.BATCH_T[i] for i in range(n_utt)} >= {1, max(dc.BATCH_T)}


def test_beam_search_many_groups_and_keeps_the_order(batch):
    model, mels, alone = batch
    dev_mels = [m.float().cuda() for m in mels]
    want = [model._nbest(a[0].tolist(), [row.tolist() + [0] for row in a[1]], a[2].tolist()) for a in alone]
    hosted = dc.BATCH_T.index(13)
    assert dc.BATCH_T.count(13) == 1
    on_host = model.beam_search(dev_mels[hosted], _lens(dev_mels[hosted]), beam_size=BATCH_BEAM, return_nbest=True, device_search=False)
    assert model.last_beam_path == "host"
    ok = model._beam_lstm_ok
    model._beam_lstm_ok = lambda audio, *a, **k: audio.shape[1] != 13 and ok(audio, *a, **k)  # one utterance forced to the host loop
    try:
        for b in (1, 5, 32):
            got = model.beam_search_many(dev_mels, beam_size=BATCH_BEAM, return_nbest=True, batch=b)
            assert model.last_beam_path == "lstm_device"
            for i, nb in enumerate(got):
                assert nb == (on_host if i == hosted else want[i]), (b, i)
        assert model.beam_search_many(dev_mels[:3], beam_size=BATCH_BEAM) == [w[0][0] for w in want[:3]]
    finally:
        del model._beam_lstm_ok
    with pytest.raises(ValueError):
        model.beam_search_many(dev_mels[:2], batch=33)


# ---- determinism, the workspace, live weights ------------------------------------------------------------------------------------------
def test_repeat_runs_and_a_nan_workspace_give_identical_bits():
    import rnnt_amd
    model = device_model("wiring_text")
    T, seed = bo.SEEDS[("wiring_text", 4)]
    mels = [bo.mel_of("wiring_text", T, seed), bo.mel_of("wiring_text", 3, 9), bo.mel_of("wiring_text", 9, 5)]
    a = raw(model, mels, 8)
    b = raw(model, mels, 8)
    assert all(same_bits(x, y) for x, y in zip(a, b))
    dev = torch.device("cuda", torch.cuda.current_device())
    ws = rnnt_amd.engine.workspace(dev, 1)  # the stream's cached scratch buffer the call will reuse
    ws.fill_(255)  # every float / double in it is a NaN
    torch.cuda.synchronize()
    c = raw(model, mels, 8)
    assert all(same_bits(x, y) for x, y in zip(a, c))


def test_parameters_are_read_live():
    """Nothing is cached on the module: a parameter changed in place between two calls changes the result, and changed back restores it."""
    model = on_device(bo.model_of("wiring"))
    T, seed = bo.SEEDS[("wiring", 4)]
    mel = bo.mel_of("wiring", T, seed)
    first = search(model, mel, beam_size=4)
    assert first[0][0]
    with torch.no_grad():
        bias = model.joint.joint_ln.bias.clone()  # (+ 1000 - 1000 does not give the fp32 value back)
        model.joint.joint_ln.bias[model.joint.blank_idx] += 1000.0
    assert search(model, mel, beam_size=4)[0] == ([], 0.0)  # (log_softmax of a logit 1000 above the rest is 0 in fp32)
    with torch.no_grad():
        model.joint.joint_ln.bias.copy_(bias)
        saved = model.predictor.lstm_layers[1].p2g.weight.clone()
        model.predictor.lstm_layers[1].p2g.weight.mul_(-3.0)
    changed = search(model, mel, beam_size=4)
    assert changed != first
    with torch.no_grad():
        model.predictor.lstm_layers[1].p2g.weight.copy_(saved)
    assert search(model, mel, beam_size=4) == first


# ---- the reference configuration's widths, once ----------------------------------------------------------------------------------------
def test_reference_widths():
    """S = 1024, E = 512, L = 3, Hd = 512, O = H = V = 1024: beam 1 is greedy_decode; beam 4 against the oracle at the frame seed found on the
    CPU among seeds 300 .. 399 (bo.REF_SEED)."""
    name = dc.REF_CASE.name
    model = device_model(name)
    mel64 = bo.mel_of(name, bo.REF_T, bo.REF_SEED)
    mel = mel64.float().cuda()
    assert model.beam_search(mel, _lens(mel), beam_size=1) == model.greedy_decode(mel, _lens(mel))
    assert model.last_beam_path == "lstm_device" and model.last_decode_path == "lstm_loop"
    want = bo.checked(name, bo.REF_T, bo.REF_SEED, bo.REF_BEAM)
    got = search(model, mel64, beam_size=bo.REF_BEAM)
    record(f"{name} beam {bo.REF_BEAM}", got, want)
    bo.assert_matches(got, want, name)
