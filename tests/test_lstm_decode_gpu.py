"""-m gpu: the device-resident greedy decode of LSTMPredictor models (rnnt_engine_greedy_decode_lstm, rnnt_amd/csrc/lstm.hip; DESIGN.md
§4p "Device decode") against the float64 torch path of the same modules driven by the greedy control flow (tests/lstm_decode_cases.py).

Token lists are compared for EQUALITY, under the premise — asserted at the head of each test — that no decision of the float64 decode
is closer than lstm_predictor_cases.DECODE_MARGIN.  An utterance's tokens, state words and state_out rows in a batch are compared for
bit equality with the same utterance decoded alone.  state_out and the text vector are held to float64 with the error relative to
the float64 tensor's largest entry and a bar of 4 x the error of the fp32 torch path on the same case (test_lstm_predictor_gpu.py's
rule).  With RNNT_LSTM_DECODE_PARITY_OUT=<file> set every measured ratio is appended to that file (profiles/lstm_decode_parity.txt is
such a run)."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import lstm_decode_cases as dc
from tests import lstm_predictor_cases as lc

pytestmark = pytest.mark.gpu


def on_device(model64):
    return copy.deepcopy(model64).float().cuda().eval()


def loop(model, mels, max_length=200, max_per_frame=10, scan_frames=32):
    """engine.greedy_decode_lstm of the mels (each (1, H, T), any dtype) on the device model: tokens per utterance, the state words, state_out
    [L,2,N,Hd] and the text vectors [N,H] as numpy arrays."""
    from rnnt_amd import engine
    frames = [model._decode_frames(model.encoder(m.float().cuda()).permute(0, 2, 1)) for m in mels]
    tl = getattr(model.joint, "text_ln", None)
    state, toks, state_out, text = engine.greedy_decode_lstm(
        frames, model.predictor._decode_bundle(), tl.weight if tl is not None else None, tl.bias if tl is not None else None,
        model.joint.joint_ln.weight, model.joint.joint_ln.bias, model.joint.blank_idx, max_length, max_per_frame=max_per_frame,
        scan_frames=scan_frames)
    text = text.clone()  # (a view of the workspace)
    torch.cuda.synchronize()
    st, tk = state.cpu().numpy(), toks.cpu().numpy()
    assert (st[:, 3] == 1).all() and (st[:, 6] == 1).all() and (st[:, 4] == 0).all(), st  # every utterance ended and settled
    assert (tk[:, 0] == model.joint.blank_idx).all()
    return dict(tokens=[tk[u, 1:1 + st[u, 2]].tolist() for u in range(len(mels))], state=st, state_out=state_out.cpu().numpy(),
                text=text.cpu().numpy())


def case_loop(case, **kw):
    o = dc.checked_oracle(case)  # the premise, on the CPU in float64
    model = on_device(dc.build_model(case))
    got = loop(model, [dc.case_frames(case)], max_length=case.max_length, max_per_frame=case.max_per_frame, **kw)
    return o, got


def parity(tag, case_model64, o, got, u=0):
    """state_out and the text vector of utterance u against float64, bar 4 x the fp32 torch path's error replaying the same tokens."""
    s32, t32 = dc.replay(copy.deepcopy(case_model64).float(), o.tokens)
    bar = 4.0 * max(lc.rel_err(s32, o.state), lc.rel_err(t32, o.text))
    errs = {"state_out": lc.rel_err(got["state_out"][:, :, u:u + 1], o.state), "text": lc.rel_err(got["text"][u], o.text)}
    lines = [f"{tag:28s} {k:10s} err {e:.3e}  bar {bar:.3e}  ratio {e / bar:.3f}" for k, e in errs.items()]
    print("\n".join(lines))
    path = os.environ.get("RNNT_LSTM_DECODE_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")
    assert max(errs.values()) <= bar, lines


# ---- model wiring --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text", [False, True], ids=["plain", "text_ln"])
def test_model_wiring(text):
    if text:
        model64, mel64 = dc.build_model(dc.WIRING_TEXT), dc.case_frames(dc.WIRING_TEXT)
        want = dc.checked_oracle(dc.WIRING_TEXT).tokens
    else:
        model64, mel64 = lc.wiring_model(), lc.decode_frames()
        o = dc.greedy_oracle(model64, mel64, 200)
        assert o.gap > dc.MARGIN and len(o.tokens) >= 10
        want = o.tokens
    model = on_device(model64)
    mel = mel64.float().cuda()
    lens = torch.tensor([mel.shape[-1]]).cuda()
    assert model.last_decode_path is None and model._device_loop_ok(mel.permute(0, 2, 1))
    model.predictor.last_backend = None
    assert model.greedy_decode(mel, lens, device_loop=True) == want
    assert model.last_decode_path == "lstm_loop" and model.predictor.last_backend == "engine"
    assert model.greedy_decode(mel, lens, device_loop=False) == want and model.last_decode_path == "host"
    assert model.greedy_decode(mel, lens) == want and model.last_decode_path == dc.DEFAULT_PATH
    with pytest.raises(RuntimeError, match="persistent"):
        model.greedy_decode(mel, lens, device_loop=True, persistent=True)
    assert model.greedy_decode(mel, lens, max_length=1, device_loop=True) == []
    # the torch backend, training mode with dropout and other dtypes keep the host loop; asking for the device loop is then an error
    model.predictor.backend = "torch"
    assert not model._device_loop_ok(mel.permute(0, 2, 1))
    with pytest.raises(RuntimeError, match="device_loop=True"):
        model.greedy_decode(mel, lens, device_loop=True)
    assert model.greedy_decode(mel, lens) == want and model.last_decode_path == "host" and model.predictor.last_backend == "torch"
    model.predictor.backend = "auto"
    model.predictor.train()
    assert not model._device_loop_ok(mel.permute(0, 2, 1))
    model.predictor.dropout.p = 0.0
    assert model._device_loop_ok(mel.permute(0, 2, 1)) and not model._device_loop_ok(mel.double().permute(0, 2, 1))


@pytest.mark.parametrize("name", dc.GOLDENS)
def test_reference_modules_token_lists(name):
    fx = dc.load_golden(name)
    assert float(fx["gap"]) > dc.MARGIN
    model64, mel = dc.golden_model(fx)
    got = loop(on_device(model64), [mel], max_length=int(fx["max_length"]))
    assert got["tokens"][0] == fx["tokens"].tolist()


# ---- widths and control flow ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.WIDTHS + dc.CONTROL, ids=[c.name for c in dc.WIDTHS + dc.CONTROL])
def test_widths_and_control_flow(case):
    o, got = case_loop(case)
    assert got["tokens"][0] == o.tokens
    assert got["state"][0, 2] == len(o.tokens)
    parity(case.name, dc.build_model(case), o, got)


def test_all_blank_utterance():
    """No label: the list is empty and state_out is the state after the start blank."""
    o, got = case_loop(dc.ALL_BLANK)
    assert got["tokens"][0] == [] == o.tokens and got["state"][0, 0] == dc.ALL_BLANK.T
    start_state, _ = dc.replay(dc.build_model(dc.ALL_BLANK), [])
    assert lc.rel_err(o.state, start_state) < 1e-12
    parity("all_blank", dc.build_model(dc.ALL_BLANK), o, got)
    assert got["state"][0, 5] == 1  # one block of 32 frames saw them all


def test_scan_frames_do_not_change_the_decode():
    model64, mel = lc.wiring_model(), lc.decode_frames()
    o = dc.greedy_oracle(model64, mel, 200)
    assert o.gap > dc.MARGIN and mel.shape[-1] % 5 != 0 and mel.shape[-1] < 32
    model = on_device(model64)
    runs = {n: loop(model, [mel], scan_frames=n) for n in dc.SCAN_FRAMES}
    for n, got in runs.items():
        assert got["tokens"][0] == o.tokens, n
        assert np.array_equal(got["state"][:, :4], runs[32]["state"][:, :4]), n
        assert np.array_equal(got["state_out"], runs[32]["state_out"]) and np.array_equal(got["text"], runs[32]["text"]), n
    assert runs[1]["state"][0, 5] > runs[32]["state"][0, 5]  # a frame per iteration took more iterations


# ---- batches -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch():
    """The device model, the 33 mels, their oracles and each utterance decoded ALONE (computed once, never changed)."""
    oracles = dc.batch_oracles()
    model = on_device(lc.wiring_model())
    mels = dc.batch_mels()
    alone = [loop(model, [m]) for m in mels]
    for u, (a, o) in enumerate(zip(alone, oracles)):
        assert a["tokens"][0] == o.tokens, u
    return model, mels, oracles, alone


def same_as_alone(got, k, alone_u):
    return (got["tokens"][k] == alone_u["tokens"][0] and np.array_equal(got["state"][k, :4], alone_u["state"][0, :4])
            and np.array_equal(got["state_out"][:, :, k], alone_u["state_out"][:, :, 0]) and np.array_equal(got["text"][k], alone_u["text"][0]))


@pytest.mark.parametrize("n_utt", dc.BATCH_SIZES)
def test_batch_equals_each_utterance_alone(batch, n_utt):
    model, mels, oracles, alone = batch
    if n_utt >= 2:
        assert mels[1].shape[-1] == 1 and mels[0].shape[-1] == max(m.shape[-1] for m in mels)  # T = 1 next to the longest
    got = loop(model, mels[:n_utt])
    for u in range(n_utt):
        assert got["tokens"][u] == oracles[u].tokens, u
        assert same_as_alone(got, u, alone[u]), u
    order = list(range(n_utt - 1, -1, -1)) if n_utt > 1 else [dc.MAX_UTT]  # every utterance at another position (alone: another one)
    moved = loop(model, [mels[u] for u in order])
    for k, u in enumerate(order):
        assert same_as_alone(moved, k, alone[u]), (k, u)


def test_greedy_decode_many_groups_and_order(batch, monkeypatch):
    """33 utterances the device loop takes and one it refuses (float64 features): two groups of 32 and 1 in input order, the refused
    one on the host loop, the results in input order."""
    from rnnt_amd import engine
    model, mels, oracles, _ = batch
    mels_dev = [m.float().cuda() for m in mels]
    at = 7
    refused = mels[3].double().cuda()
    assert not model._device_loop_ok(refused.permute(0, 2, 1))
    inputs = mels_dev[:at] + [refused] + mels_dev[at:]
    want = [o.tokens for o in oracles[:at]] + [oracles[3].tokens] + [o.tokens for o in oracles[at:]]
    groups, real = [], engine.greedy_decode_lstm
    monkeypatch.setattr(engine, "greedy_decode_lstm", lambda frames, *a, **kw: (groups.append(len(frames)), real(frames, *a, **kw))[1])
    assert model.greedy_decode_many(inputs) == want
    assert groups == [32, 1] and model.last_decode_path == "lstm_loop"
    groups.clear()
    assert model.greedy_decode_many(inputs[:10], batch=4) == want[:10] and groups == [4, 4, 1]
    groups.clear()
    assert model.greedy_decode_many([refused]) == [oracles[3].tokens] and groups == [] and model.last_decode_path == "host"


# ---- state, reproducibility, live weights ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text", [False, True], ids=["plain", "text_ln"])
def test_state_and_text_vector_parity(text):
    if text:
        model64, mel, o = dc.build_model(dc.WIRING_TEXT), dc.case_frames(dc.WIRING_TEXT), dc.checked_oracle(dc.WIRING_TEXT)
    else:
        model64, mel = lc.wiring_model(), lc.decode_frames()
        o = dc.greedy_oracle(model64, mel, 200)
        assert o.gap > dc.MARGIN
    got = loop(on_device(model64), [mel])
    assert got["tokens"][0] == o.tokens
    parity("wiring_text" if text else "wiring", model64, o, got)


def test_reproducible_with_a_poisoned_workspace(batch):
    from rnnt_amd import engine
    model, mels, oracles, _ = batch
    first = loop(model, mels[:5])
    ws = engine.workspace(torch.device("cuda", torch.cuda.current_device()), 1)
    assert ws.numel() > 1  # the buffer the call above used
    ws.fill_(0xFF)  # NaNs wherever a float is read before it is written
    second = loop(model, mels[:5])
    assert first["tokens"] == second["tokens"] == [o.tokens for o in oracles[:5]]
    for k in ("state", "state_out", "text"):
        assert np.array_equal(first[k], second[k]), k


def test_live_weights():
    """Parameters changed in place between two decodes (no version counter sees `.data` writes): the second decode reads the new ones."""
    model64, mel = lc.wiring_model(), lc.decode_frames()
    before = dc.greedy_oracle(model64, mel, 200)
    model = on_device(model64)
    assert loop(model, [mel])["tokens"][0] == before.tokens
    for m in (model64, model):
        m.predictor.linear.weight.data.mul_(2.0)
    after = dc.greedy_oracle(model64, mel, 200)
    assert before.gap > dc.MARGIN and after.gap > dc.MARGIN and after.tokens != before.tokens
    lens = torch.tensor([mel.shape[-1]]).cuda()
    assert model.greedy_decode(mel.float().cuda(), lens, device_loop=True) == after.tokens


# ---- the reference configuration's widths ------------------------------------------------------------------------------------------------
def test_reference_widths():
    """3 x 512, E = 512, H = V = 1024, T = 64, four utterances in one loop: held to the fp32 torch path's own decode, under the margin
    premise computed in float64."""
    case = dc.REF_CASE
    model64 = dc.build_model(case)
    mels = [dc.frames_of(case.H, case.T, s) for s in dc.REF_FRAME_SEEDS]
    oracles = [dc.greedy_oracle(model64, m, 200) for m in mels]
    assert all(o.gap > dc.MARGIN for o in oracles), [o.gap for o in oracles]
    model32 = copy.deepcopy(model64).float()
    want = [dc.greedy_oracle(model32, m.float(), 200).tokens for m in mels]
    assert want == [o.tokens for o in oracles]
    model = on_device(model64)
    got = loop(model, mels)
    assert got["tokens"] == want
    alone = loop(model, [mels[2]])
    assert same_as_alone(got, 2, alone)
    parity("reference widths", model64, oracles[0], got)
