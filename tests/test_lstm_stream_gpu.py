"""-m gpu: LSTM greedy streams that rest on the device (rnnt_engine_greedy_stream_lstm_*, rnnt_amd/csrc/lstm.hip; RNNTModel.greedy_streams;
DESIGN.md §4p "Device stream").

The contract: for every way of cutting each stream's frames into pushes, empty pushes and sit-outs included, after every push a
stream's token list is the greedy decode of its frames so far, and its LSTM state and text vector are BIT FOR BIT what the offline device
loop (engine.greedy_decode_lstm) returns for those frames alone — whatever the other streams do, whatever n, the slot and scan_frames.

Token lists are compared for EQUALITY with the float64 oracle of tests/lstm_decode_cases.py, under the premise — asserted at the head of
each test — that no decision of the float64 decode is closer than lstm_predictor_cases.DECODE_MARGIN.  The greedy decode is causal, so the
oracle's list for the first k frames is the labels it emitted at frames < k (`prefix`).  With RNNT_LSTM_STREAM_PARITY_OUT=<file> set the
float64 parity ratios are appended to that file (profiles/lstm_stream_parity.txt is such a run)."""
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


def offline(model, mel, max_length=200, max_per_frame=10, scan_frames=32):
    """engine.greedy_decode_lstm of one utterance (1, H, T): (tokens, state_out [L,2,Hd], text [H]) — the reference every stream is held to."""
    from rnnt_amd import engine
    frames = [model._decode_frames(mel.float().cuda().permute(0, 2, 1))]
    tl = getattr(model.joint, "text_ln", None)
    state, toks, state_out, text = engine.greedy_decode_lstm(
        frames, model.predictor._decode_bundle(), tl.weight if tl is not None else None, tl.bias if tl is not None else None,
        model.joint.joint_ln.weight, model.joint.joint_ln.bias, model.joint.blank_idx, max_length, max_per_frame=max_per_frame,
        scan_frames=scan_frames)
    text = text.clone()  # (a view of the workspace)
    torch.cuda.synchronize()
    st = state.cpu().numpy()
    assert st[0, 3] == 1 and st[0, 6] == 1 and st[0, 4] == 0, st
    return toks[0, 1:1 + st[0, 2]].tolist(), state_out[:, :, 0].cpu().numpy(), text[0].cpu().numpy()


def prefix(o, k):
    """The oracle's token list for the first k frames."""
    return o.tokens[:sum(o.per_frame[:k])]


def bits(group, i):
    state, text = group.lstm_state(i)
    return state.cpu().numpy(), text.cpu().numpy()


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def feed(group, mels, plans, oracles=None, slots=None, after=None, consumed=None):
    """Stream slots[j] (j) is pushed mels[j] (1, H, T; float32 on the device) in the chunk sizes plans[j] (None: sits that push out).  After
    every push every stream's token list is held to the oracle's for its frames so far; `after(step, at)` runs after each push.
    `consumed[j]`: the frames the stream had consumed before (0)."""
    slots = list(range(len(mels))) if slots is None else slots
    consumed = [0] * len(mels) if consumed is None else consumed
    at = [0] * len(mels)
    for step in range(max(len(p) for p in plans)):
        chunks = [None] * group.n
        for j, p in enumerate(plans):
            k = p[step] if step < len(p) else None
            if k is not None:
                chunks[slots[j]] = mels[j][..., at[j]:at[j] + k]
                at[j] += k
        before = [list(t) for t in group.tokens]
        new = group.push_encoded(chunks)
        assert group.last_path in (None, "lstm_stream")
        for j, s in enumerate(slots):
            assert before[s] + new[s] == group.tokens[s], (step, j)
            if oracles is not None:
                assert group.tokens[s] == prefix(oracles[j], at[j]), (step, j, at[j])
            if not group.done[s]:
                assert group.frames[s] == consumed[j] + at[j], (step, j)
        if after is not None:
            after(step, at)
    return at


def chunkings(T):
    uneven, left = [], T
    for k in [3, 0, 1, 4, 2, 0] * T:
        if left == 0:
            break
        uneven.append(min(k, left))
        left -= uneven[-1]
    out = {"ones": [1] * T, "uneven": uneven + [0], "all": [T], "two": [T // 2, T - T // 2]}
    assert all(sum(p) == T for p in out.values())
    return out


def case_group(case, model, n=1, **kw):
    return model.greedy_streams(n, max_length=case.max_length, max_symbols_per_frame=case.max_per_frame, device_loop=True, **kw)


# ---- chunk invariance ------------------------------------------------------------------------------------------------------------------
CASES = dc.WIDTHS + dc.CONTROL + [dc.WIRING_TEXT, dc.ALL_BLANK]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_chunk_invariance(case):
    o = dc.checked_oracle(case)  # the premise, on the CPU in float64
    model = on_device(dc.build_model(case))
    mel = dc.case_frames(case).float().cuda()
    want_tokens, want_state, want_text = offline(model, mel, case.max_length, case.max_per_frame)
    assert want_tokens == o.tokens
    for name, plan in chunkings(case.T).items():
        group = case_group(case, model)
        feed(group, [mel], [plan], [o])
        assert group.tokens[0] == o.tokens and group.last_path == "lstm_stream", name
        assert same_bits(bits(group, 0), (want_state, want_text)), name
        assert group.done[0] == (1 + len(o.tokens) >= case.max_length), name


# ---- the capped label, the cap, one frame ---------------------------------------------------------------------------------------------------
def test_a_label_capped_by_max_per_frame_is_taken_in_before_the_stream_rests():
    case = dc.BY_NAME["per_frame_2"]
    o = dc.checked_oracle(case)
    hit = [t for t, k in enumerate(o.per_frame) if k == case.max_per_frame]
    assert hit  # a push of one frame ends on a capped label
    model = on_device(dc.build_model(case))
    mel = dc.case_frames(case).float().cuda()
    group = case_group(case, model)

    def after(step, at):
        tokens, state, text = offline(model, mel[..., :at[0]], case.max_length, case.max_per_frame)
        assert tokens == group.tokens[0] and same_bits(bits(group, 0), (state, text)), step

    feed(group, [mel], [[1] * case.T], [o], after=after)
    assert group.tokens[0] == o.tokens


@pytest.mark.parametrize("name", ["cap_mid", "max_length_2"])
def test_done_rises_and_later_pushes_consume_nothing(name):
    case = dc.BY_NAME[name]
    o = dc.checked_oracle(case)
    model = on_device(dc.build_model(case))
    mel = dc.case_frames(case).float().cuda()
    _, want_state, want_text = offline(model, mel, case.max_length, case.max_per_frame)
    group = case_group(case, model, n=2)
    seen = []
    feed(group, [mel], [[1] * case.T], [o], slots=[1], after=lambda step, at: seen.append((group.done[1], group.frames[1])))
    first = next(i for i, (d, _) in enumerate(seen) if d)
    assert first < case.T - 1 and all(d and f == seen[first][1] for d, f in seen[first:])  # done before the last push; frames stay
    assert group.tokens[1] == o.tokens and same_bits(bits(group, 1), (want_state, want_text))
    snap = group._block.clone()
    assert group.push_encoded([None, mel[..., :3]]) == [[], []] and group.frames[1] == seen[first][1]
    assert torch.equal(snap, group._block)
    assert group.done == [False, True] and group.tokens[0] == []
    # the engine itself: a done stream handed frames next to a live one consumes nothing and keeps every bit
    from rnnt_amd import engine
    held = parts(group, 1)
    three = model._decode_frames(mel[..., :3].permute(0, 2, 1))
    tl = getattr(model.joint, "text_ln", None)
    out = torch.zeros(2, 3 * case.max_per_frame, dtype=torch.int32, device="cuda")
    engine.greedy_stream_lstm_push([three, three], model.predictor._decode_bundle(), tl.weight if tl is not None else None,
                                   tl.bias if tl is not None else None, model.joint.joint_ln.weight, model.joint.joint_ln.bias,
                                   model.joint.blank_idx, case.max_length, case.max_per_frame, 32, group._block, out)
    torch.cuda.synchronize()
    assert parts_equal(parts(group, 1), held)
    state = group._state.cpu()
    assert state[0, engine.LSTM_STREAM_FRAMES] == 3 and state[0, engine.LSTM_STREAM_AT_REST] == 1
    assert out[0, :state[0, engine.LSTM_STREAM_PUSH_LABELS]].tolist() == prefix(o, 3)


def test_one_frame_in_one_push():
    case = dc.BY_NAME["t1"]
    o = dc.checked_oracle(case)
    model = on_device(dc.build_model(case))
    mel = dc.case_frames(case).float().cuda()
    group = case_group(case, model)
    feed(group, [mel], [[1]], [o])
    assert same_bits(bits(group, 0), offline(model, mel, case.max_length, case.max_per_frame)[1:]) and group.frames == [1]


# ---- scan_frames ----------------------------------------------------------------------------------------------------------------------
def test_scan_frames_do_not_change_a_push():
    from rnnt_amd import engine
    o = dc.batch_oracles()[0]
    mel = dc.batch_mels()[0].float().cuda()
    T = mel.shape[-1]
    assert T == 23 and T % 5 != 0 and T < 32  # more than one scan block inside the push at 1 and 5, a count 5 does not divide
    model = on_device(lc.wiring_model())
    want = offline(model, mel)
    assert want[0] == o.tokens
    iters = {}
    for scan in (1, 5, 32):
        group = model.greedy_streams(1, scan_frames=scan, device_loop=True)
        feed(group, [mel], [[T]], [o])
        assert same_bits(bits(group, 0), want[1:]), scan
        iters[scan] = int(group._state[0, engine.LSTM_STREAM_PUSH_ITERATIONS])
        assert iters[scan] <= T * 10 + -(-T // scan) + 1, (scan, iters)  # the header's bound
    assert iters[1] > iters[5] > iters[32], iters


# ---- lockstep --------------------------------------------------------------------------------------------------------------------------
def plan_of(u, T):
    """Stream u's chunking of T frames: sizes 0 .. 5 and sit-outs, a late start for every third stream."""
    rng = np.random.default_rng(1000 + u)
    plan, left = [None] * (u % 3), T
    while left > 0:
        k = [None, 0, 1, 2, 3, 5][int(rng.integers(0, 6))]
        k = None if k is None else min(k, left)
        plan.append(k)
        left -= k or 0
    return plan


@pytest.fixture(scope="module")
def batch():
    """The device model, the 33 mels on the device, their oracles, and each utterance streamed ALONE in a group of one, all frames in one
    push (computed once, never changed)."""
    oracles = dc.batch_oracles()
    model = on_device(lc.wiring_model())
    mels = [m.float().cuda() for m in dc.batch_mels()]
    alone = []
    for u, (m, o) in enumerate(zip(mels, oracles)):
        g = model.greedy_streams(1, device_loop=True)
        feed(g, [m], [[m.shape[-1]]], [o])
        alone.append((g.tokens[0], bits(g, 0)))
    return model, mels, oracles, alone


@pytest.mark.parametrize("n", dc.BATCH_SIZES)
def test_lockstep_equals_each_stream_alone(batch, n):
    model, mels, oracles, alone = batch
    if n >= 2:
        assert mels[1].shape[-1] == 1 and mels[0].shape[-1] == max(m.shape[-1] for m in mels)  # T = 1 next to the longest
    plans = [plan_of(u, mels[u].shape[-1]) for u in range(n)]
    if n >= 2:  # streams finishing at different pushes; sit-outs; in the large groups empty pushes too
        assert len({len(p) for p in plans}) > 1 and any(None in p for p in plans) and (n < 31 or any(0 in p for p in plans))
    group = model.greedy_streams(n, device_loop=True)
    feed(group, mels[:n], plans, oracles[:n])
    for u in range(n):
        assert group.tokens[u] == alone[u][0] and same_bits(bits(group, u), alone[u][1]), u
    # every utterance in another slot (n = 1: another utterance), with the chunkings reassigned
    order = list(range(n - 1, -1, -1)) if n > 1 else [dc.MAX_UTT]
    moved = model.greedy_streams(n, device_loop=True)
    feed(moved, [mels[u] for u in order], [plan_of(k, mels[u].shape[-1]) for k, u in enumerate(order)], [oracles[u] for u in order])
    for k, u in enumerate(order):
        assert moved.tokens[k] == alone[u][0] and same_bits(bits(moved, k), alone[u][1]), (k, u)


def parts(group, i):
    """Clones of stream i's part of the block: its words, its h and c rows, its text vector."""
    return group._state[i].clone(), group._hc[:, :, i].clone(), group._text[i].clone()


def parts_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_reset_restarts_one_slot_and_touches_no_other(batch):
    model, mels, oracles, alone = batch
    group = model.greedy_streams(3, device_loop=True)
    feed(group, [mels[0], mels[2], mels[3]], [[7], [4], [5]], [oracles[0], oracles[2], oracles[3]])  # mid-utterance, all three
    assert group.frames == [7, 4, 5]
    others = [parts(group, 0), parts(group, 2)]
    group.reset(1)
    assert group.tokens[1] == [] and group.frames[1] == 0 and not group.done[1]
    assert parts_equal(parts(group, 0), others[0]) and parts_equal(parts(group, 2), others[1])
    fresh = model.greedy_streams(3, device_loop=True)
    assert parts_equal(parts(group, 1), parts(fresh, 1))  # the slot is a started stream's, bit for bit
    feed(group, [mels[5]], [[3, 0, mels[5].shape[-1] - 3]], [oracles[5]], slots=[1])  # another utterance in slot 1
    assert group.tokens[1] == alone[5][0] and same_bits(bits(group, 1), alone[5][1])
    assert parts_equal(parts(group, 0), others[0]) and parts_equal(parts(group, 2), others[1])
    at = feed(group, [mels[0][..., 7:], mels[3][..., 5:]], [[16], [9]], slots=[0, 2], consumed=[7, 5])  # the others go on from where they were
    assert group.tokens[0] == alone[0][0] and group.tokens[2] == alone[3][0] and at == [16, 9]
    assert same_bits(bits(group, 0), alone[0][1]) and same_bits(bits(group, 2), alone[3][1])


def test_a_stream_that_sits_out_keeps_every_bit(batch):
    model, mels, oracles, _ = batch
    group = model.greedy_streams(3, device_loop=True)
    started = parts(group, 2)
    feed(group, [mels[0], mels[3]], [[6], [2]], [oracles[0], oracles[3]])  # slot 2 not started yet: its start blank still waits
    assert parts_equal(parts(group, 2), started)
    held = parts(group, 1)
    feed(group, [mels[0][..., 6:], mels[5]], [[5, 5], [3, 3]], slots=[0, 2], consumed=[6, 0])  # slot 1 sits two pushes out, mid-utterance
    assert parts_equal(parts(group, 1), held)
    assert group.frames == [16, 2, 6]
    assert group.tokens[2] == prefix(oracles[5], 6) and group.tokens[0] == prefix(oracles[0], 16)


def test_the_workspace_holds_nothing_between_pushes(batch):
    from rnnt_amd import engine
    model, mels, oracles, alone = batch
    ws = engine.workspace(torch.device("cuda", torch.cuda.current_device()), 1)
    assert ws.numel() > 1  # the buffer the pushes above used
    group = model.greedy_streams(4, device_loop=True)
    plans = [plan_of(u, mels[u].shape[-1]) for u in range(4)]
    feed(group, mels[:4], plans, oracles[:4], after=lambda step, at: ws.fill_(0xFF))  # NaNs wherever a float is read before it is written
    for u in range(4):
        assert group.tokens[u] == alone[u][0] and same_bits(bits(group, u), alone[u][1]), u


def test_two_runs_give_the_same_bits(batch):
    model, mels, oracles, _ = batch
    runs = []
    for _ in range(2):
        group = model.greedy_streams(5, device_loop=True)
        feed(group, mels[:5], [plan_of(u, mels[u].shape[-1]) for u in range(5)], oracles[:5])
        runs.append((group.tokens, group._block.clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])


# ---- the single stream -----------------------------------------------------------------------------------------------------------------
def test_single_stream_is_a_device_group_of_one(monkeypatch):
    from rnnt_amd import engine
    model64, mel64 = lc.wiring_model(), lc.decode_frames()
    o = dc.greedy_oracle(model64, mel64, 200)
    assert o.gap > dc.MARGIN and len(o.tokens) >= 10
    model = on_device(model64)
    mel = mel64.float().cuda()
    T = mel.shape[-1]
    want = model.greedy_decode(mel, torch.tensor([T]).cuda(), device_loop=True)
    assert want == o.tokens
    assert model.greedy_stream().push_encoded(mel) == want and model.greedy_stream()._group is None  # the default stays the host loop
    stream = model.greedy_stream(device_loop=True)
    assert stream._group is not None and stream._host is None
    syncs = []
    real_cpu, real_tolist, real_item = torch.Tensor.cpu, torch.Tensor.tolist, torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (syncs.append("cpu") if t.is_cuda else None, real_cpu(t, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "tolist", lambda t: (syncs.append("tolist") if t.is_cuda else None, real_tolist(t))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda t: (syncs.append("item") if t.is_cuda else None, real_item(t))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: syncs.append("synchronize"))
    got = []
    for t in range(T):
        syncs.clear()
        new = stream.push_encoded(mel[..., t:t + 1])
        assert syncs == ["cpu"], (t, syncs)  # one device-to-host copy, the push's one synchronisation
        got += new
        assert got == prefix(o, t + 1) and stream.frames == t + 1 and stream.last_path == "lstm_stream"
    monkeypatch.undo()
    assert got == stream.tokens == want and not stream.done
    assert stream.push_encoded(mel[..., :0]) == []
    # a one-frame push needs one iteration, two when it emitted (the second takes the label in)
    assert int(stream._group._state[0, engine.LSTM_STREAM_PUSH_ITERATIONS]) == (2 if o.per_frame[T - 1] else 1)
    assert same_bits([x.cpu().numpy() for x in stream.lstm_state()], offline(model, mel)[1:])
    # device_loop=None: the device from the group size on at which it beat the host loops at every timed shape
    low = type(stream._group).DEVICE_MIN_STREAMS
    assert model.greedy_streams(low)._on_device and model.greedy_streams(32)._on_device and not model.greedy_streams(low - 1)._on_device
    assert not model.greedy_streams(low, device_loop=False)._on_device
    model.predictor.backend = "torch"
    with pytest.raises(RuntimeError, match="device_loop=True"):
        model.greedy_stream(device_loop=True)
    assert model.greedy_streams(8).last_path is None and not model.greedy_streams(8)._on_device  # the host path, quietly, unless forced


# ---- the reference configuration's widths ------------------------------------------------------------------------------------------------
def test_reference_widths_in_16_frame_pushes():
    case = dc.REF_CASE
    model64 = dc.build_model(case)
    mels64 = [dc.frames_of(case.H, case.T, s) for s in dc.REF_FRAME_SEEDS]
    oracles = [dc.greedy_oracle(model64, m, 200) for m in mels64]
    assert all(o.gap > dc.MARGIN for o in oracles), [o.gap for o in oracles]
    model = on_device(model64)
    mels = [m.float().cuda() for m in mels64]
    want = [offline(model, m) for m in mels]
    assert [w[0] for w in want] == [o.tokens for o in oracles]
    group = model.greedy_streams(4, max_length=200, device_loop=True)  # (the oracles' cap: these utterances reach it)
    feed(group, mels, [[16] * (case.T // 16)] * 4, oracles)
    for u in range(4):
        assert group.tokens[u] == want[u][0] and same_bits(bits(group, u), want[u][1:]), u


# ---- accuracy against float64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text", [False, True], ids=["wiring", "wiring_text"])
def test_state_and_text_vector_against_float64(text):
    """The bar of test_lstm_decode_gpu.py::test_state_and_text_vector_parity: 4 x the fp32 torch path's own error replaying the same tokens,
    errors relative to the float64 tensor's largest entry."""
    if text:
        model64, mel64, o = dc.build_model(dc.WIRING_TEXT), dc.case_frames(dc.WIRING_TEXT), dc.checked_oracle(dc.WIRING_TEXT)
    else:
        model64, mel64 = lc.wiring_model(), lc.decode_frames()
        o = dc.greedy_oracle(model64, mel64, 200)
        assert o.gap > dc.MARGIN
    group = on_device(model64).greedy_streams(1, device_loop=True)
    T = mel64.shape[-1]
    feed(group, [mel64.float().cuda()], [chunkings(T)["uneven"]], [o])
    assert group.tokens[0] == o.tokens
    state64, text64 = dc.replay(model64, o.tokens)
    s32, t32 = dc.replay(copy.deepcopy(model64).float(), o.tokens)
    bar = 4.0 * max(lc.rel_err(s32, state64), lc.rel_err(t32, text64))
    got_state, got_text = bits(group, 0)
    errs = {"state": lc.rel_err(got_state[:, :, None], state64), "text": lc.rel_err(got_text, text64)}
    tag = "wiring_text" if text else "wiring"
    lines = [f"{tag:14s} {k:6s} err {e:.3e}  bar {bar:.3e}  ratio {e / bar:.3f}" for k, e in errs.items()]
    print("\n".join(lines))
    path = os.environ.get("RNNT_LSTM_STREAM_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")
    assert max(errs.values()) <= bar, lines
