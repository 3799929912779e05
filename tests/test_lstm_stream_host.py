"""CPU tests (float64) of RNNTModel.greedy_streams / GreedyStreamGroup on its host path, and of what the new `device_loop` argument leaves
as it was: for every way of cutting each stream's frames into pushes — empty pushes and sit-outs (None) included — a stream's token
list after every push equals greedy_decode of the frames it has been pushed so far."""
import pytest
import torch

from tests import lstm_decode_cases as dc
from tests import lstm_predictor_cases as lc
from tests.stream_models import PassThroughEncoder, TorchConvPredictor

T = lc.DECODE_FRAMES
UNEVEN = [3, 0, 1, 4, 2, 0, 3, 1]
CHUNKINGS = {"ones": [1] * T, "uneven": UNEVEN, "all": [T], "two": [T // 2, T - T // 2]}
assert sum(UNEVEN) == T and 0 in UNEVEN


def conv_model():
    """A stateless-predictor model (the reference's ConvPredictor in plain torch), seeded, float64, eval mode."""
    import rnnt_amd
    torch.manual_seed(3)
    V, O, E = 16, 32, 16
    joint = rnnt_amd.JointNetwork(-1, -1, O, V)
    with torch.no_grad():
        joint.joint_ln.bias[-1] += 1.0
    return rnnt_amd.RNNTModel(TorchConvPredictor(V, O, E), PassThroughEncoder(), joint).double().eval()


MODELS = {"lstm": lc.wiring_model, "conv": conv_model}


def so_far(model, mel, k, max_length=200):
    if k == 0:
        return []
    return model.greedy_decode(mel[..., :k], torch.tensor([k]), max_length=max_length)


def feed(group, mels, plans, max_length=200, model=None, at=None):
    """Push stream i's frames in the chunk sizes plans[i] (None: sits that push out) from frame at[i] (0); after every push every
    stream is held to greedy_decode of its frames so far."""
    at = [0] * group.n if at is None else list(at)
    for step in range(max(len(p) for p in plans)):
        chunks = []
        for i, p in enumerate(plans):
            k = p[step] if step < len(p) else None
            chunks.append(None if k is None else mels[i][..., at[i]:at[i] + k])
            at[i] += k or 0
        before = [list(t) for t in group.tokens]
        new = group.push_encoded(chunks)
        for i in range(group.n):
            assert before[i] + new[i] == group.tokens[i], (step, i)
            assert group.tokens[i] == so_far(model, mels[i], at[i], max_length), (step, i)
            if not group.done[i]:
                assert group.frames[i] == at[i], (step, i)


@pytest.mark.parametrize("kind", list(MODELS))
@pytest.mark.parametrize("chunking", list(CHUNKINGS))
def test_one_stream_every_chunking(kind, chunking):
    model, mel = MODELS[kind](), lc.decode_frames()
    want = so_far(model, mel, T)
    assert len(want) >= 4
    group = model.greedy_streams(1)
    feed(group, [mel], [CHUNKINGS[chunking]], model=model)
    assert group.tokens[0] == want and group.last_path == "host" and group.frames == [T] and group.done == [False]


@pytest.mark.parametrize("kind", list(MODELS))
def test_streams_with_sit_outs_and_different_chunkings(kind):
    model = MODELS[kind]()
    mels = [lc.decode_frames()] + [m for m in dc.batch_mels()[:3]]
    Ts = [m.shape[-1] for m in mels]
    assert Ts[2] == 1  # a one-frame stream next to the longest
    plans = [[1] * Ts[0], [None, 5, 0, None, 9, 9], [None, None, 1], [Ts[3]]]
    assert all(sum(k or 0 for k in p) == t for p, t in zip(plans, Ts))
    group = model.greedy_streams(4)
    feed(group, mels, plans, model=model)
    assert group.tokens == [so_far(model, m, t) for m, t in zip(mels, Ts)] and group.last_path == "host"
    assert group.push_encoded([None] * 4) == [[], [], [], []]


@pytest.mark.parametrize("kind", list(MODELS))
def test_cap_reset_and_unbounded(kind):
    model, mel = MODELS[kind](), lc.decode_frames()
    full = so_far(model, mel, T)
    assert len(full) > 5
    group = model.greedy_streams(2, max_length=5)
    feed(group, [mel, mel], [[1] * T, [T]], max_length=5, model=model)
    assert group.done == [True, True] and group.tokens[0] == group.tokens[1] == full[:4]
    frames = list(group.frames)
    assert group.push_encoded([mel[..., :3], None]) == [[], []] and group.frames == frames
    group.reset(0)
    assert group.tokens[0] == [] and group.frames[0] == 0 and group.done == [False, True] and group.tokens[1] == full[:4]
    feed(group, [mel, mel], [[4, T - 4], [None, None]], max_length=5, model=model, at=[0, T])
    assert group.tokens[0] == full[:4]
    assert model.greedy_streams(1, max_length=1).push_encoded([mel]) == [[]]  # (the reference's loop never runs)
    unbounded = model.greedy_streams(1, max_length=None)
    unbounded.push_encoded([mel])
    assert unbounded.tokens[0] == full


def test_arguments_are_checked():
    model = lc.wiring_model()
    for n in (0, 33, -1):
        with pytest.raises(ValueError, match="outside"):
            model.greedy_streams(n)
    assert model.greedy_streams(32).n == 32
    with pytest.raises(ValueError, match="max_symbols_per_frame"):
        model.greedy_streams(1, max_symbols_per_frame=0)
    with pytest.raises(RuntimeError, match="device_loop=True"):
        model.greedy_streams(2, device_loop=True)
    with pytest.raises(RuntimeError, match="device_loop=True"):
        conv_model().greedy_streams(2, device_loop=True)
    with pytest.raises(RuntimeError, match="device_loop=True"):
        model.greedy_stream(device_loop=True)
    group = model.greedy_streams(2)
    with pytest.raises(ValueError, match="2 chunks"):
        group.push_encoded([None])
    with pytest.raises(ValueError, match=r"\(1, C, n\)"):
        group.push_encoded([torch.zeros(2, 32, 1, dtype=torch.float64), None])


def test_host_state_aid_and_max_symbols():
    """lstm_state on the host path is the predictor's state after the labels so far; max_symbols_per_frame reaches the host loops."""
    model, mel = lc.wiring_model(), lc.decode_frames()
    group = model.greedy_streams(1)
    group.push_encoded([mel])
    state, text = group.lstm_state(0)
    want_state, want_text = dc.replay(model, group.tokens[0])
    assert state.shape == (2, 2, 32) and lc.rel_err(state.numpy()[:, :, None], want_state) < 1e-12
    assert lc.rel_err(text.numpy(), want_text) < 1e-12
    case = dc.BY_NAME["per_frame_2"]
    o = dc.checked_oracle(case)
    capped = dc.build_model(case).greedy_streams(1, max_symbols_per_frame=case.max_per_frame)
    capped.push_encoded([dc.case_frames(case)])
    assert capped.tokens[0] == o.tokens


def test_default_single_stream_of_an_lstm_model_is_the_host_stream():
    model, mel = lc.wiring_model(), lc.decode_frames()
    s = model.greedy_stream()
    got = []
    for t in range(T):
        got += s.push_encoded(mel[..., t:t + 1])
    assert got == s.tokens == so_far(model, mel, T) and s.last_path == "host" and s._host is not None and s._group is None
    forced = model.greedy_stream(device_loop=False)
    forced.push_encoded(mel)
    assert forced.tokens == got and forced.last_path == "host"
