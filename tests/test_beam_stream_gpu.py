"""-m gpu: RNNTModel.beam_stream / beam_streams on the device (rnnt_engine_beam_stream_push).  The definition everything
is held to: after any sequence of pushes that delivered frames 0 .. k-1, the stream's n-best list IS beam_search(frames[:k]) — the same
token lists and the same float64 scores — and both are held to the float64 oracle of the search (tests/beam_oracle.py)."""
import numpy as np
import pytest
import torch

from tests import beam_oracle
from tests.helpers import DECODE_CASES, load_decode_case
from tests.stream_models import StreamingCausalEncoder, engine_model, partitions
from tests.test_decode_gpu import build_model

pytestmark = pytest.mark.gpu

GAP = 1e-3  # smallest oracle score gap at a keep / drop boundary for which identical n-best lists are demanded
CHUNKINGS = ("1", "3", "7", "17", "all", "random")

_cases = {}


def _case(golden_dir, name):
    """(fixture, engine model, frames (C, T) on the device), built once per module."""
    if name not in _cases:
        c = load_decode_case(golden_dir, name)
        model = build_model(c["spec"], c["pred_sd"], c["joint_sd"])
        _cases[name] = (c, model, torch.from_numpy(np.ascontiguousarray(c["frames"].T)).cuda())
    return _cases[name]


class Offline:
    """beam_search of every prefix of one utterance, computed once per prefix and never changed."""

    def __init__(self, model, frames_ct, **kw):
        self.model, self.frames_ct, self.kw, self.got = model, frames_ct, kw, {}

    def __call__(self, k):
        if k not in self.got:
            if k == 0:
                self.got[k] = [([], 0.0)]
            else:
                mel = self.frames_ct[None, :, :k]
                assert self.model._beam_device_ok(mel.permute(0, 2, 1), self.kw["beam_size"], self.kw["max_length"])
                self.got[k] = self.model.beam_search(mel, torch.tensor([k], device="cuda"), return_nbest=True, **self.kw)
        return self.got[k]


def _parts(T):
    """partitions(T) with the first seed whose "random" chunking has empty pushes first, last AND in between."""
    for seed in range(64):
        parts = partitions(T, seed=seed)
        rnd = parts["random"]
        if rnd[0] == 0 and rnd[-1] == 0 and 0 in rnd[1:-1] and sum(rnd) == T:
            return parts
    raise AssertionError(f"no seed gives {T} frames an empty push in between")


def _feed(stream, frames_ct, sizes, offline, tag):
    t = 0
    for k in sizes:
        best = stream.push_encoded(frames_ct[None, :, t:t + k])
        t += k
        want = offline(t)
        assert stream.nbest == want, (tag, t)  # tokens and float64 scores, exactly
        assert stream.frames == t and stream.tokens == want[0][0] == best, (tag, t)
        if t > 0:
            assert stream.last_path == "device", tag


EQUAL_CONFIGS = [("decode_small", 60, 2), ("decode_small", 60, 4), ("decode_small", 60, 16), ("decode_small", 9, 2), ("decode_small", 9, 4),
                 ("decode_small", 9, 16), ("decode_small_proj", 60, 8), ("decode_cap", 37, 4), ("decode_cap", 37, 16)]


@pytest.mark.parametrize("name,ml,beam", EQUAL_CONFIGS)
def test_stream_equals_the_offline_search_after_every_push(golden_dir, name, ml, beam):
    c, model, frames_ct = _case(golden_dir, name)
    T = frames_ct.shape[1]
    offline = Offline(model, frames_ct, beam_size=beam, max_length=ml)
    assert model.beam_stream(beam_size=beam, max_length=ml).nbest == [([], 0.0)]  # before the first frame
    parts = _parts(T)
    for pname in CHUNKINGS:
        s = model.beam_stream(beam_size=beam, max_length=ml)
        _feed(s, frames_ct, parts[pname], offline, (name, ml, beam, pname))
        assert s.frames == T


ORACLE_CONFIGS = [("decode_small", 60, (2, 4, 8)), ("decode_small_proj", 60, (2, 4, 8)), ("decode_cap", 37, (2, 4, 8, 16))]


@pytest.mark.parametrize("name,ml,beams", ORACLE_CONFIGS)
def test_stream_matches_the_oracle_at_every_frame_boundary(golden_dir, name, ml, beams):
    c, model, frames_ct = _case(golden_dir, name)
    T = frames_ct.shape[1]
    for beam in beams:
        s = model.beam_stream(beam_size=beam, max_length=ml)
        for k in range(1, T + 1):
            s.push_encoded(frames_ct[None, :, k - 1:k])
            want, _, gap = beam_oracle.beam_search(beam_oracle.Model(c["frames"][:k], c["pred_sd"], c["joint_sd"]), beam, ml)
            assert gap > GAP, (name, beam, k, gap)
            got = s.nbest
            assert [g[0] for g in got] == [w[0] for w in want], (name, beam, k)
            for (_, gs), (_, ws) in zip(got, want):
                assert abs(gs - ws) <= 1e-4 * max(1.0, abs(ws)), (name, beam, k, gs, ws)


@pytest.mark.parametrize("name", list(DECODE_CASES))
def test_beam1_stream_is_the_reference_greedy_decode(golden_dir, name):
    c, model, frames_ct = _case(golden_dir, name)
    parts = _parts(frames_ct.shape[1])
    for ml, want in c["tokens"].items():
        for pname in ("3", "random"):
            s = model.beam_stream(beam_size=1, max_length=ml)
            for k, t in zip(parts[pname], np.cumsum([0] + parts[pname])):
                s.push_encoded(frames_ct[None, :, t:t + k])
            assert s.last_path == "device" and s.frames == frames_ct.shape[1]
            assert s.tokens == want, (name, ml, pname)


def test_stable_prefix(golden_dir):
    c, model, frames_ct = _case(golden_dir, "decode_small")
    T = frames_ct.shape[1]
    s = model.beam_stream(beam_size=4, max_length=60)
    assert s.stable == []
    seen = []
    for t in range(0, T, 3):
        s.push_encoded(frames_ct[None, :, t:t + 3])
        lists = [y for y, _ in s.nbest]
        n = 0
        while all(len(y) > n and y[n] == lists[0][n] for y in lists):
            n += 1
        assert s.stable == lists[0][:n]
        if seen:
            assert s.stable[:len(seen[-1])] == seen[-1]  # it never shrinks
        seen.append(s.stable)
    final = s.tokens
    assert len(seen[-1]) > 3 and len(final) > len(seen[0])
    for st in seen:
        assert final[:len(st)] == st


def test_state_lives_in_the_streams_block_not_in_shared_scratch(golden_dir):
    import rnnt_amd
    c, model, frames_ct = _case(golden_dir, "decode_small_proj")
    T = frames_ct.shape[1]
    offline = Offline(model, frames_ct, beam_size=8, max_length=60)
    other = frames_ct.flip(1)[None, :, :20].contiguous()  # a different utterance of the same model
    dev = torch.device("cuda", torch.cuda.current_device())
    runs = []
    for trash in (False, True):
        s = model.beam_stream(beam_size=8, max_length=60)
        got, t = [], 0
        for k in partitions(T)["7"]:
            s.push_encoded(frames_ct[None, :, t:t + k])
            t += k
            got.append(s.nbest)
            if trash:
                assert s.nbest == offline(t), t
                model.beam_search(other, torch.tensor([20], device="cuda"), beam_size=8, max_length=60)  # reuses the shared scratch workspace
                rnnt_amd.engine.workspace(dev, 1).fill_(255)  # every float / double in it is a NaN
                torch.cuda.synchronize()
        runs.append(got)
    assert runs[0] == runs[1]  # bit-identical, trashed scratch or not
    assert runs[0][-1] == offline(T)


def test_two_streams_of_one_model_interleaved(golden_dir):
    c, model, frames_ct = _case(golden_dir, "decode_small")
    T = frames_ct.shape[1]
    a_frames, b_frames = frames_ct, frames_ct.flip(1).contiguous()
    off_a = Offline(model, a_frames, beam_size=4, max_length=60)
    off_b = Offline(model, b_frames, beam_size=4, max_length=60)
    a, b = model.beam_stream(4, 60), model.beam_stream(4, 60)
    ta = tb = 0
    while ta < T or tb < T:
        a.push_encoded(a_frames[None, :, ta:ta + 7])
        ta = min(T, ta + 7)
        b.push_encoded(b_frames[None, :, tb:tb + 5])
        tb = min(T, tb + 5)
        assert a.nbest == off_a(ta) and b.nbest == off_b(tb), (ta, tb)
    assert a.tokens != b.tokens


def _lone(model, frames_ct, sizes, **kw):
    """nbest of a lone BeamStream after every push of `sizes` (None: no push)."""
    s, t, out = model.beam_stream(**kw), 0, []
    for k in sizes:
        if k is not None:
            s.push_encoded(frames_ct[None, :, t:t + k])
            t += k
        out.append(s.nbest)
    return out


def test_group_equals_lone_streams(golden_dir):
    c, model, frames_ct = _case(golden_dir, "decode_small")
    kw = dict(beam_size=4, max_length=60)
    u0, u1, u1b, u2 = frames_ct[:, :40], frames_ct[:, 20:43], frames_ct[:, 50:75], frames_ct[:, :40]  # (u2 is u0 again, at position 2)
    # per push: (stream 0, stream 1, stream 2) chunk lengths, None = no entry; stream 1 finishes early, is reset and starts u1b
    plan = [(7, 3, 40), (7, None, None), (0, 20, None), (7, None, None), (7, "reset", None), (12, 13, None), (None, 12, None)]
    g = model.beam_streams(3, **kw)
    t = [0, 0, 0]
    utts = [u0, u1, u2]
    got = [[], [], []]
    for step in plan:
        chunks = []
        for i, k in enumerate(step):
            if k == "reset":
                g.reset(1)
                assert g.nbest[1] == [([], 0.0)] and g.frames[1] == 0 and g.stable[1] == []
                utts[1], t[1], k = u1b, 0, None
            chunks.append(None if k is None else utts[i][None, :, t[i]:t[i] + k])
            t[i] += k or 0
        best = g.push_encoded(chunks)
        assert best == g.tokens == [nb[0][0] for nb in g.nbest]
        assert g.frames == t
        for i in range(3):
            got[i].append(g.nbest[i])
    assert g.last_path == "device"
    assert got[0] == _lone(model, u0, [s[0] for s in plan], **kw)
    assert got[1][:4] == _lone(model, u1, [3, None, 20, None], **kw)
    assert got[1][4:] == _lone(model, u1b, [None, 13, 12], **kw)
    assert got[2] == _lone(model, u2, [40] + [None] * 6, **kw)
    assert got[2][-1] == got[0][-1]  # the same utterance at positions 0 and 2
    mel = u0[None]
    assert got[0][-1] == model.beam_search(mel, torch.tensor([40], device="cuda"), return_nbest=True, **kw)
    with pytest.raises(ValueError):
        g.push_encoded([None, None])
    with pytest.raises(ValueError):
        model.beam_streams(65)


def test_at_the_reference_widths(golden_dir):
    c, model, frames_ct = _case(golden_dir, "decode_ref_widths")
    frames_ct = frames_ct[:, :60]
    offline = Offline(model, frames_ct, beam_size=4, max_length=200)
    s = model.beam_stream(beam_size=4, max_length=200)
    t = 0
    for k in partitions(60)["17"]:
        s.push_encoded(frames_ct[None, :, t:t + k])
        t += k
    assert s.last_path == "device" and s.frames == 60
    assert s.nbest == offline(60) and len(s.tokens) > 3


def test_reset_and_max_length_reached_mid_push(golden_dir):
    c, model, frames_ct = _case(golden_dir, "decode_small")
    T = frames_ct.shape[1]
    offline = Offline(model, frames_ct, beam_size=4, max_length=9)
    fresh = _lone(model, frames_ct, partitions(T)["17"], beam_size=4, max_length=9)
    assert fresh[-1] == offline(T)
    # a hypothesis first holds max_length - 1 = 8 labels INSIDE a push: the frames after it in that push run with that slot blank-only
    full = min(k for k in range(1, T + 1) if any(len(y) == 8 for y, _ in offline(k)))
    assert full % 17 != 0 and full < T - 17, full
    for i, nb in enumerate(fresh):
        assert nb == offline(min(T, 17 * (i + 1))), i
    s = model.beam_stream(beam_size=4, max_length=9)
    s.push_encoded(frames_ct.flip(1)[None, :, :31].contiguous())
    assert s.frames == 31 and s.tokens
    s.reset()
    assert s.nbest == [([], 0.0)] and s.frames == 0 and s.tokens == [] and s.stable == []
    got, t = [], 0
    for k in partitions(T)["17"]:
        s.push_encoded(frames_ct[None, :, t:t + k])
        t += k
        got.append(s.nbest)
    assert got == fresh


def test_push_mel_through_a_streaming_encoder_on_the_device(golden_dir):
    c = load_decode_case(golden_dir, "decode_small")
    model = engine_model(c["spec"], c["pred_sd"], c["joint_sd"], encoder=StreamingCausalEncoder())
    rng = np.random.default_rng(11)
    mel = torch.from_numpy(rng.standard_normal((1, c["spec"]["H"], 151)).astype(np.float32)).cuda()
    want = model.beam_search(mel, torch.tensor([151], device="cuda"), beam_size=4, max_length=60, return_nbest=True)
    assert len(want[0][0]) > 3
    for step in (20, 7):
        s = model.beam_stream(beam_size=4, max_length=60)
        for i in range(0, 151, step):
            best = s.push(mel[..., i:i + step])
        assert s.nbest == want and best == want[0][0] and s.last_path == "device", step
        assert s.frames == 75
