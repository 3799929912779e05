"""CPU: RNNTModel.greedy_stream's host path (rnnt_amd/stream.py HostGreedyLoop) against the offline host greedy_decode
and the numpy oracle (oracle/decode_oracle.py) for every decode fixture, every chunking, with and without a max_length cap."""
import numpy as np
import pytest
import torch

from oracle import decode_oracle
from tests.helpers import DECODE_CASES, load_decode_case
from tests.stream_models import (LSTMLikePredictor, PassThroughEncoder, StreamingCausalEncoder, cpu_model, partitions,
                                 stream_frames)


def _offline(model, frames_ct, ml):
    mel = frames_ct[None]
    return model.greedy_decode(mel, torch.tensor([mel.shape[-1]]), max_length=ml)


@pytest.mark.parametrize("name", list(DECODE_CASES))
def test_host_stream_equals_offline_and_oracle(golden_dir, name):
    c = load_decode_case(golden_dir, name)
    spec = c["spec"]
    model = cpu_model(spec, c["pred_sd"], c["joint_sd"])
    frames_ct = torch.from_numpy(np.ascontiguousarray(c["frames"].T))
    T = frames_ct.shape[1]
    big = spec["E"] > 64  # (the reference's widths: two chunkings, the oracle with its exact 7-token window)
    parts = partitions(T, seed=len(name))
    if big:
        parts = {k: parts[k] for k in ("7", "random")}
    else:
        parts = {k: parts[k] for k in ("1", "2", "7", "16", "all", "random")}
    for ml in (2, *c["tokens"], None):
        cap = T * 10 + 2 if ml is None else ml
        want = _offline(model, frames_ct, cap)
        if ml in c["tokens"]:
            assert want == c["tokens"][ml], (name, ml)  # the reference's own lists
        else:
            ref, margins = decode_oracle.greedy_decode(c["frames"], c["pred_sd"], c["joint_sd"], max_length=cap, window=7 if big else None)
            if margins.min() > 1e-3:
                assert want == ref, (name, ml)
        for pname, sizes in parts.items():
            s = model.greedy_stream(max_length=ml)
            got, pushes = stream_frames(s, frames_ct, sizes)
            assert got == want, (name, ml, pname)
            assert all(path == "host" for _, path, k in pushes if k > 0)
            if ml is not None and len(want) + 1 >= ml:
                assert s.done
            else:
                assert not s.done and s.frames == T


def test_cap_case_runs_into_ten_labels_per_frame(golden_dir):
    c = load_decode_case(golden_dir, "decode_cap")
    model = cpu_model(c["spec"], c["pred_sd"], c["joint_sd"])
    frames_ct = torch.from_numpy(np.ascontiguousarray(c["frames"].T))
    T = frames_ct.shape[1]
    want = _offline(model, frames_ct, T * 10 + 2)
    assert len(want) >= 10 * T - 2  # (almost) every frame emits its ten labels
    for k in (1, 3, T):
        s = model.greedy_stream(max_length=None)
        sizes = [k] * (T // k) + ([T % k] if T % k else [])
        got, pushes = stream_frames(s, frames_ct, sizes)
        assert got == want
        assert max(len(p[0]) for p in pushes) <= 10 * k


def test_stateful_predictor_stream_equals_offline(golden_dir):
    import rnnt_amd
    c = load_decode_case(golden_dir, "decode_small")
    spec = c["spec"]
    joint = rnnt_amd.JointNetwork(spec["fa"], spec["ft"], spec["H"], spec["V"])
    joint.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in c["joint_sd"].items()})
    model = rnnt_amd.RNNTModel(LSTMLikePredictor(spec["V"], spec["O"], 16, seed=3), PassThroughEncoder(), joint).eval()
    assert model._predictor_is_stateful()
    frames_ct = torch.from_numpy(np.ascontiguousarray(c["frames"].T))
    T = frames_ct.shape[1]
    for ml in (60, None):
        want = _offline(model, frames_ct, T * 10 + 2 if ml is None else ml)
        assert len(want) > 5
        for sizes in ([1] * T, [7] * (T // 7) + [T % 7], [0, 30, 0, T - 30]):
            s = model.greedy_stream(max_length=ml)
            got, _ = stream_frames(s, frames_ct, sizes)
            assert got == want, (ml, sizes)


def test_push_mel_through_a_streaming_encoder(golden_dir):
    c = load_decode_case(golden_dir, "decode_small")
    model = cpu_model(c["spec"], c["pred_sd"], c["joint_sd"], encoder=StreamingCausalEncoder())
    rng = np.random.default_rng(11)
    mel = torch.from_numpy(rng.standard_normal((1, c["spec"]["H"], 151)).astype(np.float32))
    frames = model.encoder(mel)
    assert frames.shape[-1] == 75
    want = model.greedy_decode(mel, torch.tensor([151]), max_length=60)
    ref, margins = decode_oracle.greedy_decode(frames[0].T.numpy(), c["pred_sd"], c["joint_sd"], max_length=60)
    assert margins.min() > 1e-3 and want == ref and len(want) > 5
    for step in (20, 7, 151):
        s = model.greedy_stream(max_length=60)
        got = []
        for i in range(0, 151, step):
            got += s.push(mel[..., i:i + step])
        assert got == want == s.tokens, step


def test_done_streams_and_bad_shapes(golden_dir):
    import rnnt_amd
    c = load_decode_case(golden_dir, "decode_small")
    model = cpu_model(c["spec"], c["pred_sd"], c["joint_sd"])
    frames_ct = torch.from_numpy(np.ascontiguousarray(c["frames"].T))
    s = model.greedy_stream(max_length=9)
    got = s.push_encoded(frames_ct[None])
    assert got == c["tokens"][9] and s.done and s.frames < frames_ct.shape[1]
    assert s.push_encoded(frames_ct[None, :, :5]) == [] and s.tokens == c["tokens"][9]
    assert model.greedy_stream(max_length=1).done and model.greedy_stream(max_length=1).push_encoded(frames_ct[None]) == []
    s = model.greedy_stream()
    with pytest.raises(ValueError):
        s.push_encoded(torch.cat([frames_ct[None], frames_ct[None]]))  # batch 2
    with pytest.raises(ValueError):
        s.push_encoded(frames_ct)  # rank 2
    with pytest.raises(ValueError):
        model.greedy_stream(max_symbols_per_frame=0)
    with pytest.raises(TypeError, match="streaming_forward"):
        s.push(frames_ct[None])  # the pass-through encoder has no streaming interface
    assert isinstance(s, rnnt_amd.GreedyStream)
