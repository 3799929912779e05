"""CPU: RNNTModel.beam_stream's host path (rnnt_amd/stream.py HostBeamLoop): after every push the search of the frames
pushed so far, for every chunking; beam_search's own host result, which now runs the same loop, held to the float64 oracle as before."""
import numpy as np
import pytest
import torch

from tests import beam_oracle
from tests.helpers import load_decode_case
from tests.stream_models import LSTMLikePredictor, PassThroughEncoder, StreamingCausalEncoder, cpu_model, partitions


def _frames_ct(c):
    return torch.from_numpy(np.ascontiguousarray(c["frames"].T))


@pytest.mark.parametrize("beam", [1, 3, 20])  # 20: above the device's limit — the host loop on a GPU too
@pytest.mark.parametrize("name,ml", [("decode_small", 9), ("decode_cap", 37)])
def test_host_stream_equals_the_offline_host_search_after_every_push(golden_dir, name, ml, beam):
    c = load_decode_case(golden_dir, name)
    model = cpu_model(c["spec"], c["pred_sd"], c["joint_sd"])
    frames_ct = _frames_ct(c)
    T = frames_ct.shape[1]
    offline = {0: [([], 0.0)]}  # per prefix, computed once

    def want(k):
        if k not in offline:
            with torch.no_grad():
                offline[k] = model._beam_search_host(frames_ct[None, :, :k].permute(0, 2, 1), beam, ml, 10)
        return offline[k]

    assert model.beam_stream(beam_size=beam, max_length=ml).nbest == [([], 0.0)]
    for pname, sizes in partitions(T, seed=len(name)).items():
        s = model.beam_stream(beam_size=beam, max_length=ml)
        t, stable = 0, []
        for k in sizes:
            best = s.push_encoded(frames_ct[None, :, t:t + k])
            t += k
            assert s.nbest == want(t), (name, beam, pname, t)  # the same lists, the same Python floats
            assert s.frames == t and best == s.tokens == want(t)[0][0]
            if t > 0:
                assert s.last_path == "host"
            assert s.stable[:len(stable)] == stable and all(y[:len(s.stable)] == s.stable for y, _ in s.nbest)
            stable = s.stable
        assert t == T
    mel = frames_ct[None]
    assert want(T) == model.beam_search(mel, torch.tensor([T]), beam_size=beam, max_length=ml, return_nbest=True)
    if beam == 1:
        assert c["tokens"][ml] == model.beam_stream(beam_size=1, max_length=ml).push_encoded(frames_ct[None])  # beam 1: the reference's greedy list


@pytest.mark.parametrize("name,ml", [("decode_small", 60), ("decode_small_proj", 60)])
def test_host_stream_and_refactored_host_search_match_the_oracle(golden_dir, name, ml):
    """The bar of tests/test_beam_oracle.py::test_host_loop_matches_the_oracle, where the oracle's gap is established."""
    c = load_decode_case(golden_dir, name)
    model = cpu_model(c["spec"], c["pred_sd"], c["joint_sd"])
    om = beam_oracle.Model(c["frames"], c["pred_sd"], c["joint_sd"])
    frames_ct = _frames_ct(c)
    T = frames_ct.shape[1]
    mel = frames_ct[None]
    for beam in (1, 4):
        want, _, gap = beam_oracle.beam_search(om, beam, ml)
        assert gap > 1e-3
        s = model.beam_stream(beam_size=beam, max_length=ml)
        for t in range(0, T, 7):
            s.push_encoded(frames_ct[None, :, t:t + 7])
        for got in (s.nbest, model.beam_search(mel, torch.tensor([T]), beam_size=beam, max_length=ml, return_nbest=True)):
            assert [g[0] for g in got] == [w[0] for w in want], (name, beam)
            for (_, gs), (_, ws) in zip(got, want):
                assert abs(gs - ws) <= 1e-4 * max(1.0, abs(ws)), (name, beam, gs, ws)


def test_group_on_the_host_equals_lone_streams(golden_dir):
    c = load_decode_case(golden_dir, "decode_small")
    model = cpu_model(c["spec"], c["pred_sd"], c["joint_sd"])
    f = _frames_ct(c)
    kw = dict(beam_size=3, max_length=20)
    g = model.beam_streams(2, **kw)
    a, b = model.beam_stream(**kw), model.beam_stream(**kw)
    assert g.push_encoded([f[None, :, :5], None]) == [a.push_encoded(f[None, :, :5]), []]
    assert g.push_encoded([f[None, :, 5:6], f[None, :, 30:41]]) == [a.push_encoded(f[None, :, 5:6]), b.push_encoded(f[None, :, 30:41])]
    assert g.nbest == [a.nbest, b.nbest] and g.frames == [6, 11] and g.stable == [a.stable, b.stable] and g.last_path == "host"
    g.reset(0)
    assert g.nbest[0] == [([], 0.0)] and g.frames == [0, 11] and g.nbest[1] == b.nbest
    a.reset()
    assert g.push_encoded([f[None, :, 60:70], None])[0] == a.push_encoded(f[None, :, 60:70]) and g.nbest[0] == a.nbest


def test_refusals(golden_dir):
    import rnnt_amd
    c = load_decode_case(golden_dir, "decode_small")
    spec = c["spec"]
    model = cpu_model(spec, c["pred_sd"], c["joint_sd"])
    stateful = rnnt_amd.RNNTModel(LSTMLikePredictor(spec["V"], spec["O"], 16, seed=3), PassThroughEncoder(), model.joint).eval()
    with pytest.raises(NotImplementedError):
        stateful.beam_stream()
    with pytest.raises(NotImplementedError):
        stateful.beam_streams(2)
    for kw in (dict(beam_size=0), dict(max_symbols_per_frame=0)):
        with pytest.raises(ValueError):
            model.beam_stream(**kw)
        with pytest.raises(ValueError):
            model.beam_streams(2, **kw)
    for n in (0, 65):
        with pytest.raises(ValueError):
            model.beam_streams(n)
    s = model.beam_stream()
    with pytest.raises(TypeError):
        s.push(torch.zeros(1, spec["H"], 4))  # PassThroughEncoder has no streaming_forward
    with pytest.raises(ValueError):
        s.push_encoded(torch.zeros(2, spec["H"], 4))
    with pytest.raises(ValueError):
        model.beam_streams(2).push_encoded([None])


def test_push_mel_through_a_streaming_encoder_on_the_host(golden_dir):
    c = load_decode_case(golden_dir, "decode_small")
    model = cpu_model(c["spec"], c["pred_sd"], c["joint_sd"], encoder=StreamingCausalEncoder())
    rng = np.random.default_rng(11)
    mel = torch.from_numpy(rng.standard_normal((1, c["spec"]["H"], 61)).astype(np.float32))
    want = model.beam_search(mel, torch.tensor([61]), beam_size=3, max_length=20, return_nbest=True)
    s = model.beam_stream(beam_size=3, max_length=20)
    for i in range(0, 61, 7):
        best = s.push(mel[..., i:i + 7])
    assert s.nbest == want and best == want[0][0] and s.frames == 30
