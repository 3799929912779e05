"""CPU tests of rnnt_amd.LSTMPredictor's torch path — the oracle of the engine path — against the REFERENCE's own float64 module
(tests/golden/lstm_predictor_*.npz, written by tests/golden/make_golden_lstm_predictor.py), of the module's interface, and of the
premises of the GPU tests."""
import numpy as np
import pytest
import torch

from tests import lstm_predictor_cases as lc

TOL = 1e-12


@pytest.fixture(scope="module")
def fixtures():
    return {n: lc.load(n) for n in lc.FIXTURES}


@pytest.mark.parametrize("name", lc.FIXTURES)
def test_torch_path_reproduces_the_reference_in_float64(fixtures, name):
    fx = fixtures[name]
    m = lc.fixture_module(fx)
    got = lc.run(m, fx["ids"], fx["G"])
    assert m.last_backend == "torch"
    for k, v in got.items():
        ref = fx[k + "_f64"] if k in ("out", "state") else fx[k]
        assert lc.rel_err(v, ref) <= TOL, (k, lc.rel_err(v, ref))
    B = fx["spec"]["B"]
    with torch.no_grad():
        _, _, st = m(torch.from_numpy(fx["ids"]), torch.full((B,), fx["spec"]["U1"]))
        out2, lens2, st2 = m(torch.from_numpy(fx["ids2"]), torch.full((B,), 3), st)
    assert lc.rel_err(out2.numpy(), fx["out2_f64"]) <= TOL and lc.rel_err(lc.flat_state(st2), fx["state2_f64"]) <= TOL


def test_one_token_from_zero_state_has_no_p2g_gradient(fixtures):
    assert not np.any(fixtures["one"]["grad__lstm_layers__0__p2g__weight"])


@pytest.mark.parametrize("name", lc.FIXTURES)
def test_state_dict_is_the_references(fixtures, name):
    fx = fixtures[name]
    m = lc.module_of(fx["spec"])
    assert list(m.state_dict().keys()) == [str(k) for k in fx["keys"]]
    res = m.load_state_dict(lc.state_dict_of(fx, torch.float32), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    has_bias = any("x2g.bias" in k for k in m.state_dict())
    assert has_bias == (not fx["spec"]["ln"]) and not any("p2g.bias" in k for k in m.state_dict())


def test_lengths_mask_nothing_and_are_returned_as_given(fixtures):
    fx = fixtures["noln"]
    m = lc.fixture_module(fx)
    ids = torch.from_numpy(fx["ids"])
    full, short = torch.full((ids.shape[0],), ids.shape[1]), torch.ones(ids.shape[0], dtype=torch.int64)
    with torch.no_grad():
        a, la, sa = m(ids, full)
        b, lb, sb = m(ids, short)
    assert la is full and lb is short
    assert torch.equal(a, b) and all(torch.equal(x, y) for p, q in zip(sa, sb) for x, y in zip(p, q))


def test_dropout_follows_every_layer_and_the_state_is_undropped(fixtures):
    fx = fixtures["small_ln"]
    s = fx["spec"]
    m = lc.fixture_module(fx).train()
    ids = torch.from_numpy(fx["ids"])
    lens = torch.full((s["B"],), s["U1"])
    keep = torch.ones((s["L"], s["B"], s["U1"], s["Hd"]), dtype=torch.uint8)
    keep[-1] = 0  # everything the last layer hands to `linear` is dropped: the output is LayerNorm(linear.bias) in every row
    with torch.no_grad():
        out, _, st = m(ids, lens, keep_masks=keep)
        want = m.output_layer_norm(m.linear.bias)
        _, _, st_eval = m.eval()(ids, lens)
    assert torch.allclose(out, want.expand_as(out), rtol=0, atol=1e-12)
    keep[-1] = 1
    keep[0] = 0  # layer 0's output dropped: layer 0's own state is what it is without dropout
    with torch.no_grad():
        _, _, st0 = m.train()(ids, lens, keep_masks=keep)
    assert torch.equal(st0[0][0], st_eval[0][0]) and torch.equal(st0[0][1], st_eval[0][1])
    assert not torch.equal(st0[1][0], st_eval[1][0])


def test_drawn_masks_follow_torch_generator(fixtures):
    m = lc.fixture_module(fixtures["small_ln"]).train()
    ids = torch.from_numpy(fixtures["small_ln"]["ids"])
    lens = torch.full((ids.shape[0],), ids.shape[1])
    with torch.no_grad():
        torch.manual_seed(3)
        a = m(ids, lens)[0]
        torch.manual_seed(3)
        b = m(ids, lens)[0]
        c = m(ids, lens)[0]
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_model_sees_a_stateful_predictor_and_calls_it_with_lengths():
    import rnnt_amd
    model = lc.wiring_model()
    assert model._predictor_is_stateful()
    seen = {}
    inner = model.predictor.forward

    def spy(input, lengths, state=None):
        seen["lengths"], seen["shape"] = lengths.clone(), tuple(input.shape)
        return inner(input, lengths, state)

    model.predictor.forward = spy
    assert model._predictor_is_stateful()
    ids, id_lens = torch.tensor([[1, 2, 3], [4, 5, 0]]), torch.tensor([3, 2])
    feats = model._predict(torch.cat([torch.full((2, 1), 15), ids], 1), id_lens + 1)
    assert seen["shape"] == (2, 4) and seen["lengths"].tolist() == [4, 3] and feats.shape == (2, 4, lc.DECODE_SPEC["O"])
    # a stateless predictor is called exactly as before
    stateless = rnnt_amd.RNNTModel(torch.nn.Embedding(16, 8), model.encoder, model.joint)
    assert not stateless._predictor_is_stateful() and stateless._predict(ids, id_lens).shape == (2, 3, 8)


def test_backends_on_the_cpu(fixtures):
    fx = fixtures["one"]
    m = lc.fixture_module(fx, torch.float32)
    ids, lens = torch.from_numpy(fx["ids"]), torch.tensor([1])
    m.backend = "engine"
    with pytest.raises(RuntimeError, match="engine path does not apply.*HIP device"):
        m(ids, lens)
    m.backend = "auto"
    m(ids, lens)
    assert m.last_backend == "torch"
    m.backend = "hip"
    with pytest.raises(ValueError):
        m(ids, lens)


def test_greedy_decode_premise_and_host_loop():
    """The wiring test's premise (no near-tie decides a label in float64) and RNNTModel.greedy_decode's host loop on the CPU with the
    new class: per-token calls with the state handed back."""
    model, mel = lc.wiring_model(), lc.decode_frames()
    with torch.no_grad():
        want, gap = lc.greedy_with_margins(model, mel, 200)
        got = model.greedy_decode(mel, torch.tensor([mel.shape[-1]]), max_length=200)
    assert gap > lc.DECODE_MARGIN and len(want) >= 10 and len(set(want)) >= 3
    assert got == want


def test_edge_premises_hold():
    names = [e.name for e in lc.EDGES]
    assert len(set(names)) == len(names)
    assert {e.spec["B"] for e in lc.EDGES} >= {1, 31, 32, 33} and {e.spec["U1"] for e in lc.EDGES} >= {1, 2}
    assert {e.spec["L"] for e in lc.EDGES} >= {1, 3} and {e.spec["Hd"] for e in lc.EDGES} >= {36, 256, 260, 1024}
