"""-m gpu: rnnt_amd.LSTMPredictor on the engine (rnnt_engine_lstm_predictor_fwd / _bwd, rnnt_amd/csrc/lstm.hip) against float64:
the reference's own module on the four fixtures (tests/golden/lstm_predictor_*.npz) and the module's float64 torch path elsewhere.

Error measure everywhere: max |got - ref| relative to the float64 tensor's largest entry; a tensor that is identically zero in
float64 must be exactly zero.  Bars: a fixture's is 4 x the largest error the REFERENCE's fp32 module shows in that case (stored in
the fixture); an edge case's and the reference widths' is 4 x the largest error of the fp32 torch path of the same module on the
CPU, computed in the test.  The factor 4 is the margin the encoder and featurizer tests give a kernel with another summation order
and another exp / tanh.  With RNNT_LSTM_PARITY_OUT=<file> set, every measured ratio is appended to that file
(profiles/lstm_predictor_parity.txt is such a run)."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import lstm_predictor_cases as lc
from tests.helpers import assert_close_grad, assert_close_loss

pytestmark = pytest.mark.gpu


def engine_copy(m, backend="engine"):
    m = copy.deepcopy(m).float().cuda()
    m.backend = backend
    return m


def check(tag, got, ref, bar):
    """Every tensor of `ref` within `bar`; the ratios go to stdout (and RNNT_LSTM_PARITY_OUT)."""
    lines, worst = [], (-1.0, "")
    for k in sorted(ref):
        r = lc.rel_err(got[k], ref[k])
        lines.append(f"{tag:28s} {k:44s} err {r:.3e}  bar {bar:.3e}  ratio {r / bar:.3f}")
        worst = max(worst, (r, k))
    print("\n".join(lines))
    path = os.environ.get("RNNT_LSTM_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")
    assert worst[0] <= bar, f"{tag}: {worst[1]} err {worst[0]:.3e} > bar {bar:.3e}"


def fixture_ref(fx, keys=("out", "state")):
    ref = {k: fx[k + "_f64"] for k in keys}
    ref.update({k: v for k, v in fx.items() if k.startswith("grad__")})
    return ref


@pytest.fixture(scope="module")
def fixtures():
    return {n: lc.load(n) for n in lc.FIXTURES}


@pytest.mark.parametrize("name", lc.FIXTURES)
def test_fixture_parity(fixtures, name):
    fx = fixtures[name]
    m = engine_copy(lc.fixture_module(fx))
    got = lc.run(m, fx["ids"], fx["G"])
    assert m.last_backend == "engine"
    check("fixture " + name, got, fixture_ref(fx), lc.fixture_bar(fx))
    if name == "one":  # one token from zero state: h_{-1} = 0, so d p2g is exactly zero
        assert not np.any(fx["grad__lstm_layers__0__p2g__weight"]) and not np.any(got["grad__lstm_layers__0__p2g__weight"])


@pytest.mark.parametrize("name", lc.FIXTURES)
def test_continuation(fixtures, name):
    """The fixture's second call (the first call's state in, three more tokens); one call over all tokens against two calls over a
    split of them; the engine's own state handed back is read in place."""
    fx = fixtures[name]
    bar = lc.fixture_bar(fx)
    m = engine_copy(lc.fixture_module(fx))
    ids = torch.from_numpy(fx["ids"]).cuda()
    ids2 = torch.from_numpy(fx["ids2"]).cuda()
    B, U1 = ids.shape
    with torch.no_grad():
        out, _, st = m(ids, torch.full((B,), U1, device="cuda"))
        assert m.last_backend == "engine"
        packed = m._pack_state(st, B, fx["spec"]["Hd"])
        assert packed.data_ptr() == st[0][0].data_ptr() and packed.shape == (fx["spec"]["L"], 2, B, fx["spec"]["Hd"])
        out2, _, st2 = m(ids2, torch.full((B,), 3, device="cuda"), st)
        assert m.last_backend == "engine"
        check("second call " + name, {"out2": out2.cpu().numpy(), "state2": lc.flat_state(st2)},
              {"out2": fx["out2_f64"], "state2": fx["state2_f64"]}, bar)
        if U1 >= 2:
            k = U1 // 2
            a, _, sa = m(ids[:, :k], torch.full((B,), k, device="cuda"))
            b, _, sb = m(ids[:, k:], torch.full((B,), U1 - k, device="cuda"), sa)
            check("split call " + name, {"out": torch.cat([a, b], 1).cpu().numpy(), "state": lc.flat_state(sb)},
                  {"out": out.cpu().numpy().astype(np.float64), "state": lc.flat_state(st).astype(np.float64)}, bar)


def test_dropout_masks(fixtures):
    """Explicit keep masks at p = 0.5: output and gradients match the float64 torch path with the same masks; eval mode ignores them."""
    fx = fixtures["small_ln"]
    s = fx["spec"]
    keep = (torch.rand((s["L"], s["B"], s["U1"], s["Hd"]), generator=torch.Generator().manual_seed(5)) >= 0.5).to(torch.uint8)
    assert 0.3 < keep.float().mean() < 0.7
    m64 = lc.fixture_module(fx)
    m64.dropout.p = 0.5
    m = engine_copy(m64)
    ref = lc.run(m64.train(), fx["ids"], fx["G"], keep_masks=keep)
    assert m64.last_backend == "torch"
    got = lc.run(m.train(), fx["ids"], fx["G"], keep_masks=keep)
    assert m.last_backend == "engine"
    plain = lc.run(lc.fixture_module(fx), fx["ids"], fx["G"])
    assert lc.rel_err(ref["out"], plain["out"]) > 1e-2  # the masks did something
    check("dropout small_ln", got, ref, lc.fixture_bar(fx))
    with_masks, without = lc.run(m.eval(), fx["ids"], fx["G"], keep_masks=keep), lc.run(m.eval(), fx["ids"], fx["G"])
    for k in without:
        assert np.array_equal(with_masks[k], without[k]), k


def torch_path_bar(m64, ids, G, state, ref):
    """4 x the largest error of the module's fp32 torch path on the CPU against its float64 one."""
    m32 = copy.deepcopy(m64).float()
    got = lc.run(m32, ids, G, state)
    return 4.0 * max(lc.rel_err(got[k], ref[k]) for k in ref)


@pytest.mark.parametrize("edge", lc.EDGES, ids=[e.name for e in lc.EDGES])
def test_edges(edge):
    ids, G, state = lc.edge_inputs(edge)
    m64 = lc.seeded_module(edge.spec)
    ref = lc.run(m64, ids, G, state)
    assert m64.last_backend == "torch"
    bar = torch_path_bar(m64, ids, G, state, ref)
    m = engine_copy(m64)
    got = lc.run(m, ids, G, state)
    assert m.last_backend == "engine"
    check("edge " + edge.name, got, ref, bar)
    if edge.spec["U1"] == 1 and not edge.with_state:
        assert not any(np.any(v) for k, v in got.items() if k.endswith("p2g__weight"))


def test_reference_widths():
    """The reference configuration's widths (config/basic_sp.yaml: three layers of 512, layer norm, eps 1e-3) at B = 4, U1 = 24."""
    spec = dict(S=1024, O=1024, E=512, L=3, Hd=512, ln=True, B=4, U1=24, eps=1e-3, seed=31)
    g = torch.Generator().manual_seed(32)
    ids = torch.randint(0, spec["S"], (spec["B"], spec["U1"]), generator=g)
    G = torch.randn(spec["B"], spec["U1"], spec["O"], generator=g).double()
    m64 = lc.seeded_module(spec)
    ref = lc.run(m64, ids, G)
    bar = torch_path_bar(m64, ids, G, None, ref)
    m = engine_copy(m64)
    got = lc.run(m, ids, G)
    assert m.last_backend == "engine"
    check("reference widths", got, ref, bar)


def test_reproducible_and_workspace_independent(fixtures):
    """Two training calls on rows33 give bit-identical outputs and gradients, with the scratch workspace poisoned in between."""
    import rnnt_amd
    fx = fixtures["rows33"]
    m = engine_copy(lc.fixture_module(fx))
    m.dropout.p = 0.3
    s = fx["spec"]
    keep = (torch.rand((s["L"], s["B"], s["U1"], s["Hd"]), generator=torch.Generator().manual_seed(6)) >= 0.3).to(torch.uint8)
    first = lc.run(m.train(), fx["ids"], fx["G"], keep_masks=keep)
    ws = rnnt_amd.engine.workspace(torch.device("cuda", torch.cuda.current_device()), 1)
    assert ws.numel() > 1  # the buffer the calls above used
    ws.fill_(0xFF)
    second = lc.run(m.train(), fx["ids"], fx["G"], keep_masks=keep)
    assert m.last_backend == "engine"
    for k in first:
        assert np.array_equal(first[k], second[k]), k


def test_engine_backend_refuses_what_it_does_not_cover():
    m = lc.seeded_module(dict(S=8, O=8, E=8, L=1, Hd=6, ln=True, eps=1e-3, seed=1), torch.float32).cuda()
    m.backend = "engine"
    ids = torch.zeros((1, 2), dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="Hd % 4"):
        m(ids, torch.tensor([2], device="cuda"))
    m.backend = "auto"
    m(ids, torch.tensor([2], device="cuda"))
    assert m.last_backend == "torch"


# ---- RNNTModel wiring --------------------------------------------------------------------------------------------------------
def test_model_loss_backward_and_align():
    """RNNTModel.forward / align with the stateful predictor: the engine-backed predictor against the same model on its torch path."""
    model = lc.wiring_model(torch.float32).cuda().train()
    model.predictor.dropout.p = 0.0
    g = torch.Generator().manual_seed(9)
    N, T, U, blank = 3, 12, 5, model.joint.blank_idx
    mel = torch.randn(N, lc.DECODE_SPEC["O"], T, generator=g).cuda()
    mel_lens = torch.tensor([12, 9, 7]).cuda()
    ids = torch.randint(0, blank, (N, U), generator=g).cuda()
    id_lens = torch.tensor([5, 3, 4]).cuda()
    res = {}
    for backend in ("torch", "engine"):
        model.predictor.backend = backend
        model.zero_grad(set_to_none=True)
        loss = model(mel, mel_lens, ids, id_lens, blank)
        loss.backward()
        assert model.predictor.last_backend == backend
        scores, frames = model.align(mel, mel_lens, ids, id_lens, blank)
        assert model.predictor.last_backend == backend
        res[backend] = (loss.item(), {k: p.grad.cpu().numpy() for k, p in model.named_parameters()}, frames.cpu().numpy())
    assert_close_loss("loss", res["engine"][0], res["torch"][0], rtol=1e-5)
    for k, v in res["torch"][1].items():
        assert_close_grad(k, res["engine"][1][k], v)
    assert np.array_equal(res["engine"][2], res["torch"][2])


def test_greedy_decode_and_stream_match_the_torch_backend():
    m64 = lc.wiring_model()
    mel64 = lc.decode_frames()
    with torch.no_grad():
        want, gap = lc.greedy_with_margins(m64, mel64, 200)
    assert gap > lc.DECODE_MARGIN and len(want) >= 10 and len(set(want)) >= 3, (gap, want)  # the premise: no near-tie decides a label
    model = lc.wiring_model(torch.float32).cuda().eval()
    mel = mel64.float().cuda()
    lens = torch.tensor([mel.shape[-1]]).cuda()
    for backend in ("torch", "engine"):
        model.predictor.backend = backend
        assert model.greedy_decode(mel, lens, max_length=200) == want, backend
        assert model.predictor.last_backend == backend
        stream = model.greedy_stream()
        got = []
        for t in range(mel.shape[-1]):
            got += stream.push_encoded(mel[:, :, t:t + 1])
        assert got == want, backend
        assert model.predictor.last_backend == backend and stream.last_path == "host"
