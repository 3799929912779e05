"""CPU: the premises of the ConvPredictor edge cases (tests/predictor_cases.py) and a pin of the numpy oracle
(oracle/predictor_oracle.py) at segments no longer than the convolutions' taps — the committed goldens pin it at U1 = 1, 9 and 21
only, and tests/test_predictor_edges_gpu.py holds the kernels to it at U1 = 1 .. 5."""
import numpy as np
import pytest
import torch

from oracle import predictor_oracle as po
from tests import predictor_cases as pc


@pytest.mark.parametrize("name", list(pc.BUILDERS))
def test_case_premises(name):
    """Every builder runs (its premises are asserts inside it) and is a pure function of its arguments."""
    c = pc.BUILDERS[name]()
    d = pc.BUILDERS[name]()
    assert c.name == name and np.array_equal(c.ids, d.ids)
    sd = pc.state_dict(c)
    assert [tuple(sd[k].shape) for k in po.PARAMS] == [
        (c.S, c.E), (c.E,), (c.E,), (c.E, c.E, 3), (c.E,), (c.E, c.E, 5), (c.E,), (c.O, c.E), (c.O,), (c.O,), (c.O,)]
    assert all(v.dtype == np.float32 for v in sd.values())
    k1, k2, G = pc.masks_and_grad(c)
    assert (k1 is None) == (c.p == 0.0) == (k2 is None) and G.shape == (c.B, c.U1, c.O)
    if c.constant_row is not None:
        assert (sd["embedding.weight"][c.constant_row] == 0.5).all()


def test_embed_rounds_model():
    """The list-round model against cases worked by hand from k_embed_bwd's loop (a step of 256 rows is scanned while
    n + 256 <= 2048)."""
    assert pc.embed_rounds(np.full(2048, 1), 1) == [2048]
    assert pc.embed_rounds(np.full(2049, 1), 1) == [2048, 1]
    assert pc.embed_rounds(np.full(2500, 1), 0) == [0]                   # an absent symbol: one round over all rows
    ids = np.zeros(4096, dtype=np.int64)
    ids[:1793] = 1                                                        # 1793 > 1792 after step 8 (rows 0 .. 2047): round over
    assert pc.embed_rounds(ids, 1) == [1793, 0]
    ids[:] = 0
    ids[:1792] = 1                                                        # exactly 1792: one more step fits
    ids[4000] = 1
    assert pc.embed_rounds(ids, 1) == [1793]


def test_split_rule_model():
    """The split-count model against values worked by hand from sgemm_tn_splits_for (by_rows = ceil(M/448), by_fill =
    ceil(256 / workgroups per split), the larger of the two cut to min(16, ceil(M/256)))."""
    assert pc.tn_splits_for(408, 1024, 512, 1) == 2     # the largest row count of the earlier predictor tests: the cap, 2
    assert pc.tn_splits_for(6432, 1024, 512, 1) == 15   # the reference's training batch: by_rows = 15 > by_fill = 8
    assert pc.tn_splits_for(6432, 128, 128, 3) == 16    # by_fill = 86, cut to the cap
    assert pc.tn_splits_for(1, 4, 4, 1) == 1


def _torch_eval(c, dtype=torch.float64):
    """The module as plain torch in `dtype` on the CPU: Embedding, LayerNorm, rnnt_amd.predictor.CausalConv1d.forward (the reference's layout:
    (N,C,L) with left zero padding), exact GELU, explicit keep masks, Linear, LayerNorm; gradients of sum(out * G) by autograd."""
    from rnnt_amd.predictor import CausalConv1d
    F = torch.nn.functional
    sd = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in pc.state_dict(c).items()}
    k1, k2, G = pc.masks_and_grad(c)
    scale = 1.0 / (1.0 - c.p)
    convs = []
    for name, k in (("conv1", 3), ("conv2", 5)):
        m = CausalConv1d(c.E, c.E, kernel_size=k, stride=1, dilation=1).to(dtype)
        del m.conv._parameters["weight"], m.conv._parameters["bias"]
        m.conv.weight, m.conv.bias = sd[name + ".conv.weight"], sd[name + ".conv.bias"]  # (plain attributes: the autograd leaves)
        convs.append(m)
    x = F.embedding(torch.from_numpy(c.ids), sd["embedding.weight"])
    x = F.layer_norm(x, (c.E,), sd["input_layer_norm.weight"], sd["input_layer_norm.bias"], 1e-5)
    x = x.permute(0, 2, 1)
    for m, keep in zip(convs, (k1, k2)):
        x = F.gelu(m(x))
        if keep is not None:
            x = x * torch.from_numpy(keep).to(dtype).permute(0, 2, 1) * scale
    x = F.linear(x.permute(0, 2, 1), sd["linear.weight"], sd["linear.bias"])
    out = F.layer_norm(x, (c.O,), sd["output_layer_norm.weight"], sd["output_layer_norm.bias"], 1e-5)
    (out * torch.from_numpy(G).to(dtype)).sum().backward()
    return out.detach().numpy(), {k: v.grad.numpy() for k, v in sd.items()}


@pytest.mark.parametrize("U1", [1, 2, 3, 4, 5])
def test_oracle_matches_float64_torch_at_short_segments(U1):
    """Both sides float64: 1e-10 of each result's largest entry."""
    name = "short_segments_u%d" % U1
    c = pc.build(name)
    assert c.U1 == U1 and c.p > 0
    out, grads = pc.oracle(name)
    t_out, t_grads = _torch_eval(c)
    assert np.abs(out - t_out).max() <= 1e-10 * np.abs(t_out).max()
    for k in po.PARAMS:
        assert grads[k].shape == t_grads[k].shape, k
        assert np.abs(grads[k] - t_grads[k]).max() <= 1e-10 * np.abs(t_grads[k]).max(), k
