"""-m gpu: rnnt_amd.ConvPredictor (rnnt_engine_conv_predictor_fwd / _bwd) against the float64 numpy oracle at training row counts
and at the edges of its kernels — the cases of tests/predictor_cases.py, whose builders state what each one reaches: 16 weight-gradient
splits with uneven ranges and an odd row count, the embedding gradient's list rounds and its second column sweep, rows on each side of
a split boundary, utterances shorter than the convolutions' taps, E % 8 == 4, a zero-variance LayerNorm row; then exact zeros for absent
symbols, bit-reproducibility, and independence of whatever the caller-owned `saved` buffer and the gradient buffers held before."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import predictor_oracle as po
from tests import predictor_cases as pc
from tests.helpers import assert_close_grad

pytestmark = pytest.mark.gpu

# the bars of tests/test_predictor_gpu.py::test_conv_predictor_training_mode_vs_oracle
OUT_RTOL, OUT_ATOL, GRAD_RTOL = 1e-5, 2e-5, 2e-4


def _module(c):
    import rnnt_amd
    m = rnnt_amd.ConvPredictor(c.S, c.O, c.E, dropout=c.p)
    r = m.load_state_dict({k: torch.from_numpy(v) for k, v in pc.state_dict(c).items()}, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    m = m.cuda()
    return m.train() if c.p > 0 else m.eval()


def _inputs(c):
    k1, k2, G = pc.masks_and_grad(c)
    masks = None if k1 is None else (torch.from_numpy(k1).cuda(), torch.from_numpy(k2).cuda())
    return torch.from_numpy(c.ids).cuda(), masks, torch.from_numpy(G).cuda()


def _run(m, ids, masks, G):
    m.zero_grad(set_to_none=True)
    out = m(ids, keep_masks=masks)
    (out * G).sum().backward()
    got = dict(m.named_parameters())
    return out.detach(), {k: got[k].grad.clone() for k in po.PARAMS}


def _assert_oracle_bar(name, out, grads):
    ref_out, ref = pc.oracle(name)
    assert_close_grad(name + " out", out.cpu().numpy(), ref_out, rtol=OUT_RTOL, atol=OUT_ATOL)
    for k in po.PARAMS:
        assert_close_grad(name + " " + k, grads[k].cpu().numpy(), ref[k], rtol=GRAD_RTOL)


@pytest.mark.parametrize("name", pc.PARITY_CASES)
def test_conv_predictor_edge_case_vs_oracle(name):
    """out and all 11 parameter gradients at the project's bars; the embedding-gradient rows of symbols that do not occur are exactly 0."""
    c = pc.build(name)
    out, grads = _run(_module(c), *_inputs(c))
    _assert_oracle_bar(name, out, grads)
    absent = pc.absent_symbols(c)
    if name == "one_symbol":
        assert len(absent) == 7
    if len(absent):
        rows = grads["embedding.weight"][torch.from_numpy(absent).cuda()]
        assert torch.equal(rows, torch.zeros_like(rows)), name


def test_e_beyond_the_limit_is_refused():
    import rnnt_amd
    m = rnnt_amd.ConvPredictor(4, 4, pc.E_MAX + 4, dropout=0.0).cuda().eval()
    with pytest.raises(RuntimeError, match="E <= 2048"):
        m(torch.zeros(1, 3, dtype=torch.int64, device="cuda"))


@pytest.mark.parametrize("name", ["rows_4109", "one_symbol"])
def test_conv_predictor_backward_is_bit_reproducible(name):
    """Fixed summation orders through 16 slabs, 17 column-sum slabs and two list rounds: two backward passes agree bit for bit."""
    c = pc.build(name)
    m, inp = _module(c), _inputs(c)
    out_a, a = _run(m, *inp)
    out_b, b = _run(m, *inp)
    assert torch.equal(out_a, out_b)
    for k in po.PARAMS:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def _abi_run(c, fill):
    """rnnt_engine_conv_predictor_fwd / _bwd through the C ABI with `saved` and the 11 gradient buffers pre-filled with `fill`."""
    import rnnt_amd
    from rnnt_amd import engine
    from rnnt_amd.predictor import _struct
    lib = engine.lib()
    dev = torch.device("cuda", 0)
    fill32 = fill - (1 << 32) if fill >= (1 << 31) else fill
    params = [torch.from_numpy(v).cuda() for v in pc.state_dict(c).values()]
    ids, masks, G = _inputs(c)
    k1, k2 = masks if masks is not None else (None, None)
    n = ctypes.c_size_t(0)
    engine._check(lib.rnnt_engine_conv_predictor_saved_bytes(c.B, c.U1, c.S, c.E, c.O, ctypes.byref(n)))
    assert n.value % 4 == 0
    saved = torch.full((n.value // 4,), fill32, dtype=torch.int32, device=dev)
    out = torch.full((c.B, c.U1, c.O), fill32, dtype=torch.int32, device=dev).view(torch.float32)
    grads = [torch.full(p.shape, fill32, dtype=torch.int32, device=dev).view(torch.float32) for p in params]
    sp, sg = _struct(params), _struct(grads)
    with torch.cuda.device(dev):
        engine._check(lib.rnnt_engine_conv_predictor_fwd(
            engine._p(ids), c.B, c.U1, c.S, c.E, c.O, ctypes.byref(sp), engine._p(k1), engine._p(k2), ctypes.c_float(c.p),
            ctypes.c_float(1e-5), ctypes.c_float(1e-5), engine._p(out), engine._p(saved), ctypes.c_size_t(n.value), engine._stream(dev)))
        engine._check(lib.rnnt_engine_conv_predictor_bwd(
            engine._p(ids), c.B, c.U1, c.S, c.E, c.O, ctypes.byref(sp), engine._p(k1), engine._p(k2), ctypes.c_float(c.p),
            engine._p(G), ctypes.byref(sg), engine._p(saved), ctypes.c_size_t(n.value), engine._stream(dev)))
    torch.cuda.synchronize()
    return out, dict(zip(po.PARAMS, grads))


@pytest.mark.parametrize("name", ["rows_4109_b3", "short_segments_u3"])
def test_saved_buffer_and_gradient_buffers_are_scratch(name):
    """`saved` holds the backward's scratch (split-K slabs, column-sum slabs, dz / t) next to what the forward keeps, and the
    gradients are outputs: zeros, signalling NaNs or quiet NaNs in them beforehand change no bit of out or of any gradient."""
    c = pc.build(name)
    runs = [_abi_run(c, fill) for fill in (0, 0x7FA00000, 0xFFFFFFFF)]
    out0, g0 = runs[0]
    for out, g in runs[1:]:
        assert torch.equal(out.view(torch.int32), out0.view(torch.int32))
        for k in po.PARAMS:
            assert torch.equal(g[k].view(torch.int32), g0[k].view(torch.int32)), k
    assert torch.isfinite(out0).all() and all(torch.isfinite(g).all() for g in g0.values())
    _assert_oracle_bar(name, out0, g0)
