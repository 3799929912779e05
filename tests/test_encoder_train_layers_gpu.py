"""GPU tests of the encoder's training kernels layer by layer (rnnt_amd/csrc/encoder.hip through the C ABI rnnt_engine_encoder_train_*:
k_enc_norm<true>, k_enc_bwd_norm, k_enc_dw, k_enc_bwd_sum, the dX conv) against the float64 numpy oracle of
tests/encoder_train_cases.py, at the edges that module states and asserts on the plan mirror.  The bar of every tensor is
C.bars: 4 x max(the torch composition's own fp32 error against the oracle, one rounding of the largest entry); the exactly zero bias
gradient of a conv in front of an instance norm is held to M 2^-24 sum|dy| per channel.  Every comparison prints its figures.

The helper owns every buffer: `saved` and the workspace have exactly the bytes the size queries report, they, `out` and every
gradient are pre-filled with signalling NaNs and followed by guard words that must survive; so is the packed buffer.  Beside the results
abi_run hands back `saved`, the workspace after either call, the packed tables and the sizes the queries gave
(tests/golden/make_golden_encoder_bits.py pins their bytes)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import encoder_train_cases as C
from tests.encoder_layer_cases import AUTO, MANY_ROWS
from tests.test_encoder_layers_gpu import GUARD, SNAN, _buffer

pytestmark = pytest.mark.gpu


def abi_run(case, regime=AUTO):
    from rnnt_amd import engine
    from rnnt_amd.encoder import _Grads, _Layer
    lib = engine.lib()
    dev = torch.device("cuda", 0)
    nl, N, L = len(case.layers), case.N, case.L
    tp = C.train_plan(case.layers, N, L, case.lead, regime)
    hold, arr, grads = [], (_Layer * nl)(), (_Grads * nl)()

    def ptr(a):
        if a is None:
            return None
        hold.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        return hold[-1].data_ptr()

    gbuf = []
    for d, G, l in zip(arr, grads, case.layers):
        d.cin, d.cout, d.taps, d.stride, d.dilation, d.norm, d.role, d.eps = l.cin, l.cout, l.taps, l.stride, l.dil, l.norm, l.role, l.eps
        d.weight, d.bias, d.gamma, d.beta, d.mean, d.var = ptr(l.W), ptr(l.b), ptr(l.gamma), ptr(l.beta), ptr(l.mean), ptr(l.var)
        g = {"W": _buffer(l.W.size, SNAN, dev), "b": _buffer(l.cout, SNAN, dev),
             "gamma": _buffer(l.cout, SNAN, dev) if l.gamma is not None else None,
             "beta": _buffer(l.cout, SNAN, dev) if l.beta is not None else None}
        G.weight, G.bias = g["W"].data_ptr(), g["b"].data_ptr()
        G.gamma = None if g["gamma"] is None else g["gamma"].data_ptr()
        G.beta = None if g["beta"] is None else g["beta"].data_ptr()
        gbuf.append(g)
    x = torch.from_numpy(case.x).to(dev).contiguous()
    strides = (ctypes.c_int64 * 3)(*x.stride())
    lead = (ctypes.c_int32 * nl)(*case.lead)
    keep = (ctypes.c_void_p * nl)(*[ptr(k) for k in case.keep])
    p = (ctypes.c_float * nl)(*case.p)
    dout = torch.from_numpy(case.G).to(dev).contiguous()
    cout, n_out = case.layers[-1].cout, N * tp.L_final * case.layers[-1].cout
    with torch.cuda.device(dev):
        n = ctypes.c_size_t(0)
        engine._check(lib.rnnt_engine_encoder_train_packed_bytes(arr, nl, ctypes.byref(n)))
        n_packed = n.value
        packed = _buffer(n_packed // 4, SNAN, dev)
        engine._check(lib.rnnt_engine_encoder_train_pack(arr, nl, engine._p(packed), ctypes.c_size_t(n_packed), engine._stream(dev)))
        engine._check(lib.rnnt_engine_encoder_train_saved_bytes(arr, nl, N, L, lead, ctypes.byref(n)))
        assert n.value == tp.saved_bytes
        sv = n.value
        engine._check(lib.rnnt_engine_encoder_train_workspace_bytes(arr, nl, N, L, regime, lead, ctypes.byref(n)))
        assert n.value == tp.ws_bytes
        saved, ws, out = _buffer(sv // 4, SNAN, dev), _buffer(n.value // 4, SNAN, dev), _buffer(n_out, SNAN, dev)
        engine._check(lib.rnnt_engine_encoder_train_fwd(arr, nl, engine._p(packed), engine._p(x), strides, N, L, lead, keep, p, regime,
                                                        engine._p(out), engine._p(saved), ctypes.c_size_t(sv), engine._p(ws),
                                                        ctypes.c_size_t(n.value), engine._stream(dev)))
        ws_fwd = ws[:n.value // 4].clone()
        ws[:n.value // 4] = SNAN  # the workspace carries nothing from the forward to the backward
        engine._check(lib.rnnt_engine_encoder_train_bwd(arr, nl, engine._p(packed), engine._p(x), strides, N, L, lead, keep, p,
                                                        engine._p(dout), engine._p(saved), ctypes.c_size_t(sv), grads, engine._p(ws),
                                                        ctypes.c_size_t(n.value), engine._stream(dev)))
    torch.cuda.synchronize()
    named = [("out", out, n_out), ("saved", saved, sv // 4), ("workspace", ws, n.value // 4), ("packed", packed, n_packed // 4)]
    for i, (g, l) in enumerate(zip(gbuf, case.layers)):
        named += [(f"grad {k} of layer {i}", t, l.W.size if k == "W" else l.cout) for k, t in g.items() if t is not None]
    for what, t, words in named:
        assert bool((t[words:] == GUARD).all()), f"{case.name}: the guard words behind {what} were written"
    res = []
    for g, l in zip(gbuf, case.layers):
        res.append({k: None if t is None else t[:(l.W.size if k == "W" else l.cout)].view(torch.float32).cpu().numpy().reshape(
            l.W.shape if k == "W" else (l.cout,)) for k, t in g.items()})
    return SimpleNamespace(out=out[:n_out].view(torch.float32).view(N, tp.L_final, cout).cpu().numpy(), grads=res,
                           saved=saved[:sv // 4], workspace_fwd=ws_fwd, workspace_bwd=ws[:n.value // 4], packed=packed[:n_packed // 4],
                           sizes=dict(train_packed_bytes=n_packed, train_saved_bytes=sv, train_workspace_bytes=n.value))


def _compare(case, want, bars, got, label):
    out_bar, gbars = bars
    bad = []
    e = float(np.abs(got.out.astype(np.float64) - want.out).max())
    print(f"encoder train layers {label} out: engine max|y - fp64| = {e:.3e}, bar = {out_bar:.3e}")
    if not e <= out_bar:
        bad.append(("out", e, out_bar))
    for i, (g, w, b) in enumerate(zip(got.grads, want.grads, gbars)):
        for k in C.GRAD_KEYS:
            if w[k] is None:
                assert g[k] is None
                continue
            assert np.isfinite(g[k]).all(), (label, i, k)
            d = np.abs(g[k].astype(np.float64) - w[k])
            bar = np.asarray(b[k])
            print(f"encoder train layers {label} layer {i} d{k}: engine max|g - fp64| = {d.max():.3e}, bar = {bar.min():.3e}"
                  + (" (exactly zero: M 2^-24 sum|dy|)" if bar.ndim else ""))
            if not np.all(d <= bar):
                bad.append((i, k, float(d.max()), float(bar.min())))
    assert not bad, (label, bad)


@pytest.mark.parametrize("name,kind", C.case_ids())
def test_forward_and_backward_against_the_float64_oracle(name, kind):
    case, want, bars = C.prepared(name, kind)
    C.check_reach(case)
    _compare(case, want, bars, abi_run(case), f"{name} [{kind}]")


def test_forward_regimes_and_repeat_calls_give_the_same_bits():
    """The backward never depends on the forward's conv kernel beyond the forward's own bits; two identical calls agree bit for bit."""
    case, want, bars = C.prepared("triple_dropout", "instance")
    a, b = abi_run(case), abi_run(case)
    assert np.array_equal(a.out, b.out)
    for ga, gb in zip(a.grads, b.grads):
        assert all(np.array_equal(ga[k], gb[k]) for k in ga if ga[k] is not None)
    _compare(case, want, bars, abi_run(case, MANY_ROWS), "triple_dropout [instance] many_rows")
