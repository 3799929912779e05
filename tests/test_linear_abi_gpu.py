"""-m gpu: rnnt_engine_linear_fwd / _bwd (fp32-MFMA small-GEMM kernels) and rnnt_engine_linear_x2_fwd / _bwd (f16x2 matrix pipes)
called directly through the C ABI, for what rnnt_amd.linear never hands them: a row stride ldx != K (engine._rows gathers every
row-strided slice into contiguous rows first), NULL dx / db, a poisoned backward workspace; and the fp32 backend at a training
row count (16 weight-gradient splits, odd M, an N tail).  Reference: float64 torch, at the bars of tests/test_predictor_gpu.py."""
import ctypes

import pytest
import torch

from tests.helpers import assert_close_grad

pytestmark = pytest.mark.gpu

PAD = 8  # padding columns of the strided x buffer
Y_RTOL = {"fp32": 1e-5, "x2": 1e-4}  # test_engine_linear_fwd_bwd_vs_torch / test_engine_linear_x2_fwd_bwd_vs_float64; gradients: 1e-4


def _poison(t, pattern):
    t.view(torch.int32)[: t.numel() // 4].fill_(pattern - (1 << 32) if pattern >= (1 << 31) else pattern)


def _call(backend, x, ldx, W, b, dy, M, K, N, dx=True, db=True, poison=None):
    """(y, dx, dW, db) of one forward + backward through the C ABI; x is any tensor whose rows start ldx floats apart.  The outputs
    start as NaN so that an entry a kernel leaves out cannot pass; `poison`: an int32 pattern the backward workspace is filled with."""
    from rnnt_amd import engine
    lib, dev, p = engine.lib(), x.device, engine._p
    nan = float("nan")
    y = torch.full((M, N), nan, device=dev)
    gx = torch.full((M, K), nan, device=dev) if dx else None
    gW = torch.full((N, K), nan, device=dev)
    gb = torch.full((N,), nan, device=dev) if db else None
    n = ctypes.c_size_t(0)
    with torch.cuda.device(dev):
        st = engine._stream(dev)
        if backend == "x2":
            engine._check(lib.rnnt_engine_linear_x2_workspace_bytes(M, K, N, 0, ctypes.byref(n)))
            ws = torch.zeros(n.value, dtype=torch.uint8, device=dev)
            engine._check(lib.rnnt_engine_linear_x2_fwd(p(x), ctypes.c_int64(ldx), p(W), p(b), M, K, N, p(y), p(ws), ctypes.c_size_t(n.value), st))
            engine._check(lib.rnnt_engine_linear_x2_workspace_bytes(M, K, N, 1, ctypes.byref(n)))
        else:
            engine._check(lib.rnnt_engine_linear_fwd(p(x), ctypes.c_int64(ldx), p(W), p(b), M, K, N, p(y), st))
            engine._check(lib.rnnt_engine_linear_bwd_workspace_bytes(M, K, N, ctypes.byref(n)))
        ws = torch.zeros(n.value, dtype=torch.uint8, device=dev)
        if poison is not None:
            _poison(ws, poison)
        bwd = lib.rnnt_engine_linear_x2_bwd if backend == "x2" else lib.rnnt_engine_linear_bwd
        engine._check(bwd(p(x), ctypes.c_int64(ldx), p(W), p(dy), M, K, N, p(gx), p(gW), p(gb), p(ws), ctypes.c_size_t(n.value), st))
    torch.cuda.synchronize()
    return y, gx, gW, gb


def _operands(M, K, N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(M, K, device="cuda", generator=g)
    W = torch.randn(N, K, device="cuda", generator=g) / K ** 0.5
    b = torch.randn(N, device="cuda", generator=g)
    dy = torch.randn(M, N, device="cuda", generator=g)
    return x, W, b, dy


def _same_bits(name, a, b):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name


def _assert_float64_bar(backend, x, W, b, dy, got):
    x64, W64, b64 = (t.detach().double().requires_grad_(True) for t in (x, W, b))
    ref = torch.nn.functional.linear(x64, W64, b64)
    (ref * dy.double()).sum().backward()
    assert_close_grad("y", got[0].cpu().numpy(), ref.detach().cpu().numpy(), rtol=Y_RTOL[backend])
    for name, g, r in zip(("dx", "dW", "db"), got[1:], (x64, W64, b64)):
        assert_close_grad(name, g.cpu().numpy(), r.grad.cpu().numpy())


@pytest.mark.parametrize("backend,M,K,N", [("fp32", 37, 24, 32), ("fp32", 130, 20, 36), ("x2", 130, 384, 128), ("x2", 513, 640, 1152)])
def test_row_stride(backend, M, K, N):
    """x inside a buffer of K + 8 columns (ldx = K + 8) whose padding columns hold NaN, then 1e30: no kernel reads them — the
    magnitude scan, the forward GEMM, the weight gradient's operand (k_sgemm_tn / k_x2_split_rows) all give the bits they give
    on a contiguous copy — and the results are within the bars of float64 torch."""
    x, W, b, dy = _operands(M, K, N, M + K + N)
    want = _call(backend, x, K, W, b, dy, M, K, N)
    _assert_float64_bar(backend, x, W, b, dy, want)
    for pad in (float("nan"), 1e30):
        xbuf = torch.full((M, K + PAD), pad, device="cuda")
        xbuf[:, :K] = x
        assert xbuf.stride(0) == K + PAD and xbuf.data_ptr() % 16 == 0
        got = _call(backend, xbuf, K + PAD, W, b, dy, M, K, N)
        for name, g, w in zip(("y", "dx", "dW", "db"), got, want):
            _same_bits("%s (padding %r)" % (name, pad), g, w)


@pytest.mark.parametrize("backend,M,K,N", [("fp32", 130, 20, 36), ("x2", 130, 384, 128)])
def test_null_outputs(backend, M, K, N):
    """dx == NULL, db == NULL, both: the outputs that remain keep their bits."""
    x, W, b, dy = _operands(M, K, N, 7)
    full = _call(backend, x, K, W, b, dy, M, K, N)
    for dx, db in ((False, True), (True, False), (False, False)):
        y, gx, gW, gb = _call(backend, x, K, W, b, dy, M, K, N, dx=dx, db=db)
        assert (gx is None) == (not dx) and (gb is None) == (not db)
        _same_bits("y", y, full[0])
        _same_bits("dW", gW, full[2])
        if dx:
            _same_bits("dx", gx, full[1])
        if db:
            _same_bits("db", gb, full[3])


@pytest.mark.parametrize("backend,M,K,N", [("fp32", 130, 20, 36), ("x2", 130, 384, 128)])
def test_need_dx_false_through_python(backend, M, K, N):
    """rnnt_amd.linear with an input that needs no gradient: backward passes dx = NULL (need_dx=False), x.grad stays None and
    W.grad / b.grad are what they are when x does require one."""
    import rnnt_amd
    x, W, b, dy = _operands(M, K, N, 11)
    grads = []
    for need in (True, False):
        xr = x.clone().requires_grad_(need)
        Wr, br = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
        rnnt_amd.linear(xr, Wr, br, backend=backend).backward(dy)
        assert (xr.grad is None) == (not need)
        grads.append((Wr.grad, br.grad))
    _same_bits("W.grad", grads[0][0], grads[1][0])
    _same_bits("b.grad", grads[0][1], grads[1][1])


def test_fp32_backend_at_training_rows():
    """M = 4109 (odd, ceil(M/256) = 17 > 16), K = 128, N = 132: one split's grid is ceil(132/128) * ceil(128/128) = 2 workgroups, so
    by_fill = 128 and the weight gradient runs at the cap of 16 splits over uneven ranges, with a 4-column N tail in every GEMM."""
    from tests.predictor_cases import tn_splits_for
    M, K, N = 4109, 128, 132
    assert tn_splits_for(M, N, K, 1) == 16 and M % 2 == 1 and N % 128 == 4
    x, W, b, dy = _operands(M, K, N, 4109)
    _assert_float64_bar("fp32", x, W, b, dy, _call("fp32", x, K, W, b, dy, M, K, N))


@pytest.mark.parametrize("pattern", [0x7FA00000, 0xFFFFFFFF])
@pytest.mark.parametrize("backend,M,K,N", [("fp32", 513, 128, 132), ("x2", 513, 640, 1152)])
def test_poisoned_backward_workspace_does_not_leak(backend, M, K, N, pattern):
    """The backward workspace is caller-owned scratch (split-K slabs, column-sum slabs; planes, packs, tables, progress words on the
    f16x2 route): signalling or quiet NaNs in it beforehand change no bit of any result."""
    x, W, b, dy = _operands(M, K, N, 513)
    clean = _call(backend, x, K, W, b, dy, M, K, N)
    got = _call(backend, x, K, W, b, dy, M, K, N, poison=pattern)
    for name, g, w in zip(("y", "dx", "dW", "db"), got, clean):
        assert torch.isfinite(g).all(), name
        _same_bits(name, g, w)
