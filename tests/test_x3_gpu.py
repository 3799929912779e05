"""-m gpu: what is specific to the RNNT_DTYPE_F32_BF16X3 route (rnnt_amd/csrc/x3.hip: fp32-accurate products as six
bf16 MFMA products of 3-way split operands).  The route is held to EXACTLY the fp32 route's bar by
tests/test_gpu_parity.py itself: every fp32-bar test there takes the `route` fixture ("fp32", "bf16x3") — shape
list, ragged / random / poisoned batches, the golden fixtures, configs 1, 2, 4 and 5 at full size — at the unchanged
1e-4 tolerances (tests/helpers.py LOSS_RTOL / GRAD_RTOL) against the plain fp64 oracle (no rounding-point oracle:
the route claims fp32 accuracy).  Here: each bf16x3 kernel checked in isolation (the other stages on the fp32
route's kernels, RNNT_VARIANT_X3_FP32_*), its measured error beside the fp32-MFMA route's on the same inputs,
dense full-size data against the fp32-MFMA route, reproducibility / graph capture, the C boundary's checks."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import (GRAD_RTOL, LOSS_RTOL, assert_close_grad, assert_close_loss, make_inputs, oracle_fused)
from tests.test_gpu_parity import _dev, _run_fused

pytestmark = pytest.mark.gpu
X3 = "bf16x3"


@pytest.fixture(scope="module")
def amd():
    import rnnt_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    rnnt_amd.engine.lib()
    return rnnt_amd


@pytest.fixture(scope="module")
def golden_dir():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("variant", ["dw_only", "dw_dhidden", "all"])
@pytest.mark.parametrize("shape", [(2, 9, 4, 128, 128), (3, 23, 19, 256, 384), (2, 40, 33, 512, 1024), (2, 13, 20, 1024, 256),
                                   (3, 21, 9, 640, 128), (2, 130, 50, 512, 256)])
def test_x3_kernels_in_isolation(amd, variant, shape):
    """One bf16x3 kernel at a time: with RNNT_VARIANT_X3_FP32_FWD | _DH only k_dw_x3 runs (forward and dHidden
    on the fp32 route's kernels, plain splitting kernels in between), with _FWD alone k_dhidden_x3 + k_dw_x3,
    without a variant all three — each against the fp64 oracle at the fp32 tolerances."""
    e = amd.engine
    var = {"dw_only": e.VARIANT_X3_FP32_FWD | e.VARIANT_X3_FP32_DH, "dw_dhidden": e.VARIANT_X3_FP32_FWD, "all": 0}[variant]
    B, T, U, H, V = shape
    d = make_inputs(B, T, U, H, V, seed=sum(shape))
    g = _dev(d)
    outs = e.joint_loss_fwd_bwd(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"],
                                V - 1, 1.0 / B, dtype=X3, variant=var)
    torch.cuda.synchronize()
    ref = oracle_fused(d)
    assert_close_loss("costs", outs[0].cpu().numpy(), ref["costs"])
    for o, k in zip(outs[1:], ("grad_enc", "grad_pred", "grad_W", "grad_bias")):
        assert_close_grad(k, o.cpu().numpy(), ref[k])


def test_x3_error_beside_the_fp32_mfma_route(amd):
    """Both routes against the fp64 oracle on the same inputs (a lattice of 10 k cells at config 2's H, V): the
    bf16x3 route stays inside the fp32 bar with the same two orders of magnitude to spare as the fp32-MFMA route
    (errors of a few 1e-7 of the largest gradient entry on both; the numbers go to stdout for DESIGN.md)."""
    d = make_inputs(4, 100, 24, 512, 1024, seed=1234)
    ref = oracle_fused(d)
    err = {}
    for dt in ("fp32", X3):
        r = _run_fused(amd, d, dt)
        err[dt] = {k: float(np.abs(r[k] - ref[k]).max() / np.abs(ref[k]).max()) for k in ("grad_enc", "grad_pred", "grad_W", "grad_bias")}
        err[dt]["loss"] = abs(r["loss"] - ref["loss"]) / abs(ref["loss"])
    print("\nerror vs fp64 oracle:", {dt: {k: "%.1e" % v for k, v in e.items()} for dt, e in err.items()})
    for k, v in err[X3].items():
        assert v < 0.05 * GRAD_RTOL, (k, v)              # 20x inside the 1e-4 bar
        # same error class as the exact-fp32 MFMA route (<= 2x): within 2.5x of its error — or of one fp32
        # rounding (6e-8) where that route is more accurate than a single rounding (its bias gradient: 2.5e-9)
        assert v < 2.5 * max(err["fp32"][k], 6e-8), (k, v, err["fp32"][k])


def test_x3_fullsize_config2_vs_fp32(amd):
    """BASELINE config 2 at full size (B=32,T=1000,U=200,H=512,V=1024): dense ragged data against the fp32-MFMA
    route at the fp32 tolerances (row offsets beyond 2^31 bytes, every tile / pass / split).  (The closed-form
    loss at full size: tests/test_gpu_parity.py::test_fullsize_config2_closed_form[bf16x3].)"""
    d = make_inputs(32, 1000, 200, 512, 1024, seed=32)
    amd.engine.release_workspaces()
    ref = _run_fused(amd, d, "fp32")
    amd.engine.release_workspaces()
    r = _run_fused(amd, d, X3)
    amd.engine.release_workspaces()
    assert_close_loss("costs", r["costs"], ref["costs"], rtol=LOSS_RTOL)
    for k in ("grad_enc", "grad_pred", "grad_W", "grad_bias"):
        assert_close_grad(k, r[k], ref[k], rtol=GRAD_RTOL)


def test_x3_reference_joint_width_vs_fp32(amd):
    """The reference's real joint width (hidden_features: 1024) at a training-sized ragged batch, against the
    fp32-MFMA route."""
    d = make_inputs(8, 500, 100, 1024, 1024, seed=11)
    ref = _run_fused(amd, d, "fp32")
    r = _run_fused(amd, d, X3)
    assert_close_loss("costs", r["costs"], ref["costs"], rtol=LOSS_RTOL)
    for k in ("grad_enc", "grad_pred", "grad_W", "grad_bias"):
        assert_close_grad(k, r[k], ref[k], rtol=GRAD_RTOL)
    amd.engine.release_workspaces()


def test_x3_is_bitwise_reproducible_and_graph_capturable(amd):
    """Fixed summation orders: two eager calls agree bit for bit; a captured call replayed on new buffer
    contents gives the eager answer bit for bit (kernel nodes only, no memset / memcpy nodes)."""
    B, T, U, H, V = 3, 40, 12, 256, 512
    d1, d2 = make_inputs(B, T, U, H, V, seed=501), make_inputs(B, T, U, H, V, seed=502)
    g = _dev(d1)
    e = amd.engine
    run = lambda outs=None: e.joint_loss_fwd_bwd(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"],
                                                 g["target_lens"], V - 1, 0.25, outs=outs, dtype=X3)
    a = [o.clone() for o in run()]
    b = [o.clone() for o in run()]
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        outs = run()  # warm-up on the capture stream (sizes its workspace)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            run(outs)
    for k, v in _dev(d2).items():
        g[k].copy_(v)
    graph.replay()
    torch.cuda.synchronize()
    want = run()
    torch.cuda.synchronize()
    for x, y in zip(outs, want):
        assert torch.equal(x, y)
    ref = oracle_fused(d2)
    assert_close_loss("costs", want[0].cpu().numpy(), ref["costs"])


def test_x3_rejects_unsupported_dims_at_the_c_abi(amd):
    """include/rnnt_engine.h: RNNT_DTYPE_F32_BF16X3 needs H % 128 == 0 and V % 128 == 0 at the C boundary (the
    Python operator pads); a variant that runs a stage on the fp32 kernels needs the larger workspace."""
    d = make_inputs(2, 9, 4, 64, 128, seed=1)
    g = _dev(d)
    with pytest.raises(RuntimeError, match="RNNT_DTYPE_F32_BF16X3"):
        amd.engine.joint_loss_fwd_bwd(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"],
                                      g["target_lens"], 127, 0.5, dtype=X3)
