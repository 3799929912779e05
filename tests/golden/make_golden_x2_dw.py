"""Record what the f16x2 dW GEMM (rnnt_amd/csrc/x2.hip: k_dw_x2<4>, k_dw_x2<4, true>, k_dw_x2m) leaves behind, for
tests/test_x2_dw_bits_gpu.py: every kernel form and every branch of the k-step pipeline the three share (rnnt_amd/csrc/split_dw.hpp: dw_kstep2, dw_ring) — several h blocks (db from
blocks 0 and 1, operand tiles shared between workgroups under the lockstep), empty split shares, a walk longer than the ring, the
walk without the flush rule, and the Linear layer's lists (identity, padding rows) — so that the kernels' source can be rearranged
freely as long as every case keeps every bit of dW and db (the route is bitwise reproducible: fixed list order, fixed slab order).

Run once on a GPU with the library whose output is the reference (RNNT_ENGINE_LIB = the build of the commit BEFORE the change):
    python tests/golden/make_golden_x2_dw.py
writes tests/golden/x2_dw.npz.  Per case `<name>`: /costs raw (uint32), /grad_enc, /grad_pred, /grad_W, /grad_bias (fused step) or
/dx, /dW, /db (Linear backward) as SHA-256.  Workspace and output buffers hold the quiet-NaN pattern of
make_golden_fused_routes.py before a call (the Linear layer allocates its own outputs: its workspace does).  A case is written only
if it passes its parity bar — the fused step against oracle_fused at the bars of tests/test_x2_gpu.py, the Linear backward against
float64 torch at those of tests/test_linear_abi_gpu.py — so a broken build cannot be recorded, and only after the library's own
tile count (x2_dw_tiles, through the workspace layout: host code) says the case runs the kernel form it is listed for.
This module is also the test's source of the cases and of the code that runs them (the test loads it by path).
"""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.helpers import GRAD_RTOL, LOSS_RTOL, assert_close_grad, assert_close_loss, make_inputs, oracle_fused  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_golden_fused_routes", os.path.join(HERE, "make_golden_fused_routes.py"))
F = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(F)

GOLDEN = os.path.join(HERE, "x2_dw.npz")
GRADS = F.GRADS
LINEAR_OUT = ("dx", "dW", "db")

# kernel forms: launch_dw_x2's choice for (H, V)
WHOLE, PARTH, MIXED = "k_dw_x2<4>", "k_dw_x2<4, true>", "k_dw_x2m"

# name -> (kind, shape, variant, kernel form).  fused: (B, T, U, H, V), inputs make_inputs(seed = sum of the shape, ragged);
# linear: (M, K, N), the dW kernel's H = K, V = N, operands seeded with the sum of the shape
CASES = {
    "blocks_2x2": ("fused", (2, 9, 6, 512, 512), 0, WHOLE),          # db from h blocks 0 and 1, tiles in lockstep
    "mixed_3h_2tall": ("fused", (2, 9, 6, 896, 1024), 0, MIXED),     # three whole h blocks, two tall tiles; 18 splits of ~8 k-steps: empty shares
    "wrap_whole": ("fused", (1, 2, 127, 512, 512), 0, WHOLE),        # 256 cells in <= 2 splits: a split walks ~8 k-steps, twice round the ring
    "wrap_parth": ("fused", (1, 2, 127, 384, 256), 0, PARTH),
    "wrap_mixed": ("fused", (1, 2, 127, 640, 512), 0, MIXED),
    "mixed_no_flush_skip": ("fused", (2, 9, 6, 640, 512), F.X2_NO_FLUSH_SKIP, MIXED),  # the walk over every k-step, flushed cells included
    "linear_identity": ("linear", (18, 256, 128), 0, WHOLE),         # the identity list; one h block: two db tiles per wave
    "linear_padding": ("linear", (130, 384, 128), 0, PARTH),         # 130 rows: a half group of padding rows
    "linear_mixed": ("linear", (70, 640, 512), 0, MIXED),            # k_dw_x2m reached from the Linear layer
}


def kernel_form(H, V):
    """(form, workgroup tiles per split) of launch_dw_x2 at (H, V): x2_dw_mixed_ok / x2_dw_tiles, by their definitions."""
    if H % 256 == 128 and H >= 640 and V % 512 == 0:
        return MIXED, (V // 256) * (H // 256) + V // 512
    nv, nh = (V + 255) // 256, (H + 255) // 256
    return (PARTH if H % 256 else WHOLE), nv * nh


def check_form(lib, name):
    """The case reaches the kernel form it is listed for: kernel_form says so, and the library's x2_dw_tiles agrees with kernel_form's
    tile count — read off the split count 256 // tiles of a workspace layout large enough not to cap it (tests/test_abi.py).  Host
    code only."""
    from rnnt_amd.engine import WsLayout, dtype_code
    kind, shape, _, form = CASES[name]
    H, V = shape[-2:]
    got, tiles = kernel_form(H, V)
    assert got == form, (name, got, form)
    L = WsLayout()
    assert lib.rnnt_engine_workspace_layout(8, 4000, 601, H, V, dtype_code("f16x2"), ctypes.byref(L)) == 0
    assert L.n_split == 256 // tiles, (name, L.n_split, tiles)
    other = (V + 255) // 256 * ((H + 255) // 256)  # the tile count without tall tiles gives another split count: the check tells the forms apart
    assert form != MIXED or 256 // other != 256 // tiles, name


def linear_operands(name):
    M, K, N = CASES[name][1]
    rng = np.random.default_rng(M + K + N)
    x = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    dy = rng.standard_normal((M, N)).astype(np.float32)
    return x, W, b, dy


def run_case(engine, name):
    """One run of a case over a poisoned workspace -> dict of numpy arrays (as uint32)."""
    import rnnt_amd
    kind, shape, variant, _ = CASES[name]
    dev = torch.device("cuda:0")
    if kind == "linear":
        M, K, N = shape
        x, W, b, dy = (torch.from_numpy(a).to(dev) for a in linear_operands(name))
        n = ctypes.c_size_t(0)
        engine._check(engine.lib().rnnt_engine_linear_x2_workspace_bytes(M, K, N, 1, ctypes.byref(n)))
        F._poison(engine, dev, n.value)
        x.requires_grad_(True), W.requires_grad_(True), b.requires_grad_(True)
        rnnt_amd.linear(x, W, b, backend="x2").backward(dy)
        r = dict(zip(LINEAR_OUT, (x.grad, W.grad, b.grad)))
    else:
        B, T, U, H, V = shape
        g = {k: torch.from_numpy(v).to(dev) for k, v in make_inputs(B, T, U, H, V, seed=sum(shape), ragged=True).items()}
        U1 = U + 1
        L = engine.layout(B, T, U1, H, V, "f16x2")
        F._poison(engine, dev, L.total + L.aux_bytes)
        outs = (F._poisoned((B,), dev), F._poisoned((B, T, H), dev), F._poisoned((B, U1, H), dev), F._poisoned((V, H), dev), F._poisoned((V,), dev))
        engine.joint_loss_fwd_bwd(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"], V - 1, 1.0 / B,
                                  outs=outs, dtype="f16x2", variant=variant)
        r = dict(zip(("costs",) + GRADS, outs))
    torch.cuda.synchronize()
    return {k: t.cpu().numpy().view(np.uint32) for k, t in r.items()}


def check_parity(name, result):
    kind, shape, _, _ = CASES[name]
    if kind == "linear":
        x, W, b, dy = (torch.from_numpy(a).double().requires_grad_(True) for a in linear_operands(name))
        (torch.nn.functional.linear(x, W, b) * dy.detach()).sum().backward()
        for k, t in zip(LINEAR_OUT, (x, W, b)):
            assert_close_grad(name + " " + k, result[k].view(np.float32), t.grad.numpy())
    else:
        ref = oracle_fused(make_inputs(*shape, seed=sum(shape), ragged=True), blank=shape[4] - 1)
        assert_close_loss(name + " costs", result["costs"].view(np.float32), ref["costs"], rtol=LOSS_RTOL)
        for k in GRADS:
            assert_close_grad(name + " " + k, result[k].view(np.float32), ref[k], rtol=GRAD_RTOL)


def main():
    import rnnt_amd
    e = rnnt_amd.engine
    e.lib()
    print("recording from %s" % e.LIB_PATH, flush=True)
    out = {}
    for name in CASES:
        check_form(e.lib(), name)
        res = run_case(e, name)
        check_parity(name, res)
        for k, a in F.recorded(res).items():
            out["%s/%s" % (name, k)] = a
        print("%-22s %-18s parity ok %s" % (name, CASES[name][3], sorted(res)), flush=True)
    np.savez_compressed(GOLDEN, **out)
    print("%d cases -> %s (%d bytes)" % (len(CASES), GOLDEN, os.path.getsize(GOLDEN)), flush=True)


if __name__ == "__main__":
    main()
