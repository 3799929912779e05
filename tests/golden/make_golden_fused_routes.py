"""Record what every route of the fused joint+loss step leaves behind, for tests/test_fused_routes_bits_gpu.py: the host code
that validates a call, carves the workspace and sequences the kernels (rnnt_amd/csrc/engine.hip) can be rearranged freely as
long as every case below keeps every bit.

Run once on a GPU with the library whose output is the reference (RNNT_ENGINE_LIB = the build of the commit BEFORE the change):
    python tests/golden/make_golden_fused_routes.py
writes tests/golden/fused_routes.npz.  Per case `<name>`:
  <name>/costs, /scores   raw, as uint32;  <name>/frames  int32
  <name>/grad_enc, /grad_pred, /grad_W, /grad_bias, /logits, /grad_logits   SHA-256 (tests.helpers.sha256_of_arrays)
The whole workspace (and every output buffer) holds the quiet NaN PATTERN before a call: a carve that moved reads poison.
A case of the plain loss is written only if it passes the route's parity bar against the fp64 oracle (oracle_fused; the bars of
tests/test_gpu_parity.py / test_x3_gpu.py / test_x2_gpu.py), so a broken build cannot be recorded.
This module is also the test's source of the cases and of the code that runs them (the test loads it by path).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.helpers import (BF16_GRAD_RTOL_EXACT, BF16_LOSS_RTOL_EXACT, GRAD_RTOL, LOSS_RTOL, assert_close_grad,  # noqa: E402
                           assert_close_loss, make_inputs, oracle_fused, relabel_blank, sha256_of_arrays)
from tests.x2_live_list_cases import TINY  # noqa: E402

GOLDEN = os.path.join(HERE, "fused_routes.npz")
PATTERN = 0x7FC0BEEF  # a quiet NaN no kernel produces
GRADS = ("grad_enc", "grad_pred", "grad_W", "grad_bias")
RAW = ("costs", "scores", "frames")  # stored as they are; everything else as a SHA-256

# include/rnnt_engine.h RNNT_VARIANT_*
SEPARATE_G, SEPARATE_HIDDEN, FWD_LDS_RING, FWD_ONE_WG_PER_TILE, X2_NO_FLUSH_SKIP, X3_FP32_FWD, X3_FP32_DH = 32, 64, 128, 256, 512, 4096, 8192

# route -> shapes (B, T, U, H, V), the smallest first (U1 = U + 1; inputs: make_inputs(seed = sum of the shape, ragged))
SHAPES = {
    "fp32": [(2, 9, 6, 64, 32),    # G inside the tile kernel, 8-wide u tiles
             (2, 8, 16, 64, 32),   # 16-wide u tiles
             (2, 9, 6, 64, 28),    # V % 32 != 0: k_make_g + the persistent dHidden on every column
             (2, 9, 6, 640, 32),   # one 512-column group on the tile kernel, the rest persistent
             (1, 9, 6, 1024, 32)],  # two column groups on the tile kernel
    "bf16": [(2, 9, 6, 128, 128), (2, 9, 6, 256, 384)],
    "bf16x3": [(2, 9, 6, 128, 128), (2, 9, 6, 640, 256)],
    "f16x2": [(2, 9, 6, 128, 128),
              (2, 9, 6, 384, 256),   # H % 256 == 128, group walk
              (2, 9, 6, 640, 512)],  # k_dw_x2m, the k-step walk
}
# variants run at a route's smallest shape (through rnnt_engine_run_stages)
VARIANTS = {
    "fp32": {"separate_g": SEPARATE_G, "separate_hidden": SEPARATE_HIDDEN, "fwd_lds_ring": FWD_LDS_RING,
             "fwd_one_wg_per_tile": FWD_ONE_WG_PER_TILE},
    "bf16": {},
    "bf16x3": {"fp32_fwd": X3_FP32_FWD, "fp32_fwd_dh": X3_FP32_FWD | X3_FP32_DH},  # the last: a workspace of total + aux_bytes
    "f16x2": {"no_flush_skip": X2_NO_FLUSH_SKIP, "fp32_fwd": X3_FP32_FWD, "fp32_fwd_dh": X3_FP32_FWD | X3_FP32_DH},
}
# per route, at its smallest shape
MODES = ("permuted_enc", "blank0", "reg", "fwd_only", "align", "stage_by_stage")
STANDALONE = ("joint_fwd", "joint_bwd", "loss_clamp", "align")  # fp32 at SHAPES["fp32"][0]
FASTEMIT, DELAY, CLAMP = 0.01, 0.005, 0.5


def _cases():
    """name -> (route, shape, seed, mode, variant); mode "fused": the whole call."""
    c = {}
    for route, shapes in SHAPES.items():
        for s in shapes:
            c["%s_%s" % (route, "x".join(map(str, s)))] = (route, s, sum(s), "fused", 0)
        s = shapes[0]
        for vname, v in VARIANTS[route].items():
            c["%s_variant_%s" % (route, vname)] = (route, s, sum(s), "fused", v)
        for m in MODES:
            c["%s_%s" % (route, m)] = (route, s, sum(s), m, 0)
    c["f16x2_tiny_dead_tiles"] = ("f16x2", TINY[:5], TINY[5], "fused", 0)  # dead tiles: the flagged reductions and k_x2_dead_rows
    for m in STANDALONE:
        c["standalone_%s" % m] = ("fp32", SHAPES["fp32"][0], sum(SHAPES["fp32"][0]), "standalone_" + m, 0)
    return c


CASES = _cases()
# the case whose bytes a stage-by-stage run must reproduce
WHOLE_CALL_OF = {"%s_stage_by_stage" % r: "%s_%s" % (r, "x".join(map(str, SHAPES[r][0]))) for r in SHAPES}


def case_inputs(name):
    """(numpy inputs, blank) of a case."""
    route, (B, T, U, H, V), seed, mode, _ = CASES[name]
    d = make_inputs(B, T, U, H, V, seed=seed, ragged=True)
    if mode == "blank0":
        d, _ = relabel_blank(d, 0)
        return d, 0
    return d, V - 1


def _poison(engine, dev, nbytes):
    """The stream's (grow-only) workspace, at least nbytes of it, every word PATTERN."""
    ws = engine.workspace(dev, max(int(nbytes), 1 << 22))
    ws[:ws.numel() // 4 * 4].view(torch.int32).fill_(PATTERN)


def _poisoned(shape, dev, dtype=torch.float32):
    return torch.full(shape, PATTERN, dtype=torch.int32, device=dev).view(dtype)


def run_case(engine, name):
    """One run of a case over a poisoned workspace -> dict of numpy arrays (float outputs as uint32)."""
    route, (B, T, U, H, V), _, mode, variant = CASES[name]
    d, blank = case_inputs(name)
    dev = torch.device("cuda:0")
    g = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
    U1 = U + 1
    if mode == "permuted_enc":  # the (B, H, T) tensor's permuted view: rnnt_engine copies it into the workspace
        g["enc"] = g["enc"].permute(0, 2, 1).contiguous().permute(0, 2, 1)
        assert not g["enc"].is_contiguous()
    ins = (g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"])
    lens = (g["targets"], g["logit_lens"], g["target_lens"])
    L = engine.layout(B, T, U1, H, V, route)
    _poison(engine, dev, L.total + L.aux_bytes)
    outs = (_poisoned((B,), dev), _poisoned((B, T, H), dev), _poisoned((B, U1, H), dev), _poisoned((V, H), dev), _poisoned((V,), dev))
    scale = 1.0 / B
    r = None
    if mode in ("fused", "permuted_enc", "blank0"):
        engine.joint_loss_fwd_bwd(*ins, blank, scale, outs=outs, dtype=route, variant=variant)
    elif mode == "stage_by_stage":
        for stage in range(8):
            engine.joint_loss_fwd_bwd(*ins, blank, scale, outs=outs, stage=stage, dtype=route)
    elif mode == "reg":
        engine.joint_loss_fwd_bwd_reg(*ins, blank, scale, FASTEMIT, DELAY, outs=outs, dtype=route)
    elif mode == "fwd_only":
        r = dict(costs=engine.joint_loss_fwd(*ins, blank, dtype=route))
    elif mode == "align":
        scores, frames = engine.joint_align(*ins, blank, dtype=route)
        r = dict(scores=scores, frames=frames)
    else:  # the standalone entries, on seeded dense tensors
        rng = np.random.default_rng(B + T + U + H + V)
        dense = torch.from_numpy(rng.standard_normal((B, T, U1, V)).astype(np.float32)).to(dev)
        if mode == "standalone_joint_fwd":
            r = dict(logits=engine.joint_fwd(g["enc"], g["pred"], g["W"], g["bias"]))
        elif mode == "standalone_joint_bwd":
            r = dict(zip(GRADS, engine.joint_bwd(g["enc"], g["pred"], g["W"], dense)))
        elif mode == "standalone_loss_clamp":
            costs, grad = engine.loss_fwd_bwd(dense, *lens, blank, clamp=CLAMP)
            r = dict(costs=costs, grad_logits=grad)
        else:
            scores, frames = engine.align(dense, *lens, blank)
            r = dict(scores=scores, frames=frames)
    if r is None:
        r = dict(zip(("costs",) + GRADS, outs))
    torch.cuda.synchronize()
    out = {}
    for k, t in r.items():
        a = t.cpu().numpy()
        out[k] = a.view(np.uint32) if a.dtype == np.float32 else a
    return out


def recorded(result):
    """What the fixture keeps of a run: RAW outputs as they are, a SHA-256 of every other."""
    return {k: (a if k in RAW else np.array(sha256_of_arrays(a))) for k, a in result.items()}


def check_against_oracle(name, result):
    """A case of the plain loss against oracle_fused, at the bar of the route's parity test (bf16: the bar against the UNROUNDED
    oracle).  Regularised, alignment and standalone cases have no counterpart in oracle_fused."""
    route, _, _, mode, _ = CASES[name]
    if mode not in ("fused", "permuted_enc", "blank0", "stage_by_stage", "fwd_only"):
        return False
    d, blank = case_inputs(name)
    ref = oracle_fused(d, blank=blank)
    lt, gt = (BF16_LOSS_RTOL_EXACT, BF16_GRAD_RTOL_EXACT) if route == "bf16" else (LOSS_RTOL, GRAD_RTOL)
    assert_close_loss(name + " costs", result["costs"].view(np.float32), ref["costs"], rtol=lt)
    for k in GRADS:
        if k in result:
            assert_close_grad(name + " " + k, result[k].view(np.float32), ref[k], rtol=gt)
    return True


def main():
    import rnnt_amd
    e = rnnt_amd.engine
    e.lib()
    print("recording from %s" % e.LIB_PATH, flush=True)
    out = {}
    for name in CASES:
        res = run_case(e, name)
        checked = check_against_oracle(name, res)
        for k, a in recorded(res).items():
            out["%s/%s" % (name, k)] = a
        print("%-36s %s %s" % (name, "oracle ok" if checked else "         ", sorted(res)), flush=True)
    for stages, whole in WHOLE_CALL_OF.items():
        for k in ("costs",) + GRADS:
            assert np.array_equal(out["%s/%s" % (stages, k)], out["%s/%s" % (whole, k)]), (stages, k)
    np.savez_compressed(GOLDEN, **out)
    print("%d cases -> %s (%d bytes)" % (len(CASES), GOLDEN, os.path.getsize(GOLDEN)), flush=True)


if __name__ == "__main__":
    main()
