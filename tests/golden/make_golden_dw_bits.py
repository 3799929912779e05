"""Record what the dW GEMMs of the bf16 and bf16x3 routes (rnnt_amd/csrc/bf16.hip: k_dw_bf16; x3.hip: k_dw_x3) leave behind, for
tests/test_dw_bits_gpu.py: what these kernels share with the f16x2 dW kernels — tile decode, operand sources, the prologue DMA, fragment
addressing, the k-step pieces, the walk of the live-row table, the slab store (rnnt_amd/csrc/split_dw.hpp) — can be restated freely as
long as every case keeps every bit.  fused_routes.npz, split_planes.npz and dhidden_bits.npz hold these routes at no more than 126 cells:
one or two granules per split and never two live ranges in one split.  The cases here add what those leave out: splits that run two
ranges (touching, and with dead granules between them), walks longer than the ring, a lockstep that is on, empty shares, db from one,
two and three h blocks, half-empty v and h blocks.  (The f16x2 dW kernels have x2_dw.npz.)

Run once on a GPU with the library whose output is the reference (RNNT_ENGINE_LIB = the build of the commit BEFORE the change):
    python tests/golden/make_golden_dw_bits.py
writes tests/golden/dw_bits.npz.  Per case `<name>`:
  <name>/slab_w, /slab_b   SHA-256 of the split-K slabs (rnnt_engine_ws_layout: n_split * V * H and n_split * V floats) after the stages
                           up to and including dW (stage_mask = 127) over a workspace whose every word holds the quiet-NaN pattern of
                           make_golden_fused_routes.py: a split whose share is empty must still have written its zeros
  <name>/costs             raw, as uint32;  <name>/grad_enc, /grad_pred, /grad_W, /grad_bias   SHA-256, of the whole call
A case is written only if two runs give the same bytes and the whole call passes the route's parity bar against the fp64 oracle
(tests.helpers.oracle_fused; the bars of make_golden_fused_routes.py), so a broken build cannot be recorded.
This module is also the test's source of the cases, of the code that runs them and of the host-side arithmetic (k_dw_table, dw_splits)
the test checks the cases' claims with (the test loads it by path)."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.helpers import (BF16_GRAD_RTOL_EXACT, BF16_LOSS_RTOL_EXACT, GRAD_RTOL, LOSS_RTOL, assert_close_grad,  # noqa: E402
                           assert_close_loss, make_inputs, oracle_fused, sha256_of_arrays)

_spec = importlib.util.spec_from_file_location("make_golden_fused_routes", os.path.join(HERE, "make_golden_fused_routes.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

GOLDEN = os.path.join(HERE, "dw_bits.npz")
STAGES_TO_DW = 127  # engine.hip: ST_PROD | ST_FWD | ST_LATTICE | ST_COEF | ST_DH | ST_DH_RED | ST_DW
ROUTES = ("bf16", "bf16x3")
GRAN = 32  # cells per granule of the live-row table (k_dw_table as both routes call it): one ring stage on bf16, two k-steps on bf16x3
SLABS = ("slab_w", "slab_b")
# (B, T, U, H, V) -> logit_lens (None: make_inputs' ragged draw); U1 = U + 1; inputs: make_inputs(seed = sum of the shape, ragged)
SHAPES = {
    # one tile, 12 splits over 12 + 9 + 6 granules: split 5 runs two ranges that touch, split 9 two with three dead granules between
    # them, every other split one range of 2-3 granules; one h block (bf16x3: two db tiles per wave), half a v block
    (3, 4, 95, 128, 128): (4, 3, 2),
    # 2 x 2 tiles, 2 splits of 6 granules in one range: longer than either ring; bf16's lockstep is on; db from h blocks 0 and 1
    (1, 2, 191, 512, 512): (2,),
    # three h blocks (the last half empty, and without a share of db), two v blocks (the second half empty), 18 splits over at most
    # 4 granules: most shares are empty
    (2, 9, 6, 640, 384): None,
}
CASES = {"%s_%s" % (route, "x".join(map(str, s))): (route, s, sum(s)) for route in ROUTES for s in SHAPES}


def case_inputs(name):
    """The numpy inputs of a case."""
    _, s, seed = CASES[name]
    d = make_inputs(*s, seed=seed, ragged=True)
    if SHAPES[s] is not None:
        d["logit_lens"] = np.array(SHAPES[s], dtype=np.int32)
    return d


# ---- the host-side arithmetic of the walk, restated (joint_bwd.hip: k_dw_table; engine.hip: dw_splits; the kernels' share and walk)
def dw_table(logit_lens, T, U1, gran=GRAN):
    """k_dw_table -> (first granule of each utterance's live range, live granules before it, their total)."""
    first, before, prev_end, cum = [], [], 0, 0
    for b, lb in enumerate(logit_lens):
        c0 = b * T * U1
        s, e = c0 // gran, (c0 + min(max(int(lb), 0), T) * U1 + gran - 1) // gran
        s = max(s, prev_end)
        e = max(e, s)
        first.append(s)
        before.append(cum)
        cum += e - s
        prev_end = e
    return first, before, cum


def dw_blocks(H, V):
    return (V + 255) // 256, (H + 255) // 256  # v blocks, h blocks of the 256 x 256 workgroup tile


def dw_splits(B, T, H, V):
    n_vblk, n_hblk = dw_blocks(H, V)
    return min(max(256 // (n_vblk * n_hblk), 1), B * T)


def split_ranges(logit_lens, T, U1, n_split):
    """Per split: the live ranges its share [nlive s / n_split, nlive (s + 1) / n_split) is walked as, each (first granule, granules)."""
    first, before, nlive = dw_table(logit_lens, T, U1)
    B = len(first)
    out = []
    for s in range(n_split):
        g_lo, g_hi = nlive * s // n_split, nlive * (s + 1) // n_split
        runs, ub = [], 0
        while ub + 1 < B and before[ub + 1] <= g_lo:
            ub += 1
        gq = g_lo
        while gq < g_hi:
            cum1 = before[ub + 1] if ub + 1 < B else nlive
            ge = min(cum1, g_hi)
            if ge > gq:
                runs.append((first[ub] + (gq - before[ub]), ge - gq))
                gq = ge
            ub += 1
        out.append(runs)
    return out


def _device_inputs(name):
    d = case_inputs(name)
    V = CASES[name][1][4]
    g = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    return d, (g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"], V - 1, 1.0 / CASES[name][1][0])


def run_case(engine, name):
    """One run of a case over a poisoned workspace: the stages up to dW, then the whole call -> {key: array}."""
    route, (B, T, U, H, V), _ = CASES[name]
    _, ins = _device_inputs(name)
    dev = ins[0].device
    U1 = U + 1
    L = engine.layout(B, T, U1, H, V, route)
    assert L.n_split == dw_splits(B, T, H, V), (name, L.n_split)
    R._poison(engine, dev, L.total + L.aux_bytes)
    engine.joint_loss_fwd_bwd(*ins, dtype=route, stage_mask=STAGES_TO_DW)
    torch.cuda.synchronize()
    ws = engine.workspace(dev, L.total)
    reg = {"slab_w": (L.slab_w, L.n_split * V * H * 4), "slab_b": (L.slab_b, L.n_split * V * 4)}
    out = {k: np.array(sha256_of_arrays(ws[reg[k][0]:reg[k][0] + reg[k][1]].cpu().numpy())) for k in SLABS}
    R._poison(engine, dev, L.total + L.aux_bytes)
    outs = (R._poisoned((B,), dev), R._poisoned((B, T, H), dev), R._poisoned((B, U1, H), dev), R._poisoned((V, H), dev), R._poisoned((V,), dev))
    engine.joint_loss_fwd_bwd(*ins, outs=outs, dtype=route)
    torch.cuda.synchronize()
    out["costs"] = outs[0].cpu().numpy().view(np.uint32)
    for k, t in zip(R.GRADS, outs[1:]):
        out[k] = np.array(sha256_of_arrays(t.cpu().numpy().view(np.uint32)))
    return out


def check_against_oracle(engine, name):
    """The whole call of a case against oracle_fused at the route's parity bar (bf16: the bar against the unrounded oracle)."""
    route, (B, T, U, H, V), _ = CASES[name]
    d, ins = _device_inputs(name)
    outs = engine.joint_loss_fwd_bwd(*ins, dtype=route)
    torch.cuda.synchronize()
    ref = oracle_fused(d, blank=V - 1)
    lt, gt = (BF16_LOSS_RTOL_EXACT, BF16_GRAD_RTOL_EXACT) if route == "bf16" else (LOSS_RTOL, GRAD_RTOL)
    assert_close_loss(name + " costs", outs[0].cpu().numpy(), ref["costs"], rtol=lt)
    for k, t in zip(R.GRADS, outs[1:]):
        assert_close_grad(name + " " + k, t.cpu().numpy(), ref[k], rtol=gt)


def keys(name):
    return SLABS + ("costs",) + R.GRADS


def main():
    import rnnt_amd
    e = rnnt_amd.engine
    e.lib()
    print("recording from %s" % e.LIB_PATH, flush=True)
    out = {}
    for name in CASES:
        check_against_oracle(e, name)
        first, second = run_case(e, name), run_case(e, name)
        assert sorted(first) == sorted(second) == sorted(keys(name)), (name, sorted(first))
        assert all(np.array_equal(first[k], second[k]) for k in first), (name, first, second)
        for k, a in first.items():
            out["%s/%s" % (name, k)] = a
        route, (B, T, U, H, V), _ = CASES[name]
        print("%-28s oracle ok, two runs equal; walks %s" % (name, split_ranges(case_inputs(name)["logit_lens"], T, U + 1, dw_splits(B, T, H, V))),
              flush=True)
    np.savez_compressed(GOLDEN, **out)
    print("%d cases -> %s (%d bytes)" % (len(CASES), GOLDEN, os.path.getsize(GOLDEN)), flush=True)


if __name__ == "__main__":
    main()
