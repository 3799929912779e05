"""Record what the dHidden kernels of the two split routes (rnnt_amd/csrc/x3.hip: k_dhidden_x3<FIRST>; x2.hip: k_dhidden_x2<FIRST, PART>,
k_dhidden_x2r) leave behind, for tests/test_dhidden_bits_gpu.py: the parts of these kernels that are not their k-step schedule — the
producer set-up, G's production, the whole-line stores, the epilogue (rnnt_amd/csrc/split_dhidden.hpp) — can be restated freely as long
as every case keeps every bit.  tests/golden/split_planes.npz and fused_routes.npz hold H = 128, 384 and 640 at U + 1 = 7; the cases here
add what those leave out: a second u block, every kernel form, k_dhidden_x2r at hp = 2 and with two u blocks, dead tiles, a tile row
that ends inside the lengths and one past them (bf16x3's early zero-fill branch).

Run once on a GPU with the library whose output is the reference (RNNT_ENGINE_LIB = the build of the commit BEFORE the change):
    python tests/golden/make_golden_dhidden_bits.py
writes tests/golden/dhidden_bits.npz.  Per case `<name>`:
  <name>/logits_g[, /g_lo]   SHA-256 of the region after the stages up to and including dHidden (stage_mask = 31) over a workspace whose
                             every word holds the quiet-NaN pattern of make_golden_fused_routes.py (regions: make_golden_split_planes.py)
  <name>/costs               raw, as uint32;  <name>/grad_enc, /grad_pred, /grad_W, /grad_bias   SHA-256, of the whole call
A case is written only if two runs give the same bytes and the whole call passes the route's parity bar against the fp64 oracle
(tests.helpers.oracle_fused; the bars of tests/test_x3_gpu.py / test_x2_gpu.py), so a broken build cannot be recorded.
This module is also the test's source of the cases and of the code that runs them (the test loads it by path)."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.helpers import GRAD_RTOL, LOSS_RTOL, assert_close_grad, assert_close_loss, make_inputs, oracle_fused, sha256_of_arrays  # noqa: E402
from tests.x2_live_list_cases import TINY  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_golden_split_planes", os.path.join(HERE, "make_golden_split_planes.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)
R = S.R  # make_golden_fused_routes

GOLDEN = os.path.join(HERE, "dhidden_bits.npz")
G_REGIONS = {"bf16x3": ("logits_g", "g_lo"), "f16x2": ("logits_g",)}
# name -> (route, (B, T, U, H, V), seed); U1 = U + 1; inputs: make_inputs(seed, ragged=True); seed = sum of the shape but for TINY
_SHAPES = [("f16x2", (2, 9, 17, 768, 128)),    # <true, false> + <false, true> with two live column groups; U1 = 18: two u blocks, the second 2 of 16 wide
           ("f16x2", (2, 9, 17, 1152, 128)),   # <true, false>, <false, false>, k_dhidden_x2r at hp = 2
           ("f16x2", (2, 9, 17, 640, 128)),    # k_dhidden_x2r with two u blocks
           ("bf16x3", (2, 9, 17, 128, 128)),   # two u blocks
           ("bf16x3", (2, 9, 17, 1024, 128)),  # k_dhidden_x3<false> over a full 512-column pass
           ("bf16x3", (2, 17, 6, 640, 128))]   # three t tiles, the last with one row; a ragged length ends inside a tile and before the last: the early zero-fill branch
CASES = {"%s_%s" % (route, "x".join(map(str, s))): (route, s, sum(s)) for route, s in _SHAPES}
CASES["f16x2_tiny_dead_tiles"] = ("f16x2", TINY[:5], TINY[5])  # dead tiles: the live-tile list is shorter than the grid


def kernel_forms(route, H):
    """The dHidden kernel forms a call of this H launches, as launch_dhidden_x2 / launch_dhidden_x3 decide them."""
    if route == "bf16x3":
        return ["k_dhidden_x3<true>"] + ["k_dhidden_x3<false>" for hp in range(1, (H + 511) // 512)]
    forms = ["k_dhidden_x2<true, true>" if H < 512 else "k_dhidden_x2<true, false>"]
    for hp in range(1, (H + 511) // 512):
        rem = H - 512 * hp
        forms.append("k_dhidden_x2r@hp=%d" % hp if rem == 128 else "k_dhidden_x2<false, true>" if rem < 512 else "k_dhidden_x2<false, false>")
    return forms


def _inputs(name):
    route, (B, T, U, H, V), seed = CASES[name]
    d = make_inputs(B, T, U, H, V, seed=seed, ragged=True)
    g = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    return d, (g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"], V - 1, 1.0 / B)


def run_case(engine, name):
    """One run of a case over a poisoned workspace: the stages up to dHidden, then the whole call -> {key: array}."""
    route, (B, T, U, H, V), _ = CASES[name]
    _, ins = _inputs(name)
    dev = ins[0].device
    U1 = U + 1
    L, reg = S.regions(engine, route, B, T, U1, H, V)
    R._poison(engine, dev, L.total + L.aux_bytes)
    engine.joint_loss_fwd_bwd(*ins, dtype=route, stage_mask=S.STAGES_TO_DHIDDEN)
    torch.cuda.synchronize()
    ws = engine.workspace(dev, L.total)
    out = {k: np.array(sha256_of_arrays(ws[reg[k][0]:reg[k][0] + reg[k][1]].cpu().numpy())) for k in G_REGIONS[route]}
    R._poison(engine, dev, L.total + L.aux_bytes)
    outs = (R._poisoned((B,), dev), R._poisoned((B, T, H), dev), R._poisoned((B, U1, H), dev), R._poisoned((V, H), dev), R._poisoned((V,), dev))
    engine.joint_loss_fwd_bwd(*ins, outs=outs, dtype=route)
    torch.cuda.synchronize()
    out["costs"] = outs[0].cpu().numpy().view(np.uint32)
    for k, t in zip(R.GRADS, outs[1:]):
        out[k] = np.array(sha256_of_arrays(t.cpu().numpy().view(np.uint32)))
    return out


def check_against_oracle(engine, name):
    """The whole call of a case against oracle_fused at the route's parity bar."""
    route, (B, T, U, H, V), _ = CASES[name]
    d, ins = _inputs(name)
    outs = engine.joint_loss_fwd_bwd(*ins, dtype=route)
    torch.cuda.synchronize()
    ref = oracle_fused(d, blank=V - 1)
    assert_close_loss(name + " costs", outs[0].cpu().numpy(), ref["costs"], rtol=LOSS_RTOL)
    for k, t in zip(R.GRADS, outs[1:]):
        assert_close_grad(name + " " + k, t.cpu().numpy(), ref[k], rtol=GRAD_RTOL)


def keys(name):
    return G_REGIONS[CASES[name][0]] + ("costs",) + R.GRADS


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
        print("%-36s oracle ok, two runs equal %s" % (name, kernel_forms(CASES[name][0], CASES[name][1][3])), flush=True)
    np.savez_compressed(GOLDEN, **out)
    print("%d cases -> %s (%d bytes)" % (len(CASES), GOLDEN, os.path.getsize(GOLDEN)), flush=True)


if __name__ == "__main__":
    main()
