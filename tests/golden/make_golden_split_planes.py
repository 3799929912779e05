"""Record the operand planes and W packs the two split routes (rnnt_amd/csrc/x3.hip: bf16x3, x2.hip: f16x2) leave in the workspace,
for tests/test_split_planes_bits_gpu.py.  tests/golden/fused_routes.npz hashes a call's OUTPUTS; what the plain kernels of
rnnt_amd/csrc/split_common.hpp write — the hidden planes (k_split_make_hidden), G's planes (k_split_g), the two W packs
(k_split_pack_w_fwd / _dh) and the zeroed padding rows — and what the fused kernels write in their place is held here, byte for
byte, so the piece format and the pack layouts can be restated freely as long as every case keeps every bit.

Run once on a GPU with the library whose output is the reference (RNNT_ENGINE_LIB = the build of the commit BEFORE the change):
    python tests/golden/make_golden_split_planes.py
writes tests/golden/split_planes.npz.  Per case the stages up to and including dHidden run through rnnt_engine_run_stages over a
workspace whose every word holds the quiet-NaN pattern of make_golden_fused_routes.py; the fixture keeps the SHA-256 of the regions
REGIONS names, addressed through rnnt_engine_workspace_layout.  A case is written only if two runs give the same bytes and the whole
call's costs and gradients pass the route's parity bar against the fp64 oracle (tests.helpers.oracle_fused; the bars of
tests/test_x3_gpu.py / test_x2_gpu.py), so a broken build cannot be recorded.
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

_spec = importlib.util.spec_from_file_location("make_golden_fused_routes", os.path.join(HERE, "make_golden_fused_routes.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

GOLDEN = os.path.join(HERE, "split_planes.npz")
STAGES_TO_DHIDDEN = 31  # engine.hip: ST_PROD | ST_FWD | ST_LATTICE | ST_COEF | ST_DH
PLANES = {"bf16x3": 3, "f16x2": 2}
# (B, T, U, H, V), U1 = U + 1; inputs: make_inputs(seed = sum of the shape, ragged)
SHAPES = [(2, 9, 6, 128, 128),   # the smallest the routes take; V < 512 and H < 512: both packs zero-fill the tiles past V and past H
          (2, 9, 6, 640, 256)]   # a second 512-column dHidden pass partly past H, 40 k-steps, half a forward pass past V
# form -> variant: the fused kernels write the planes and the plain kernels the packs | k_split_make_hidden and k_split_g write the
# planes behind the fp32 route's forward and dHidden (a workspace of total + aux_bytes)
FORMS = {"default": 0, "fp32_fwd_dh": R.X3_FP32_FWD | R.X3_FP32_DH}
CASES = {"%s_%s_%s" % (route, "x".join(map(str, s)), form): (route, s, variant)
         for route in PLANES for s in SHAPES for form, variant in FORMS.items()}
REGIONS = {"bf16x3": ("hidden", "wpack_fwd", "wpack_dh", "logits_g", "g_lo"),
           "f16x2": ("hidden", "wpack_fwd", "wpack_dh", "logits_g", "w_scales")}
X2_SCALES_AT = 640  # engine.hip ControlBlock::x2_scales, from rnnt_engine_ws_layout.counters


def _align_up(x):
    return (x + 255) & ~255


def regions(engine, route, B, T, U1, H, V):
    """name -> (byte offset, bytes) in the workspace (engine.hip layout(); the pack sizes are split_common.hpp's)."""
    L = engine.layout(B, T, U1, H, V, route)
    n_planes = PLANES[route]
    ra = (L.rows_pad + 96 + 127) // 128 * 128  # engine.hip bf16_rows_alloc
    fwd = ((V + 511) // 512) * (H // 16) * n_planes * 16 * 64 * 16
    dh = ((H + 511) // 512) * (V // 16) * n_planes * 16 * 64 * 16
    r = dict(hidden=(L.hidden, n_planes * ra * H * 2), wpack_fwd=(L.wpack, fwd), wpack_dh=(L.wpack + _align_up(fwd), dh),
             logits_g=(L.logits, ra * V * 4))
    if route == "bf16x3":
        r["g_lo"] = (L.g_lo, ra * V * 2)
    else:
        r["w_scales"] = (L.counters + X2_SCALES_AT, 8)
    assert sorted(r) == sorted(REGIONS[route])
    return L, r


def _args(name):
    route, (B, T, U, H, V), variant = CASES[name]
    d = make_inputs(B, T, U, H, V, seed=B + T + U + H + V, ragged=True)
    g = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    ins = (g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"], V - 1, 1.0 / B)
    return d, ins


def run_case(engine, name):
    """One run of a case's stages up to dHidden over a poisoned workspace -> {region: SHA-256}."""
    route, (B, T, U, H, V), variant = CASES[name]
    _, ins = _args(name)
    dev = ins[0].device
    L, reg = regions(engine, route, B, T, U + 1, H, V)
    R._poison(engine, dev, L.total + L.aux_bytes)
    engine.joint_loss_fwd_bwd(*ins, dtype=route, stage_mask=STAGES_TO_DHIDDEN, variant=variant)
    torch.cuda.synchronize()
    ws = engine.workspace(dev, L.total)
    return {k: np.array(sha256_of_arrays(ws[off:off + n].cpu().numpy())) for k, (off, n) in reg.items()}


def check_against_oracle(engine, name):
    """The whole call of a case against oracle_fused at the route's parity bar."""
    route, (B, T, U, H, V), variant = CASES[name]
    d, ins = _args(name)
    outs = engine.joint_loss_fwd_bwd(*ins, dtype=route, variant=variant)
    torch.cuda.synchronize()
    ref = oracle_fused(d, blank=V - 1)
    assert_close_loss(name + " costs", outs[0].cpu().numpy(), ref["costs"], rtol=LOSS_RTOL)
    for k, t in zip(R.GRADS, outs[1:]):
        assert_close_grad(name + " " + k, t.cpu().numpy(), ref[k], rtol=GRAD_RTOL)


def main():
    import rnnt_amd
    e = rnnt_amd.engine
    e.lib()
    print("recording from %s" % e.LIB_PATH, flush=True)
    out = {}
    for name in CASES:
        check_against_oracle(e, name)
        first, second = run_case(e, name), run_case(e, name)
        assert sorted(first) == sorted(second) and all(np.array_equal(first[k], second[k]) for k in first), (name, first, second)
        for k, a in first.items():
            out["%s/%s" % (name, k)] = a
        print("%-40s oracle ok, two runs equal %s" % (name, sorted(first)), flush=True)
    np.savez_compressed(GOLDEN, **out)
    print("%d cases -> %s (%d bytes)" % (len(CASES), GOLDEN, os.path.getsize(GOLDEN)), flush=True)


if __name__ == "__main__":
    main()
