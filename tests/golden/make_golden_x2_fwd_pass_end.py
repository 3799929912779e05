"""Record what the f16x2 joint forward (k_joint_fwd_x2, all three forms) leaves behind at its pass end, for
tests/test_x2_fwd_pass_end_gpu.py: the logits and the per-cell log-softmax statistics must keep every bit when the pass end
is rescheduled.

Run once on a GPU with the library whose output is the reference (the commit BEFORE a change to the pass end):
    python tests/golden/make_golden_x2_fwd_pass_end.py
writes tests/golden/x2_fwd_pass_end.npz.  Per joint case `<name>`:
  <name>/denom_s, /lpb_s, /lpe_s   the whole skewed region of the workspace as uint32 (entry (b, t, u) at
                                   (b D + t + u) U1 + u); the regions are filled with PATTERN before the call, so the
                                   entries the kernel does not write keep it
  <name>/logits_sha256             SHA-256 of the logits region's first B T U1 rows (also pre-filled: dead tiles keep PATTERN)
per Linear case `<name>`: <name>/y, the output as uint32.
  worst_err, worst_err_linear      the recorded library's own largest distance from a float64 evaluation (independent_error /
                                   linear_error below): the test's bar is 4x these, and only guards against a recording from a
                                   broken build
This module is also the test's source of the cases and of the code that runs them (the test loads it by path).
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.helpers import make_inputs, relabel_blank  # noqa: E402

GOLDEN = os.path.join(HERE, "x2_fwd_pass_end.npz")
PATTERN = 0x7FC0BEEF  # a quiet NaN no kernel produces
X2 = "f16x2"
REGIONS = ("denom_s", "lpb_s", "lpe_s")

# name -> (shape (B, T, U, H, V), ragged, blank or None for V - 1, exact form)
JOINT_CASES = {
    "v128": ((2, 9, 7, 128, 128), True, None, False),    # one pass, half 0: single-group epilogue, half 1: none; 144 cells = 2 tiles, the last partial
    "v256": ((2, 9, 7, 128, 256), True, None, False),
    "v384": ((2, 9, 7, 128, 384), True, None, False),
    "v512": ((2, 9, 7, 128, 512), True, None, False),
    "v640": ((2, 9, 7, 128, 640), True, None, False),    # second pass partial
    "v1536": ((2, 9, 7, 128, 1536), True, None, False),  # three passes: the running update more than once
    "cfg2_hv": ((2, 40, 33, 512, 1024), True, None, False),
    "tiles282": ((3, 150, 79, 128, 640), False, None, False),  # 36 000 cells = 282 tiles > 256 CUs: a workgroup's second tile
    "v640_blank0": ((2, 9, 7, 128, 640), True, 0, False),
    "v640_blank300": ((2, 9, 7, 128, 640), True, 300, False),
    "v384_exact": ((2, 9, 7, 128, 384), True, None, True),  # two enc entries at +-50: the exact form (MODE 0) runs
}
LINEAR_CASES = {"lin_n128": (130, 128, 128), "lin_n384": (130, 128, 384), "lin_n640": (130, 128, 640)}


def joint_inputs(name):
    (B, T, U, H, V), ragged, blank, exact = JOINT_CASES[name]
    d = make_inputs(B, T, U, H, V, seed=B + T + U + H + V, ragged=ragged)
    if blank is None:
        blank = V - 1
    else:
        d, _ = relabel_blank(d, blank)
    if exact:
        d["enc"][0, 0, 0] = 50.0
        d["enc"][1, 1, 3] = -50.0
    return d, blank


def run_joint(engine, d, blank):
    """Producers + forward on the f16x2 route over pre-filled regions.  Returns (regions: name -> uint32 array, logits: fp32 [cells, V])."""
    B, T, H = d["enc"].shape
    U1, V = d["pred"].shape[1], d["W"].shape[0]
    dev = torch.device("cuda:0")
    g = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
    L = engine.layout(B, T, U1, H, V, X2)
    ws = engine.workspace(dev, engine.workspace_bytes(B, T, U1, H, V, X2))
    skew, cells = B * L.D * U1, B * T * U1

    def view(off, n):
        return ws[off:off + 4 * n].view(torch.int32)

    for r in REGIONS:
        view(getattr(L, r), skew).fill_(PATTERN)
    view(L.logits, cells * V).fill_(PATTERN)
    engine.joint_loss_fwd_bwd(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"],
                              blank, 1.0 / B, dtype=X2, stage_mask=0b11)
    torch.cuda.synchronize()
    regions = {r: view(getattr(L, r), skew).cpu().numpy().view(np.uint32).copy() for r in REGIONS}
    logits = view(L.logits, cells * V).cpu().numpy().view(np.float32).reshape(cells, V).copy()
    return regions, logits


def logits_sha256(logits):
    return hashlib.sha256(np.ascontiguousarray(logits).view(np.uint8).tobytes()).hexdigest()


def independent_error(d, blank, regions, logits):
    """Largest |stored - float64 evaluation| over denom_s, lpb_s, lpe_s of the lattice's cells, from the STORED fp32 logits
    (so the GEMM's own error is not in it); asserts that every other entry of the regions still holds PATTERN and that
    lpe_s is 0 in the last label column."""
    B, T, _ = d["enc"].shape
    U1, V = d["pred"].shape[1], d["W"].shape[0]
    D = T + U1 - 1
    b, t, u = np.meshgrid(np.arange(B), np.arange(T), np.arange(U1), indexing="ij")
    ll, tl = d["logit_lens"].astype(np.int64)[b], d["target_lens"].astype(np.int64)[b]
    live = (t < ll) & (u <= tl)
    si = ((b * D + t + u) * U1 + u)[live]
    cell = ((b * T + t) * U1 + u)[live]
    lg = logits[cell].astype(np.float64)
    assert np.isfinite(lg).all(), "a live cell's logits row holds a non-finite entry"
    m = lg.max(axis=1)
    den = m + np.log(np.exp(lg - m[:, None]).sum(axis=1))
    den_s, lpb_s, lpe_s = (regions[r].view(np.float32) for r in REGIONS)
    err = max(np.abs(den_s[si] - den).max(), np.abs(lpb_s[si] - (lg[:, blank] - den)).max())
    emit = (u < tl)[live]
    if emit.any():
        tg = np.concatenate([d["targets"], np.zeros((B, 1), d["targets"].dtype)], axis=1) if d["targets"].shape[1] < U1 else d["targets"]
        y = tg[b, u][live][emit]
        err = max(err, np.abs(lpe_s[si][emit] - (lg[emit, y] - den[emit])).max())
    assert (regions["lpe_s"][si][~emit] == 0).all(), "lpe_s is not +0 in a row's last label column"
    rest = np.ones(B * D * U1, bool)
    rest[si] = False
    for r in REGIONS:
        assert (regions[r][rest] == PATTERN).all(), "%s written outside the lattice" % r
    return float(err)


def linear_inputs(name):
    M, K, N = LINEAR_CASES[name]
    rng = np.random.default_rng(M + K + N)
    k = 1.0 / np.sqrt(K)
    return dict(x=rng.standard_normal((M, K)).astype(np.float32), W=rng.uniform(-k, k, (N, K)).astype(np.float32),
                bias=rng.uniform(-k, k, (N,)).astype(np.float32))


def run_linear(engine, d):
    g = {k: torch.from_numpy(v).to("cuda:0") for k, v in d.items()}
    y = engine.linear_fwd(g["x"], g["W"], g["bias"], backend="x2")
    torch.cuda.synchronize()
    return y.cpu().numpy()


def linear_error(d, y):
    ref = d["x"].astype(np.float64) @ d["W"].astype(np.float64).T + d["bias"].astype(np.float64)
    return float(np.abs(y - ref).max())


def main():
    import rnnt_amd
    e = rnnt_amd.engine
    e.lib()
    out, worst, worst_lin = {}, 0.0, 0.0
    for name in JOINT_CASES:
        d, blank = joint_inputs(name)
        regions, logits = run_joint(e, d, blank)
        err = independent_error(d, blank, regions, logits)
        worst = max(worst, err)
        for r in REGIONS:
            out["%s/%s" % (name, r)] = regions[r]
        out["%s/logits_sha256" % name] = np.array(logits_sha256(logits))
        print("%-14s err %.3e  logits %s" % (name, err, logits_sha256(logits)[:16]), flush=True)
    for name in LINEAR_CASES:
        d = linear_inputs(name)
        y = run_linear(e, d)
        err = linear_error(d, y)
        worst_lin = max(worst_lin, err)
        out["%s/y" % name] = y.view(np.uint32)
        print("%-14s err %.3e" % (name, err), flush=True)
    out["worst_err"] = np.float64(worst)
    out["worst_err_linear"] = np.float64(worst_lin)
    np.savez_compressed(GOLDEN, **out)
    print("worst_err %.3e worst_err_linear %.3e -> %s (%d bytes)" % (worst, worst_lin, GOLDEN, os.path.getsize(GOLDEN)), flush=True)


if __name__ == "__main__":
    main()
