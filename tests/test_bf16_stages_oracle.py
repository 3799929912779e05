"""CPU: the comparators of tests/bf16_stage_cases.py are neither too tight nor too loose, before any GPU time is spent.
  * not too tight: an fp32 numpy emulation of each stage (bf16 operands, float32 products and sums, round-to-nearest-even stores to
    fp16 and bf16, the kernels' fp32 formulas for tanh and G) passes its own comparator on every case.  This is the condition the
    cases are chosen under: a case that fails it is changed here, not on the GPU;
  * not too loose: each seeded fault (a dropped k chunk, rotated rows, a wrong W group, a wrong pred row, a neighbour's denominator,
    a u block or an H pass lost, a cell dropped from or a stale row added to dW, a split lost from db) applied to that emulation is
    rejected by its comparator on every case that has the geometry for it;
  * the twin's final gradients are oracle_fused_bf16's."""
import functools

import numpy as np
import pytest

from tests.bf16_stage_cases import (CASES, LOG2E, YARD, check_dhidden, check_dw, check_g, check_hidden, check_logits, coef64, dims, fast_tanh_f32,
                                    g_from_coef, inside, loss64, make_case, probe_cell, twin, ulp_bf16)
from tests.helpers import assert_close_grad, assert_close_loss, bf16_round, oracle_fused_bf16

F32 = np.float32


def _acc32(hidden, Wb):
    return hidden.astype(F32) @ Wb.astype(F32).T


def _store_f16(acc, bias):
    return (acc + bias.astype(F32)).astype(np.float16).astype(np.float64)


def _coef32(logits, d, gs):
    """The coefficients as the device forms them: fp64 alpha / beta (the oracle's), an fp32 log-softmax denominator, fp32 c1 / sb / se."""
    B, T, U1, _, V = dims(d)
    costs, _, work = loss64(logits, d)
    work["logits"] = np.where(inside(d)[..., None], logits.reshape(B, T, U1, V), 0.0)
    lg = work["logits"].astype(F32)
    m = lg.max(-1)
    denom = m + np.log(np.exp(lg - m[..., None]).sum(-1, dtype=F32))
    work["denom"] = denom.astype(np.float64)
    c = coef64(d, work, costs, gs)
    return {k: (v if k == "y" else v.astype(F32)) for k, v in c.items()}, work["denom"].reshape(-1)


def _g32(logits, coef, V):
    return g_from_coef(logits, coef, V, real=F32)


def _dpre32(G, hidden, Wb, d):
    B, T, U1, H, _ = dims(d)
    h = hidden.astype(F32)
    return ((G.astype(F32) @ Wb.astype(F32)) * (F32(1) - h * h)).reshape(B, T, U1, H)


@functools.lru_cache(maxsize=None)
def _emulate(name):
    """The faithful fp32 emulation of one case, each stage fed by the emulated stage before it (as on the device)."""
    d, gs = make_case(name)
    _, _, _, H, V = dims(d)
    Wb = bf16_round(d["W"]).astype(np.float64)
    hidden = bf16_round(fast_tanh_f32(d)).astype(np.float64).reshape(-1, H)
    acc = _acc32(hidden, Wb)
    logits = _store_f16(acc, d["bias"])
    coef, denom = _coef32(logits, d, gs)
    g_yard = _g32(logits, coef, V)  # the fp32 route's gradient on these logits: the same formula, no bf16 store
    G = bf16_round(g_yard).astype(np.float64)
    dpre = _dpre32(G, hidden, Wb, d)
    return dict(name=name, d=d, gs=gs, Wb=Wb, hidden=hidden, acc=acc, logits=logits, coef=coef, denom=denom,
                g_yard=g_yard.astype(np.float64), G=G, dpre=dpre, grad_enc=dpre.sum(2, dtype=F32).astype(np.float64),
                grad_pred=dpre.sum(1, dtype=F32).astype(np.float64),
                grad_W=(G.astype(F32).T @ hidden.astype(F32)).astype(np.float64), grad_bias=G.astype(F32).sum(0, dtype=F32).astype(np.float64))


@pytest.fixture(params=sorted(CASES))
def emu(request):
    return _emulate(request.param)


def _yard_dw(e):
    return e["grad_W"], e["grad_bias"]  # (the emulation IS a plain fp32 product: the yardstick of the CPU file)


def test_faithful_emulation_passes_every_comparator(emu):
    e, d = emu, emu["d"]
    r = dict(hidden=check_hidden(e["hidden"], d), logits=check_logits(e["logits"], e["hidden"], d),
             G=check_g(e["G"], e["logits"], d, e["gs"], e["g_yard"])[0])
    r["grad_enc"], r["grad_pred"] = check_dhidden(e["grad_enc"], e["grad_pred"], e["G"], e["hidden"], d)
    r.update(check_dw(e["grad_W"], e["grad_bias"], e["G"], e["hidden"], *_yard_dw(e)))
    print(e["name"], {k: "%.3f" % v for k, v in r.items()})


def test_twin_is_the_rounding_point_oracle(emu):
    """Same rounding points, same fp64 arithmetic; the twin scales G by the fp32 1/B the engine is called with, the oracle divides by B."""
    d = emu["d"]
    tw, ref = twin(d, emu["gs"]), oracle_fused_bf16(d)
    assert_close_loss("costs", tw["costs"], ref["costs"])
    for k in ("grad_enc", "grad_pred", "grad_W", "grad_bias"):
        assert_close_grad(k, tw[k], ref[k])
    # and its coefficients reproduce its G: per entry within an fp32 rounding of the terms (both sides are fp64)
    V = d["W"].shape[0]
    G2 = g_from_coef(tw["logits"], tw["coef"], V)
    assert (np.abs(G2 - tw["G64"]) <= 2.0 ** -24 * (np.abs(tw["G64"]) + tw["coef"]["sb"][:, None] + tw["coef"]["se"][:, None])).all()


def test_half_an_ulp_is_not_2_pow_minus_9_relative():
    """Why G's bar is ulp_bf16(G64) / 2 and not 2^-9 |G64|: the correctly rounded store of a value just above a power of two is off by
    nearly 2^-8 of it.  On config3_hv the faithful emulation exceeds 2^-9 |G64| + E (at a label entry of -0.0656675, stored as -0.0654297:
    2.378e-4 off, half an ulp is 2.441e-4, 2^-9 |G64| is 1.283e-4)."""
    x = 1.0 + 2.0 ** -8 - 2.0 ** -12
    off = abs(float(bf16_round(np.float32(x)).reshape(-1)[0]) - x)
    assert 2.0 ** -9 * x < off <= 0.5 * float(ulp_bf16(x))
    e = _emulate("config3_hv")
    ins = inside(e["d"]).reshape(-1)
    G64 = loss64(e["logits"], e["d"])[1] * e["gs"]
    E = YARD * np.abs(e["g_yard"] - G64)[ins].max()
    assert (np.abs(e["G"] - G64)[ins] > 2.0 ** -9 * np.abs(G64[ins]) + E).any()


# ---- seeded faults: each returns None where the case lacks the geometry
def _tile_rows(e):
    cells = e["hidden"].shape[0]
    c = probe_cell(e["d"])[3]
    return np.arange(128 * (c // 128), min(128 * (c // 128) + 128, cells))


def fault_logits_k_chunk(e):
    """One 32-wide k chunk left out of one 128-cell tile."""
    H = e["hidden"].shape[1]
    rows, k0 = _tile_rows(e), 32 * (H // 64)
    acc = e["acc"].copy()
    acc[rows] -= _acc32(e["hidden"][rows, k0:k0 + 32], e["Wb"][:, k0:k0 + 32])
    return _store_f16(acc, e["d"]["bias"])


def fault_logits_rows_rotated(e):
    rows = _tile_rows(e)
    if len(rows) < 2:
        return None
    lg = e["logits"].copy()
    lg[rows] = np.roll(lg[rows], 1, axis=0)
    return lg


def fault_logits_last_group_from_previous_w(e):
    V = e["Wb"].shape[0]
    if V < 256:
        return None
    acc = e["acc"].copy()
    acc[:, V - 128:] = acc[:, V - 256:V - 128]
    return _store_f16(acc, e["d"]["bias"])


def fault_hidden_pred_from_u_minus_1(e):
    d = e["d"]
    _, T, U1, _, _ = dims(d)
    b, t, u, _ = probe_cell(d)
    u = max(u, 1)
    if u > int(d["target_lens"][b]):
        return None
    d2 = dict(d, pred=d["pred"].copy())
    d2["pred"][b, u] = d["pred"][b, u - 1]
    hid = e["hidden"].copy()
    hid[(b * T + t) * U1 + u] = bf16_round(fast_tanh_f32(d2)[b, t, u]).astype(np.float64)
    return hid


def fault_g_neighbours_denom(e):
    """One wave's 32 cells take the log-softmax denominator of the next cell."""
    ins = inside(e["d"]).reshape(-1)
    c0 = 32 * (probe_cell(e["d"])[3] // 32)
    cs = np.array([c for c in range(c0, min(c0 + 32, len(ins) - 1)) if ins[c] and ins[c + 1]], dtype=np.int64)
    if len(cs) == 0:
        return None
    coef = dict(e["coef"], c1=e["coef"]["c1"].copy())
    coef["c1"][cs] = (coef["c1"][cs].astype(np.float64) + (e["denom"][cs] - e["denom"][cs + 1]) * LOG2E).astype(F32)
    return bf16_round(_g32(e["logits"], coef, e["Wb"].shape[0])).astype(np.float64)


def fault_grad_enc_u_block_lost(e):
    """One 16-wide u block left out of one time step's sum."""
    b, t, u, _ = probe_cell(e["d"])
    dp = e["dpre"].copy()
    dp[b, t, 16 * (u // 16):16 * (u // 16) + 16] = 0
    return dp.sum(2, dtype=F32).astype(np.float64)


def fault_grad_enc_rest_from_pass_0(e):
    H = e["hidden"].shape[1]
    if H <= 512:
        return None
    ge = e["grad_enc"].copy()
    n = H - 512 if H % 512 else 512
    ge[..., H - n:] = ge[..., :n]
    return ge


def _heaviest_cell(e):
    """The cell that carries the most gradient (on a peaked softmax the cells off the likely alignments carry next to none:
    dropping one of those is no fault)."""
    return int(np.abs(e["G"]).sum(1).argmax())


def fault_grad_w_live_cell_dropped(e):
    G = e["G"].copy()
    G[_heaviest_cell(e)] = 0
    return (G.astype(F32).T @ e["hidden"].astype(F32)).astype(np.float64)


def fault_grad_w_stale_row_added(e):
    """A dead cell's G row as a stale buffer might leave it: N(0, 1) instead of zeros."""
    dead = np.flatnonzero(~inside(e["d"]).reshape(-1))
    if len(dead) == 0:
        return None
    G = e["G"].copy()
    G[dead[len(dead) // 2]] = bf16_round(np.random.default_rng(1).standard_normal(G.shape[1]).astype(F32))
    return (G.astype(F32).T @ e["hidden"].astype(F32)).astype(np.float64)


def fault_grad_bias_split_lost(e):
    """One split's cells (a 32-cell stage of the dW ring, around the heaviest cell) left out of the column sum."""
    c0 = 32 * (_heaviest_cell(e) // 32)
    G = e["G"].copy()
    G[c0:c0 + 32] = 0
    return G.astype(F32).sum(0, dtype=F32).astype(np.float64)


FAULTS = {
    "logits_k_chunk": (fault_logits_k_chunk, lambda e, x: check_logits(x, e["hidden"], e["d"])),
    "logits_rows_rotated": (fault_logits_rows_rotated, lambda e, x: check_logits(x, e["hidden"], e["d"])),
    "logits_last_group_from_previous_w": (fault_logits_last_group_from_previous_w, lambda e, x: check_logits(x, e["hidden"], e["d"])),
    "hidden_pred_from_u_minus_1": (fault_hidden_pred_from_u_minus_1, lambda e, x: check_hidden(x, e["d"])),
    "g_neighbours_denom": (fault_g_neighbours_denom, lambda e, x: check_g(x, e["logits"], e["d"], e["gs"], e["g_yard"])),
    "grad_enc_u_block_lost": (fault_grad_enc_u_block_lost, lambda e, x: check_dhidden(x, e["grad_pred"], e["G"], e["hidden"], e["d"])),
    "grad_enc_rest_from_pass_0": (fault_grad_enc_rest_from_pass_0, lambda e, x: check_dhidden(x, e["grad_pred"], e["G"], e["hidden"], e["d"])),
    "grad_w_live_cell_dropped": (fault_grad_w_live_cell_dropped, lambda e, x: check_dw(x, e["grad_bias"], e["G"], e["hidden"], *_yard_dw(e))),
    "grad_w_stale_row_added": (fault_grad_w_stale_row_added, lambda e, x: check_dw(x, e["grad_bias"], e["G"], e["hidden"], *_yard_dw(e))),
    "grad_bias_split_lost": (fault_grad_bias_split_lost, lambda e, x: check_dw(e["grad_W"], x, e["G"], e["hidden"], *_yard_dw(e))),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_seeded_fault_is_rejected(emu, fault):
    make, check = FAULTS[fault]
    x = make(emu)
    if x is None:
        return  # the case lacks the geometry (one cell, H <= 512, V = 128, no dead cell)
    with pytest.raises(AssertionError):
        check(emu, x)


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_fault_applies_to_several_cases(fault):
    """A fault that never applied would prove nothing."""
    assert sum(FAULTS[fault][0](_emulate(name)) is not None for name in CASES) >= 2
