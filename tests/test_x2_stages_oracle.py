"""CPU: the comparators of tests/x2_stage_cases.py are neither too tight nor too loose, before any GPU time is spent.
  * not too tight: a numpy emulation of the f16x2 route (exact fp16 splits, the three products accumulated in fp32, the forward's fp32
    statistics in 512-column passes carried as (max, sum exp), G from the coefficients in fp32 and then split, fp32 sums) passes every
    comparator on every case; the two large cases run hidden, logits and statistics only;
  * not too loose: each of fourteen seeded faults, applied to that emulation at probe_cell (faults 8, 10 and 14 at the cell that
    carries the most gradient: on a peaked softmax the probe cell may carry none), is rejected on every case that has the
    geometry for it — and four of them (a second-order product or a mid plane lost) pass the suite's 1e-4 bar on the final gradients;
  * the three products drop no more than x2.hip's header claims; the twin's final gradients are oracle_fused's."""
import functools

import numpy as np
import pytest

from tests.helpers import assert_close_grad, assert_close_loss, oracle_fused
from tests.x2_stage_cases import (CASES, F32, LARGE, LOG2E_F32, SH, check_dhidden, check_dw, check_ep, check_g, check_hidden, check_logits,
                                  check_scales, check_stats, coef64, dfac_f32, dims, dropped_terms, ep_tables, g_from_coef, g_scale_of,
                                  hidden_scaled_f32, inside, kstep_major, loss64, make_case, probe_cell, read_rows, rows_alloc, seen, split16,
                                  t_for_cus, twin, ulp_fp32, w_pieces, w_scale)

SMALL = [n for n in CASES if n not in LARGE]
L64 = float(LOG2E_F32)


def _mm3(ah, am, bh, bm, drop=None):
    """The three products accumulated in fp32 (every fp16 x fp16 product is exact in fp32); `drop`: one of 'ah.bm', 'am.bh' left out."""
    a_h, a_m, b_h, b_m = (x.astype(F32) for x in (ah, am, bh, bm))
    acc = a_h @ b_h
    if drop != "ah.bm":
        acc = acc + a_h @ b_m
    if drop != "am.bh":
        acc = acc + a_m @ b_h
    return acc


def _store_logits(acc, d, sW):
    """fma(acc, 2^-14 / s_W, bias): exact in fp64, rounded once."""
    return (acc.astype(np.float64) / (SH * sW) + d["bias"].astype(np.float64)).astype(F32)


def _pass_stats(x):
    """(max, sum exp2((x - max) log2e)) of one pass's columns as the pass end forms them: nm2 = -(max log2e) rounded, one fma per entry."""
    M = x.max(1)
    nm2 = -(M * LOG2E_F32)
    arg = (x.astype(np.float64) * L64 + nm2.astype(np.float64)[:, None]).astype(F32)
    return M, np.exp2(arg).sum(1, dtype=F32)


def _denom32(lg, passes=None):
    """k_joint_fwd_x2's log-softmax denominator of each row of fp32 logits [N, V]: per column half (wn) a running (max, sum) over the
    512-column passes, the two halves merged, max + log(sum).  `passes`: only the first so many (a seeded fault)."""
    N, V = lg.shape
    m_run = np.full((2, N), -np.inf, dtype=F32)
    s_run = np.zeros((2, N), dtype=F32)
    npass = (V + 511) // 512 if passes is None else passes
    with np.errstate(invalid="ignore"):
        for p in range(npass):
            for wn in range(2):
                c0 = 512 * p + 256 * wn
                if c0 >= V:
                    continue
                M, S = _pass_stats(lg[:, c0:min(c0 + 256, V)])
                mo, so = m_run[wn], s_run[wn]
                mn = np.maximum(mo, M)
                a, b = np.exp2((mo - mn) * LOG2E_F32), np.exp2((M - mn) * LOG2E_F32)
                s_run[wn] = (so.astype(np.float64) * a.astype(np.float64) + (S * b).astype(np.float64)).astype(F32)
                m_run[wn] = mn
        M = np.maximum(m_run[0], m_run[1])
        S = s_run[0] * np.exp2((m_run[0] - M) * LOG2E_F32) + s_run[1] * np.exp2((m_run[1] - M) * LOG2E_F32)
    return M + np.log(S)


def _skew(x):
    B, T, U1 = x.shape
    out = np.zeros((B, T + U1 - 1, U1), dtype=x.dtype)
    t, u = np.arange(T)[:, None], np.arange(U1)[None, :]
    out[:, t + u, u] = x
    return out


def _stats(logits, denom, d):
    """(denom_s, lpb_s, lpe_s) skewed, as the forward's last phase writes them from the logits and the row denominators."""
    B, T, U1, _, V = dims(d)
    lg, den = logits.reshape(B, T, U1, V), denom.reshape(B, T, U1)
    y = np.zeros((B, U1), dtype=np.int64)
    y[:, :U1 - 1] = d["targets"]
    lpe = np.take_along_axis(lg, np.broadcast_to(y[:, None, :, None], (B, T, U1, 1)), axis=3)[..., 0] - den
    return _skew(den), _skew(lg[..., V - 1] - den), _skew(lpe)


def _loss_stage(logits, denom, d, gs):
    """Coefficients as the device forms them (fp64 alpha / beta, the forward's fp32 denominator, fp32 c1 / sb / se), the fp32 G they give
    (the fp32 route's gradient on these logits: the yardstick) and its two planes."""
    B, T, U1, _, V = dims(d)
    lg64 = logits.astype(np.float64)
    costs, _, work = loss64(lg64, d)
    work["logits"] = np.where(inside(d)[..., None], lg64.reshape(B, T, U1, V), 0.0)
    work["denom"] = np.where(inside(d), denom.astype(np.float64).reshape(B, T, U1), work["denom"])
    coef = {k: (v if k == "y" else v.astype(F32)) for k, v in coef64(d, work, costs, gs).items()}
    g32 = g_from_coef(lg64, coef, V, real=F32)
    gh, gm = split16(g32 * F32(g_scale_of(gs)))
    return costs, g32.astype(np.float64), gh, gm


def _dpre32(gh, gm, e):
    d = e["d"]
    B, T, U1, H, _ = dims(d)
    acc = _mm3(gh, gm, e["wh"], e["wm"]).reshape(B, T, U1, H)
    return (acc * (e["dfac"] * F32(0.25))) * F32(4.0 / (g_scale_of(e["gs"]) * e["sW"]))


def _dw32(gh, gm, hh, hm, gs, drop=None):
    return (_mm3(gh.T, gm.T, hh, hm, drop).astype(np.float64) / (g_scale_of(gs) * SH)).astype(F32).astype(np.float64)


def _db32(gh, gm, gs):
    return ((gh.astype(F32) + gm.astype(F32)).sum(0, dtype=F32).astype(np.float64) / g_scale_of(gs)).astype(F32).astype(np.float64)


def _backward(e, logits, hh, hm, dw_drop=None):
    """Everything behind the forward, from (possibly faulted) logits and hidden planes."""
    d, gs = e["d"], e["gs"]
    costs, g_yard, gh, gm = _loss_stage(logits, _denom32(logits), d, gs)
    dpre = _dpre32(gh, gm, e)
    return dict(costs=costs, g_yard=g_yard, gh=gh, gm=gm, dpre=dpre, grad_enc=dpre.sum(2, dtype=F32).astype(np.float64),
                grad_pred=dpre.sum(1, dtype=F32).astype(np.float64), grad_W=_dw32(gh, gm, hh, hm, gs, dw_drop), grad_bias=_db32(gh, gm, gs))


@functools.lru_cache(maxsize=None)
def _emulate(name):
    """The faithful emulation of one case, each stage fed by the emulated stage before it (as on the device)."""
    d, gs = make_case(name)
    B, T, U1, H, V = dims(d)
    cells = B * T * U1
    flag = bool((np.abs(d["enc"]) > 43).any() or (np.abs(d["pred"]) > 43).any())
    sW = w_scale(d["W"])
    wh, wm = w_pieces(d["W"], sW)
    a = hidden_scaled_f32(d, flag).reshape(cells, H)
    hh, hm = split16(a)
    pad = np.zeros((rows_alloc(cells) - cells, H))
    acc = _mm3(hh, hm, wh.T, wm.T)
    logits = _store_logits(acc, d, sW)
    denom = _denom32(logits)
    e = dict(name=name, d=d, gs=gs, flag=flag, sW=sW, wh=wh, wm=wm, a=a, hh=hh, hm=hm, hi=np.vstack([hh, pad]), mid=np.vstack([hm, pad]),
             acc=acc, logits=logits, denom=denom)
    if name not in LARGE:
        e["dfac"] = dfac_f32(d)
        e.update(_backward(e, logits, hh, hm))
        # the plain fp32 product of the de-scaled planes: the yardstick beside grad_W / grad_bias
        g32 = ((e["gh"] + e["gm"]) / g_scale_of(gs)).astype(F32)
        e["yard_W"] = (g32.T @ ((hh + hm) / SH).astype(F32)).astype(np.float64)
        e["yard_b"] = g32.sum(0, dtype=F32).astype(np.float64)
    return e


@pytest.fixture(params=SMALL)
def emu(request):
    return _emulate(request.param)


def _forward_checks(e):
    d = e["d"]
    E, P = ep_tables(d)
    r = dict(ep=check_ep(kstep_major(E), kstep_major(P), d))
    assert check_scales(e["sW"], 1.0 / e["sW"], e["flag"], d, e["name"] == "exact_forward") == e["sW"]
    r["hidden_structure"], r["hidden"] = check_hidden(e["hi"], e["mid"], d, e["flag"])
    r["logits"], r["logits/fp32-yardstick"] = _chk_logits(e, e["logits"].astype(np.float64))
    r["denom"], r["lpb"], r["lpe"] = check_stats(*_stats(e["logits"], e["denom"], d), e["logits"], d)
    return r


def _dw(e, gW=None, gb=None):
    gh, gm = seen(e["gh"], e["gm"], e["d"])
    return check_dw(e["grad_W"] if gW is None else gW, e["grad_bias"] if gb is None else gb, gh, gm, e["hh"], e["hm"], e["gs"],
                    e["yard_W"], e["yard_b"])


def _dh(e, ge=None, gp=None):
    gh, gm = seen(e["gh"], e["gm"], e["d"])
    return check_dhidden(e["grad_enc"] if ge is None else ge, e["grad_pred"] if gp is None else gp, gh, gm, e["d"], e["sW"], e["gs"])


def test_faithful_emulation_passes_every_comparator(emu):
    e, d = emu, emu["d"]
    r = _forward_checks(e)
    r["G"], costs = check_g(e["gh"], e["gm"], e["logits"].astype(np.float64), d, e["gs"], e["g_yard"])
    assert_close_loss("costs", e["costs"], costs)
    r["grad_enc"], r["grad_pred"] = _dh(e)
    r.update(_dw(e))
    print(e["name"], {k: "%.3f" % v for k, v in r.items()})


@pytest.mark.parametrize("name", LARGE)
def test_large_cases_forward_emulation_passes(name):
    """hidden, logits and statistics only (the CPU suite's time); more_tiles_than_cus is built for 256 CUs."""
    e = _emulate(name)
    B, T, U1, _, _ = dims(e["d"])
    if name == "more_tiles_than_cus":
        assert T == t_for_cus(256) == 330 and (B * T * U1 + 127) // 128 == 256 + 7
    print(name, {k: "%.3f" % v for k, v in _forward_checks(e).items()})


@pytest.mark.parametrize("name", list(CASES))
def test_three_products_drop_what_the_header_says(name):
    """x2.hip: a.b ~ ah.bh + ah.bm + am.bh, 'dropped: am.bm and the residuals, <= 3 x 2^-22 |a.b|' — per logit, against sum_k |a w|."""
    e = _emulate(name)
    ins = inside(e["d"]).reshape(-1)
    r = dropped_terms(e["a"][ins], e["hh"][ins], e["hm"][ins], e["d"]["W"], e["sW"])
    print(name, "dropped / bound %.3f" % r)


def test_twin_is_the_rounding_point_oracle(emu):
    """The fp64 twin with the route's rounding points agrees with the plain fp64 oracle at the fp32 bar (the twin scales G by the fp32
    grad_scale the engine is called with, the oracle takes the mean: linear in the scale)."""
    d = emu["d"]
    tw, ref = twin(d, emu["gs"]), oracle_fused(d)
    k = emu["gs"] * d["enc"].shape[0]
    assert_close_loss("costs", tw["costs"], ref["costs"])
    for key in ("grad_enc", "grad_pred", "grad_W", "grad_bias"):
        assert_close_grad(key, tw[key], ref[key] * k, atol=1e-7 * k)


# ---- seeded faults at probe_cell: each returns what its comparator is handed, or None where the case lacks the geometry
def _row(e):
    return probe_cell(e["d"])[3]


def _acc_row_minus(e, c, what):
    acc = e["acc"].copy()
    acc[c] -= what
    lg = _store_logits(acc, e["d"], e["sW"])
    if (np.abs(lg.astype(np.float64) - e["logits"].astype(np.float64)) <= ulp_fp32(e["logits"][c]).max()).all():
        return None  # (scaled_operands: |W| ~ 1e-6 under a bias of 0.1 — a second-order product moves no entry by more than an fp32 ulp of the row's largest: it is below what the fp32 store resolves)
    return lg.astype(np.float64)


def fault_01_kstep_dropped(e):
    c, H = _row(e), e["hh"].shape[1]
    k = slice(16 * (H // 32), 16 * (H // 32) + 16)
    return _acc_row_minus(e, c, _mm3(e["hh"][c:c + 1, k], e["hm"][c:c + 1, k], e["wh"][:, k].T, e["wm"][:, k].T)[0])


def fault_02_am_wh_dropped(e):
    c = _row(e)
    return _acc_row_minus(e, c, (e["hm"][c:c + 1].astype(F32) @ e["wh"].T.astype(F32))[0])


def fault_03_ah_wm_dropped(e):
    c = _row(e)
    return _acc_row_minus(e, c, (e["hh"][c:c + 1].astype(F32) @ e["wm"].T.astype(F32))[0])


def fault_04_hidden_mid_zeroed(e):
    mid = e["mid"].copy()
    mid[_row(e)] = 0
    return e["hi"], mid


def fault_05_hidden_from_neighbour(e):
    c = _row(e)
    if e["hh"].shape[0] < 2:
        return None
    n = c + 1 if c + 1 < e["hh"].shape[0] else c - 1
    hi, mid = e["hi"].copy(), e["mid"].copy()
    hi[c], mid[c] = hi[n], mid[n]
    return hi, mid


def _with_denom(e, c, value):
    den = e["denom"].copy()
    den[c] = value
    return _stats(e["logits"], den, e["d"])


def fault_06_denom_without_second_pass(e):
    if e["logits"].shape[1] <= 512:
        return None
    c = _row(e)
    return _with_denom(e, c, _denom32(e["logits"][c:c + 1], passes=1)[0])


def fault_07_denom_carries_previous_tile(e):
    """The running (max, sum) not started afresh: the row 128 cells earlier goes through the update formula first."""
    c = _row(e)
    if c < 128:
        return None
    return _with_denom(e, c, F32(np.logaddexp(np.float64(e["denom"][c]), np.float64(e["denom"][c - 128]))))


def fault_08_g_chunk_halves_swapped(e):
    c = _heaviest_cell(e)  # (and its largest entry's chunk: on a peaked softmax most of a row's hi pieces are below fp16's normal range)
    y = int(np.abs(e["gh"][c]).argmax())
    k = slice(32 * (y // 32), 32 * (y // 32) + 32)
    gh, gm = e["gh"].copy(), e["gm"].copy()
    gh[c, k], gm[c, k] = e["gm"][c, k], e["gh"][c, k]
    return gh, gm


def fault_09_g_scale_off_by_a_binade(e):
    return e["grad_enc"] * 2.0, e["grad_pred"] * 2.0


def _heaviest_cell(e):
    return int((np.abs(e["gh"]).sum(1) * inside(e["d"]).reshape(-1)).argmax())


def fault_10_group_left_out(e):
    c0 = 4 * (_heaviest_cell(e) // 4)
    gh, gm = e["gh"].copy(), e["gm"].copy()
    gh[c0:c0 + 4] = 0
    gm[c0:c0 + 4] = 0
    return _dw32(gh, gm, e["hh"], e["hm"], e["gs"]), _db32(gh, gm, e["gs"])


def fault_11_dead_row_keeps_its_logits(e):
    """A row outside the lattices in a live group, not zeroed: the dW GEMM reads its fp32 logits' bytes as fp16 planes."""
    ins = inside(e["d"]).reshape(-1)
    rows = np.flatnonzero(read_rows(e["d"]) & ~ins)
    if len(rows) == 0:
        return None
    c = rows[len(rows) // 2]
    raw = np.ascontiguousarray(e["logits"][c]).view(np.float16).astype(np.float64).reshape(-1, 2, 32)
    gh, gm = seen(e["gh"], e["gm"], e["d"])
    gh[c], gm[c] = raw[:, 0].reshape(-1), raw[:, 1].reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        return _dw32(gh, gm, e["hh"], e["hm"], e["gs"]), _db32(gh, gm, e["gs"])


def fault_12_gm_hh_dropped(e):
    return _dw32(e["gh"], e["gm"], e["hh"], e["hm"], e["gs"], drop="am.bh"), e["grad_bias"]


def fault_13_t_row_missing_from_grad_pred(e):
    b, t, _, _ = probe_cell(e["d"])
    dp = e["dpre"].copy()
    dp[b, t] = 0
    return e["grad_enc"], dp.sum(1, dtype=F32).astype(np.float64)


def fault_14_tanh_prime_of_neighbouring_column(e):
    _, T, U1, _, _ = dims(e["d"])
    c = _heaviest_cell(e)  # (on a peaked softmax the probe cell may carry next to no gradient: no fault to see)
    b, t, u = c // (T * U1), (c // U1) % T, c % U1
    e2 = dict(e, dfac=e["dfac"].copy())
    e2["dfac"][b, t, u] = np.roll(e["dfac"][b, t, u], 1)
    dp = _dpre32(e["gh"], e["gm"], e2)
    return dp.sum(2, dtype=F32).astype(np.float64), dp.sum(1, dtype=F32).astype(np.float64)


def _chk_logits(e, x):
    # (the emulation IS a plain fp32 evaluation of the three products: the yardstick of the CPU file)
    return check_logits(x, e["hi"], e["mid"], e["d"], e["sW"], yard=e["logits"].astype(np.float64))


def _chk_hidden(e, x):
    return check_hidden(x[0], x[1], e["d"], e["flag"])


def _chk_stats(e, x):
    return check_stats(*x, e["logits"], e["d"])


def _chk_g(e, x):
    return check_g(x[0], x[1], e["logits"].astype(np.float64), e["d"], e["gs"], e["g_yard"])


FAULTS = {
    "01_kstep_dropped": (fault_01_kstep_dropped, _chk_logits),
    "02_am_wh_dropped": (fault_02_am_wh_dropped, _chk_logits),
    "03_ah_wm_dropped": (fault_03_ah_wm_dropped, _chk_logits),
    "04_hidden_mid_zeroed": (fault_04_hidden_mid_zeroed, _chk_hidden),
    "05_hidden_from_neighbour": (fault_05_hidden_from_neighbour, _chk_hidden),
    "06_denom_without_second_pass": (fault_06_denom_without_second_pass, _chk_stats),
    "07_denom_carries_previous_tile": (fault_07_denom_carries_previous_tile, _chk_stats),
    "08_g_chunk_halves_swapped": (fault_08_g_chunk_halves_swapped, _chk_g),
    "09_g_scale_off_by_a_binade": (fault_09_g_scale_off_by_a_binade, lambda e, x: _dh(e, *x)),
    "10_group_left_out": (fault_10_group_left_out, lambda e, x: _dw(e, *x)),
    "11_dead_row_keeps_its_logits": (fault_11_dead_row_keeps_its_logits, lambda e, x: _dw(e, *x)),
    "12_gm_hh_dropped": (fault_12_gm_hh_dropped, lambda e, x: _dw(e, *x)),
    "13_t_row_missing_from_grad_pred": (fault_13_t_row_missing_from_grad_pred, lambda e, x: _dh(e, *x)),
    "14_tanh_prime_of_neighbouring_column": (fault_14_tanh_prime_of_neighbouring_column, lambda e, x: _dh(e, *x)),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_seeded_fault_is_rejected(emu, fault):
    make, check = FAULTS[fault]
    x = make(emu)
    if x is None:
        return  # the case lacks the geometry (V <= 512, fewer than 129 cells, no readable row outside the lattices)
    with pytest.raises(AssertionError):
        check(emu, x)


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_fault_applies_somewhere(fault):
    """A fault that never applied would prove nothing."""
    assert sum(FAULTS[fault][0](_emulate(name)) is not None for name in SMALL) >= 1


@pytest.mark.parametrize("fault", ["02_am_wh_dropped", "03_ah_wm_dropped", "04_hidden_mid_zeroed", "12_gm_hh_dropped"])
def test_the_final_outputs_bar_cannot_see_the_second_order_faults(fault):
    """Why the stages are compared: on cfg2_hv the emulation WITH the fault, carried through every later stage, still passes the suite's
    bar on the final outputs (assert_close_loss / assert_close_grad against the plain fp64 oracle, 1e-4 of the largest entry) — while
    test_seeded_fault_is_rejected shows its stage comparator rejecting it."""
    e = _emulate("cfg2_hv")
    make = FAULTS[fault][0]
    x = make(e)
    if fault == "12_gm_hh_dropped":
        out = dict(e, grad_W=x[0])
    elif fault == "04_hidden_mid_zeroed":
        cells = e["hh"].shape[0]
        hm = x[1][:cells]
        out = _backward(e, _store_logits(_mm3(e["hh"], hm, e["wh"].T, e["wm"].T), e["d"], e["sW"]), e["hh"], hm)
    else:
        out = _backward(e, x.astype(F32), e["hh"], e["hm"])
    ref = oracle_fused(e["d"])
    k = e["gs"] * e["d"]["enc"].shape[0]
    assert_close_loss("costs", out["costs"], ref["costs"])
    for key in ("grad_enc", "grad_pred", "grad_W", "grad_bias"):
        assert_close_grad(key, out[key], ref[key] * k)
