"""The f16x2 route (rnnt_amd/csrc/x2.hip) stage by stage: cases, the exact fp16 splits, an fp64 twin and one comparator per stage.
Pure numpy: tests/test_x2_stages_oracle.py proves the comparators on the CPU (a faithful fp32 emulation passes, seeded faults do
not), tests/test_x2_stages_gpu.py feeds them the device's buffers.

Every comparator takes the operand PIECES the device produced upstream (its two fp16 hidden planes, its fp32 logits, its two fp16 G
planes; W's pieces are recomputed bit-exactly from W and the device's s_W), so the fp64 reference forms exactly the three products
the kernel forms, ah.bh + ah.bm + am.bh, and only fp32 accumulation error remains.  Each element is held to a bar built from
    U24 = 2^-24          fp32 unit roundoff: an fp32 sum of n terms, in any order, is within n U24 sum |terms|
    ulp_fp16 / ulp_fp32  the spacing of the format at a value; a round-to-nearest store is within half of it
    2^-22, 2^-25         the two-piece representation x = hi + mid: hi = f16(x) leaves |x - hi| <= 2^-11 |x|, mid = f16(x - hi) leaves
                         2^-11 of that; below fp16's normal range the spacing is 2^-24, a rounding half of it
    YARD = 4             the project's factor on a measured fp32 yardstick (tests/bf16_stage_cases.py)
No other tolerance appears below; every other number is computed from the reference or from an fp32 yardstick on the same operands."""
import math

import numpy as np

from oracle import cpu_oracle
from tests.bf16_stage_cases import LOG2E_F32, U24, YARD, _judge, _ulp, coef64, dims, fast_tanh_f32, g_from_coef, inside, loss64, probe_cell, tanh64, ulp_fp16  # noqa: F401
from tests.helpers import make_inputs
from tests.x2_flush_twin import CASES as FLUSH_CASES, g_scale_log2

SH = 2.0 ** 14  # x2.hip X2_SH: the hidden operand's scale
F16_MAX = 65504.0
F32 = np.float32
TWO_LOG2E = 2.8853900817779268  # k_x2_make_ep: 2 log2 e, a double

# name: (B, T, U, H, V) and the path the shape takes (x2.hip); the smallest shape that takes it.
#   lens / logit_std / permuted: as tests/bf16_stage_cases.py;  enc_row_times: (b, t, factor);  w_max: max |W| rescaled to it;
#   grad_scale: instead of float32(1 / B);  n_cu: T is chosen for the device's CU count;  flush: tests/x2_flush_twin.py's case
CASES = {
    "one_cell": dict(shape=(1, 1, 0, 128, 128)),  # one cell; the tile's padding rows
    "tile_over_two_utterances": dict(shape=(2, 9, 4, 128, 128)),  # ragged; k_dhidden_x2<true,true>; dW's half-empty h block
    "partial_pass_v384": dict(shape=(3, 23, 19, 256, 384)),  # one partial column pass; k_dw_x2<4>
    "two_passes_v640": dict(shape=(2, 12, 5, 128, 640)),  # a full pass + a 128-column rest: the statistics carried across passes
    "cfg2_hv": dict(shape=(2, 20, 9, 512, 1024)),  # two full passes; k_dhidden_x2<true,false>
    "h1024": dict(shape=(1, 37, 6, 1024, 256)),  # second dHidden pass <false,false>
    "h896": dict(shape=(1, 20, 9, 896, 128)),  # second pass <false,true>; odd dW block
    "h640_x2r": dict(shape=(2, 13, 20, 640, 128)),  # k_dhidden_x2r; k_dw_x2<4,true>
    "h640_dw_mixed": dict(shape=(1, 21, 9, 640, 512)),  # k_dw_x2m (k-step list walk) + k_dhidden_x2r
    "u1_is_one": dict(shape=(2, 70, 0, 128, 128)),  # no label arc
    "u1_17": dict(shape=(1, 20, 16, 128, 128)),  # a second u block that holds one column
    "dead_tiles": dict(shape=(5, 3, 40, 256, 128), lens=([3, 1, 2, 3, 1], [40, 0, 13, 40, 7])),
    "exact_forward": dict(shape=(2, 12, 5, 128, 128), enc_row_times=(0, 3, 40.0)),  # |enc| > 43: ep_flag, k_joint_fwd_x2<0>
    "peaked_softmax": dict(shape=(2, 20, 9, 512, 1024), logit_std=8.0),  # G spans many binades
    "scaled_operands": dict(shape=(2, 9, 4, 128, 128), w_max=1e-6, grad_scale=4096.0),  # s_W, g_scale far from 1
    "permuted_enc": dict(shape=(2, 21, 6, 128, 128), permuted=True),
    "more_tiles_than_cus": dict(shape=(2, None, 50, 128, 128), n_cu=True),  # a persistent forward workgroup's second tile
    "flushed_band": dict(shape=FLUSH_CASES["ragged"][:5], flush="ragged"),  # live-tile / live-group lists shorter than by length
}
LARGE = ("more_tiles_than_cus", "flushed_band")


def t_for_cus(n_cu):
    """The T of `more_tiles_than_cus`: the largest with ceil(2 T 51 / 128) forward tiles = n_cu + 7 (a step of T adds 102 / 128 of a
    tile, so one exists for every n_cu; 330 for 256 CUs)."""
    T = 1
    while (2 * (T + 1) * 51 + 127) // 128 <= n_cu + 7:
        T += 1
    assert (2 * T * 51 + 127) // 128 == n_cu + 7
    return T


def make_case(name, n_cu=256):
    """-> (d, grad_scale): a make_inputs dict and the scale the engine is called with (as the fp32 the C ABI takes)."""
    spec = CASES[name]
    if "flush" in spec:
        B, T, U, H, V, seed, ragged, gs = FLUSH_CASES[spec["flush"]]
        return make_inputs(B, T, U, H, V, seed, ragged=ragged), float(F32(gs))
    B, T, U, H, V = spec["shape"]
    if spec.get("n_cu"):
        T = t_for_cus(n_cu)
    d = make_inputs(B, T, U, H, V, seed=B + T + U + H + V)
    if "lens" in spec:
        d["logit_lens"] = np.array(spec["lens"][0], dtype=np.int32)
        d["target_lens"] = np.array(spec["lens"][1], dtype=np.int32)
    if "logit_std" in spec:
        lg = cpu_oracle.joint_fwd(d["enc"][:1, :8], d["pred"][:1, :8], d["W"], np.zeros_like(d["bias"]), dtype=np.float64)
        d["W"] = (d["W"] * (spec["logit_std"] / lg.std())).astype(F32)
        d["bias"] = np.zeros_like(d["bias"])
    if "enc_row_times" in spec:
        b, t, f = spec["enc_row_times"]
        d["enc"][b, t] *= F32(f)
        assert (np.abs(d["enc"]) > 43.0).any()
    if "w_max" in spec:
        d["W"] = (d["W"] / np.abs(d["W"]).max() * spec["w_max"]).astype(F32)
    return d, float(F32(spec.get("grad_scale", 1.0 / B)))


def ulp_fp32(x):
    return _ulp(x, 23, -126)


def g_scale_of(gs):
    return 2.0 ** g_scale_log2(gs)


def rows_alloc(cells):
    """engine.hip layout / bf16_rows_alloc: the rows of a hidden plane."""
    rows_pad = (cells + 1 + 31) // 32 * 32
    return (rows_pad + 96 + 127) // 128 * 128


# ---- the route's exact arithmetic
def split16(x):
    """fp32 (scaled) values -> their (hi, mid) fp16 pieces as float64 (split_common.hpp F16x2::prepare + split2): hi = f16(x), mid = f16(x - hi),
    round-to-nearest-even each; the residual is exact in fp32 (v_fma_mix), so numpy's conversions give the device's bits."""
    x = np.clip(np.asarray(x, dtype=F32), F32(-F16_MAX), F32(F16_MAX))
    hi = x.astype(np.float16)
    mid = (x - hi.astype(F32)).astype(np.float16)
    return hi.astype(np.float64), mid.astype(np.float64)


def w_scale(W):
    """k_x2_wscale: s_W = 2^k with max |W| 2^k in [2^13, 2^14), k clamped to +-100; 1 for W == 0 (or a subnormal maximum)."""
    m = float(np.abs(W).max())
    if m < 2.0 ** -126 or not np.isfinite(m):
        return 1.0
    _, e = math.frexp(m)  # m in [2^(e-1), 2^e)
    return 2.0 ** max(-100, min(100, 14 - e))


def w_pieces(W, sW):
    """(wh, wm) [V, H] float64: the pieces of s_W W as both W packs hold them (s_W is a power of two: the scaling is exact)."""
    return split16(W.astype(F32) * F32(sW))


def ep_tables(d):
    """k_x2_make_ep in fp64: exp2(clamp(2 log2e x, +-126)) — exp(2 x), held inside fp32's normal range — rounded once to fp32,
    -> (E [B, T, H], P [B, U1, H]) float32, row major."""
    def tab(x):
        return np.exp2(np.clip(x.astype(np.float64) * TWO_LOG2E, -126.0, 126.0)).astype(F32)
    return tab(d["enc"]), tab(d["pred"])


def kstep_major(x):
    """[B, R, H] -> [B][H/16][R][16]: the tables' layout in the workspace."""
    B, R, H = x.shape
    return np.ascontiguousarray(x.reshape(B, R, H // 16, 16).transpose(0, 2, 1, 3))


def _f32_of(x64):
    return np.asarray(x64, dtype=np.float64).astype(F32)


def hidden_scaled_f32(d, ep_flag):
    """The forward's 2^14 tanh(enc + pred) [B, T, U1, H] operation by operation in fp32 (each fma: exact in fp64, rounded once).
    ep_flag == 0: k_joint_fwd_x2<1>, r = rcp(fma(E, P, 1)), fma(-2^15, r, 2^14);  else <0>: common.hpp fast_tanh, scaled."""
    with np.errstate(over="ignore", invalid="ignore"):
        if ep_flag:
            return fast_tanh_f32(d) * F32(SH)  # (a power of two: the same rounding as the kernel's scaled form)
        E, P = ep_tables(d)
        s = _f32_of(E[:, :, None, :].astype(np.float64) * P[:, None, :, :].astype(np.float64) + 1.0)
        r = F32(1.0) / s
        return _f32_of(SH - 2.0 * SH * r.astype(np.float64))


def dfac_f32(d):
    """k_dhidden_x2's tanh' = 4 w / (1 + w)^2, w = exp2(-|2 log2e x|), x = enc + pred, in fp32 -> [B, T, U1, H]."""
    x = d["enc"][:, :, None, :] + d["pred"][:, None, :, :]
    with np.errstate(under="ignore"):
        w = np.exp2(-np.abs(x * (F32(2.0) * LOG2E_F32)))
        r = F32(1.0) / (w + F32(1.0))
        return F32(4.0) * ((w * r) * r)


def dtanh64(d):
    """1 - tanh^2(enc + pred) in fp64 as 4 w / (1 + w)^2, w = exp(-2 |x|): the same function, without the cancellation that leaves
    1 - tanh64^2 with no correct digit beyond |x| ~ 18 (exact_forward reaches |x| > 100)."""
    x = d["enc"][:, :, None, :].astype(np.float64) + d["pred"][:, None, :, :].astype(np.float64)
    w = np.exp(-2.0 * np.abs(x))
    return 4.0 * w / (1.0 + w) ** 2


def three(ah, am, bh, bm):
    """ah.bh + ah.bm + am.bh (the products the route forms) and the same sum of absolute values, in fp64: (a [m, k], b [k, n])."""
    return ah @ bh + ah @ bm + am @ bh, np.abs(ah) @ np.abs(bh) + np.abs(ah) @ np.abs(bm) + np.abs(am) @ np.abs(bh)


def unskew(x, B, T, U1):
    """[B][T + U1 - 1][U1] -> [B, T, U1]: cell (t, u) sits at row t + u, column u."""
    x = np.asarray(x).reshape(B, T + U1 - 1, U1)
    t, u = np.arange(T)[:, None], np.arange(U1)[None, :]
    return x[:, t + u, u]


def read_rows(d):
    """[cells] bool: the G rows the dW GEMM can read without the flush rule — every cell of a 4-cell group (linear index // 4) that
    holds a lattice cell.  k_dhidden_x2 writes the rows of its live tiles, k_x2_dead_rows zeroes the other rows of live groups;
    a row outside both is never read and keeps its logits (x2.hip "The flush rule and the live structures")."""
    ins = inside(d).reshape(-1)
    n = (ins.size + 3) // 4 * 4
    g = np.zeros(n, dtype=bool)
    g[:ins.size] = ins
    return np.repeat(g.reshape(-1, 4).any(1), 4)[:ins.size]


def twin(d, gs):
    """The route in fp64 with its rounding points: hidden and g_scale G as two fp16 pieces of their fp32 values, W's pieces, three
    products each, fp32 logits.  -> dict(costs, grad_enc, grad_pred, grad_W, grad_bias) (gradients of sum_b grad_scale cost_b)."""
    B, T, U1, H, V = dims(d)
    sW, gsc = w_scale(d["W"]), g_scale_of(gs)
    wh, wm = w_pieces(d["W"], sW)
    t64 = tanh64(d)
    hh, hm = split16((t64 * SH).astype(F32).reshape(-1, H))
    logits = (three(hh, hm, wh.T, wm.T)[0] / (SH * sW) + d["bias"].astype(np.float64)).astype(F32).astype(np.float64)
    costs, G, _ = loss64(logits, d)
    gh, gm = split16((G * gs * gsc).astype(F32))
    dpre = (three(gh, gm, wh, wm)[0] / (gsc * sW)).reshape(B, T, U1, H) * dtanh64(d)
    return dict(costs=costs, grad_enc=dpre.sum(2), grad_pred=dpre.sum(1), grad_W=three(gh.T, gm.T, hh, hm)[0] / (gsc * SH),
                grad_bias=(gh + gm).sum(0) / gsc)


# ---- comparators: pure functions of numpy arrays; each asserts error <= bar per element and returns the worst error / bar
def check_scales(sW_dev, inv_dev, ep_flag, d, want_flag):
    """s_W = 2^(14 - e), max |W| in [2^(e-1), 2^e) (k_x2_wscale; 1 for W == 0), 1 / s_W its reciprocal: powers of two, exact.
    ep_flag is non-zero exactly where an |enc| or |pred| exceeds 43 (k_x2_make_ep)."""
    sW = w_scale(d["W"])
    assert float(sW_dev) == sW and float(inv_dev) == 1.0 / sW, (sW_dev, inv_dev, sW)
    assert bool(ep_flag) == bool(want_flag), ep_flag
    assert bool(want_flag) == bool((np.abs(d["enc"]) > 43).any() or (np.abs(d["pred"]) > 43).any())
    return sW


def check_ep(E_dev, P_dev, d):
    """ep = exp(2 enc) | exp(2 pred) as [B][H/16][rows][16] fp32, computed in double and rounded once: each entry within one fp32 ulp
    of float32(exp(2 float64(x))) (the device's double exp2 is good to ~1e-14 relative: it can only move a value that sits on a
    rounding boundary).  The kernel clamps 2 log2e x to +-126 — the tables stay inside fp32's normal range — and so does the
    reference (exact_forward is the one case that reaches the clamp).  -> worst |dev - ref| / ulp_fp32(ref) over both tables"""
    worst = 0.0
    for dev, ref in zip((E_dev, P_dev), ep_tables(d)):
        ref = kstep_major(ref).astype(np.float64)
        dev = np.asarray(dev, dtype=np.float64).reshape(ref.shape)
        worst = max(worst, _judge("ep", np.abs(dev - ref), ulp_fp32(ref)))
    return worst


def check_hidden(hi, mid, d, ep_flag):
    """hidden planes [rows_alloc, H] each (2^14 tanh(enc + pred) as hi + mid), every cell's row:
      structure, exact: |mid| <= ulp_fp16(hi) / 2 wherever hi is a normal fp16 below 65504 (mid = f16(x - hi), |x - hi| <= ulp / 2, the
        conversion is monotone and ulp / 2 is an fp16 number or, in the lowest normal binade, a tie that rounds to 0);
      value: |(hi + mid) / 2^14 - tanh64| <= 2^-22 |tanh64| + 2^-25 2^-14 + A — the two-piece representation, fp16's subnormal floor
        (spacing 2^-24 of the scaled value), and A = YARD x the largest |fp32 numpy evaluation of the kernel's formula - tanh64| over the
        case (ep_flag = 0: 1 - 2 / (1 + E P) with E, P rounded once to fp32; else common.hpp fast_tanh);
      the rows past the last cell: exactly zero in both planes.
    -> (worst structure ratio, worst value ratio)"""
    B, T, U1, H, _ = dims(d)
    cells = B * T * U1
    assert hi.shape == mid.shape == (rows_alloc(cells), H), (hi.shape, cells)
    assert (hi[cells:] == 0).all() and (mid[cells:] == 0).all(), "hidden: a padding row is not zero"
    h, m = hi[:cells], mid[:cells]
    normal = (np.abs(h) >= 2.0 ** -14) & (np.abs(h) < F16_MAX)
    rs = _judge("hidden structure", np.abs(m[normal]), 0.5 * ulp_fp16(h[normal]))
    ref = tanh64(d)
    A = YARD * float(np.abs(hidden_scaled_f32(d, ep_flag).astype(np.float64) / SH - ref).max())
    ref = ref.reshape(cells, H)
    return rs, _judge("hidden", np.abs((h + m) / SH - ref), 2.0 ** -22 * np.abs(ref) + 2.0 ** -25 / SH + A)


def check_logits(dev, hi, mid, d, sW, yard=None):
    """logits [cells, V] fp32 = fma(acc, 2^-14 / s_W, bias), acc the fp32 MFMA accumulation of the 3 H exact fp16 products ah.wh, ah.wm,
    am.wh:  against ref64 = (sum_k ah wh + ah wm + am wh) / (2^14 s_W) + bias on the device's hidden pieces,
        |dev - ref64| <= (3 H + 2) U24 mag + ulp_fp32(ref64) / 2,   mag = the same sum of absolute values + |bias|
    (an fp32 sum of 3 H terms in any order, two more roundings allowed for, and the final fma's rounding; the unscale is a power of
    two).  Lattice cells.
    That bound grows with H and is loose for a sum of terms of both signs (one second-order product lost from a row stays inside it from
    H = 256 on), so with `yard` — a plain fp32 evaluation of the same three products, unscale and bias on the same pieces, [cells, V]: numpy
    in the CPU test, torch on the device in the GPU test — the case's largest error must also be <= YARD x the yardstick's largest.
    -> worst ratio to the bound, or (that, ratio beside the yardstick)"""
    H = hi.shape[1]
    ins = inside(d).reshape(-1)
    cells = ins.size
    wh, wm = w_pieces(d["W"], sW)
    acc, mag = three(hi[:cells][ins], mid[:cells][ins], wh.T, wm.T)
    bias = d["bias"].astype(np.float64)
    ref = acc / (SH * sW) + bias
    mag = mag / (SH * sW) + np.abs(bias)
    x = dev[ins]
    assert np.isfinite(x).all(), "logits: non-finite values"
    r = _judge("logits", np.abs(x - ref), (3 * H + 2) * U24 * mag + 0.5 * ulp_fp32(ref))
    if yard is None:
        return r
    return r, _judge("logits beside fp32", np.abs(x - ref).max(), YARD * np.abs(yard[ins] - ref).max())


def dropped_terms(a_scaled, hh, hm, W, sW):
    """What the three products leave out of a (s_W w) — am.wm and both operands' residuals — against the claim of x2.hip's header,
    <= 3 x 2^-22 sum_k |a w|, per logit: `a_scaled` [rows, H] the fp32 values that were split into (hh, hm).  fp64 holds every product
    exactly (24 x 24 bits).  -> worst |dropped| / (3 2^-22 sum |a w|)"""
    w = (W.astype(F32) * F32(sW)).astype(np.float64)
    wh, wm = w_pieces(W, sW)
    a = a_scaled.astype(np.float64)
    kept = three(hh, hm, wh.T, wm.T)[0]
    return _judge("dropped terms", np.abs(a @ w.T - kept), 3 * 2.0 ** -22 * (np.abs(a) @ np.abs(w).T))


def lse_f32(lg):
    """A plain fp32 log-sum-exp of each row: the yardstick of the forward's statistics."""
    lg = lg.astype(F32)
    m = lg.max(-1)
    return m + np.log(np.exp(lg - m[..., None]).sum(-1, dtype=F32))


def check_stats(denom_s, lpb_s, lpe_s, logits_dev, d):
    """The forward's per-row statistics (skewed [B][T + U1 - 1][U1] fp32), on every lattice cell, against the device's own logits row:
      denom_s within Y + ulp_fp32(lse64) of lse64, Y = YARD x the largest |plain fp32 numpy log-sum-exp - lse64| over the case's lattice
        rows (the ulp: the store of the value itself, which the yardstick's error may happen to miss);
      lpb_s = logit[blank] - denom_s and, where u < U_b, lpe_s = logit[y] - denom_s: one fp32 subtraction of the device's own
        denominator — to the same bar, the ulp taken at the difference.
    -> (ratio of denom, of lpb, of lpe)"""
    B, T, U1, _, V = dims(d)
    ins = inside(d)
    lg = np.asarray(logits_dev, dtype=np.float64).reshape(B, T, U1, V)
    rows = lg[ins]
    m = rows.max(-1)
    lse = m + np.log(np.exp(rows - m[:, None]).sum(-1))
    Y = YARD * float(np.abs(lse_f32(rows).astype(np.float64) - lse).max())
    den = unskew(denom_s, B, T, U1).astype(np.float64)
    rd = _judge("denom_s", np.abs(den[ins] - lse), Y + ulp_fp32(lse))
    ref_b = lg[..., V - 1] - den
    rb = _judge("lpb_s", np.abs(unskew(lpb_s, B, T, U1).astype(np.float64) - ref_b)[ins], Y + ulp_fp32(ref_b[ins]))
    lab = ins & (np.arange(U1)[None, None, :] < d["target_lens"][:, None, None])
    re = 0.0
    if lab.any():
        y = np.zeros((B, U1), dtype=np.int64)
        y[:, :U1 - 1] = d["targets"]
        ref_e = np.take_along_axis(lg, np.broadcast_to(y[:, None, :, None], (B, T, U1, 1)), axis=3)[..., 0] - den
        re = _judge("lpe_s", np.abs(unskew(lpe_s, B, T, U1).astype(np.float64) - ref_e)[lab], Y + ulp_fp32(ref_e[lab]))
    return rd, rb, re


def g_chunks(planes):
    """[cells, 2 V] fp16 as stored (per 32-wide chunk: 32 x hi | 32 x mid) -> (hi, mid) [cells, V]."""
    c = planes.reshape(planes.shape[0], -1, 2, 32)
    return c[:, :, 0, :].reshape(planes.shape[0], -1), c[:, :, 1, :].reshape(planes.shape[0], -1)


def check_g(gh, gm, logits_dev, d, gs, yard):
    """G's planes [cells, V] each (g_scale grad_scale d cost / d logits as hi + mid; statistics, lattice sweep, coefficients and the
    production inside k_dhidden_x2 in one comparison), produced with the flush rule off:  against G64 = loss64(device logits) grad_scale,
        |(hi + mid) / g_scale - G64| <= 2^-22 |G64| + 2^-25 / g_scale + E,   E = YARD x max |yard - G64|
    (`yard`: an fp32 evaluation of the same gradient on the same logits — on the GPU the fp32 route's standalone rnnt_amd.rnnt_loss).
    Structure, exact, as for hidden: |mid| <= ulp_fp16(hi) / 2 wherever hi is a normal fp16 below 65504 (the value hi + mid alone cannot
    tell the two halves of a chunk apart).  A cell outside the lattices in a row the dW GEMM can read (read_rows) holds exactly 0, as values; the other rows outside the
    lattices are never read and not looked at.  -> (worst ratio, the fp64 costs)"""
    ins = inside(d).reshape(-1)
    gsc = g_scale_of(gs)
    costs, G, _ = loss64(logits_dev, d)
    G64 = G * gs
    z = read_rows(d) & ~ins
    assert (gh[z] == 0).all() and (gm[z] == 0).all(), "G: a readable cell outside the lattices is not zero"
    assert np.isfinite(yard[ins]).all(), "G: the fp32 yardstick is not finite"
    E = YARD * float(np.abs(yard[ins] - G64[ins]).max())
    normal = ins[:, None] & (np.abs(gh) >= 2.0 ** -14) & (np.abs(gh) < F16_MAX)
    _judge("G structure", np.abs(gm[normal]), 0.5 * ulp_fp16(gh[normal]))
    dev = (gh[ins] + gm[ins]) / gsc
    return _judge("G", np.abs(dev - G64[ins]), 2.0 ** -22 * np.abs(G64[ins]) + 2.0 ** -25 / gsc + E), costs


def seen(gh, gm, d):
    """G's planes as the backward GEMMs see them: the rows outside the lattices zeroed (check_g proves the readable ones are)."""
    ins = inside(d).reshape(-1)[:, None]
    return np.where(ins, gh, 0.0), np.where(ins, gm, 0.0)


DT_FLOOR = 2.0 ** -124  # 4 x fp32's smallest normal: below it the kernel's w = exp2(-|.|) is subnormal (the hardware may flush it)


def check_dhidden(grad_enc, grad_pred, gh, gm, d, sW, gs):
    """grad_enc [B, T, H] / grad_pred [B, U1, H]:  against dpre64 = (sum_v gh wh + gh wm + gm wh) / (g_scale s_W) (1 - tanh64(enc + pred)^2)
    (evaluated as dtanh64) on the device's G pieces, summed over u / over t, per entry
        ((3 V + n + 4) U24 + D) sum |terms| + 2^-124 sum |products|
    n = U1 / T rows summed; 3 V terms per dot product, n per sum, 4 for the factor's product, the unscale and the slabs' stores;
    D = YARD x the largest relative error of an fp32 numpy evaluation of the kernel's 4 w / (1 + w)^2, w = exp(-2 |x|), against
    1 - tanh64^2 over the case's entries >= 2^-124; below that — |x| > 43, only exact_forward — w leaves fp32's normal range and the
    factor may be flushed to 0: the last term (sum |products|: the sum without the factor).  Rows past an utterance's lengths: exactly 0.
    -> (worst ratio of grad_enc, of grad_pred)"""
    B, T, U1, H, V = dims(d)
    gsc = g_scale_of(gs)
    wh, wm = w_pieces(d["W"], sW)
    dt = dtanh64(d)
    big = dt >= DT_FLOOR
    D = YARD * float((np.abs(dfac_f32(d).astype(np.float64) - dt)[big] / dt[big]).max())
    acc, mag = three(gh, gm, wh, wm)
    acc, mag = acc.reshape(B, T, U1, H) / (gsc * sW), mag.reshape(B, T, U1, H) / (gsc * sW)
    dpre, mdt = acc * dt, mag * dt
    dead_t = np.arange(T)[None, :] >= d["logit_lens"][:, None]
    dead_u = np.arange(U1)[None, :] > d["target_lens"][:, None]
    assert (grad_enc[dead_t] == 0).all(), "grad_enc: a row past its utterance's length is not zero"
    assert (grad_pred[dead_u] == 0).all(), "grad_pred: a row past its utterance's labels is not zero"
    re = _judge("grad_enc", np.abs(grad_enc - dpre.sum(2)), ((3 * V + U1 + 4) * U24 + D) * mdt.sum(2) + DT_FLOOR * mag.sum(2))
    rp = _judge("grad_pred", np.abs(grad_pred - dpre.sum(1)), ((3 * V + T + 4) * U24 + D) * mdt.sum(1) + DT_FLOOR * mag.sum(1))
    return re, rp


def check_dw(grad_W, grad_bias, gh, gm, hh, hm, gs, yard_W, yard_b):
    """grad_W [V, H] / grad_bias [V]:  against refW = sum_cells (gh hh + gh hm + gm hh) / (g_scale 2^14), refb = sum_cells (gh + gm) / g_scale
    in fp64 on the device's planes (hh, hm: the cells' rows), per entry  (3 cells + 8) U24 sum |g| |h|  (three products per cell; 8: the
    split-K slabs' reduction).  That bound is loose for a sum over cells, so each array's largest error must also be <= YARD x that
    of a plain fp32 product / sum of the same de-scaled planes (`yard_W`, `yard_b`: torch on the device in the GPU test).
    -> dict of the four worst ratios"""
    cells = gh.shape[0]
    gsc = g_scale_of(gs)
    refW, magW = three(gh.T, gm.T, hh, hm)
    refW, magW = refW / (gsc * SH), magW / (gsc * SH)
    refb, magb = (gh + gm).sum(0) / gsc, (np.abs(gh) + np.abs(gm)).sum(0) / gsc
    out = dict(W_bound=_judge("grad_W", np.abs(grad_W - refW), (3 * cells + 8) * U24 * magW),
               b_bound=_judge("grad_bias", np.abs(grad_bias - refb), (3 * cells + 8) * U24 * magb))
    out["W_yard"] = _judge("grad_W beside fp32", np.abs(grad_W - refW).max(), YARD * np.abs(yard_W - refW).max())
    out["b_yard"] = _judge("grad_bias beside fp32", np.abs(grad_bias - refb).max(), YARD * np.abs(yard_b - refb).max())
    return out
