"""The fp32 route (rnnt_amd/csrc/joint_fwd.hip, joint_bwd.hip) and the bf16x3 route (x3.hip) stage by stage, with the lattice sweep and
the coefficient kernel they share (lattice.hip): cases, the exact 3-way bf16 split, fp64 references and one comparator per stage.
Pure numpy: tests/test_f32_stages_oracle.py proves the comparators on the CPU (a faithful fp32 emulation passes, seeded faults do
not), tests/test_f32_stages_gpu.py feeds them the device's buffers.

Every comparator takes the operands the DEVICE produced upstream (its fp32 hidden or its three bf16 hidden planes, its logits, its
lp / alpha / beta planes, its coefficients, its G), so only the error of the stage under test remains.  On the bf16x3 route the fp64
reference forms exactly the six products the kernels form, ah.bh + ah.bm + am.bh + am.bm + ah.bl + al.bh (W's pieces are recomputed
bit-exactly from W), so only fp32 accumulation error remains.  Each element is held to a bar built from
    U24 = 2^-24     fp32 unit roundoff: an fp32 sum of n terms, in any order, is within n U24 sum |terms|
    ulp_fp32        the spacing of fp32 at a value; a round-to-nearest store (or a library function good to one ulp) is within it
    YARD = 4        the project's factor on a measured yardstick: an fp32 numpy evaluation of the kernel's formula against fp64
No other tolerance appears below; every other number is computed from the reference or from a yardstick on the same operands.

Where the issue's derivations were off:
  * the fp32 forward's tiles never span two utterances (64 compact live cells of ONE utterance, grid (tiles, B)): the case that was
    to share a tile between two ragged utterances gives each its own, partly filled tile;
  * three bf16 pieces of an fp32 value sum to it EXACTLY (8 + 8 + 8 bits, each residual exact), so "hi + mid + lo to 2^-24 relative"
    is held as equality wherever the value is a normal fp32; and the bit-exact split conditions cannot see a wrong lo piece (any lo
    that is a proper residual is self-consistent) — the value bars do;
  * a per-entry n-term bound cannot see one lost second-order product (2^-17 of 16 terms under a bound of 6 H U24 of all of them):
    logits and dW also get YARD x a plain fp32 yardstick on the same pieces, as tests/x2_stage_cases.py found necessary, and the
    bf16x3 logits a projection on every product of every k-step (check_products_x3);
  * a library GEMM or column sum (blockwise, pairwise) is no yardstick for an MFMA accumulator's chain: its error is a fraction of any
    single chain's.  On an MI355X the bf16x3 logits at H >= 640 were 1.2 x, grad_bias up to 3.5 x over YARD x torch's; the
    yardsticks are therefore the plain chains they were meant to be (chain_six, chain_mm, chain_colsum), + half an ulp for the store;
  * the bf16x3 dot products have 6 x (their length) terms, not (their length): the bounds count them;
  * lp_emit of a cell without a label (u >= U_b) is never read: left out of the statistics' and the lattice's comparisons;
  * bf16_stage_cases.coef64 rebuilds lp_blank / lp_emit from logits and the oracle's denominator; k_coef reads the device's own
    fp32 lp planes and takes the cost from beta[0, 0], so the coefficients' reference here is coef_f64 on exactly those planes."""
import functools

import numpy as np

from tests.bf16_stage_cases import LOG2E, LOG2E_F32, U24, YARD, _judge, dims, fast_tanh_f32, g_from_coef, inside, loss64, probe_cell, tanh64  # noqa: F401
from tests.helpers import bf16_round, make_inputs
from tests.x2_stage_cases import DT_FLOOR, check_stats, dfac_f32, dtanh64, t_for_cus, ulp_fp32, unskew  # noqa: F401
from oracle import cpu_oracle

F32 = np.float32
LN2_F32 = F32(0.6931471805599453)  # lattice.hip: the factor on v_log_f32
FLOOR32 = 2.0 ** -126  # fp32's smallest normal number

# ---- cases.  name: (B, T, U, H, V) and the path the shape takes; the smallest shape that takes it.
#   lens / logit_std / permuted: as tests/bf16_stage_cases.py;  n_cu: T is chosen for the device's CU count;  full: no ragged lengths
F32_CASES = {
    "one_cell": dict(shape=(1, 1, 0, 4, 4)),  # one cell; V % 32 != 0: k_make_g, k_dhidden on every column
    "ragged_pair": dict(shape=(2, 9, 4, 64, 32)),  # two ragged utterances, one partly filled forward tile each
    "fwd_odd_chunks_h136": dict(shape=(2, 7, 5, 136, 64)),  # ceil(H / 8) = 17: the forward without the two-register-set loop
    "fwd_persistent_h128": dict(shape=(2, 11, 6, 128, 64)),  # ceil(H / 8) even: the persistent forward; three tiles an utterance
    "more_tiles_than_2_cus": dict(shape=(2, None, 50, 16, 32), n_cu=True, full=True),  # a persistent workgroup's second tile
    "make_g_v36": dict(shape=(2, 9, 4, 64, 36)),  # V % 32 != 0: mask 15 leaves G in place of the logits
    "dhidden_tiles_16t_8u": dict(shape=(2, 16, 4, 64, 64)),  # dhidden_gen_bu = 8
    "dhidden_tiles_8t_16u": dict(shape=(2, 9, 11, 64, 64)),  # dhidden_gen_bu = 16
    "h1024_two_column_groups": dict(shape=(1, 9, 5, 1024, 32)),  # k_dhidden_gen<., true> then <., false> at column 512
    "h640_tile_plus_persistent": dict(shape=(2, 10, 7, 640, 32)),  # k_dhidden_gen on 512 columns, k_dhidden on the other 128
    "u1_is_one": dict(shape=(2, 70, 0, 64, 32)),  # no label arc
    "dw_list_walk": dict(shape=(5, 3, 40, 64, 32), lens=([3, 1, 2, 3, 1], [40, 0, 13, 40, 7])),  # dead granules inside live time steps
    "dw_range_walk": dict(shape=(3, 12, 6, 64, 32), lens=([12, 5, 9], [6, 6, 6])),  # full targets, ragged T: contiguous ranges
    "peaked_softmax": dict(shape=(2, 20, 9, 128, 256), logit_std=8.0),
    "permuted_enc": dict(shape=(2, 21, 6, 64, 32), permuted=True),
    "wave_boundary_u1_71": dict(shape=(1, 40, 70, 8, 32)),  # the chained sweep's mailbox between two waves
    "barrier_sweep": dict(shape=(1, 5400, 64, 8, 8)),  # (NW - 1) D 12 > 64 KiB: launch_lattice takes k_lattice
}
F32_LARGE = ("more_tiles_than_2_cus", "barrier_sweep")
X3_CASES = {
    "one_cell": dict(shape=(1, 1, 0, 128, 128)),
    "tile_of_90_cells": dict(shape=(2, 9, 4, 128, 128)),  # one 128-cell forward tile over two ragged utterances
    "tile_of_130_cells": dict(shape=(2, 13, 4, 128, 128)),  # the second tile has two live rows
    "v640_partial_pass": dict(shape=(2, 12, 5, 128, 640)),  # a full 512-column pass + a 128-column one
    "cfg2_hv": dict(shape=(2, 20, 9, 512, 1024)),  # V = 1024: two full passes, at the training configuration's H and V
    "more_tiles_than_cus": dict(shape=(2, None, 50, 128, 128), n_cu=True),  # a persistent forward workgroup's second tile
    "h640_second_dhidden_launch": dict(shape=(2, 13, 20, 640, 128)),  # k_dhidden_x3<false> on 128 columns; partial 256 x 256 dW tiles
    "h1024": dict(shape=(1, 37, 6, 1024, 256)),  # k_dhidden_x3<false> on a whole 512
    "partial_8t_16u_tiles": dict(shape=(1, 11, 18, 128, 128)),  # T % 8 != 0, U1 % 16 != 0
    "v384_h640": dict(shape=(1, 9, 4, 640, 384)),  # partial dW tiles in both directions
    "fewer_ksteps_than_slabs": dict(shape=(2, 20, 2, 128, 128)),  # 8 16-cell k-steps for n_split = 40 slabs
    "u1_is_one": dict(shape=(2, 70, 0, 128, 128)),
    "dead_tiles": dict(shape=(5, 3, 40, 256, 128), lens=([3, 1, 2, 3, 1], [40, 0, 13, 40, 7])),  # the 32-row live table
    "peaked_softmax": dict(shape=(2, 20, 9, 128, 512), logit_std=8.0),
    "permuted_enc": dict(shape=(2, 21, 6, 128, 128), permuted=True),
    "rows_past_a_live_end": dict(shape=(3, 24, 8, 128, 128), lens=([24, 24, 6], [8, 8, 8])),  # the live table's 32-row rounding reaches a dead tile
}
X3_LARGE = ("more_tiles_than_cus",)


def t_for_2_cus(n_cu):
    """The T of `more_tiles_than_2_cus`: the smallest with 2 ceil(51 T / 64) forward tiles >= 2 n_cu + 8 (323 for 256 CUs)."""
    T = 1
    while 2 * ((51 * T + 63) // 64) < 2 * n_cu + 8:
        T += 1
    return T


def make_case(route, name, n_cu=256):
    """-> (d, grad_scale): a make_inputs dict and the scale the engine is called with (as the fp32 the C ABI takes)."""
    spec = (F32_CASES if route == "fp32" else X3_CASES)[name]
    B, T, U, H, V = spec["shape"]
    if spec.get("n_cu"):
        T = t_for_2_cus(n_cu) if route == "fp32" else t_for_cus(n_cu)
    d = make_inputs(B, T, U, H, V, seed=B + T + U + H + V, ragged=not spec.get("full"))
    if "lens" in spec:
        d["logit_lens"] = np.array(spec["lens"][0], dtype=np.int32)
        d["target_lens"] = np.array(spec["lens"][1], dtype=np.int32)
    if "logit_std" in spec:
        lg = cpu_oracle.joint_fwd(d["enc"][:1, :8], d["pred"][:1, :8], d["W"], np.zeros_like(d["bias"]), dtype=np.float64)
        d["W"] = (d["W"] * (spec["logit_std"] / lg.std())).astype(F32)
        d["bias"] = np.zeros_like(d["bias"])
    return d, float(F32(1.0 / B))


# ---- the launchers' decisions restated (engine.hip, joint_fwd.hip, joint_bwd.hip, lattice.hip): what path a shape takes
def fwd_pairs(H):
    return ((H + 7) // 8) % 2 == 0


def gen_bu(T, U1):
    c16 = (U1 + 15) // 16 * 16 * ((T + 7) // 8 * 8)
    c8 = (U1 + 7) // 8 * 8 * ((T + 15) // 16 * 16)
    return 8 if c8 < c16 else 16


def tile_cols(H, V):
    """Columns of H the fp32 route's tile kernel takes (0: k_make_g and the persistent kernel on every column)."""
    return 0 if V % 32 else 512 * (1 if H <= 512 else H // 512)


def barrier_sweep(U1, D):
    return ((U1 + 63) // 64 - 1) * D * 12 > 64 * 1024


def rows_pad(cells, gran):
    return (cells + 1 + gran - 1) // gran * gran


def rows_alloc(cells):
    return (rows_pad(cells, 32) + 96 + 127) // 128 * 128


def table_rows(d, gran):
    """[cells] bool: the rows the dW GEMMs' live-row table covers (k_dw_table): each utterance's first T_b U1 cells, rounded out to
    whole granules of `gran` cells (16 on the fp32 route, 32 on bf16x3).  The fp32 route's granule list is a subset of them."""
    B, T, U1, _, _ = dims(d)
    r = np.zeros((B * T * U1 + gran - 1) // gran * gran, dtype=bool)
    for b in range(B):
        c0 = b * T * U1
        r[c0 // gran * gran:(c0 + int(d["logit_lens"][b]) * U1 + gran - 1) // gran * gran] = True
    return r[:B * T * U1]


# ---- the bf16x3 route's exact arithmetic
def split3(x):
    """fp32 values -> their (hi, mid, lo) bf16 pieces as float64 (split_common.hpp Bf16x3::split2): hi = bf16(x), mid = bf16(x - hi), lo = bf16(x -
    hi - mid), round-to-nearest-even each; both residuals are exact in fp32, so numpy gives the device's bits."""
    x = np.asarray(x, dtype=F32)
    hi = bf16_round(x)
    r = x - hi
    mid = bf16_round(r)
    return hi.astype(np.float64), mid.astype(np.float64), bf16_round(r - mid).astype(np.float64)


def six(a, b):
    """The six products the route forms of a = (ah, am, al) [m, k] and b = (bh, bm, bl) [k, n], and the same sum of absolute values."""
    ah, am, al = a
    bh, bm, bl = b
    v = ah @ bh + ah @ bm + am @ bh + am @ bm + ah @ bl + al @ bh
    ah, am, al, bh, bm, bl = (np.abs(x) for x in (ah, am, al, bh, bm, bl))
    return v, ah @ bh + ah @ bm + am @ bh + am @ bm + ah @ bl + al @ bh


def tr(p):
    return tuple(x.T for x in p)


def chain_six(a, b, first=None):
    """The plain fp32 yardstick of a six-product GEMM: ONE fp32 accumulator per entry, the six products of each 16-deep k-step added to
    it in turn, k-step after k-step — the chain an MFMA accumulator runs.  (A library GEMM sums blockwise: its error is a fraction of
    any single chain's and no yardstick for one.)  `a`, `b`: three fp32 planes each, [m, k] / [k, n]; numpy arrays or torch tensors.
    `first`: the accumulator's first value (the bias)."""
    acc = first
    for k0 in range(0, a[0].shape[1], 16):
        for i, j in ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)):
            p = a[i][:, k0:k0 + 16] @ b[j][k0:k0 + 16, :]
            acc = p if acc is None else acc + p
    return acc


def chain_mm(a, b, step, first=None):
    """The plain fp32 yardstick of a GEMM a [m, k] . b [k, n]: one fp32 accumulator per entry over k-steps of `step` (2: the fp32
    MFMA's), as chain_six.  numpy arrays or torch tensors."""
    acc = first
    for k0 in range(0, a.shape[1], step):
        p = a[:, k0:k0 + step] @ b[k0:k0 + step, :]
        acc = p if acc is None else acc + p
    return acc


def chain_colsum(planes, group):
    """The plain fp32 yardstick of a column sum over cells: one fp32 accumulator per column, each plane's `group`-row sums added to it
    in turn, group after group — 16 for k_dw_x3 (an MFMA against ones per plane and k-step), 1 for k_dw (in-lane adds, cell after
    cell).  numpy arrays [cells, V]; numpy's cumsum is a sequential scan."""
    n, V = planes[0].shape
    if n == 0:
        return np.zeros(V)
    pad = (-n) % group
    g = np.stack([np.vstack([p.astype(F32), np.zeros((pad, V), dtype=F32)]).reshape(-1, group, V).sum(1, dtype=F32) for p in planes], axis=1)
    return np.cumsum(g.reshape(-1, V), axis=0, dtype=F32)[-1].astype(np.float64)


def g_chunks(planes):
    """[cells, 2 V] bf16 as stored (per 32-wide chunk: 32 x hi | 32 x mid) -> (hi, mid) [cells, V]."""
    c = planes.reshape(planes.shape[0], -1, 2, 32)
    return c[:, :, 0, :].reshape(planes.shape[0], -1), c[:, :, 1, :].reshape(planes.shape[0], -1)


def skew(x):
    """[B, T, U1] -> [B][T + U1 - 1][U1]: cell (t, u) at row t + u, column u (zeros elsewhere)."""
    B, T, U1 = x.shape
    out = np.zeros((B, T + U1 - 1, U1), dtype=x.dtype)
    t, u = np.arange(T)[:, None], np.arange(U1)[None, :]
    out[:, t + u, u] = x
    return out


# ---- the lattice sweep: one recurrence, the correction term exchangeable
def corr64(dl):
    return np.log1p(np.exp(dl))


def corr32(dl):
    """lattice.hip's correction operation by operation in fp32: the difference rounded to fp32, x log2e, exp2, 1 + x, log2, x ln 2."""
    x = np.exp2(np.asarray(dl).astype(F32) * LOG2E_F32)
    return (np.log2(F32(1.0) + x) * LN2_F32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def step_yard():
    """The largest |corr32 - corr64| over differences in [-110, 0] (401 001 points; beyond -104 the fp32 term is 0 and the true one
    below 1e-45): the measured error of an fp32 numpy evaluation of one step's correction — 1.04e-7, YARD x it = 2^-21.2 (the issue's own count of
    the step's roundings came to "about 2^-21")."""
    dl = -np.concatenate([np.linspace(0.0, 110.0, 400001), np.exp2(-np.arange(1, 1001) / 20.0)])
    return float(np.abs(corr32(dl) - corr64(dl)).max())


def sweep(lpb, lpe, d, corr=corr64, stale_col=None, beta_from_zero=False):
    """alpha, beta [B, T, U1] float64 (-inf outside the lattices) from lp_blank / lp_emit [B, T, U1]: the recurrence of lattice.hip,
    v = max(a, e) + corr(min(a, e) - max(a, e)), every sum in fp64.  Seeded faults: `stale_col` — the label predecessor of that
    column arrives one step late (alpha[t - 1, col - 1] for alpha[t, col - 1]: the chained sweep's mailbox);  `beta_from_zero`."""
    B, T, U1 = lpb.shape
    lpb, lpe = lpb.astype(np.float64), lpe.astype(np.float64)
    alpha, beta = np.full((B, T, U1), -np.inf), np.full((B, T, U1), -np.inf)

    def lse(a, e):
        with np.errstate(invalid="ignore", over="ignore"):
            m = np.maximum(a, e)
            return m + corr(np.where(np.isfinite(m), np.minimum(a, e) - m, 0.0))  # (a missing predecessor: corr(-inf) = 0)

    for b in range(B):
        Tb, Ub = int(d["logit_lens"][b]), int(d["target_lens"][b])
        al = np.full((Tb + 1, Ub + 2), -np.inf)  # al[t + 1, u + 1] = alpha[t, u]
        al[1, 1] = 0.0
        be = np.full((Tb + 1, Ub + 2), -np.inf)  # be[t, u] = beta[t, u]
        be[Tb - 1, Ub] = 0.0 if beta_from_zero else lpb[b, Tb - 1, Ub]
        for k in range(1, Tb + Ub):
            u = np.arange(max(0, k - Tb + 1), min(k, Ub) + 1)
            t = k - u
            a = al[t, u + 1] + lpb[b, np.maximum(t - 1, 0), u]
            late = (u == stale_col) & (t >= 1) if stale_col is not None else np.zeros(len(u), dtype=bool)
            e = np.where(late, al[t, u], al[t + 1, u]) + lpe[b, t, np.maximum(u - 1, 0)]
            al[t + 1, u + 1] = lse(a, e)
            dd = Tb + Ub - 1 - k
            u = np.arange(max(0, dd - Tb + 1), min(dd, Ub) + 1)
            t = dd - u
            be[t, u] = lse(be[t + 1, u] + lpb[b, t, u], be[t, u + 1] + np.where(u < Ub, lpe[b, t, np.minimum(u, U1 - 1)], 0.0))
        alpha[b, :Tb, :Ub + 1] = al[1:, 1:]
        beta[b, :Tb, :Ub + 1] = be[:Tb, :Ub + 1]
    return alpha, beta


def coef_f64(alpha, beta, denom, lpb, lpe, d, gs):
    """lattice.hip k_coef in fp64 from the planes it reads ([B, T, U1] each; the cost is -beta[b, 0, 0]) -> dict of [cells] arrays:
    c1 (-inf outside the lattices), sb, se, y (-1 where no label), xb / xe, the arguments of the two exponentials, and c1mag, the sum of
    the absolute values of c1's terms."""
    B, T, U1, _, _ = dims(d)
    ins = inside(d)
    c1, sb, se = np.full((B, T, U1), -np.inf), np.zeros((B, T, U1)), np.zeros((B, T, U1))
    xb, xe, m1 = np.zeros((B, T, U1)), np.zeros((B, T, U1)), np.zeros((B, T, U1))
    y = np.full((B, T, U1), -1, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for b in range(B):
            Tb, Ub = int(d["logit_lens"][b]), int(d["target_lens"][b])
            ac = alpha[b].astype(np.float64) - beta[b, 0, 0]
            c1[b][ins[b]] = ((ac + beta[b] - denom[b].astype(np.float64) + np.log(gs)) * LOG2E)[ins[b]]
            m1[b][ins[b]] = ((np.abs(alpha[b]) + abs(beta[b, 0, 0]) + np.abs(beta[b]) + np.abs(denom[b]) + abs(np.log(gs))) * LOG2E)[ins[b]]
            xb[b, :Tb - 1, :Ub + 1] = (ac[:Tb - 1] + beta[b, 1:Tb] + lpb[b, :Tb - 1])[:, :Ub + 1]
            xb[b, Tb - 1, Ub] = ac[Tb - 1, Ub] + lpb[b, Tb - 1, Ub]
            hasb = np.zeros((T, U1), dtype=bool)
            hasb[:Tb - 1, :Ub + 1] = True
            hasb[Tb - 1, Ub] = True
            sb[b] = np.where(hasb, gs * np.exp(xb[b]), 0.0)
            if Ub > 0:
                xe[b, :Tb, :Ub] = ac[:Tb, :Ub] + beta[b, :Tb, 1:Ub + 1] + lpe[b, :Tb, :Ub]
                se[b, :Tb, :Ub] = gs * np.exp(xe[b, :Tb, :Ub])
                y[b, :Tb, :Ub] = d["targets"][b, :Ub][None, :]
    return {k: v.reshape(-1) for k, v in dict(c1=c1, sb=sb, se=se, y=y, xb=xb, xe=xe, c1mag=m1).items()}


def twin(route, d, gs):
    """The route in fp64 with its rounding points (fp32: none but the fp32 logits; bf16x3: operands as three bf16 pieces of their
    fp32 values, six products).  -> dict(costs, grad_enc, grad_pred, grad_W, grad_bias) (gradients of sum_b grad_scale cost_b)."""
    B, T, U1, H, V = dims(d)
    t64 = tanh64(d).reshape(-1, H)
    if route == "fp32":
        W = d["W"].astype(np.float64)
        logits = (t64 @ W.T + d["bias"].astype(np.float64)).astype(F32).astype(np.float64)
        costs, G, _ = loss64(logits, d)
        G = G * gs
        acc, gW, gb = G @ W, G.T @ t64, G.sum(0)
    else:
        hp, wp = split3(t64.astype(F32)), split3(d["W"])
        logits = (six(hp, tr(wp))[0] + d["bias"].astype(np.float64)).astype(F32).astype(np.float64)
        costs, G, _ = loss64(logits, d)
        gp = split3((G * gs).astype(F32))
        acc, gW, gb = six(gp, wp)[0], six(tr(gp), hp)[0], sum(gp).sum(0)
    dpre = acc.reshape(B, T, U1, H) * dtanh64(d)
    return dict(costs=costs, grad_enc=dpre.sum(2), grad_pred=dpre.sum(1), grad_W=gW, grad_bias=gb)


# ---- comparators: pure functions of numpy arrays; each asserts error <= bar per element and returns the worst error / bar
def _tanh_yard(d):
    ref = tanh64(d)
    return ref, YARD * float(np.abs(fast_tanh_f32(d).astype(np.float64) - ref).max())


def check_hidden_f32(dev, d):
    """hidden [cells, H] fp32 = common.hpp fast_tanh(enc + pred):  |dev - tanh64| <= A + ulp_fp32(tanh64) on every cell of a lattice,
    A = YARD x the largest |fp32 numpy evaluation of 1 - 2 / (1 + 2^(2 x log2 e)) - tanh64| over the case (the factor covers the
    hardware's approximate exp2 and rcp), the ulp the store of the value itself.  Every other row the backward GEMMs read (they
    multiply it by exact zeros) must be finite."""
    H = dev.shape[1]
    ref, A = _tanh_yard(d)
    ref = ref.reshape(-1, H)
    ins = inside(d).reshape(-1)
    assert np.isfinite(dev).all(), "hidden: a non-finite value"
    return _judge("hidden", np.abs(dev[ins] - ref[ins]), A + ulp_fp32(ref[ins]))


def check_split(what, hi, mid, lo):
    """The split conditions of three bf16 planes, bit-exact: S = hi + mid + lo (fp64: exact) is an fp32 number, hi = bf16(S), mid =
    bf16(S - hi), lo = bf16(S - hi - mid) — wherever |S| >= 2^-100: every piece is then a multiple of S's last bit, >= 2^-123, and none
    falls below bf16's normal range (below, a residual is rounded on the subnormal grid — or flushed — and the sum is no longer the
    value that was split: a peaked softmax has such entries).  -> S"""
    S = hi + mid + lo
    S32 = S.astype(F32)
    normal = np.abs(S) >= 2.0 ** -100
    assert (S32.astype(np.float64)[normal] == S[normal]).all(), f"{what}: hi + mid + lo is not an fp32 number"
    h2, m2, l2 = split3(S32)
    for k, got, want in (("hi", hi, h2), ("mid", mid, m2), ("lo", lo, l2)):
        bad = (got != want) & normal
        assert not bad.any(), f"{what}: {k} is not the bf16 rounding of its residual at {np.argwhere(bad)[0]}"
    return S


def check_hidden_x3(planes, d):
    """hidden planes [3][rows_alloc][H] (as float64): the split conditions on every cell's row, the value hi + mid + lo to
    check_hidden_f32's bar on every lattice cell (the kernel rounds its fp32 tanh into the pieces exactly); the rows past the last
    cell: exactly zero in all three planes."""
    B, T, U1, H, _ = dims(d)
    cells = B * T * U1
    assert planes.shape == (3, rows_alloc(cells), H), (planes.shape, cells)
    assert (planes[:, cells:] == 0).all(), "hidden: a padding row is not zero"
    assert np.isfinite(planes).all(), "hidden: a non-finite value"
    ins = inside(d).reshape(-1)
    S = check_split("hidden", planes[0, :cells][ins], planes[1, :cells][ins], planes[2, :cells][ins])
    ref, A = _tanh_yard(d)
    ref = ref.reshape(cells, H)[ins]
    return _judge("hidden", np.abs(S - ref), A + ulp_fp32(ref))


def check_logits_f32(dev, hidden_dev, d, yard=None):
    """logits [cells, V] fp32 = hidden . W^T + bias, fp32 accumulation:  against ref64 on the device's fp32 hidden,
        |dev - ref64| <= (H + 1) U24 (sum_k |h w| + |bias|) + ulp_fp32(ref64) / 2
    (an fp32 sum of H + 1 terms in any order, and the store).  Lattice cells.  With `yard` — a plain fp32 evaluation of the same
    product on the same operands — the case's largest error must also be <= YARD x the yardstick's.  -> ratio | (ratio, beside yard)"""
    H = hidden_dev.shape[1]
    ins = inside(d).reshape(-1)
    W, bias = d["W"].astype(np.float64), d["bias"].astype(np.float64)
    h = hidden_dev[ins]
    ref = h @ W.T + bias
    mag = np.abs(h) @ np.abs(W).T + np.abs(bias)
    x = dev[ins]
    assert np.isfinite(x).all(), "logits: non-finite values"
    r = _judge("logits", np.abs(x - ref), (H + 1) * U24 * mag + 0.5 * ulp_fp32(ref))
    if yard is None:
        return r
    return r, _judge("logits beside fp32", np.abs(x - ref).max(), YARD * np.abs(yard[ins] - ref).max())


def check_logits_x3(dev, planes, d, yard):
    """logits [cells, V] fp32, the fp32 MFMA accumulation of the 6 H exact bf16 products, bias as the accumulator's first value:
    against ref64 = the six products of the device's hidden planes with W's pieces + bias,
        |dev - ref64| <= (6 H + 1) U24 (the same sum of absolute values + |bias|) + ulp_fp32(ref64) / 2.
    That bound is loose for a sum of terms of both signs (one k-step's al.bh is 2^-17 of 16 of the 6 H terms), so the case's largest
    error must also be <= YARD x that of `yard`, a plain fp32 evaluation of the same six products + bias on the same pieces (chain_six:
    numpy in the CPU test, torch on the device in the GPU test), and check_products_x3 holds.
    -> (ratio to the bound, ratio beside the yardstick, ratio of the products' shares)"""
    H = planes.shape[2]
    ins = inside(d).reshape(-1)
    cells = ins.size
    hp = tuple(planes[p, :cells][ins] for p in range(3))
    bias = d["bias"].astype(np.float64)
    acc, mag = six(hp, tr(split3(d["W"])))
    ref, mag = acc + bias, mag + np.abs(bias)
    x = dev[ins]
    assert np.isfinite(x).all(), "logits: non-finite values"
    return (_judge("logits", np.abs(x - ref), (6 * H + 1) * U24 * mag + 0.5 * ulp_fp32(ref)),
            _judge("logits beside fp32", np.abs(x - ref).max(), YARD * np.abs(yard[ins] - ref).max()),
            check_products_x3(_place(x - ref, ins), _place(yard[ins] - ref, ins), planes, d))


def _place(x, ins):
    out = np.zeros((ins.size, x.shape[1]))
    out[ins] = x
    return out


def check_products_x3(err, yard_err, planes, d):
    """Is every product of every k-step in the logits?  From H = 256 on, one k-step's al.bh (2^-17 of 16 terms) is below the fp32
    accumulation noise of a single entry, so no per-entry bar can see it lost; over a forward tile (128 consecutive cells x V
    columns) it is plain.  For product j of k-step s and tile r, P = that product alone [tile rows, V] (fp64, exact) and
        c(j, s, r) = <err, P> / <P, P>,     err = dev - ref64 on the tile's lattice rows (zero elsewhere)
    estimates how much of P is MISSING from the device's logits: 0 when it is there, -1 when it was dropped; rounding noise moves it by
    about noise / (|P| sqrt(entries)).  The bar: |c| <= YARD x the largest |c| that `yard_err` shows (the error of a plain fp32
    evaluation of the same six products on the same pieces, projected the same way) over all j, s, r.  -> worst |c| / bar"""
    H = planes.shape[2]
    cells = err.shape[0]
    hp = [planes[p, :cells] for p in range(3)]
    wp = split3(d["W"])
    starts = np.arange(0, cells, 128)
    got, yd = [], []
    for s in range(H // 16):
        k = slice(16 * s, 16 * s + 16)
        for i, j in ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)):
            P = hp[i][:, k] @ wp[j][:, k].T
            pp = np.add.reduceat((P * P).sum(1), starts)
            ok = pp > 0
            got.append((np.add.reduceat((err * P).sum(1), starts)[ok] / pp[ok]))
            yd.append((np.add.reduceat((yard_err * P).sum(1), starts)[ok] / pp[ok]))
    got, yd = np.abs(np.concatenate(got)), np.abs(np.concatenate(yd))
    return _judge("logits: a product's share", got.max() if got.size else 0.0, YARD * (yd.max() if yd.size else 0.0))


def dropped_terms(a, W):
    """What the six products leave out of a . w — am.bl, al.bm, al.bl — against x3.hip's header, "the terms dropped are <= 2^-24
    |a.b|", per logit against sum_k |a w| (fp64 holds every product of two fp32 numbers exactly).  -> worst |dropped| / bound"""
    a, w = np.asarray(a, dtype=F32), np.asarray(W, dtype=F32)
    kept = six(split3(a), tr(split3(w)))[0]
    a, w = a.astype(np.float64), w.astype(np.float64)
    return _judge("dropped terms", np.abs(a @ w.T - kept), U24 * (np.abs(a) @ np.abs(w).T))


def check_lattice(alpha_s, beta_s, costs, lpb_s, lpe_s, d):
    """alpha_s / beta_s (skewed [B][D][U1] fp64) and costs [B] fp32 against the fp64 sweep on the device's own lp planes.
    One step forms v = max(a, e) + c(min - max) with the sums in fp64 and the correction c in fp32 (lattice.hip lae / the chained
    step: the difference rounded to fp32, x log2e, v_exp_f32, 1 + x, v_log_f32, x ln 2); dv / da + dv / de = 1 with both >= 0, so a
    cell's error is at most its worse predecessor's plus the step's own: cell (t, u) of alpha is t + u dependent steps from
    alpha[0, 0] = 0 (exact), of beta (T_b - 1 - t) + (U_b - u) from beta[T_b - 1, U_b] = lp_blank there (exact):
        |dev - ref64| <= steps x E + steps x 8 x 2^-53 max |ref64|,   E = YARD x step_yard()
    (step_yard: the measured error of an fp32 numpy evaluation of the correction; the last term: the fp64 sums of both sides).
    costs[b] is float32(-beta[b, 0, 0]) of the device's own plane, bit for bit.  -> (ratio of alpha, of beta)"""
    B, T, U1, _, _ = dims(d)
    ins = inside(d)
    lpb = unskew(lpb_s, B, T, U1)
    lpe = np.where(np.arange(U1)[None, None, :] < d["target_lens"][:, None, None], unskew(lpe_s, B, T, U1), 0.0)
    ra, rb = sweep(lpb, lpe, d)
    al, be = unskew(alpha_s, B, T, U1), unskew(beta_s, B, T, U1)
    t, u = np.arange(T)[None, :, None], np.arange(U1)[None, None, :]
    sa = np.broadcast_to(t + u, ins.shape)
    sb = (d["logit_lens"][:, None, None] - 1 - t) + (d["target_lens"][:, None, None] - u)
    E = YARD * step_yard()
    out = []
    for what, dev, ref, steps in (("alpha", al, ra, sa), ("beta", be, rb, sb)):
        assert np.isfinite(dev[ins]).all(), f"{what}: a non-finite value inside a lattice"
        fl = 8 * 2.0 ** -53 * float(np.abs(ref[ins]).max())
        out.append(_judge(what, np.abs(dev[ins] - ref[ins]), steps[ins] * (E + fl)))
    want = (-be[:, 0, 0]).astype(F32)
    assert np.array_equal(np.asarray(costs, dtype=F32).view(np.uint32), want.view(np.uint32)), ("costs are not float32(-beta[0, 0])", costs, want)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def exp_yard():
    """The largest relative error of numpy's fp32 exp on fp32 arguments in [-87, 0.01] (normal results) against fp64."""
    x = np.linspace(-87.0, 0.01, 200001).astype(F32)
    r = np.exp(x.astype(np.float64))
    return float((np.abs(np.exp(x).astype(np.float64) - r) / r).max())


def check_coef(coef_dev, y_dev, alpha, beta, denom, lpb, lpe, d, gs):
    """coef [cells][4] = (c1, sb, se) fp32 and y int32 (lattice.hip k_coef) against coef_f64 on the planes the device's kernel
    read ([B, T, U1], unskewed).  Exact parts: c1 = -inf, sb = se = 0, y = -1 outside the lattices; y the cell's label; sb = 0 where
    no blank arc leaves (t = T_b - 1, u < U_b); se = 0 where no label arc does.
      c1 = float32((alpha + cost + beta - denom + logf(scale)) log2e), the sum in fp64:  |dev - c1_64| <= ulp_fp32(c1_64) / 2 +
        log2e ulp_fp32(log scale) + 8 x 2^-53 sum |terms| (the one rounding — the store is correctly rounded, so ratios sit just under 1 —,
        logf good to one ulp, and the fp64 sums of both sides, which may put the two on either side of a rounding boundary);
      sb, se = scale x expf(float32(x)), x the fp64 sum of three terms:  |dev - s_64| <= (|x| U24 + YARD x exp_yard() + U24) s_64
        + 2^-126 — the argument's rounding moves exp by |x| U24 relative, the fp32 exp, the product with the scale, and a result below
        fp32's normal range may be flushed to zero.
    -> (ratio of c1, of sb, of se)"""
    ins = inside(d).reshape(-1)
    ref = coef_f64(alpha, beta, denom, lpb, lpe, d, gs)
    c1, sb, se = (coef_dev[:, i].astype(np.float64) for i in range(3))
    assert (c1[~ins] == -np.inf).all() and (sb[~ins] == 0).all() and (se[~ins] == 0).all(), "coef: a cell outside the lattices is not dead"
    assert np.array_equal(np.asarray(y_dev, dtype=np.int64), ref["y"]), "coef: labels"
    assert (sb[ref["sb"] == 0] == 0).all() and (se[ref["se"] == 0] == 0).all(), "coef: an arc that does not exist has a weight"
    assert np.isfinite(c1[ins]).all(), "coef: c1 of a lattice cell is not finite"
    with np.errstate(invalid="ignore"):
        e1 = np.abs(c1 - ref["c1"])[ins]
    r1 = _judge("c1", e1, 0.5 * ulp_fp32(ref["c1"][ins]) + LOG2E * ulp_fp32(np.log(gs)) * (gs != 1.0) + 8 * 2.0 ** -53 * ref["c1mag"][ins])
    rel = YARD * exp_yard() + U24
    rb = _judge("sb", np.abs(sb - ref["sb"]), (np.abs(ref["xb"]) * U24 + rel) * ref["sb"] + FLOOR32)
    re = _judge("se", np.abs(se - ref["se"]), (np.abs(ref["xe"]) * U24 + rel) * ref["se"] + FLOOR32)
    return r1, rb, re


@functools.lru_cache(maxsize=None)
def exp2_yard():
    """The largest relative error of numpy's fp32 exp2 on fp32 arguments in [-126, 1] against fp64."""
    x = np.linspace(-126.0, 1.0, 200001).astype(F32)
    r = np.exp2(x.astype(np.float64))
    return float((np.abs(np.exp2(x).astype(np.float64) - r) / r).max())


def coef_dict(coef_dev, y_dev):
    return dict(c1=coef_dev[:, 0].astype(np.float64), sb=coef_dev[:, 1].astype(np.float64), se=coef_dev[:, 2].astype(np.float64),
                y=np.asarray(y_dev, dtype=np.int64))


def g_ref(logits_dev, coef, d, floor=FLOOR32):
    """-> (G64, bar) [cells, V]: G = 2^(fma(logit, log2e_f32, c1)) - [v = blank] sb - [v = y] se from the device's logits and
    coefficients (g_from_coef with the kernels' fp32 constant), and what an fp32 evaluation may differ by: the fma's rounding of the
    exponent x moves 2^x by ln 2 |x| U24 relative, v_exp_f32 by YARD x exp2_yard(), each of the two subtractions rounds once:
        bar = 2^x (ln 2 |x| U24 + YARD exp2_yard()) + 2 U24 (2^x + sb + se) + floor
    (2^-126: a result below fp32's normal range may be flushed to zero)."""
    V = logits_dev.shape[1]
    G = g_from_coef(logits_dev, coef, V, log2e=float(LOG2E_F32))
    live = np.isfinite(coef["c1"])
    with np.errstate(invalid="ignore"):
        x = np.where(live[:, None], np.where(live[:, None], logits_dev, 0.0) * float(LOG2E_F32) + coef["c1"][:, None], -np.inf)
    e = np.exp2(x)
    sub = np.zeros_like(e)
    sub[:, V - 1] += coef["sb"]
    lab = coef["y"] >= 0
    sub[np.flatnonzero(lab), coef["y"][lab]] += coef["se"][lab]
    ax = np.where(live[:, None], np.abs(x), 0.0)
    return G, e * (np.log(2.0) * ax * U24 + YARD * exp2_yard()) + 2 * U24 * (e + sub) + floor


def check_g_f32(dev, logits_dev, coef, d, read):
    """G [cells, V] fp32 in place of the logits (k_dhidden_gen's production, or k_make_g) against g_ref on the device's logits and
    coefficients, on every lattice cell.  Structure: a row outside the lattices that a kernel can read (`read`: table_rows(d, 16),
    the dW walk's ranges) holds exact zeros; the tile kernel leaves the tiles of dead time steps beyond them unwritten."""
    ins = inside(d).reshape(-1)
    z = read & ~ins
    assert (dev[z] == 0).all(), "G: a readable row outside the lattices is not zero"
    G, bar = g_ref(logits_dev, coef, d)
    return _judge("G", np.abs(dev[ins] - G[ins]), bar[ins])


def check_g_x3(gh, gm, gl, logits_dev, coef, d, read):
    """G's planes [cells, V] each (hi | mid in place per 32-wide chunk, lo beside): the split conditions on every lattice cell's row
    (they tell the two halves of a chunk apart, which the value cannot), the value hi + mid + lo to check_g_f32's bar (the kernel
    rounds its fp32 G into the pieces exactly; below 2^-100 a piece may fall under bf16's normal range and be flushed, up to 2^-8 of the
    value: the floor is 2^-108), and exact zeros in all three planes on every row of `read` outside the lattices
    (k_dhidden_x3 writes every row: all of them; the fp32 tile kernel standing in for it: table_rows(d, 32))."""
    ins = inside(d).reshape(-1)
    z = read & ~ins
    assert (gh[z] == 0).all() and (gm[z] == 0).all() and (gl[z] == 0).all(), "G: a readable row outside the lattices is not zero in every plane"
    S = check_split("G", gh[ins], gm[ins], gl[ins])
    G, bar = g_ref(logits_dev, coef, d, floor=2.0 ** -108)
    return _judge("G", np.abs(S - G[ins]), bar[ins])


def _dh_judge(grad_enc, grad_pred, acc, mag, dt, dterr, n_dot, d):
    B, T, U1, H, _ = dims(d)
    acc, mag = acc.reshape(B, T, U1, H), mag.reshape(B, T, U1, H)
    dpre = acc * dt
    bar = lambda n, ax: ((n_dot + n + 4) * U24 * (mag * dt) + dterr * mag).sum(ax)  # noqa: E731
    dead_t = np.arange(T)[None, :] >= d["logit_lens"][:, None]
    dead_u = np.arange(U1)[None, :] > d["target_lens"][:, None]
    assert (grad_enc[dead_t] == 0).all(), "grad_enc: a row past its utterance's length is not zero"
    assert (grad_pred[dead_u] == 0).all(), "grad_pred: a row past its utterance's labels is not zero"
    return _judge("grad_enc", np.abs(grad_enc - dpre.sum(2)), bar(U1, 2)), _judge("grad_pred", np.abs(grad_pred - dpre.sum(1)), bar(T, 1))


def check_dhidden_f32(grad_enc, grad_pred, G_dev, hidden_dev, d):
    """grad_enc [B, T, H] / grad_pred [B, U1, H] = ((G . W) (1 - hidden^2)) summed over u / over t (joint_bwd.hip):  against the same
    expression in fp64 on the device's G (rows outside the lattices as zeros: check_g_f32 proves the readable ones are) and its fp32 hidden, per entry
        (V + n + 4) U24 sum |terms| + 2 U24 sum |G . W|
    n = U1 / T rows summed; V terms per dot product, n per sum, 4 for the factor's product and the slabs' stores; the last term: the
    fp32 factor 1 - h h is within U24 h^2 + U24 (1 - h^2) <= 2 U24 of the fp64 one, ABSOLUTELY (it cancels near |h| = 1).  Rows past
    an utterance's lengths: exactly 0.  -> (worst ratio of grad_enc, of grad_pred)"""
    B, T, U1, H, V = dims(d)
    W = d["W"].astype(np.float64)
    dt = (1.0 - hidden_dev ** 2).reshape(B, T, U1, H)
    return _dh_judge(grad_enc, grad_pred, G_dev @ W, np.abs(G_dev) @ np.abs(W), np.abs(dt), 2 * U24, V, d)


def check_dhidden_x3(grad_enc, grad_pred, gp, d):
    """The same for k_dhidden_x3:  against the six products of the device's G planes `gp` = (hi, mid, lo) with W's pieces, times
    1 - tanh64(enc + pred)^2 evaluated as 4 w / (1 + w)^2, w = exp(-2 |x|) — the kernel recomputes the factor from enc and pred in
    that form, and 1 - tanh64^2 cancels in fp64 too (tests/x2_stage_cases.py dtanh64) —, per entry
        ((6 V + n + 4) U24 + D) sum |terms| + 2^-124 sum |products|
    D = YARD x the largest relative error of an fp32 numpy evaluation of the kernel's factor over the case's entries >= 2^-124 (below,
    w leaves fp32's normal range: the last term), as tests/x2_stage_cases.py check_dhidden."""
    V = d["W"].shape[0]
    dt = dtanh64(d)
    big = dt >= DT_FLOOR
    D = YARD * float((np.abs(dfac_f32(d).astype(np.float64) - dt)[big] / dt[big]).max())
    acc, mag = six(gp, split3(d["W"]))
    return _dh_judge(grad_enc, grad_pred, acc, mag, dt, D * dt + DT_FLOOR, 6 * V, d)


def check_dw(grad_W, grad_bias, refW, magW, refb, magb, n, yard_W, yard_b):
    """grad_W [V, H] / grad_bias [V] against the fp64 products `refW`, `refb` of the device's planes (and the sums of absolute values),
    per entry  (n + 8) U24 sum |terms|  — n terms, 8 for the split-K slabs' reduction.  That bound is loose for a sum over cells, so
    each array's largest error must also be <= YARD x that of a plain fp32 product / sum of the same planes + ulp_fp32(largest |ref|) / 2
    (`yard_W`: torch on the device in the GPU test; `yard_b`: chain_colsum — a library's pairwise column sum is no yardstick for a chain
    of accumulations; the half ulp: the store of the result, which a yardstick's error may happen to miss).  -> dict of the four worst ratios"""
    out = dict(W_bound=_judge("grad_W", np.abs(grad_W - refW), (n + 8) * U24 * magW),
               b_bound=_judge("grad_bias", np.abs(grad_bias - refb), (n + 8) * U24 * magb))
    out["W_yard"] = _judge("grad_W beside fp32", np.abs(grad_W - refW).max(), YARD * np.abs(yard_W - refW).max() + 0.5 * ulp_fp32(np.abs(refW).max()))
    out["b_yard"] = _judge("grad_bias beside fp32", np.abs(grad_bias - refb).max(), YARD * np.abs(yard_b - refb).max() + 0.5 * ulp_fp32(np.abs(refb).max()))
    return out


def check_dw_f32(grad_W, grad_bias, G_dev, hidden_dev, yard_W):
    """k_dw: grad_W = G^T . hidden, grad_bias = colsum(G) over the cells (G: rows outside the lattices as zeros; hidden: the device's fp32 rows of the cells)."""
    return check_dw(grad_W, grad_bias, G_dev.T @ hidden_dev, np.abs(G_dev).T @ np.abs(hidden_dev), G_dev.sum(0), np.abs(G_dev).sum(0),
                    G_dev.shape[0], yard_W, chain_colsum((G_dev,), 1))


def check_dw_x3(grad_W, grad_bias, gp, hp, yard_W):
    """k_dw_x3: grad_W = the six products of G's planes (transposed) with hidden's, grad_bias = colsum(hi + mid + lo) (the selector
    MFMA multiplies every plane by one), 6 x cells / 3 x cells terms."""
    refW, magW = six(tr(gp), hp)
    cells = gp[0].shape[0]
    return check_dw(grad_W, grad_bias, refW, magW, sum(gp).sum(0), sum(np.abs(x) for x in gp).sum(0), 6 * cells, yard_W, chain_colsum(gp, 16))
