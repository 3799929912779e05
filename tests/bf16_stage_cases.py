"""The bf16 route (rnnt_amd/csrc/bf16.hip) stage by stage: cases, an fp64 twin that keeps every intermediate, and one comparator per
stage.  Pure numpy: tests/test_bf16_stages_oracle.py proves the comparators on the CPU (a faithful fp32 emulation passes, seeded
faults do not), tests/test_bf16_stages_gpu.py feeds them the device's buffers.

Every comparator takes the operands the DEVICE produced upstream (its bf16 hidden plane, its fp16 logits, its bf16 G), so only the
error of the stage under test remains, and holds each element to a derived bar:
    U24 = 2^-24        fp32 unit roundoff: an fp32 dot product of n terms, in any order, is within n U24 sum |terms|
    ulp_fp16 / ulp_bf16  the spacing of the format at a value; a round-to-nearest store is within half of it.  (Relative to the value
                       half a bf16 ulp is 2^-9 only at the top of a binade and 2^-8 at its bottom: a bar of 2^-9 |x| fails a correctly
                       rounded store, tests/test_bf16_stages_oracle.py test_half_an_ulp_is_not_2_pow_minus_9_relative.)
    YARD = 4           the project's factor on a measured fp32 yardstick (tests/test_encoder_gpu.py, tests/test_featurizer_gpu.py)
No other tolerance appears below; every other number is computed from the reference or from an fp32 yardstick the caller measured."""
import numpy as np

from oracle import cpu_oracle
from tests.helpers import bf16_round, make_inputs

U24 = 2.0 ** -24
YARD = 4
LOG2E = 1.4426950408889634
LOG2E_F32 = np.float32(1.4426950408889634)  # common.hpp RNNT_LOG2E

# name: (B, T, U, H, V) and what the shape is for.  The smallest shapes that still take each path; at most 1 380 cells.
#   lens: (logit_lens, target_lens) instead of make_inputs' ragged ones;  logit_std: W scaled to that logit standard deviation
#   (tests/test_x2_gpu.py _scale_logits);  permuted: the GPU test hands enc over as a (B,H,T)->(B,T,H) view
CASES = {
    "one_cell": dict(shape=(1, 1, 0, 128, 128)),
    "tile_over_two_utterances": dict(shape=(2, 9, 4, 128, 128)),  # 90 cells: one forward tile, two utterances, ragged
    "partial_forward_pass": dict(shape=(3, 23, 19, 256, 384)),  # V = 256 + 128
    "generic_forward_h384": dict(shape=(2, 40, 12, 384, 256)),  # H not in {128, 256, 512, 1024}: k_joint_fwd_bf16
    "dhidden_rest_h640": dict(shape=(2, 13, 20, 640, 128)),  # second dHidden launch for the H % 512 rest
    "register_forward_h1024": dict(shape=(1, 37, 6, 1024, 256)),  # k_joint_fwd_bf16_ra<16>, two dHidden passes
    "config3_hv": dict(shape=(2, 20, 9, 512, 1024)),
    "u1_is_one": dict(shape=(2, 70, 0, 128, 128)),
    "dead_tiles": dict(shape=(5, 3, 40, 256, 128), lens=([3, 1, 2, 3, 1], [40, 0, 13, 40, 7])),
    "peaked_softmax": dict(shape=(2, 20, 9, 512, 1024), logit_std=8.0),
    "permuted_enc": dict(shape=(2, 21, 6, 128, 128), permuted=True),
}


def make_case(name):
    """-> (d, grad_scale): a make_inputs dict and the scale the engine is called with (1/B as the fp32 the C ABI takes)."""
    spec = CASES[name]
    B, T, U, H, V = spec["shape"]
    d = make_inputs(B, T, U, H, V, seed=sum(spec["shape"]))
    if "lens" in spec:
        d["logit_lens"] = np.array(spec["lens"][0], dtype=np.int32)
        d["target_lens"] = np.array(spec["lens"][1], dtype=np.int32)
    if "logit_std" in spec:
        lg = cpu_oracle.joint_fwd(d["enc"][:1, :8], d["pred"][:1, :8], d["W"], np.zeros_like(d["bias"]), dtype=np.float64)
        d["W"] = (d["W"] * (spec["logit_std"] / lg.std())).astype(np.float32)
        d["bias"] = np.zeros_like(d["bias"])
    return d, float(np.float32(1.0 / B))


def dims(d):
    B, T, H = d["enc"].shape
    return B, T, d["pred"].shape[1], H, d["W"].shape[0]


def inside(d):
    """[B, T, U1] bool: the cells of each utterance's lattice (t < logit_lens[b], u <= target_lens[b])."""
    B, T, U1, _, _ = dims(d)
    return (np.arange(T)[None, :, None] < d["logit_lens"][:, None, None]) & (np.arange(U1)[None, None, :] <= d["target_lens"][:, None, None])


def probe_cell(d):
    """(b, t, u, linear index) of a cell in the middle of utterance 0's lattice, near its diagonal: where the seeded faults strike
    (a cell the alignments pass through, so that its gradient is not negligible)."""
    _, T, U1, _, _ = dims(d)
    Tb, Ub = int(d["logit_lens"][0]), int(d["target_lens"][0])
    t = Tb // 2
    u = int(round(Ub * t / max(Tb - 1, 1)))
    return 0, t, u, t * U1 + u


def _ulp(x, mant_bits, emin):
    x = np.abs(np.asarray(x, dtype=np.float64))
    _, e = np.frexp(x)  # |x| = m 2^e, m in [0.5, 1)
    e = np.where(x == 0, emin, np.maximum(e - 1, emin))
    return np.ldexp(1.0, e - mant_bits)


def ulp_bf16(x):
    return _ulp(x, 7, -126)


def ulp_fp16(x):
    return _ulp(x, 10, -14)


def tanh64(d):
    return np.tanh(d["enc"][:, :, None, :].astype(np.float64) + d["pred"][:, None, :, :].astype(np.float64))


def fast_tanh_f32(d):
    """common.hpp fast_tanh on enc + pred, operation by operation in fp32: 1 - 2 / (1 + 2^(2 x log2 e))."""
    x = d["enc"][:, :, None, :] + d["pred"][:, None, :, :]
    with np.errstate(over="ignore"):
        e = np.exp2(x * (np.float32(2.0) * LOG2E_F32))
    return np.float32(1.0) - np.float32(2.0) * (np.float32(1.0) / (e + np.float32(1.0)))


def loss64(logits, d):
    """cpu_oracle.rnnt_loss in fp64 on [cells, V] logits; rows outside the lattices (never read by the route; on the device they
    may hold anything) are zeroed first.  -> (costs, d cost / d logits [cells, V], work)"""
    B, T, U1, _, V = dims(d)
    lg = np.where(inside(d).reshape(-1, 1), np.asarray(logits, dtype=np.float64), 0.0).reshape(B, T, U1, V)
    costs, G, work = cpu_oracle.rnnt_loss(lg, d["targets"], d["logit_lens"], d["target_lens"], blank=-1, dtype=np.float64, want_work=True)
    return costs, G.reshape(-1, V), work


def coef64(d, work, costs, gs):
    """common.hpp CellCoef in fp64 from the oracle's alpha, beta, denom ([B, T, U1]): G[v] = 2^(logit[v] log2e + c1) - [v = blank] sb -
    [v = y] se.  Outside the lattice: c1 = -inf, sb = se = 0, y = -1 (lattice.hip k_coef)."""
    B, T, U1, _, V = dims(d)
    al, be, de = work["alpha"], work["beta"], work["denom"]
    ins = inside(d)
    lg = work["logits"]
    c1 = np.full((B, T, U1), -np.inf)
    sb = np.zeros((B, T, U1))
    se = np.zeros((B, T, U1))
    y = np.full((B, T, U1), -1, dtype=np.int64)
    for b in range(B):
        Tb, Ub = int(d["logit_lens"][b]), int(d["target_lens"][b])
        ac = al[b] + costs[b]
        lpb = lg[b, :, :, V - 1] - de[b]
        c1[b][ins[b]] = ((ac + be[b] - de[b] + np.log(gs)) * LOG2E)[ins[b]]
        sb[b, :Tb - 1, :Ub + 1] = gs * np.exp(ac[:Tb - 1, :Ub + 1] + be[b, 1:Tb, :Ub + 1] + lpb[:Tb - 1, :Ub + 1])
        sb[b, Tb - 1, Ub] = gs * np.exp(ac[Tb - 1, Ub] + lpb[Tb - 1, Ub])
        if Ub > 0:
            yb = d["targets"][b, :Ub].astype(np.int64)
            lpe = np.take_along_axis(lg[b, :, :Ub, :], yb[None, :, None], axis=2)[:, :, 0] - de[b, :, :Ub]
            se[b, :Tb, :Ub] = gs * np.exp(ac[:Tb, :Ub] + be[b, :Tb, 1:Ub + 1] + lpe[:Tb])
            y[b, :Tb, :Ub] = yb[None, :]
    return dict(c1=c1.reshape(-1), sb=sb.reshape(-1), se=se.reshape(-1), y=y.reshape(-1))


def g_from_coef(logits, coef, V, real=np.float64, log2e=LOG2E):
    """G [cells, V] from logits and coefficients, in `real` arithmetic (fp32: the kernels' formula, one fma and one exp2 per entry).
    `log2e`: the constant of the fp64 form (tests/f32_stage_cases.py passes the kernels' fp32 one, to refer to their exponent)."""
    lg = np.where(np.isfinite(coef["c1"])[:, None], logits, 0.0).astype(real)
    c1 = coef["c1"].astype(real)[:, None]
    if real == np.float32:
        x = (lg.astype(np.float64) * float(LOG2E_F32) + c1.astype(np.float64)).astype(np.float32)  # fma: one rounding
    else:
        x = lg * log2e + c1
    G = np.exp2(x).astype(real)
    rows = np.arange(G.shape[0])
    G[rows, V - 1] -= coef["sb"].astype(real)
    lab = coef["y"] >= 0
    G[rows[lab], coef["y"][lab]] -= coef["se"].astype(real)[lab]
    return G


def twin(d, gs):
    """The route in fp64 with its rounding points (tests/helpers.py oracle_fused_bf16: bf16 hidden and W, fp16 logits, bf16 G), every
    intermediate kept: hidden [cells, H], logits [cells, V], coef, costs, G64 (unrounded) and G [cells, V], the four gradients."""
    B, T, U1, H, V = dims(d)
    hidden = bf16_round(tanh64(d).astype(np.float32)).astype(np.float64).reshape(-1, H)
    Wb = bf16_round(d["W"]).astype(np.float64)
    logits = (hidden @ Wb.T + d["bias"].astype(np.float64)).astype(np.float32).astype(np.float16).astype(np.float64)
    costs, G, work = loss64(logits, d)
    work["logits"] = logits.reshape(B, T, U1, V)
    G64 = G * gs
    Gb = bf16_round(G64.astype(np.float32)).astype(np.float64)
    dpre = (Gb @ Wb).reshape(B, T, U1, H) * (1.0 - hidden.reshape(B, T, U1, H) ** 2)
    return dict(hidden=hidden, logits=logits, coef=coef64(d, work, costs, gs), costs=costs, G64=G64, G=Gb, work=work,
                grad_enc=dpre.sum(2), grad_pred=dpre.sum(1), grad_W=Gb.T @ hidden, grad_bias=Gb.sum(0))


# ---- comparators: pure functions of numpy arrays; each asserts error <= bar per element and returns the worst error / bar
def _judge(what, err, bar):
    err, bar = np.asarray(err, dtype=np.float64), np.asarray(bar, dtype=np.float64)
    assert np.isfinite(err).all(), f"{what}: non-finite values"
    if err.size == 0:
        return 0.0
    ratio = np.where(err > 0, err / np.where(bar > 0, bar, 1.0), 0.0)
    ratio = np.where((err > 0) & (bar <= 0), np.inf, ratio)
    i = int(np.argmax(ratio))
    worst = float(ratio.reshape(-1)[i])
    assert worst <= 1.0, f"{what}: error {err.reshape(-1)[i]:.3e} is {worst:.3g} x its bar {bar.reshape(-1)[i]:.3e} at {np.unravel_index(i, err.shape)}"
    return worst


def check_hidden(dev, d):
    """hidden [cells, H] = bf16(tanh(enc + pred)):  |dev - tanh64| <= ulp_bf16(tanh64) / 2 + A on every cell of a lattice, where A allows
    for the kernel's fp32 formula 1 - 2 / (1 + 2^(2 x log2 e)) (common.hpp fast_tanh): YARD x the largest |fp32 numpy evaluation of that
    formula - tanh64| over the case's inputs (the factor covers the hardware's approximate exp2 and rcp).  Every other row the
    backward GEMMs read (they multiply it by exact zeros) must be finite."""
    H = dev.shape[1]
    ref = tanh64(d)
    A = YARD * float(np.abs(fast_tanh_f32(d).astype(np.float64) - ref).max())
    ref = ref.reshape(-1, H)
    ins = inside(d).reshape(-1)
    assert np.isfinite(dev[~ins]).all(), "hidden: non-finite row outside the lattices"
    return _judge("hidden", np.abs(dev[ins] - ref[ins]), 0.5 * ulp_bf16(ref[ins]) + A)


def check_logits(dev, hidden_dev, d):
    """logits [cells, V] = f16(hidden . bf16(W)^T + bias), fp32 accumulation:  against ref64 = hidden_dev @ bf16(W)^T + bias (the device's
    hidden plane is exact in bf16),  |dev - ref64| <= ulp_fp16(max(|dev|, |ref64|)) / 2 + (H + 2) U24 (sum_k |h_k w_k| + |bias|): the
    store's rounding plus the bound on an fp32 dot product of H terms (and the bias add) in any summation order.  Lattice cells."""
    H = hidden_dev.shape[1]
    ins = inside(d).reshape(-1)
    Wb = bf16_round(d["W"]).astype(np.float64)
    bias = d["bias"].astype(np.float64)
    h = hidden_dev[ins]
    ref = h @ Wb.T + bias
    mag = np.abs(h) @ np.abs(Wb).T + np.abs(bias)
    x = dev[ins]
    assert np.isfinite(x).all(), "logits: non-finite values"
    return _judge("logits", np.abs(x - ref), 0.5 * ulp_fp16(np.maximum(np.abs(x), np.abs(ref))) + (H + 2) * U24 * mag)


def check_g(dev, logits_dev, d, gs, yard):
    """G [cells, V] = bf16(grad_scale d cost / d logits) from the device's fp16 logits (softmax statistics of the forward epilogue,
    lattice sweep, k_coef and the G production in one comparison):  against G64 = cpu_oracle.rnnt_loss(logits_dev)[1] grad_scale in fp64,
    |dev - G64| <= ulp_bf16(G64) / 2 + E,  E = YARD x the largest |yard - G64| of an fp32 evaluation of the same gradient on the same logits
    (`yard`: on the GPU the fp32 route's standalone rnnt_amd.rnnt_loss, whose lattice and coefficient kernels the route shares).  Cells
    outside the lattices hold exactly 0, as values.  -> (worst ratio, the fp64 costs)"""
    ins = inside(d).reshape(-1)
    costs, G, _ = loss64(logits_dev, d)
    G64 = G * gs
    assert (dev[~ins] == 0).all(), "G: a cell outside the lattices is not zero"
    assert np.isfinite(yard[ins]).all(), "G: the fp32 yardstick is not finite"
    E = YARD * float(np.abs(yard[ins] - G64[ins]).max())
    return _judge("G", np.abs(dev[ins] - G64[ins]), 0.5 * ulp_bf16(G64[ins]) + E), costs


def check_dhidden(grad_enc, grad_pred, G_dev, hidden_dev, d):
    """grad_enc [B, T, H] / grad_pred [B, U1, H] = ((G . bf16(W)) (1 - hidden^2)) summed over u / over t:  against the same expression in
    fp64 on the device's G and hidden planes, per entry  (V + n + 4) U24 sum |terms|  (n = U1 / T rows summed; V terms per dot product,
    n per sum, 4 for 1 - h^2, the product and the final stores).  Rows with t >= logit_lens[b] / u > target_lens[b]: exactly 0.
    -> (worst ratio of grad_enc, of grad_pred)"""
    B, T, U1, H, V = dims(d)
    Wb = bf16_round(d["W"]).astype(np.float64)
    dt = (1.0 - hidden_dev ** 2).reshape(B, T, U1, H)
    dpre = (G_dev @ Wb).reshape(B, T, U1, H) * dt
    mag = (np.abs(G_dev) @ np.abs(Wb)).reshape(B, T, U1, H) * np.abs(dt)
    dead_t = np.arange(T)[None, :] >= d["logit_lens"][:, None]
    dead_u = np.arange(U1)[None, :] > d["target_lens"][:, None]
    assert (grad_enc[dead_t] == 0).all(), "grad_enc: a row past its utterance's length is not zero"
    assert (grad_pred[dead_u] == 0).all(), "grad_pred: a row past its utterance's labels is not zero"
    re = _judge("grad_enc", np.abs(grad_enc - dpre.sum(2)), (V + U1 + 4) * U24 * mag.sum(2))
    rp = _judge("grad_pred", np.abs(grad_pred - dpre.sum(1)), (V + T + 4) * U24 * mag.sum(1))
    return re, rp


def check_dw(grad_W, grad_bias, G_dev, hidden_dev, yard_W, yard_b):
    """grad_W [V, H] = G^T . hidden, grad_bias [V] = colsum(G), fp32 accumulation over the cells:  against the fp64 products of the device's
    planes, per entry  (cells + 8) U24 sum_c |g| |h|  (8: the split-K slabs' reduction).  That bound is loose for a sum over cells, so the
    largest error of each array must also be <= YARD x the largest error of a plain fp32 evaluation of the same product / sum on the
    same planes (`yard_W`, `yard_b`: torch on the device in the GPU test).  -> dict of the four worst ratios"""
    cells = G_dev.shape[0]
    refW, refb = G_dev.T @ hidden_dev, G_dev.sum(0)
    magW, magb = np.abs(G_dev).T @ np.abs(hidden_dev), np.abs(G_dev).sum(0)
    out = dict(W_bound=_judge("grad_W", np.abs(grad_W - refW), (cells + 8) * U24 * magW),
               b_bound=_judge("grad_bias", np.abs(grad_bias - refb), (cells + 8) * U24 * magb))
    out["W_yard"] = _judge("grad_W beside fp32", np.abs(grad_W - refW).max(), YARD * np.abs(yard_W - refW).max())
    out["b_yard"] = _judge("grad_bias beside fp32", np.abs(grad_bias - refb).max(), YARD * np.abs(yard_b - refb).max())
    return out
