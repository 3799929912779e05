"""Float64 numpy oracle of the alignment-restricted transducer loss, independent of the engine.

TEST INFRASTRUCTURE ONLY.  Built on tests/latency_reg_oracle.py (log_softmax, lattice_logprobs, alpha_beta): for utterance b
with reference frames f[u], u < U_b, the label arc (t,u) -> (t,u+1) exists only for f[u] - left <= t <= f[u] + right; the others
get lp_emit = -inf before the recurrences.  Blank arcs are unrestricted; FastEmit and the delay penalty act on the arcs that
remain, with their definitions of latency_reg_oracle.
  cost_b = -log sum over the surviving paths; d cost_b / d logits: the plain formulas on the masked lattice;
  a cell with alpha = -inf or beta = -inf contributes exactly zero;
  no surviving path: cost_b = +inf and a zero gradient, stated explicitly (the formulas give inf - inf = NaN there).
"""
import numpy as np

from oracle import cpu_oracle
from tests import latency_reg_oracle as lro
from tests.helpers import bf16_round


def window_mask(frames, Tb, Ub, left, right):
    """bool [Tb, Ub]: True where the label arc out of (t,u) survives."""
    f = np.asarray(frames[:Ub], dtype=np.int64)[None, :]
    t = np.arange(Tb, dtype=np.int64)[:, None]
    return (t >= f - int(left)) & (t <= f + int(right))


def alpha_beta_diag(lpb, lpe):
    """latency_reg_oracle.alpha_beta, one anti-diagonal at a time (the same sums in the same order per cell): for lattices
    where the double loop takes too long."""
    Tb, Ub = lpb.shape[0], lpb.shape[1] - 1
    NINF = -np.inf
    alpha = np.full((Tb, Ub + 1), NINF)
    beta = np.full((Tb, Ub + 1), NINF)
    lpe_pad = np.concatenate([lpe, np.full((Tb, 1), NINF)], axis=1)  # no label arc out of column Ub
    alpha[0, 0] = 0.0
    beta[Tb - 1, Ub] = lpb[Tb - 1, Ub]
    for d in range(1, Tb + Ub):
        u = np.arange(max(0, d - Tb + 1), min(d, Ub) + 1)
        t = d - u
        a = np.where(t > 0, alpha[np.maximum(t - 1, 0), u] + lpb[np.maximum(t - 1, 0), u], NINF)
        e = np.where(u > 0, alpha[t, np.maximum(u - 1, 0)] + lpe_pad[t, np.maximum(u - 1, 0)], NINF)
        alpha[t, u] = np.logaddexp(a, e)
    for d in range(Tb + Ub - 2, -1, -1):
        u = np.arange(max(0, d - Tb + 1), min(d, Ub) + 1)
        t = d - u
        a = np.where(t < Tb - 1, beta[np.minimum(t + 1, Tb - 1), u] + lpb[t, u], NINF)
        e = np.where(u < Ub, beta[t, np.minimum(u + 1, Ub)] + lpe_pad[t, u], NINF)
        beta[t, u] = np.logaddexp(a, e)
    return alpha, beta


def loss_and_grad(logits, targets, logit_lens, target_lens, frames, left, right, blank=-1, fastemit_lambda=0.0,
                  delay_penalty=0.0, clamp=-1.0, want_grad=True, want_occupancy=False):
    """Per-utterance costs [B] and d cost_b / d logits [B,T,U1,V] (unscaled; zero outside each lattice and in every cell no
    surviving path crosses; `clamp` > 0 clips elementwise).  `want_occupancy`: also gamma [B,T,U1] = exp(alpha + beta - log P),
    the probability that a surviving path crosses the cell (0 outside the lattice and for an infeasible utterance)."""
    logits = np.asarray(logits, dtype=np.float64)
    B, T, U1, V = logits.shape
    blank = blank + V if blank < 0 else blank
    targets = np.asarray(targets).reshape(B, U1 - 1)
    frames = np.asarray(frames).reshape(B, U1 - 1)
    Tbs, Ubs = lro.clamp_lengths(logit_lens, target_lens, T, U1)
    lam = float(fastemit_lambda)
    costs = np.zeros(B)
    grad = np.zeros_like(logits) if want_grad else None
    occ = np.zeros((B, T, U1))
    for b in range(B):
        Tb, Ub = int(Tbs[b]), int(Ubs[b])
        y = targets[b, :Ub].astype(np.int64)
        lp = lro.log_softmax(logits[b, :Tb, :Ub + 1])
        lpb, lpe = lro.lattice_logprobs(lp, y, Tb, Ub, blank, delay_penalty)
        lpe = np.where(window_mask(frames[b], Tb, Ub, left, right), lpe, -np.inf)
        with np.errstate(invalid="ignore"):
            alpha, beta = (lro.alpha_beta if Tb * (Ub + 1) <= 1 << 14 else alpha_beta_diag)(lpb, lpe)
        logp = beta[0, 0]
        costs[b] = -logp
        if logp == -np.inf:  # infeasible: +inf, and nothing flows
            costs[b] = np.inf
            continue
        gamma = np.exp(alpha + beta - logp)
        occ[b, :Tb, :Ub + 1] = gamma
        if not want_grad:
            continue
        p = np.exp(lp)
        g = gamma[..., None] * p
        nxt = np.full((Tb, Ub + 1), -np.inf)  # beta after the blank arc; 0 for the final blank
        nxt[:-1] = beta[1:]
        nxt[-1, Ub] = 0.0
        g[..., blank] -= np.exp(alpha + lpb + nxt - logp)
        if Ub:
            E = np.exp(alpha[:, :Ub] + lpe + beta[:, 1:] - logp)
            g[:, :Ub, :] += lam * E[..., None] * p[:, :Ub, :]
            g[:, np.arange(Ub), y] -= (1.0 + lam) * E
        if clamp > 0:
            g = np.clip(g, -clamp, clamp)
        grad[b, :Tb, :Ub + 1] = g
    return (costs, grad, occ) if want_occupancy else (costs, grad)


def _joint_fwd_numpy(enc, pred, W, bias):
    hidden = np.tanh(enc[:, :, None, :].astype(np.float64) + pred[:, None, :, :].astype(np.float64))
    return hidden, hidden @ W.astype(np.float64).T + bias.astype(np.float64)


def fused(d, frames, left, right, fastemit_lambda=0.0, delay_penalty=0.0, grad_scale=None, blank=-1, numpy_joint=False,
          want_occupancy=False):
    """joint + restricted loss, forward and backward, on a tests.helpers.make_inputs dict: dict(loss, costs, grad_enc,
    grad_pred, grad_W, grad_bias[, occupancy]) of grad_scale * sum_b cost_b (default 1/B: reduction "mean").  An infeasible
    utterance contributes +inf to `loss` and nothing to the gradients.  `numpy_joint`: the joint's two GEMMs through numpy's
    matmul instead of oracle/cpu_oracle's C loops (float64 either way; for lattices of 1e5 cells and more)."""
    if numpy_joint:
        hidden, logits = _joint_fwd_numpy(d["enc"], d["pred"], d["W"], d["bias"])
    else:
        logits = cpu_oracle.joint_fwd(d["enc"], d["pred"], d["W"], d["bias"])
    B, T, U1, V = logits.shape
    scale = 1.0 / B if grad_scale is None else grad_scale
    costs, G, occ = loss_and_grad(logits, d["targets"], d["logit_lens"], d["target_lens"], frames, left, right, blank,
                                  fastemit_lambda, delay_penalty, want_occupancy=True)
    if numpy_joint:
        Gs = (G * scale).reshape(-1, V)
        dpre = (Gs @ d["W"].astype(np.float64)).reshape(hidden.shape) * (1.0 - hidden * hidden)
        ge, gp, gW, gb = dpre.sum(2), dpre.sum(1), Gs.T @ hidden.reshape(-1, hidden.shape[-1]), Gs.sum(0)
    else:
        ge, gp, gW, gb = cpu_oracle.joint_bwd(d["enc"], d["pred"], d["W"], G * scale)
    out = dict(loss=costs.sum() * scale, costs=costs, grad_enc=ge, grad_pred=gp, grad_W=gW, grad_bias=gb)
    if want_occupancy:
        out["occupancy"] = occ
    return out


def fused_bf16(d, frames, left, right, fastemit_lambda=0.0, delay_penalty=0.0, blank=-1):
    """`fused` with the bf16 route's rounding points (latency_reg_oracle.fused_bf16): bf16 hidden and W, fp16 logits, bf16 G of
    the mean."""
    enc, pred, W, bias = d["enc"], d["pred"], d["W"], d["bias"]
    B, T, H = enc.shape
    U1, V = pred.shape[1], W.shape[0]
    hidden = bf16_round(np.tanh(enc[:, :, None, :].astype(np.float64) +
                                pred[:, None, :, :].astype(np.float64)).astype(np.float32)).astype(np.float64)
    Wb = bf16_round(W).astype(np.float64)
    logits = (hidden.reshape(-1, H) @ Wb.T + bias.astype(np.float64)).astype(np.float32)
    logits = logits.astype(np.float16).astype(np.float32).reshape(B, T, U1, V)
    costs, G = loss_and_grad(logits, d["targets"], d["logit_lens"], d["target_lens"], frames, left, right, blank,
                             fastemit_lambda, delay_penalty)
    Gb = bf16_round((G / B).astype(np.float32)).astype(np.float64).reshape(-1, V)
    dpre = (Gb @ Wb).reshape(B, T, U1, H) * (1.0 - hidden * hidden)
    return dict(loss=costs.mean(), costs=costs, grad_enc=dpre.sum(2), grad_pred=dpre.sum(1),
                grad_W=Gb.T @ hidden.reshape(-1, H), grad_bias=Gb.sum(0))


def viterbi_frames(d, blank=-1, logits=None):
    """frames [B,U] int32 (-1 past target_lens) of the float64 Viterbi path (tests/align_oracle.py) on the joint's logits."""
    from tests import align_oracle
    if logits is None:
        logits = cpu_oracle.joint_fwd(d["enc"], d["pred"], d["W"], d["bias"])
    V = logits.shape[-1]
    scores, frames, _ = align_oracle.viterbi_logits(logits, d["targets"], d["logit_lens"], d["target_lens"],
                                                    blank + V if blank < 0 else blank)
    return scores, frames
