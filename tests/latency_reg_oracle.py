"""Float64 numpy oracle of the transducer loss with FastEmit and the delay penalty, independent of the engine.

For utterance b (T_b = logit_lens[b] clamped into [1, T], U_b = target_lens[b] clamped into [0, U1-1], as the kernels clamp):
  lp_emit'(t,u) = lp_emit(t,u) + delta ((T_b - 1) / 2 - t)          for u < U_b (k2's delay_penalty)
  cost_b        = -log P'_b, alpha / beta on lp_emit'               (lambda does not change it)
  d cost_b / d z[t,u,k] = the plain coefficient formula on the penalised lattice
                          + lambda E(t,u) (p_k - [k = y_{u+1}]),    E = exp(alpha + lp_emit' + beta(t,u+1) - log P'_b)
The fused form goes through oracle/cpu_oracle (joint forward and joint backward in C, float64).
"""
import numpy as np

from oracle import cpu_oracle
from tests.helpers import bf16_round


def log_softmax(x):
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def clamp_lengths(logit_lens, target_lens, T, U1):
    return (np.clip(np.asarray(logit_lens, dtype=np.int64), 1, T),
            np.clip(np.asarray(target_lens, dtype=np.int64), 0, U1 - 1))


def lattice_logprobs(lp, y, Tb, Ub, blank, delay_penalty):
    """(lp_blank [Tb, Ub+1], lp_emit' [Tb, Ub]) of one utterance from its log-softmax lp[t, u, v]."""
    lpb = lp[:Tb, :Ub + 1, blank]
    lpe = lp[:Tb, np.arange(Ub), np.asarray(y[:Ub], dtype=np.int64)]
    return lpb, lpe + delay_penalty * ((Tb - 1) / 2.0 - np.arange(Tb))[:, None]


def alpha_beta(lpb, lpe):
    Tb, Ub = lpb.shape[0], lpb.shape[1] - 1
    alpha = np.full((Tb, Ub + 1), -np.inf)
    beta = np.full((Tb, Ub + 1), -np.inf)
    for t in range(Tb):
        for u in range(Ub + 1):
            if t == 0 and u == 0:
                alpha[0, 0] = 0.0
                continue
            a = alpha[t - 1, u] + lpb[t - 1, u] if t > 0 else -np.inf
            e = alpha[t, u - 1] + lpe[t, u - 1] if u > 0 else -np.inf
            alpha[t, u] = np.logaddexp(a, e)
    for t in range(Tb - 1, -1, -1):
        for u in range(Ub, -1, -1):
            if t == Tb - 1 and u == Ub:
                beta[t, u] = lpb[t, u]
                continue
            a = beta[t + 1, u] + lpb[t, u] if t < Tb - 1 else -np.inf
            e = beta[t, u + 1] + lpe[t, u] if u < Ub else -np.inf
            beta[t, u] = np.logaddexp(a, e)
    return alpha, beta


def loss_and_grad(logits, targets, logit_lens, target_lens, blank=-1, fastemit_lambda=0.0, delay_penalty=0.0,
                  clamp=-1.0, want_grad=True):
    """Per-utterance costs [B] and d cost_b / d logits [B,T,U1,V] (unscaled; zero outside each lattice; `clamp` > 0 clips
    the regularised gradient elementwise, as rnnt_loss's clamp does)."""
    logits = np.asarray(logits, dtype=np.float64)
    B, T, U1, V = logits.shape
    blank = blank + V if blank < 0 else blank
    targets = np.asarray(targets).reshape(B, U1 - 1)
    Tbs, Ubs = clamp_lengths(logit_lens, target_lens, T, U1)
    lam = float(fastemit_lambda)
    costs = np.zeros(B)
    grad = np.zeros_like(logits) if want_grad else None
    for b in range(B):
        Tb, Ub = int(Tbs[b]), int(Ubs[b])
        y = targets[b, :Ub].astype(np.int64)
        lp = log_softmax(logits[b, :Tb, :Ub + 1])
        lpb, lpe = lattice_logprobs(lp, y, Tb, Ub, blank, delay_penalty)
        alpha, beta = alpha_beta(lpb, lpe)
        logp = beta[0, 0]
        costs[b] = -logp
        if not want_grad:
            continue
        p = np.exp(lp)
        g = np.exp(alpha + beta - logp)[..., None] * p
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
    return costs, grad


def fused(d, fastemit_lambda=0.0, delay_penalty=0.0, grad_scale=None, blank=-1):
    """joint + regularised loss, forward and backward, on a tests.helpers.make_inputs dict: dict(loss, costs, grad_enc,
    grad_pred, grad_W, grad_bias) of grad_scale * sum_b cost_b (grad_scale = 1/B: reduction "mean"), blank = V - 1 by default."""
    logits = cpu_oracle.joint_fwd(d["enc"], d["pred"], d["W"], d["bias"])
    scale = 1.0 / logits.shape[0] if grad_scale is None else grad_scale
    costs, G = loss_and_grad(logits, d["targets"], d["logit_lens"], d["target_lens"], blank, fastemit_lambda, delay_penalty)
    ge, gp, gW, gb = cpu_oracle.joint_bwd(d["enc"], d["pred"], d["W"], G * scale)
    return dict(loss=costs.sum() * scale, costs=costs, grad_enc=ge, grad_pred=gp, grad_W=gW, grad_bias=gb)


def fused_bf16(d, fastemit_lambda=0.0, delay_penalty=0.0, blank=-1):
    """`fused` with the bf16 route's rounding points (tests.helpers.oracle_fused_bf16): bf16 hidden and W, fp16 logits,
    bf16 G of the mean."""
    enc, pred, W, bias = d["enc"], d["pred"], d["W"], d["bias"]
    B, T, H = enc.shape
    U1, V = pred.shape[1], W.shape[0]
    hidden = bf16_round(np.tanh(enc[:, :, None, :].astype(np.float64) +
                                pred[:, None, :, :].astype(np.float64)).astype(np.float32)).astype(np.float64)
    Wb = bf16_round(W).astype(np.float64)
    logits = (hidden.reshape(-1, H) @ Wb.T + bias.astype(np.float64)).astype(np.float32)
    logits = logits.astype(np.float16).astype(np.float32).reshape(B, T, U1, V)
    costs, G = loss_and_grad(logits, d["targets"], d["logit_lens"], d["target_lens"], blank, fastemit_lambda, delay_penalty)
    Gb = bf16_round((G / B).astype(np.float32)).astype(np.float64).reshape(-1, V)
    dpre = (Gb @ Wb).reshape(B, T, U1, H) * (1.0 - hidden * hidden)
    return dict(loss=costs.mean(), costs=costs, grad_enc=dpre.sum(2), grad_pred=dpre.sum(1),
                grad_W=Gb.T @ hidden.reshape(-1, H), grad_bias=Gb.sum(0))
