"""float64 numpy oracle of the forced alignment (include/rnnt_engine.h rnnt_engine_align).

TEST INFRASTRUCTURE ONLY.  The best path through the transducer lattice of one utterance: label arc (t,u) -> (t,u+1) adds
lp_emit[t,u], blank arc (t,u) -> (t+1,u) adds lp_blank[t,u], the final blank out of (T_b-1, U_b) ends the path.  Same tie rule
as the engine (exactly equal predecessors: the blank one, (t-1,u)) and the same NaN rule (a NaN log-prob on a cell the
recurrence reads: NaN score, every frame -1).  `margin` is the smallest |blank candidate - label candidate| over the
decisions on the returned path where both predecessors exist: where it exceeds the device's rounding, the device's path
must be the oracle's."""
import numpy as np


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def lattice_logprobs(logits, targets, blank):
    """logits [T,U1,V] (one utterance) -> (lp_blank [T,U1], lp_emit [T,U1]) in float64; lp_emit[:, U1-1] = 0 (no label)."""
    lp = log_softmax(logits)
    T, U1, _ = lp.shape
    lpb = lp[:, :, blank].copy()
    lpe = np.zeros((T, U1))
    for u in range(U1 - 1):
        lpe[:, u] = lp[:, u, int(targets[u])]
    return lpb, lpe


def _nan_read(lpb, lpe, Tb, Ub):
    return bool(np.isnan(lpb[:Tb - 1, :Ub + 1]).any() or np.isnan(lpb[Tb - 1, Ub]) or np.isnan(lpe[:Tb, :Ub]).any())


def viterbi(lpb, lpe, Tb, Ub):
    """-> (score, frames int array [Ub], margin).  lpb / lpe [>= Tb, >= Ub+1] float64."""
    lpb = np.asarray(lpb, dtype=np.float64)
    lpe = np.asarray(lpe, dtype=np.float64)
    if _nan_read(lpb, lpe, Tb, Ub):
        return float("nan"), np.full(Ub, -1, dtype=np.int32), float("inf")
    NINF = -np.inf
    val = np.full((Tb, Ub + 1), NINF)
    emit = np.zeros((Tb, Ub + 1), dtype=bool)
    gap = np.full((Tb, Ub + 1), np.inf)
    val[0, 0] = 0.0
    for d in range(1, Tb + Ub):
        u = np.arange(max(0, d - Tb + 1), min(d, Ub) + 1)
        t = d - u
        a = np.where(t > 0, val[np.maximum(t - 1, 0), u] + lpb[np.maximum(t - 1, 0), u], NINF)
        e = np.where(u > 0, val[t, np.maximum(u - 1, 0)] + lpe[t, np.maximum(u - 1, 0)], NINF)
        em = (u > 0) & ((t == 0) | (e > a))
        val[t, u] = np.where(em, e, a)
        emit[t, u] = em
        both = (t > 0) & (u > 0)
        with np.errstate(invalid="ignore"):
            gap[t, u] = np.where(both, np.abs(a - e), np.inf)
    score = val[Tb - 1, Ub] + lpb[Tb - 1, Ub]
    frames = np.full(Ub, -1, dtype=np.int32)
    margin = np.inf
    t, u = Tb - 1, Ub
    while t + u > 0:
        if t > 0 and u > 0 and not np.isnan(gap[t, u]):
            margin = min(margin, gap[t, u])
        if emit[t, u]:
            u -= 1
            frames[u] = t
        else:
            t -= 1
    return float(score), frames, float(margin)


def viterbi_batch(lpb, lpe, logit_lens, target_lens):
    """lpb / lpe [B,T,U1] -> (scores [B] float64, frames [B,U1-1] int32 (-1 padded), margins [B])."""
    B, T, U1 = lpb.shape
    scores = np.zeros(B)
    frames = np.full((B, U1 - 1), -1, dtype=np.int32)
    margins = np.zeros(B)
    for b in range(B):
        Tb, Ub = int(logit_lens[b]), int(target_lens[b])
        s, f, m = viterbi(lpb[b], lpe[b], Tb, Ub)
        scores[b], margins[b] = s, m
        if not np.isnan(s):
            frames[b, :Ub] = f
    return scores, frames, margins


def viterbi_logits(logits, targets, logit_lens, target_lens, blank):
    """logits [B,T,U1,V] -> viterbi_batch of their log-softmax (float64)."""
    logits = np.asarray(logits, dtype=np.float64)
    B, T, U1, V = logits.shape
    lpb = np.zeros((B, T, U1))
    lpe = np.zeros((B, T, U1))
    for b in range(B):
        lpb[b], lpe[b] = lattice_logprobs(logits[b], targets[b], blank)
    return viterbi_batch(lpb, lpe, logit_lens, target_lens)


def rescore(lpb, lpe, frames, Tb, Ub):
    """Log-probability of the path that emits label u at frame frames[u] (non-decreasing, in [0, Tb-1]); float64."""
    f = np.asarray(frames[:Ub], dtype=np.int64)
    assert len(f) == Ub and (Ub == 0 or (f.min() >= 0 and f.max() <= Tb - 1 and (np.diff(f) >= 0).all())), frames
    s = 0.0
    u = 0
    for t in range(Tb):
        while u < Ub and f[u] == t:
            s += float(lpe[t, u])
            u += 1
        s += float(lpb[t, u])
    return s
