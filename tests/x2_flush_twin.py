"""fp64 twin of the f16x2 route's flush rule (rnnt_amd/csrc/lattice.hip k_coef, FLUSH, x2.hip "flush rule").

The device gives a lattice cell the coefficients of a cell outside the lattice when
    s1 = log2(grad_scale * gamma) < -26 - log2 g_scale     and     sb + se < 2^-26 / g_scale
(gamma = exp(alpha + beta - log P), sb / se the blank / label arc occupancies times grad_scale, g_scale the power of two
engine.hip derives from grad_scale).  Here the same quantities come from the fp64 oracle's logits, alpha and beta.
Shared by the CPU test of the rule and the GPU tests (which check the shapes they pick with it)."""
import math

import numpy as np

from oracle import cpu_oracle

# (B, T, U, H, V, seed, ragged, grad_scale) of the GPU A/B cases: U + 1 not a multiple of 16, a ragged batch, H = 1024
# (second dHidden pass), H = 640 (cfg4's kernels: k_dhidden_x2r, k_dw_x2m); four different g_scale
CASES = {
    "u1_63": (2, 360, 62, 128, 256, 11, False, 0.5),
    "ragged": (3, 360, 62, 128, 128, 12, True, 1.0 / 3.0),
    "h1024": (1, 360, 62, 1024, 128, 13, False, 1.0),
    "h640": (1, 360, 62, 640, 512, 14, False, 0.125),
}


def g_scale_log2(grad_scale):
    """k with g_scale = 2^k (engine.hip run_fused: |G| <= grad_scale <= 2^e -> 2^(13 - e))."""
    _, e = math.frexp(np.float32(grad_scale))
    return max(-100, min(100, 13 - e))


def twin(d, grad_scale, blank=None):
    """Per-cell fp64 quantities of the rule for inputs `d` (tests.helpers.make_inputs).  Returns a dict:
    inside [B,T,U1] (t < T_b, u <= U_b), s1, sbse (sb + se), flush (the predicate), gamma_small (g_scale grad_scale gamma <
    2^-25: the set the device's flags must lie in), logp [B,T,U1,V] (log-softmax), costs, k."""
    logits = cpu_oracle.joint_fwd(d["enc"], d["pred"], d["W"], d["bias"], dtype=np.float64)
    B, T, U1, V = logits.shape
    blank = V - 1 if blank is None else blank
    costs, _, work = cpu_oracle.rnnt_loss(logits, d["targets"], d["logit_lens"], d["target_lens"], blank=blank,
                                          dtype=np.float64, want_grad=False, want_work=True)
    m = logits.max(axis=-1, keepdims=True)
    logp = logits - (m + np.log(np.exp(logits - m).sum(axis=-1, keepdims=True)))
    alpha, beta = work["alpha"], work["beta"]
    k = g_scale_log2(grad_scale)
    lim = -26.0 - k
    inside = np.zeros((B, T, U1), dtype=bool)
    s1 = np.full((B, T, U1), np.nan)
    sb = np.zeros((B, T, U1))
    se = np.zeros((B, T, U1))
    for b in range(B):
        Tb, Ub = int(d["logit_lens"][b]), int(d["target_lens"][b])
        inside[b, :Tb, :Ub + 1] = True
        a = alpha[b, :Tb, :Ub + 1] + costs[b]
        be = beta[b, :Tb, :Ub + 1]
        s1[b, :Tb, :Ub + 1] = (a + be + math.log(grad_scale)) / math.log(2.0)
        lpb = logp[b, :Tb, :Ub + 1, blank]
        sbb = np.zeros_like(a)
        sbb[:-1] = grad_scale * np.exp(a[:-1] + be[1:] + lpb[:-1])
        sbb[-1, Ub] = grad_scale * np.exp(a[-1, Ub] + lpb[-1, Ub])
        sb[b, :Tb, :Ub + 1] = sbb
        if Ub > 0:
            y = d["targets"][b, :Ub].astype(np.int64)
            lpe = np.take_along_axis(logp[b, :Tb, :Ub], np.broadcast_to(y[None, :, None], (Tb, Ub, 1)), axis=-1)[..., 0]
            se[b, :Tb, :Ub] = grad_scale * np.exp(a[:, :Ub] + be[:, 1:] + lpe)
    with np.errstate(invalid="ignore"):
        flush = inside & (s1 < lim) & (sb + se < 2.0 ** lim)  # ordered comparisons: False for NaN
        gamma_small = inside & (s1 + k < -25.0)
    return dict(inside=inside, s1=s1, sbse=sb + se, sb=sb, se=se, flush=flush, gamma_small=gamma_small, logp=logp,
                costs=costs, alpha=alpha, beta=beta, k=k)


def live_fractions(tw):
    """What the device counts (rnnt_engine_ws_layout::x2_live), from the twin's flags: live = inside and not flushed.
    Returns (live dHidden tiles, tiles, live 16-cell k-steps, k-steps with a cell)."""
    live = tw["inside"] & ~tw["flush"]
    B, T, U1 = live.shape
    ntt, nub = (T + 7) // 8, (U1 + 15) // 16
    pad = np.zeros((B, ntt * 8, nub * 16), dtype=bool)
    pad[:, :T, :U1] = live
    tiles = pad.reshape(B, ntt, 8, nub, 16).any(axis=(2, 4))
    flat = live.reshape(-1)
    nks = (flat.size + 15) // 16
    fl = np.zeros(nks * 16, dtype=bool)
    fl[:flat.size] = flat
    ks = fl.reshape(nks, 16).any(axis=1)
    return int(tiles.sum()), int(tiles.size), int(ks.sum()), int(nks)
