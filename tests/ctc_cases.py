"""Shared pieces of the CTC tests (tests/test_ctc_*.py): the float64 oracle, the numpy collapse, seeded inputs.

The oracle is torch.nn.functional.ctc_loss on the CPU in float64 over the float64 log_softmax of the SAME fp32 logits, with
reduction="none" and zero_infinity=True; whether an utterance is infeasible (cost +inf) is decided separately by `infeasible`.
Frames t >= T_n are zeroed first (torch never reads them in the loss, but a NaN there would pass through log_softmax's
backward), so their oracle gradient is exactly zero."""
import numpy as np
import torch


def infeasible(targets, logit_lens, target_lens):
    """[N] bool: T_n < U_n + (adjacent equal labels among the first U_n)."""
    out = []
    for y, T, U in zip(np.asarray(targets), logit_lens, target_lens):
        y = y[:U]
        out.append(int(T) < int(U) + int((y[1:] == y[:-1]).sum()))
    return np.array(out, dtype=bool)


def oracle(logits, targets, logit_lens, target_lens, blank, weights=None):
    """-> (costs [N] float64 with 0 for infeasible utterances, d sum_n weights[n] costs[n] / d logits [N,T,V] float64)."""
    x = np.array(logits, dtype=np.float64)
    N, T, V = x.shape
    ll, tl = np.asarray(logit_lens, dtype=np.int64), np.asarray(target_lens, dtype=np.int64)
    x[np.arange(T)[None, :] >= ll[:, None]] = 0.0
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tg = np.asarray(targets, dtype=np.int64)
    U = tg.shape[1]
    tg = np.where(np.arange(U)[None, :] < tl[:, None], tg, 0) if U else np.zeros((N, 1), dtype=np.int64)
    lp = torch.log_softmax(xt, dim=-1).transpose(0, 1)
    costs = torch.nn.functional.ctc_loss(lp, torch.tensor(tg), torch.tensor(ll), torch.tensor(tl), blank=blank, reduction="none",
                                         zero_infinity=True)
    w = torch.ones(N, dtype=torch.float64) if weights is None else torch.tensor(np.asarray(weights, dtype=np.float64))
    (costs * w).sum().backward()
    return costs.detach().numpy(), xt.grad.numpy()


def collapse(best, logit_lens, blank):
    """The numpy collapse: per utterance, the frame-wise argmax `best` [N,T] with repeats merged and blanks dropped."""
    out = []
    for row, T in zip(np.asarray(best), logit_lens):
        row = row[:int(T)]
        keep = np.ones(len(row), dtype=bool)
        keep[1:] = row[1:] != row[:-1]
        keep &= row != blank
        out.append(row[keep].tolist())
    return out


def make_targets(rng, N, U, V, blank, repeat_p=0.3):
    """[N,U] int32 labels != blank; a label equals its predecessor with probability `repeat_p` and differs from it otherwise."""
    labels = np.array([v for v in range(V) if v != blank])
    L = len(labels)
    idx = rng.integers(0, L, (N, max(U, 0)))
    for u in range(1, U):
        rep = rng.random(N) < repeat_p
        idx[:, u] = np.where(rep, idx[:, u - 1], (idx[:, u - 1] + 1 + rng.integers(0, max(L - 1, 1), N)) % L)
    return labels[idx].astype(np.int32)
