"""CPU: pins the float64 oracle of tests/latency_reg_oracle.py (FastEmit and the delay penalty).  At
lambda = delta = 0 it is oracle/cpu_oracle's loss; under the delay penalty its costs are brute-force sums over every path of
the penalised lattice and its gradients central finite differences of those costs; under FastEmit its gradients are torch
float64 autograd of the stop-gradient surrogate cost + lambda sum sg[E] (-log y), with E taken from an independent autograd
lattice as -d cost / d lp_emit; lambda never changes a cost."""
import itertools

import numpy as np
import pytest
import torch

from oracle import cpu_oracle
from tests import latency_reg_oracle as lro
from tests.helpers import make_inputs, oracle_fused

# (B, T, U, V, logit_lens, target_lens): ragged batches, T_b = 1, U_b = 0, a batch of one single-cell lattice
CASES = [
    (3, 5, 3, 5, [5, 1, 3], [3, 2, 0]),
    (2, 4, 2, 4, [4, 4], [2, 0]),
    (1, 1, 0, 4, [1], [0]),
    (2, 1, 3, 6, [1, 1], [3, 1]),
    (2, 5, 3, 4, [5, 2], [1, 3]),
]


def _case(c, seed):
    B, T, U, V, ll, tl = c
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((B, T, U + 1, V)) * 1.5
    targets = rng.integers(0, V - 1, (B, U)).astype(np.int32)
    return logits, targets, np.asarray(ll, dtype=np.int32), np.asarray(tl, dtype=np.int32)


def _brute_force_costs(logits, targets, ll, tl, delta):
    """-log of the sum over every path of exp(sum of its arcs' log-probs), lp_emit penalised by delta ((T_b-1)/2 - t)."""
    out = []
    for b in range(logits.shape[0]):
        Tb, Ub = int(ll[b]), int(tl[b])
        lp = lro.log_softmax(logits[b])
        V = logits.shape[-1]
        scores = []
        for emits in itertools.combinations_with_replacement(range(Tb), Ub):  # frame of each label, non-decreasing
            s, u = 0.0, 0
            for t in range(Tb):
                while u < Ub and emits[u] == t:
                    s += lp[t, u, targets[b, u]] + delta * ((Tb - 1) / 2.0 - t)
                    u += 1
                s += lp[t, u, V - 1]  # blank out of (t, u); the last one ends the path
            scores.append(s)
        out.append(-np.logaddexp.reduce(np.array(scores)))
    return np.array(out)


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_zero_options_are_the_plain_oracle(ci):
    logits, targets, ll, tl = _case(CASES[ci], seed=ci)
    c0, g0 = cpu_oracle.rnnt_loss(logits, targets, ll, tl, blank=-1)
    c, g = lro.loss_and_grad(logits, targets, ll, tl)
    np.testing.assert_allclose(c, c0, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g, g0, rtol=1e-10, atol=1e-12)
    c, g = lro.loss_and_grad(logits, targets, ll, tl, clamp=0.2)
    _, g0 = cpu_oracle.rnnt_loss(logits, targets, ll, tl, blank=-1, clamp=0.2)
    np.testing.assert_allclose(g, g0, rtol=1e-10, atol=1e-12)


def test_zero_options_fused_is_the_plain_fused_oracle():
    d = make_inputs(3, 7, 4, 16, 12, seed=4)
    r, ref = lro.fused(d), oracle_fused(d)
    np.testing.assert_allclose(r["costs"], ref["costs"], rtol=1e-12)
    for k in ("grad_enc", "grad_pred", "grad_W", "grad_bias"):
        np.testing.assert_allclose(r[k], ref[k], rtol=1e-9, atol=1e-13)


@pytest.mark.parametrize("delta", [0.0, 0.3, 1.7])
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_delay_penalty_cost_is_the_sum_over_penalised_paths(ci, delta):
    logits, targets, ll, tl = _case(CASES[ci], seed=10 + ci)
    c, _ = lro.loss_and_grad(logits, targets, ll, tl, delay_penalty=delta, want_grad=False)
    np.testing.assert_allclose(c, _brute_force_costs(logits, targets, ll, tl, delta), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_delay_penalty_gradient_is_the_cost_derivative(ci):
    logits, targets, ll, tl = _case(CASES[ci], seed=20 + ci)
    delta, eps = 0.4, 1e-6
    _, g = lro.loss_and_grad(logits, targets, ll, tl, delay_penalty=delta)
    fd = np.zeros_like(logits)
    for idx in np.ndindex(logits.shape):
        x = logits.copy()
        x[idx] += eps
        cp = lro.loss_and_grad(x, targets, ll, tl, delay_penalty=delta, want_grad=False)[0].sum()
        x[idx] -= 2 * eps
        cm = lro.loss_and_grad(x, targets, ll, tl, delay_penalty=delta, want_grad=False)[0].sum()
        fd[idx] = (cp - cm) / (2 * eps)
    np.testing.assert_allclose(g, fd, rtol=1e-6, atol=1e-8)


def _torch_cost(lpb, lpe):
    """-log P of one lattice by the alpha recursion in torch (autograd through every arc)."""
    Tb, U1b = lpb.shape
    alpha = [[None] * U1b for _ in range(Tb)]
    for t in range(Tb):
        for u in range(U1b):
            if t == 0 and u == 0:
                alpha[0][0] = torch.zeros((), dtype=torch.float64)
                continue
            terms = []
            if t > 0:
                terms.append(alpha[t - 1][u] + lpb[t - 1, u])
            if u > 0:
                terms.append(alpha[t][u - 1] + lpe[t, u - 1])
            alpha[t][u] = terms[0] if len(terms) == 1 else torch.logaddexp(terms[0], terms[1])
    return -(alpha[Tb - 1][U1b - 1] + lpb[Tb - 1, U1b - 1])


@pytest.mark.parametrize("delta", [0.0, 0.5])
@pytest.mark.parametrize("lam", [0.01, 0.7, 16.0])
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_fastemit_gradient_is_autograd_of_the_surrogate(ci, lam, delta):
    logits, targets, ll, tl = _case(CASES[ci], seed=30 + ci)
    B, T, U1, V = logits.shape
    _, g = lro.loss_and_grad(logits, targets, ll, tl, fastemit_lambda=lam, delay_penalty=delta)
    for b in range(B):
        Tb, Ub = int(ll[b]), int(tl[b])
        y = torch.from_numpy(targets[b, :Ub].astype(np.int64))
        pen = delta * ((Tb - 1) / 2.0 - torch.arange(Tb, dtype=torch.float64))[:, None]
        z = torch.from_numpy(logits[b, :Tb, :Ub + 1]).clone().requires_grad_(True)
        lp = torch.log_softmax(z, dim=-1)
        lpb = lp[:, :, V - 1]
        lpe = lp[:, torch.arange(Ub), y] + pen
        # E(t,u) = -d cost / d lp_emit'(t,u), from an autograd lattice of its own (no alpha / beta of the oracle)
        leaf = lpe.detach().clone().requires_grad_(True)
        E = -torch.autograd.grad(_torch_cost(lpb.detach(), leaf), leaf)[0] if Ub else torch.zeros(Tb, 0, dtype=torch.float64)
        surrogate = _torch_cost(lpb, lpe) + lam * (E * -lp[:, torch.arange(Ub), y]).sum()
        want = torch.autograd.grad(surrogate, z)[0].numpy()
        np.testing.assert_allclose(g[b, :Tb, :Ub + 1], want, rtol=1e-9, atol=1e-12)
        assert not g[b, Tb:].any() and not g[b, :, Ub + 1:].any()


@pytest.mark.parametrize("delta", [0.0, 0.5])
def test_fastemit_leaves_the_costs_unchanged(delta):
    for ci, c in enumerate(CASES):
        logits, targets, ll, tl = _case(c, seed=40 + ci)
        c0, g0 = lro.loss_and_grad(logits, targets, ll, tl, delay_penalty=delta)
        c1, g1 = lro.loss_and_grad(logits, targets, ll, tl, fastemit_lambda=0.5, delay_penalty=delta)
        assert np.array_equal(c0, c1)
        if int(tl.max()) > 0:
            assert np.abs(g1 - g0).max() > 1e-3


def test_lengths_are_clamped_as_the_kernels_clamp_them():
    logits, targets, _, _ = _case(CASES[0], seed=50)
    c, g = lro.loss_and_grad(logits, targets, [9, 0, 3], [7, -2, 1], fastemit_lambda=0.3, delay_penalty=0.2)
    c2, g2 = lro.loss_and_grad(logits, targets, [5, 1, 3], [3, 0, 1], fastemit_lambda=0.3, delay_penalty=0.2)
    assert np.array_equal(c, c2) and np.array_equal(g, g2)
