"""CPU: the float64 oracle of the alignment-restricted loss (tests/restricted_oracle.py) against brute-force path
enumeration on tiny lattices (costs, and gradients by central differences of the enumerated cost), and its identities: a
zero-width window around the Viterbi path leaves that path alone, a window of T frames and more restricts nothing, frames
that decrease leave no path."""
import itertools

import numpy as np
import pytest

from tests import align_oracle
from tests import latency_reg_oracle as lro
from tests import restricted_oracle as ro
from tests.helpers import make_inputs


def _brute_cost(logits, targets, Tb, Ub, frames, left, right, blank):
    """-log of the summed probability of every path whose label u is emitted at a frame inside its window."""
    lpb, lpe = align_oracle.lattice_logprobs(logits, targets, blank)
    total, n = -np.inf, 0
    for f in itertools.combinations_with_replacement(range(Tb), Ub):
        if all(frames[u] - left <= f[u] <= frames[u] + right for u in range(Ub)):
            total = np.logaddexp(total, align_oracle.rescore(lpb, lpe, np.asarray(f, dtype=np.int64), Tb, Ub))
            n += 1
    return -total, n


def _tiny(T, U, V, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((1, T, U + 1, V)) * 1.5), rng.integers(0, V - 1, (1, U)).astype(np.int32)


# (T, U, frames, left, right, surviving paths)
TINY = [
    (5, 3, (1, 2, 4), 0, 0, 1),       # all but one path removed
    (5, 3, (1, 2, 4), 5, 5, 35),      # none removed: C(5 + 3 - 1, 3)
    (5, 3, (1, 2, 4), 1, 0, None),
    (4, 2, (0, 3), 0, 2, None),
    (5, 3, (2, 2, 2), 1, 1, None),
    (3, 1, (1,), 0, 1, 2),
    (1, 3, (0, 0, 0), 0, 0, 1),       # one frame: the only path
    (4, 0, (), 0, 0, 1),              # no labels: nothing to restrict
]


@pytest.mark.parametrize("T,U,frames,left,right,npaths", TINY)
def test_oracle_matches_path_enumeration(T, U, frames, left, right, npaths):
    V, blank = 4, 3
    logits, targets = _tiny(T, U, V, seed=T * 10 + U)
    fr = np.asarray(frames, dtype=np.int32).reshape(1, U)
    ll, tl = np.array([T], dtype=np.int32), np.array([U], dtype=np.int32)
    costs, G = ro.loss_and_grad(logits, targets, ll, tl, fr, left, right, blank)
    want, n = _brute_cost(logits[0], targets[0], T, U, frames, left, right, blank)
    if npaths is not None:
        assert n == npaths
    assert n >= 1 and abs(costs[0] - want) <= 1e-12 * max(1.0, abs(want))
    eps = 1e-6
    num = np.zeros_like(G[0])
    for idx in np.ndindex(*num.shape):
        hi, lo = logits[0].copy(), logits[0].copy()
        hi[idx] += eps
        lo[idx] -= eps
        num[idx] = (_brute_cost(hi, targets[0], T, U, frames, left, right, blank)[0] -
                    _brute_cost(lo, targets[0], T, U, frames, left, right, blank)[0]) / (2 * eps)
    assert np.abs(G[0] - num).max() <= 1e-8


def test_unreachable_cells_have_zero_gradient_and_occupancy():
    logits, targets = _tiny(5, 3, 4, seed=3)
    fr = np.array([[1, 2, 4]], dtype=np.int32)
    _, G, occ = ro.loss_and_grad(logits, targets, [5], [3], fr, 0, 0, 3, want_occupancy=True)
    on_path = np.zeros((5, 4), dtype=bool)
    for t, u in ((0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (3, 2), (4, 2), (4, 3)):
        on_path[t, u] = True
    assert np.array_equal(occ[0] > 0, on_path) and np.allclose(occ[0][on_path], 1.0, atol=1e-12)
    assert (G[0][~on_path] == 0.0).all() and (np.abs(G[0][on_path]).max(axis=-1) > 0).all()


CASES = [(4, 23, 9), (2, 9, 3)]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "B%dT%dU%d" % c)
def case(request):
    B, T, U = request.param
    d = make_inputs(B, T, U, 32, 16, seed=B + T, ragged=True)
    logits = lro.cpu_oracle.joint_fwd(d["enc"], d["pred"], d["W"], d["bias"])
    scores, frames = ro.viterbi_frames(d, logits=logits)
    return d, logits, scores, frames


def test_zero_window_around_the_viterbi_path_is_minus_its_score(case):
    d, logits, scores, frames = case
    costs, _ = ro.loss_and_grad(logits, d["targets"], d["logit_lens"], d["target_lens"], frames, 0, 0)
    assert np.abs(costs + scores).max() <= 1e-12 * np.abs(scores).max()


@pytest.mark.parametrize("lam,dp", [(0.0, 0.0), (0.5, 0.05)])
def test_wide_window_is_the_unrestricted_loss(case, lam, dp):
    d, logits, _, frames = case
    T = logits.shape[1]
    a = ro.loss_and_grad(logits, d["targets"], d["logit_lens"], d["target_lens"], frames, T, T, -1, lam, dp)
    b = lro.loss_and_grad(logits, d["targets"], d["logit_lens"], d["target_lens"], -1, lam, dp)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("window", [(0, 0), (2, 1), (0, 3)])
def test_windows_keep_costs_finite_and_move_the_gradient(case, window):
    d, logits, _, frames = case
    costs, G = ro.loss_and_grad(logits, d["targets"], d["logit_lens"], d["target_lens"], frames, *window)
    c0, G0 = lro.loss_and_grad(logits, d["targets"], d["logit_lens"], d["target_lens"])
    assert np.isfinite(costs).all() and (costs >= c0 - 1e-9).all()  # fewer paths: never a smaller cost
    assert np.abs(G - G0).max() > 0.1 * np.abs(G0).max()


def test_decreasing_frames_leave_no_path(case):
    d, logits, _, frames = case
    bad = frames.copy()
    assert d["target_lens"][0] >= 2 and d["logit_lens"][0] >= 3
    bad[0, 0], bad[0, 1] = 2, 0  # label 1 would have to come before label 0
    for lam in (0.0, 0.5):
        costs, G = ro.loss_and_grad(logits, d["targets"], d["logit_lens"], d["target_lens"], bad, 0, 1, -1, lam)
        ok, G_ok = ro.loss_and_grad(logits, d["targets"], d["logit_lens"], d["target_lens"], frames, 0, 1, -1, lam)
        assert costs[0] == np.inf and (G[0] == 0.0).all() and np.isfinite(G).all()
        assert np.array_equal(costs[1:], ok[1:]) and np.array_equal(G[1:], G_ok[1:])
    r = ro.fused(d, bad, 0, 1)
    assert r["costs"][0] == np.inf and all(np.isfinite(r[k]).all() for k in ("grad_enc", "grad_pred", "grad_W", "grad_bias"))
    assert (r["grad_enc"][0] == 0.0).all() and (r["grad_pred"][0] == 0.0).all()


def test_diagonal_sweep_is_the_double_loop():
    rng = np.random.default_rng(0)
    lpb = -rng.random((7, 5)) - 0.1
    lpe = -rng.random((7, 4)) - 0.1
    lpe[rng.random((7, 4)) < 0.5] = -np.inf
    a0, b0 = lro.alpha_beta(lpb, lpe)
    a1, b1 = ro.alpha_beta_diag(lpb, lpe)
    assert np.array_equal(a0, a1) and np.array_equal(b0, b1)


def test_numpy_joint_is_the_c_joint():
    d = make_inputs(2, 6, 3, 16, 8, seed=4, ragged=True)
    _, frames = ro.viterbi_frames(d)
    a, b = ro.fused(d, frames, 1, 1, 0.5, 0.05), ro.fused(d, frames, 1, 1, 0.5, 0.05, numpy_joint=True)
    for k in a:
        assert np.allclose(a[k], b[k], rtol=1e-12, atol=1e-14), k
