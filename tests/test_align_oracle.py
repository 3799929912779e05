"""CPU: the float64 alignment oracle (tests/align_oracle.py) against a brute-force maximum over every enumerated alignment on
tiny ragged lattices, and against the brute-force likelihood of oracle/brute_force.py where the two must meet."""
import itertools

import numpy as np
import pytest

from oracle.brute_force import nll_bruteforce
from tests import align_oracle as ao


def _all_paths(Tb, Ub):
    """Every alignment of a Tb x (Ub+1) lattice as its label frames: a path is T_b + U_b - 1 arcs before the final blank,
    of which U_b are label arcs; label u sits at the frame reached when it is emitted."""
    n = Tb + Ub - 1
    for pos in itertools.combinations(range(n), Ub):
        frames, t = [], 0
        ps = set(pos)
        for i in range(n):
            if i in ps:
                frames.append(t)
            else:
                t += 1
        yield np.array(frames, dtype=np.int32)


def _brute_best(lpb, lpe, Tb, Ub):
    best, arg = -np.inf, None
    for f in _all_paths(Tb, Ub):
        s = ao.rescore(lpb, lpe, f, Tb, Ub)
        if s > best:
            best, arg = s, f
    return best, arg


@pytest.mark.parametrize("seed", range(40))
def test_oracle_equals_brute_force_maximum(seed):
    rng = np.random.default_rng(seed)
    T, U, V = int(rng.integers(1, 7)), int(rng.integers(0, 5)), 6
    blank = int(rng.integers(0, V))
    B = 3
    logits = rng.standard_normal((B, T, U + 1, V)) * 2.0
    targets = rng.choice([v for v in range(V) if v != blank], size=(B, max(U, 1)))[:, :U].astype(np.int32)
    ll = rng.integers(1, T + 1, B)
    tl = rng.integers(0, U + 1, B)
    ll[0], tl[0] = T, U
    scores, frames, _ = ao.viterbi_logits(logits, targets, ll, tl, blank)
    for b in range(B):
        Tb, Ub = int(ll[b]), int(tl[b])
        lpb, lpe = ao.lattice_logprobs(logits[b], targets[b], blank)
        best, arg = _brute_best(lpb, lpe, Tb, Ub)
        assert scores[b] == pytest.approx(best, rel=1e-12, abs=1e-12)
        assert frames[b, :Ub].tolist() == arg.tolist()
        assert (frames[b, Ub:] == -1).all()
        assert ao.rescore(lpb, lpe, frames[b], Tb, Ub) == pytest.approx(scores[b], rel=1e-12, abs=1e-12)
        # the best path never beats the sum over all paths
        nll = nll_bruteforce(logits[b], targets[b], Tb, Ub, blank)
        assert scores[b] <= -nll + 1e-12
        if Ub == 0 or Tb == 1:  # a single path: best == sum
            assert scores[b] == pytest.approx(-nll, rel=1e-12, abs=1e-12)


def test_path_count_is_binomial():
    from math import comb
    for Tb in range(1, 6):
        for Ub in range(0, 5):
            assert sum(1 for _ in _all_paths(Tb, Ub)) == comb(Tb + Ub - 1, Ub)


def test_uniform_logits_emit_every_label_at_frame_zero():
    T, U, V = 6, 4, 5
    logits = np.zeros((2, T, U + 1, V))
    targets = np.array([[0, 1, 2, 3], [3, 3, 0, 1]], dtype=np.int32)
    scores, frames, margins = ao.viterbi_logits(logits, targets, np.array([6, 4]), np.array([4, 2]), blank=4)
    assert frames[0].tolist() == [0, 0, 0, 0]
    assert frames[1].tolist() == [0, 0, -1, -1]
    assert scores[0] == pytest.approx((T + U) * np.log(1.0 / V))
    assert margins[0] == 0.0  # every decision was a tie


def test_nan_rule():
    rng = np.random.default_rng(3)
    lpb, lpe = np.log(rng.uniform(0.1, 0.9, (5, 4))), np.log(rng.uniform(0.1, 0.9, (5, 4)))
    s, f, _ = ao.viterbi(lpb, lpe, 5, 3)
    assert np.isfinite(s) and (f >= 0).all()
    for (arr, t, u, read) in ((lpb, 2, 1, True), (lpe, 4, 2, True), (lpb, 4, 3, True), (lpe, 4, 3, False), (lpb, 4, 2, False)):
        x = arr.copy()
        x[t, u] = np.nan
        s2, f2, _ = ao.viterbi(x if arr is lpb else lpb, x if arr is lpe else lpe, 5, 3)
        assert np.isnan(s2) == read, (t, u)
        assert ((f2 == -1).all()) == read


def test_rescore_rejects_non_paths():
    lpb = np.zeros((3, 3))
    with pytest.raises(AssertionError):
        ao.rescore(lpb, lpb, np.array([2, 1]), 3, 2)  # decreasing
    with pytest.raises(AssertionError):
        ao.rescore(lpb, lpb, np.array([0, 3]), 3, 2)  # beyond T_b - 1
