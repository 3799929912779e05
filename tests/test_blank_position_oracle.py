"""CPU tests: the references of tests/test_blank_position_gpu.py at a blank other than V - 1.  tests/helpers.relabel_blank moves
the blank of a make_inputs problem; the float64 oracles are invariant under that relabelling (costs equal, gradients permuted),
agree with each other at an interior blank, and reproduce a committed end-to-end fixture (expected values from the
reference's own JointNetwork) after its vocabulary is relabelled."""
import os

import numpy as np
import pytest

from oracle import cpu_oracle
from tests import latency_reg_oracle as lro
from tests.helpers import blank_index_map, has_live_label, make_inputs, oracle_fused, relabel_blank

# (B, T, U, H, V), blank: first / interior / first column of the second 128-wide chunk, V % 128 != 0 twice
CASES = [((2, 9, 4, 128, 128), 0), ((3, 23, 19, 36, 132), 5), ((2, 12, 5, 128, 260), 128), ((2, 9, 4, 20, 12), 10)]


def _close(name, got, ref, tol=1e-12):
    """Both sides are float64 evaluations of the same sums in another order: 1e-12 of the largest entry (measured: 2e-14)."""
    err = np.abs(np.asarray(got) - np.asarray(ref)).max()
    assert err <= tol * np.abs(ref).max(), (name, err, np.abs(ref).max())


@pytest.mark.parametrize("V,blank", [(4, 0), (7, 3), (128, 127), (128, -1), (128, -128), (132, 130)])
def test_index_map_is_the_order_preserving_permutation(V, blank):
    m = blank_index_map(V, blank)
    b = blank % V
    assert sorted(m.tolist()) == list(range(V)) and m[V - 1] == b
    assert (np.diff(m[:V - 1]) > 0).all()  # the labels keep their order
    assert b not in m[:V - 1].tolist()


@pytest.mark.parametrize("shape,blank", CASES)
def test_relabel_blank_moves_rows_and_targets_and_never_emits_the_blank(shape, blank):
    B, T, U, H, V = shape
    d = make_inputs(B, T, U, H, V, seed=sum(shape))
    for b in range(V):
        for nb in (False, True):
            r, m = relabel_blank(d, b - V if b % 2 else b, neighbours=nb)
            assert not (r["targets"] == b).any()
            assert (r["targets"] >= 0).all() and (r["targets"] < V).all() and r["targets"].dtype == np.int32
            assert np.array_equal(r["W"][m], d["W"]) and np.array_equal(r["bias"][m], d["bias"])
            assert np.array_equal(r["W"][b], d["W"][V - 1])
            for k in ("enc", "pred", "logit_lens", "target_lens"):
                assert r[k] is d[k]
            if not nb:
                assert np.array_equal(r["targets"], m[d["targets"]])
                continue
            want = m[d["targets"]]
            if b >= 1:
                want[0, 0] = b - 1
            if b + 1 < V:
                want[0, 1] = b + 1
            assert np.array_equal(r["targets"], want)
            # the last real column (beside the host's padding) is a live label once the blank is the one before it
            assert b != V - 2 or has_live_label(r, V - 1)
    assert not (d["targets"] == V - 1).any()  # the input dict was left alone


@pytest.mark.parametrize("shape,blank", CASES)
def test_fused_oracle_is_invariant_under_the_relabelling(shape, blank):
    B, T, U, H, V = shape
    d = make_inputs(B, T, U, H, V, seed=sum(shape))
    r, m = relabel_blank(d, blank)
    ref, got = oracle_fused(d), oracle_fused(r, blank=blank)
    np.testing.assert_allclose(got["loss"], ref["loss"], rtol=1e-12)
    np.testing.assert_allclose(got["costs"], ref["costs"], rtol=1e-12)
    _close("grad_enc", got["grad_enc"], ref["grad_enc"])
    _close("grad_pred", got["grad_pred"], ref["grad_pred"])
    _close("grad_W", got["grad_W"][m], ref["grad_W"])
    _close("grad_bias", got["grad_bias"][m], ref["grad_bias"])
    # and under the two spellings of the same index
    neg = oracle_fused(r, blank=blank - V)
    for k in got:
        assert np.array_equal(neg[k], got[k]), k


def _logits_case(shape, seed):
    B, T, U, V = shape
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((B, T, U + 1, V)) * 2
    return logits, make_inputs(B, T, U, 4, V, seed=seed)


@pytest.mark.parametrize("shape,blank", [((2, 6, 3, 40), 0), ((2, 6, 3, 40), 17), ((2, 8, 4, 7), 3), ((3, 11, 9, 132), 128)])
def test_loss_oracles_at_a_moved_blank(shape, blank):
    """cpu_oracle.rnnt_loss (C) at the relabelled blank is its V - 1 result permuted, and tests/latency_reg_oracle's numpy
    loss_and_grad at lambda = delta = 0 is the same function at that blank (an independent implementation: plain and clamped)."""
    logits, d = _logits_case(shape, sum(shape))
    r, m = relabel_blank(d, blank)
    moved = np.empty_like(logits)
    moved[..., m] = logits
    c0, g0 = cpu_oracle.rnnt_loss(logits, d["targets"], d["logit_lens"], d["target_lens"], blank=-1)
    c, g = cpu_oracle.rnnt_loss(moved, r["targets"], r["logit_lens"], r["target_lens"], blank=blank)
    np.testing.assert_allclose(c, c0, rtol=1e-12)
    _close("grad_logits", g[..., m], g0)
    assert np.abs(g[..., blank]).max() > 0
    for clamp in (-1.0, 0.05):
        cc, gc = cpu_oracle.rnnt_loss(moved, r["targets"], r["logit_lens"], r["target_lens"], blank=blank, clamp=clamp)
        cl, gl = lro.loss_and_grad(moved, r["targets"], r["logit_lens"], r["target_lens"], blank, 0.0, 0.0, clamp=clamp)
        np.testing.assert_allclose(cl, cc, rtol=1e-12, atol=1e-12)       # (the bars of tests/test_latency_reg_oracle.py at V - 1)
        np.testing.assert_allclose(gl, gc, rtol=1e-10, atol=1e-12)


def test_regularised_fused_oracle_is_invariant_under_the_relabelling():
    d = make_inputs(4, 23, 9, 128, 128, seed=3)
    ref = lro.fused(d, 0.5, 0.05)
    for blank in (0, 7, 8, 126):
        r, m = relabel_blank(d, blank)
        got = lro.fused(r, 0.5, 0.05, blank=blank)
        np.testing.assert_allclose(got["costs"], ref["costs"], rtol=1e-12)
        for k in ("grad_enc", "grad_pred"):
            _close(k, got[k], ref[k])
        for k in ("grad_W", "grad_bias"):
            _close(k, got[k][m], ref[k])
    assert np.array_equal(lro.fused(d, 0.5, 0.05, blank=-1)["grad_W"], ref["grad_W"])  # the keyword's default is the old value


@pytest.mark.parametrize("blank", [0, 5, 16, 30])
def test_relabelled_end_to_end_fixture(golden_dir, blank):
    """tests/golden/e2e_mid.npz (reference JointNetwork in fp64 + an independent autograd loss, blank = V - 1 = 31) with
    joint_ln's rows and the targets relabelled: the oracle at `blank` reproduces the fixture's loss and its gradients, permuted,
    at the bars of tests/test_oracle.py::test_oracle_e2e_matches_golden."""
    z = np.load(os.path.join(golden_dir, "e2e_mid.npz"))
    V = z["sd__joint_ln__weight"].shape[0]
    d = dict(enc=z["audio"], pred=z["text"], W=z["sd__joint_ln__weight"], bias=z["sd__joint_ln__bias"], targets=z["targets"],
             logit_lens=z["logit_lens"], target_lens=z["target_lens"])
    r, m = relabel_blank(d, blank)
    assert not np.array_equal(r["targets"], d["targets"]) and not (r["targets"] == blank).any()
    got = cpu_oracle.joint_loss_fwd_bwd(r["enc"].astype(np.float64), r["pred"].astype(np.float64), r["W"], r["bias"],
                                        r["targets"], r["logit_lens"], r["target_lens"], blank=blank)
    np.testing.assert_allclose(got["loss"], z["loss"], rtol=1e-12)
    np.testing.assert_allclose(got["costs"], z["costs"], rtol=1e-12)
    np.testing.assert_allclose(got["grad_W"][m], z["grad__joint_ln__weight"], atol=1e-11)
    np.testing.assert_allclose(got["grad_bias"][m], z["grad__joint_ln__bias"], atol=1e-11)
    np.testing.assert_allclose(got["grad_enc"], z["grad_audio"], atol=1e-11)
    np.testing.assert_allclose(got["grad_pred"], z["grad_text"], atol=1e-11)
    assert V == 32 and np.abs(z["grad__joint_ln__weight"][V - 1]).max() > 1e-3  # the blank's row carries gradient to move
