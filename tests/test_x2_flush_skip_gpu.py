"""-m gpu: the f16x2 route's flush rule (rnnt_amd/csrc/lattice.hip k_coef, FLUSH, x2.hip "flush rule") against its own A/B
partner, RNNT_VARIANT_X2_NO_FLUSH_SKIP, in one process: skipping dHidden tiles and dW k-steps without a live cell changes no bit
of costs, grad_enc, grad_pred, and grad_W / grad_bias by no more than the route's own distance from the fp32 route.  The
shapes (tests/x2_flush_twin.py CASES) are checked on the CPU (tests/test_x2_flush_oracle.py) to leave >= 25 % of the dHidden
tiles dead; every case asserts through the device's counts that tiles and k-steps WERE skipped."""
import numpy as np
import pytest
import torch

from tests.helpers import make_inputs
from tests.test_gpu_parity import _dev
from tests.x2_flush_twin import CASES, live_fractions, twin

pytestmark = pytest.mark.gpu
X2 = "f16x2"


@pytest.fixture(scope="module")
def e():
    import rnnt_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    rnnt_amd.engine.lib()
    return rnnt_amd.engine


def _run(e, g, V, gs, dtype=X2, variant=0, stage_mask=None):
    outs = e.joint_loss_fwd_bwd(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"],
                                V - 1, gs, dtype=dtype, variant=variant, stage_mask=stage_mask)
    torch.cuda.synchronize()
    return outs


def _counts(e, g, V):
    B, T, H = g["enc"].shape
    return e.x2_live_counts(g["enc"].device, B, T, g["pred"].shape[1], H, V)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name", sorted(CASES))
def test_flush_skip_is_exact_beside_its_variant(e, name):
    """costs / grad_enc / grad_pred: torch.equal.  grad_W / grad_bias differ in summation order only (the split-K ranges cut the
    shorter live list at other cells): max |flush - variant| must not exceed max |variant - fp32 route| on the same inputs —
    the exact route is the reference, no number is fixed in advance.
    Measured on MI355X (max |flush - variant| / max |variant - fp32 route|; profiles/x2_flush_skip_ab.txt section 8):
        h1024   grad_W 1.526e-05 / 1.221e-04   grad_bias 4.768e-07 / 9.155e-05
        h640    grad_W 3.815e-06 / 1.717e-05   grad_bias 2.980e-08 / 2.289e-05
        ragged  grad_W 7.629e-06 / 9.155e-05   grad_bias 2.384e-07 / 7.629e-05
        u1_63   grad_W 7.629e-06 / 2.136e-04   grad_bias 1.192e-07 / 1.831e-04
    (the route sums its split-K slabs in fp64 and rounds once, k_x2_reduce_slabs: with an fp32 running sum over the 256 slabs of
    u1_63 the left figure was 1.831e-04 — 3 ulp of the largest entries — against 9.155e-05.)"""
    B, T, U, H, V, seed, ragged, gs = CASES[name]
    d = make_inputs(B, T, U, H, V, seed, ragged=ragged)
    lt, nt, lk, nk = live_fractions(twin(d, gs))
    print(f"{name}: fp64 twin: live tiles {lt}/{nt}, live k-steps {lk}/{nk}")
    assert nt - lt >= 0.25 * nt  # the case's condition
    g = _dev(d)
    ref = _run(e, g, V, gs, variant=e.VARIANT_X2_NO_FLUSH_SKIP)
    cn = _counts(e, g, V)
    new = _run(e, g, V, gs)
    c = _counts(e, g, V)
    f32 = _run(e, g, V, gs, dtype="fp32")
    print(f"{name}: device counts with the variant bit {cn}, without {c}")
    for k, a, b in zip(("costs", "grad_enc", "grad_pred"), new[:3], ref[:3]):
        assert torch.equal(a, b), k
    for k, a, b, x in zip(("grad_W", "grad_bias"), new[3:], ref[3:], f32[3:]):
        diff, bound = float((a - b).abs().max()), float((b - x).abs().max())
        print(f"{name}: {k}: |flush - variant| max {diff:.3e}, |variant - fp32 route| max {bound:.3e}")
        assert diff <= bound, k
    # skipping happened: the device ran fewer tiles / walked fewer k-steps than by length, and left >= 25 % of the tiles out
    assert c["tiles"] == cn["tiles"] == nt and c["ksteps"] == cn["ksteps"] == nk
    assert c["live_tiles"] < cn["live_tiles"] and c["live_ksteps"] < cn["live_ksteps"]
    assert c["tiles"] - c["live_tiles"] >= 0.25 * c["tiles"]


@pytest.mark.parametrize("name", ["u1_63", "ragged"])
def test_flagged_cells_hold_zero_planes(e, name):
    """Soundness of the device predicate, directly: with the variant bit (nothing skipped) the stages up to dHidden leave G's two
    fp16 planes in place of the logits; every cell the predicate flags without the bit holds zeros in both (as VALUES: a
    negative G below the threshold rounds to -0, bits 0x8000, which adds nothing to an accumulator either).  And the flagged
    cells lie inside {g_scale grad_scale gamma < 2^-25} of the fp64 oracle's alpha, beta."""
    B, T, U, H, V, seed, ragged, gs = CASES[name]
    d = make_inputs(B, T, U, H, V, seed, ragged=ragged)
    g = _dev(d)
    U1, cells = U + 1, B * T * (U + 1)
    L = e.layout(B, T, U1, H, V, X2)

    def coef():
        ws = e.workspace(g["enc"].device, L.total)
        return ws[L.coef:L.coef + cells * 16].view(torch.float32).reshape(cells, 4)[:, :3].clone()

    def null(c):
        return (c[:, 0] == float("-inf")) & (c[:, 1] == 0) & (c[:, 2] == 0)

    _run(e, g, V, gs, stage_mask=15)  # producers, forward, lattice, coefficients: the predicate's flags
    flagged = null(coef())
    _run(e, g, V, gs, variant=e.VARIANT_X2_NO_FLUSH_SKIP, stage_mask=31)  # ... + dHidden: G's planes of every cell
    flagged &= ~null(coef())
    assert flagged.any()
    ws = e.workspace(g["enc"].device, L.total)
    planes = ws[L.logits:L.logits + cells * V * 4].view(torch.float16).reshape(cells, 2 * V)
    assert bool((planes[flagged] == 0).all())
    assert not bool((planes[~flagged] == 0).all())  # (the buffer read is the one the kernel wrote)
    tw = twin(d, gs)
    dev_flag = flagged.cpu().numpy().reshape(B, T, U1)
    assert not (dev_flag & ~tw["gamma_small"]).any()
    print(f"{name}: device flags {int(dev_flag.sum())} cells, the fp64 twin {int(tw['flush'].sum())}")


def test_lattice_too_small_to_flush(e):
    d = make_inputs(2, 9, 4, 128, 128, seed=7)
    g = _dev(d)
    ref = _run(e, g, 128, 0.5, variant=e.VARIANT_X2_NO_FLUSH_SKIP)
    cn = _counts(e, g, 128)
    new = _run(e, g, 128, 0.5)
    assert _counts(e, g, 128) == cn and cn["live_ksteps"] > 0
    for a, b in zip(new, ref):
        assert torch.equal(a, b)


def test_nan_utterance_beside_healthy_ones(e):
    """A non-finite cost keeps every cell of its utterance live; the healthy utterance is flushed as usual and changes no bit."""
    B, T, U, H, V = 2, 360, 62, 128, 128
    d = make_inputs(B, T, U, H, V, seed=21, ragged=False)
    d["enc"][1, 4, :] = np.nan
    g = _dev(d)
    ref = _run(e, g, V, 0.5, variant=e.VARIANT_X2_NO_FLUSH_SKIP)
    cn = _counts(e, g, V)
    new = _run(e, g, V, 0.5)
    c = _counts(e, g, V)
    assert bool(torch.isnan(new[0][1])) and bool(torch.isfinite(new[0][0]))
    for a, b in zip(new[:3], ref[:3]):
        assert _same_bits(a, b)
    for a, b in zip(new[3:], ref[3:]):
        assert torch.equal(torch.isnan(a), torch.isnan(b))
    per = cn["tiles"] // B  # utterance 1 keeps all its tiles; utterance 0 loses some
    assert cn["live_tiles"] == cn["tiles"] and per <= c["live_tiles"] < cn["live_tiles"]


def test_regularised_entry_flushes_nothing(e):
    B, T, U, H, V, seed, ragged, gs = CASES["u1_63"]
    g = _dev(make_inputs(B, T, U, H, V, seed, ragged=ragged))
    _run(e, g, V, gs, variant=e.VARIANT_X2_NO_FLUSH_SKIP)
    cn = _counts(e, g, V)
    for lam, dp in ((0.5, 0.05), (0.0, 0.0)):
        e.joint_loss_fwd_bwd_reg(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"],
                                 V - 1, gs, lam, dp, dtype=X2)
        torch.cuda.synchronize()
        assert _counts(e, g, V) == cn
