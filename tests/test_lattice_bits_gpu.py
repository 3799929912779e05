"""rnnt_amd/csrc/lattice.hip, ctc.hip and align.hip keep EVERY BIT they left before the loss tail was put on one argument block, one
kernel template per stage and shared leaf pieces: the standalone loss entries (plain, FastEmit, delay penalty, alignment
restriction, with and without grad_logits) on every form of the sweep, the fused entries' five coefficient kernels, the CTC head and
the forced alignment.  Costs, scores and frames raw, small arrays raw, everything else and the calls' whole workspaces as SHA-256,
against tests/golden/lattice_bits.npz, written by tests/golden/make_golden_lattice_bits.py, which also holds the cases and the code
that runs them.  Every path is a fixed kernel sequence with fixed summation orders, so the bar is equality — on integer views, which
keeps NaN payloads and the sign of zero."""
import importlib.util
import os

import numpy as np
import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_lattice_bits", os.path.join(_HERE, "golden", "make_golden_lattice_bits.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def engine():
    import rnnt_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    rnnt_amd.engine.lib()
    return rnnt_amd.engine


@pytest.fixture(scope="module")
def golden():
    return np.load(G.GOLDEN)


def test_recording_covers_exactly_the_cases(golden):
    assert {k.rsplit("/", 1)[0] for k in golden.files} == set(G.CASES)


def test_the_cases_are_the_paths():
    """Host code only: every shape through every option of the three standalone entries, the two further one-wave cases, the five
    coefficient kernels of the fused entries, the CTC list, the two alignments; the chain / barrier split by the launchers' formula."""
    assert {n for n in G.CASES if n.startswith("loss/")} == (
        {"loss/%s/%s" % (s, m) for s in G.SHAPES for m in G.MODES} | {"loss/one_wave/no_path", "loss/one_wave/nan_logit"})
    assert len(G.MODES) == 7 and set(G.SHAPES) == {"one_wave", "two_waves", "three_waves", "barrier"}
    for name, (B, T, U1, V, ll, tl) in G.SHAPES.items():
        waves, mbox = (U1 + 63) // 64, G.chain_mailbox_bytes(U1, T + U1 - 1)
        assert (waves, mbox > 64 * 1024) == {"one_wave": (1, False), "two_waves": (2, False), "three_waves": (3, False),
                                             "barrier": (9, True)}[name]
        assert len(ll) == len(tl) == B and max(ll) <= T and max(tl) <= U1 - 1
        assert B == 1 or (1 in ll and 0 in tl)
    assert G.SHAPES["three_waves"][2] == 2 * 64 + 1 and G.chain_mailbox_bytes(520, 689) == 8 * 689 * 12
    assert {n for n in G.CASES if n.startswith("fused/")} == {"fused/" + f for f in G.FUSED}
    assert {n for n in G.CASES if n.startswith("ctc/")} == {"ctc/" + c for c in G.CTC}
    N, T, U, _, _, tl, _ = G.CTC["barrier"]
    assert G.chain_mailbox_bytes(U + 1, T) > 64 * 1024 and any(0 in c[5] for c in G.CTC.values())
    assert {n for n in G.CASES if n.startswith("align/")} == {"align/one_wave", "align/two_waves"}


def test_recorded_flush_cases_hold_flushed_and_live_cells(golden):
    """Host code only: in the f16x2 cases' recorded coefficients the flush rule took lattice cells (null where the fp32 route's same
    call left a live cell) and left others — with and without the restriction.  The FLUSH branch cannot pass by never firing."""
    fired = G.flush_fired(lambda k: golden[k])
    assert set(fired) == {"x2_plain", "x2_restrict"}
    for name, (flushed, live) in fired.items():
        assert flushed > 0 and live > 0, (name, flushed, live)
    for f in G.FUSED:  # the masks are those of the recorded coefficients
        assert golden["fused/%s/coef" % f].dtype.kind == "U" and golden["fused/%s/coef_null" % f].dtype == np.uint8


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(G.CASES))
def test_case_keeps_every_bit(engine, golden, name):
    for run in range(2):
        got = G.run_checked(engine, name)
        assert sorted(got) == sorted(k.rsplit("/", 1)[1] for k in golden.files if k.rsplit("/", 1)[0] == name)
        for k, a in got.items():
            want = golden["%s/%s" % (name, k)]
            assert a.dtype == want.dtype and a.shape == want.shape, (run, k)
            assert np.array_equal(a, want), "run %d: %s differs from the recorded bytes: %s != %s" % (run, k, a, want)
