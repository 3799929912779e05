"""CPU tests of tests/encoder_layer_cases.py: the float64 oracle against torch in float64, the plan mirror against the shipped
rnnt_engine_encoder_workspace_bytes, the edges every case claims, and wrong variants of the oracle against the bar."""
import ctypes

import numpy as np
import pytest
import torch

from tests import encoder_layer_cases as ec

ALL = ec.case_ids(layouts_too=False)


def _id(t):
    return "-".join(t)


def test_constants_are_the_packages():
    import rnnt_amd.encoder as E
    assert (ec.NORM_NONE, ec.NORM_BATCH, ec.NORM_INSTANCE) == (E.NORM_NONE, E.NORM_BATCH, E.NORM_INSTANCE)
    assert (ec.PLAIN, ec.FIRST, ec.LAST, ec.RESIDUAL, ec.FINAL) == (E.ROLE_PLAIN, E.ROLE_FIRST, E.ROLE_LAST, E.ROLE_RESIDUAL, E.ROLE_FINAL)
    assert (ec.AUTO, ec.MANY_ROWS) == (E.REGIME_AUTO, E.REGIME_MANY_ROWS)
    assert (ec.FEW_ROWS, ec.FEW_FRAMES) == (E.ENGINE_AUTO_MAX_ROWS, E.ENGINE_AUTO_MAX_FRAMES)


@pytest.mark.parametrize("name", sorted(ec.SHAPES))
def test_every_case_reaches_its_edges(name):
    case = ec.build(name)
    ec.check_reach(case)
    assert all(np.all(l.W != 0) for l in case.layers)  # every weight matters
    if case.states is not None:
        assert all(s is None or (s.size > 0 and np.all(s != 0)) for s in case.states)  # non-zero state frames


@pytest.mark.parametrize("cid", ALL, ids=_id)
def test_oracle_agrees_with_torch_in_float64(cid):
    """1e-12, plus the bar's own rounding floor taken in float64 (4 x 2^-52 x (max |pre-norm| x gamma x rstd + max |y|)): ~1e-14 for
    most cases, but the offset kind over two frames has values of 300 and an rstd of 200, where ONE float64 rounding of the conv sum
    is 1.5e-11 in the output (few_epilogue differs from torch by 9e-12 there)."""
    case, want, _ = ec.prepared(*cid)
    y, states = ec.torch_forward(case, torch.float64)
    assert y.shape == want.out.shape
    tol = 1e-12 + ec.FACTOR * 2.0 ** -52 * (float(np.abs(want.pre).max()) * want.scale + float(np.abs(want.out).max()))
    assert float(np.abs(y.numpy() - want.out).max()) <= tol
    for i, (a, b) in enumerate(zip(states, want.states)):
        assert (a is None) == (b is None)
        if a is not None and ec.reads_input(case, i):
            assert np.array_equal(a.numpy(), b)  # a state of the list's input is a copy
        elif a is not None:
            assert a.shape == b.shape and float(np.abs(a.numpy() - b).max()) <= 1e-12  # ... of a computed activation


@pytest.mark.parametrize("cid", ALL, ids=_id)
def test_bar_terms(cid):
    """The bar is a few fp32 roundings of the case's own values: positive, and nowhere near the faults the cases exist for."""
    _, want, (b, e_ref, e_round) = ec.prepared(*cid)
    assert 0.0 < e_round and b == ec.FACTOR * max(e_ref, e_round)
    assert b <= 1e-4 * max(1.0, float(np.abs(want.pre).max()) * want.scale)


@pytest.fixture(scope="module")
def lib():
    import os
    from rnnt_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build()
    L = engine.lib()
    L.rnnt_engine_last_error.restype = ctypes.c_char_p
    return L


def _descriptors(case):
    from rnnt_amd.encoder import _Layer
    arr = (_Layer * len(case.layers))()
    for d, l in zip(arr, case.layers):
        d.cin, d.cout, d.taps, d.stride, d.dilation, d.norm, d.role, d.eps = l.cin, l.cout, l.taps, l.stride, l.dil, l.norm, l.role, l.eps
    return arr


@pytest.mark.parametrize("name", sorted(ec.SHAPES))
def test_mirror_gives_the_librarys_workspace_bytes(lib, name):
    for kind in ("none", "instance"):
        case = ec.build(name, kind)
        lens = None if case.state_lens is None else (ctypes.c_int32 * len(case.layers))(*case.state_lens)
        for regime in (ec.AUTO, ec.MANY_ROWS):
            n = ctypes.c_size_t(0)
            rc = lib.rnnt_engine_encoder_workspace_bytes(_descriptors(case), len(case.layers), case.N, case.L, regime, lens, ctypes.byref(n))
            assert rc == 0, lib.rnnt_engine_last_error()
            assert n.value == ec.case_plan(case, regime).ws_bytes, (name, kind, regime)


def test_mirror_refuses_what_the_library_refuses(lib):
    case = ec.build("few_c68_s2", "instance")
    n = ctypes.c_size_t(0)
    for L, lens in ((1, [2]), (2, [0])):  # one output frame under instance norm; too short for any
        with pytest.raises(ValueError):
            ec.plan(case.layers, case.N, L, lens, ec.AUTO)
        assert lib.rnnt_engine_encoder_workspace_bytes(_descriptors(case), 1, case.N, L, ec.AUTO, (ctypes.c_int32 * 1)(*lens),
                                                       ctypes.byref(n)) == -1


@pytest.mark.parametrize("name", ec.CHAIN_CASES)
@pytest.mark.parametrize("norm", ("none", "batch"))
def test_chained_oracle_is_the_whole_utterance(name, norm):
    """The oracle's state rule: pushes of CHAIN_CHUNKS from zero state, each fed the states the push before left, concatenate to the
    whole utterance's output, and every state has the length the arithmetic gives."""
    whole, states, push = ec.chain(name, norm)
    outs = []
    for k in range(len(ec.CHAIN_CHUNKS)):
        case = push(states, k)
        got = ec.oracle(case)
        rows = ec.case_plan(case, ec.AUTO).rows
        assert [s.shape[2] for s in got.states] == [r.slen_out for r in rows]
        states = got.states
        assert np.array_equal(states[0].astype(np.float32), states[0])  # the first layer's: copies of fp32 input frames
        outs.append(got.out)
    want = ec.oracle(whole).out
    got = np.concatenate(outs, axis=1)
    assert got.shape == want.shape
    assert float(np.abs(got - want).max()) <= 1e-12


# mutant -> (case, norm kind, regime whose plan names the slabs): the case built for that fault
MUTANT_CASES = [
    ("drop_channel", "few_c201_o70/whole", "none"), ("drop_channel", "mfma_c201_o130_s2/whole", "instance_offset"),
    ("drop_tap", "mfma_c201_o130_s2/whole", "none"), ("drop_tap", "few_c68_s2", "batch"),
    ("shift", "few_c68_s2", "none"), ("shift", "mfma_c201_o130_s2/streamed", "instance"),
    ("drop_row", "few_rows17_d2", "none"), ("drop_row", "few_c201_o70/whole", "instance_offset"),
    ("drop_out_channel", "few_c201_o70/whole", "none"), ("drop_out_channel", "mfma_c201_o130_s2/whole", "batch"),
    ("unbiased_var", "norm_lanes/L65", "instance"), ("unbiased_var", "norm_lanes/L129", "instance_offset"),
    ("unbiased_var", "norm_lanes/L2", "instance_plain"),
    ("res_after_gelu", "block_one_sub", "batch"), ("res_after_gelu", "block_three_sub/final", "instance"),
    ("state_early", "few_c68_s2", "none"), ("state_early", "few_epilogue", "none"),
    ("skip_slab_8", "few_1x1_slabs/c520/plain", "none"), ("skip_slab_8", "few_1x1_slabs/c1028/final", "none"),
    ("skip_slab_8", "few_epilogue", "batch"),
]


@pytest.mark.parametrize("mutant,name,kind", MUTANT_CASES, ids=lambda v: v)
def test_the_bar_catches_each_mutant(mutant, name, kind):
    case, want, (b, _, _) = ec.prepared(name, kind)
    bad = ec.oracle(case, mutant)
    if mutant == "state_early":
        diff = max(float(np.abs(a - c).max()) for a, c in zip(bad.states, want.states) if a is not None)
        assert not any(np.array_equal(a, c) for a, c in zip(bad.states, want.states) if a is not None)
    else:
        diff = float(np.abs(bad.out - want.out).max())
    print(f"mutant {mutant} on {name} ({kind}): max difference {diff:.3e}, bar {b:.3e}")
    assert diff > 10.0 * b  # not a near miss


def test_every_mutant_has_a_case():
    assert {m for m, _, _ in MUTANT_CASES} == set(ec.MUTANTS)
