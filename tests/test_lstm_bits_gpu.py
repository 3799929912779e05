"""rnnt_amd/csrc/lstm.hip keeps EVERY BIT it left before its copies were put on shared pieces — one LSTM cell body, one scratch
layout, shared argument checks: the predictor's forward (with and without `saved`)
and backward, the greedy loop, the device streams and the beam search's predictor step, at the shapes of the existing case lists.
Tokens, state words and scores raw, every float buffer and the calls' whole workspaces and blocks as SHA-256, against
tests/golden/lstm_bits.npz, written by tests/golden/make_golden_lstm_bits.py, which also holds the cases and the code that runs
them.  Every path is a fixed kernel sequence with fixed summation orders, so the bar is equality."""
import importlib.util
import os

import numpy as np
import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_lstm_bits", os.path.join(_HERE, "golden", "make_golden_lstm_bits.py"))
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


def test_recording_covers_the_cases(golden):
    assert {k.rsplit("/", 1)[0] for k in golden.files} == set(G.CASES)


def test_the_cases_are_the_case_lists():
    """Host code only: every edge of the predictor's list, the decode widths and the wiring case, by name."""
    from tests import lstm_decode_cases as dc
    from tests import lstm_predictor_cases as lc
    assert {n.split("/", 1)[1] for n in G.CASES if n.startswith("pred/")} == {e.name for e in lc.EDGES}
    assert {n.split("/", 1)[1] for n in G.CASES if n.startswith("greedy/")} == {c.name for c in dc.WIDTHS + [dc.WIRING_TEXT]} | {"batch_n3", "batch_n32"}
    assert all(what == "batch" or what in dc.BY_NAME or what in G.EDGES for _, what, _ in G.CASES.values())


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
