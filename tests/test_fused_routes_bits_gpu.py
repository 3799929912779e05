"""-m gpu: every route of the fused joint+loss step, and the standalone joint / loss / alignment entries, leave EVERY BIT of what the
library left before the host sequencing of rnnt_amd/csrc/engine.hip was split into one function per route (validation, one call
context, fp32 / bf16 / bf16x3 / f16x2 stage lists, one map of each workspace): costs, scores and frames raw and a SHA-256 of every
gradient against tests/golden/fused_routes.npz (written by tests/golden/make_golden_fused_routes.py, which also holds the cases and
the code that runs them).  The whole workspace holds a quiet-NaN pattern before each call, so a carve that moved reads poison; a
second call must give the same bytes; the eight stages run one at a time must give the whole call's."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_fused_routes", os.path.join(_HERE, "golden", "make_golden_fused_routes.py"))
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
    assert {k.split("/")[0] for k in golden.files} == set(G.CASES)


@pytest.mark.parametrize("name", list(G.CASES))
def test_case_keeps_every_bit(engine, golden, name):
    first = G.recorded(G.run_case(engine, name))
    second = G.recorded(G.run_case(engine, name))
    assert sorted(first) == sorted(k.split("/", 1)[1] for k in golden.files if k.startswith(name + "/"))
    for k, got in first.items():
        want = golden["%s/%s" % (name, k)]
        assert got.dtype == want.dtype and got.shape == want.shape, k
        assert np.array_equal(got, want), "%s differs from the recorded bytes: %s != %s" % (k, got, want)
        assert np.array_equal(second[k], got), "%s: a second call gives other bytes" % k


@pytest.mark.parametrize("stages", list(G.WHOLE_CALL_OF))
def test_stage_by_stage_recording_is_the_whole_calls(golden, stages):
    for k in ("costs",) + G.GRADS:
        assert np.array_equal(golden["%s/%s" % (stages, k)], golden["%s/%s" % (G.WHOLE_CALL_OF[stages], k)]), k
