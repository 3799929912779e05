"""-m gpu: the pass end of the f16x2 joint forward (k_joint_fwd_x2: unscale + bias, the logits stores, the rows' running
(max, sum exp) and what the tile's tail makes of them) keeps EVERY BIT of what the kernel left before its pass end was batched
over groups of row slots: the logits and the three per-cell outputs denom_s / lpb_s / lpe_s against bytes recorded from the
commit before (tests/golden/x2_fwd_pass_end.npz, written by tests/golden/make_golden_x2_fwd_pass_end.py, which also holds the
cases and the code that runs them), and — independently of that recording — against a float64 log-sum-exp of the stored
logits rows.  Cases: one column pass with one or both of a wave's 128-column groups, a partial second pass, three passes
(the running update more than once), cfg2's H and V, more tiles than CUs (a workgroup's second tile starts from fresh
statistics), a blank at 0 and inside the vocabulary, the exact tanh form (MODE 0), and the plain-GEMM form (MODE 2) through
engine.linear_fwd on the f16x2 kernels."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_x2_fwd_pass_end",
                                               os.path.join(_HERE, "golden", "make_golden_x2_fwd_pass_end.py"))
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


@pytest.mark.parametrize("name", list(G.JOINT_CASES))
def test_joint_forward_pass_end_keeps_every_bit(engine, golden, name):
    d, blank = G.joint_inputs(name)
    regions, logits = G.run_joint(engine, d, blank)
    # independent of the recording: the statistics against a float64 evaluation of the stored rows, 4x the recorded
    # library's own worst distance (fp32 roundings of exp2 / log and of the subtraction: ~1e-6)
    err = G.independent_error(d, blank, regions, logits)
    print("\n%s: max |stored - float64| %.3e (recorded worst %.3e)" % (name, err, float(golden["worst_err"])))
    assert err <= 4.0 * float(golden["worst_err"])
    # bit identity with the recording
    assert G.logits_sha256(logits) == str(golden["%s/logits_sha256" % name]), "logits differ from the recorded bytes"
    for r in G.REGIONS:
        want = golden["%s/%s" % (name, r)]
        diff = np.flatnonzero(regions[r] != want)
        assert diff.size == 0, "%s: %d of %d entries differ from the recorded bytes, first at %d: %08x != %08x" % (
            r, diff.size, want.size, diff[0], regions[r][diff[0]], want[diff[0]])


@pytest.mark.parametrize("name", list(G.LINEAR_CASES))
def test_linear_pass_end_keeps_every_bit(engine, golden, name):
    d = G.linear_inputs(name)
    y = G.run_linear(engine, d)
    err = G.linear_error(d, y)
    print("\n%s: max |y - float64| %.3e (recorded worst %.3e)" % (name, err, float(golden["worst_err_linear"])))
    assert err <= 4.0 * float(golden["worst_err_linear"])
    want = golden["%s/y" % name]
    assert y.shape == want.shape
    diff = np.flatnonzero(y.view(np.uint32).ravel() != want.ravel())
    assert diff.size == 0, "%d of %d entries of Y differ from the recorded bytes" % (diff.size, want.size)


def test_pass_end_is_reproducible(engine):
    """Three consecutive calls on the case with more tiles than CUs: identical bytes (which workgroup runs which tile, and as
    its first or a later one, changes from call to call)."""
    d, blank = G.joint_inputs("tiles282")
    runs = []
    for _ in range(3):
        regions, logits = G.run_joint(engine, d, blank)
        runs.append((regions, G.logits_sha256(logits)))
    for regions, sha in runs[1:]:
        assert sha == runs[0][1]
        for r in G.REGIONS:
            assert np.array_equal(regions[r], runs[0][0][r]), r
