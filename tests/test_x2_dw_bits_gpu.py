"""The f16x2 dW GEMM keeps EVERY BIT of dW and db (and of the step's other outputs) that the library left before k_dw_x2<4>,
k_dw_x2<4, true> and k_dw_x2m were rebuilt from one set of k-step pipeline pieces (now rnnt_amd/csrc/split_dw.hpp, the dW tile toolkit: dw_kstep2, dw_ring):
SHA-256 against tests/golden/x2_dw.npz, written by tests/golden/make_golden_x2_dw.py, which also holds the cases, what each one
reaches and the code that runs them.  The route is bitwise reproducible (tests/test_x2_dw_groups_gpu.py), so the bar is equality.
tests/test_fused_routes_bits_gpu.py pins one small shape per kernel form; the cases here add several h blocks, empty split shares,
walks longer than the ring, the walk without the flush rule and the Linear layer's lists."""
import importlib.util
import os

import numpy as np
import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_x2_dw", os.path.join(_HERE, "golden", "make_golden_x2_dw.py"))
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
    for name, (kind, _, _, _) in G.CASES.items():
        keys = ("costs",) + G.GRADS if kind == "fused" else G.LINEAR_OUT
        assert sorted(k.split("/", 1)[1] for k in golden.files if k.startswith(name + "/")) == sorted(keys)


@pytest.mark.parametrize("name", list(G.CASES))
def test_case_reaches_its_kernel_form(name):
    """Host code only: launch_dw_x2's choice for the case's (H, V), and the library's tile count behind it.  The Linear layer at
    (M, K, N) = (70, 640, 512) does reach k_dw_x2m (H = K = 640, V = N = 512)."""
    from rnnt_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build()
    G.check_form(engine.lib(), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(G.CASES))
def test_case_keeps_every_bit(engine, golden, name):
    first = G.F.recorded(G.run_case(engine, name))
    second = G.F.recorded(G.run_case(engine, name))
    for k, got in first.items():
        want = golden["%s/%s" % (name, k)]
        assert got.dtype == want.dtype and got.shape == want.shape, k
        assert np.array_equal(got, want), "%s differs from the recorded bytes: %s != %s" % (k, got, want)
        assert np.array_equal(second[k], got), "%s: a second call gives other bytes" % k


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["wrap_whole", "wrap_parth", "wrap_mixed"])
def test_wrap_cases_walk_round_the_ring(engine, name):
    """At most B T = 2 splits over 256 cells: the k-steps the kernel walks (k_dw_x2m: the live 16-cell k-steps, k_dw_x2: four live
    groups each), shared among the splits, are more than the ring's four stages."""
    B, T, U, H, V = G.CASES[name][1]
    assert B * T == 2 and B * T * (U + 1) == 256
    G.run_case(engine, name)
    dev = torch.device("cuda:0")
    if G.CASES[name][3] == G.MIXED:
        walked = engine.x2_live_counts(dev, B, T, U + 1, H, V)["live_ksteps"]
    else:
        walked = -(-engine.x2_live_group_counts(dev, B, T, U + 1, H, V)["live_groups"] // 4)
    n_split = engine.layout(B, T, U + 1, H, V, "f16x2").n_split
    assert n_split <= 2 and -(-walked // n_split) > 4, (walked, n_split)
