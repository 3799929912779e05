"""The operand planes and W packs of the two split routes (bf16x3, f16x2) keep EVERY BIT of what the library wrote before the routes'
plain kernels — make-hidden, split-G, the forward and dHidden W packs, the padding zeroing — became one set of templates over a piece
format (rnnt_amd/csrc/split_common.hpp): per case, the stages up to dHidden run over a quiet-NaN workspace and the SHA-256 of the hidden
planes, both packs, the logits / G region, g_lo (bf16x3) and the two W scales (f16x2) must equal tests/golden/split_planes.npz (written
by tests/golden/make_golden_split_planes.py, which also holds the cases and the code that runs them).  Both routes x two shapes x the
default form (fused kernels write the planes, plain kernels the packs) and RNNT_VARIANT_X3_FP32_FWD | _DH (k_split_make_hidden and
k_split_g write the planes).  The GPU test is marked gpu; the tests of the recording itself need none."""
import importlib.util
import os

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_split_planes", os.path.join(_HERE, "golden", "make_golden_split_planes.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def engine():
    import torch

    import rnnt_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    rnnt_amd.engine.lib()
    return rnnt_amd.engine


@pytest.fixture(scope="module")
def golden():
    return np.load(G.GOLDEN)


def test_recording_covers_exactly_the_cases(golden):
    assert len(G.CASES) == 8
    assert {(r, s, v) for r, s, v in G.CASES.values()} == {(r, s, v) for r in ("bf16x3", "f16x2") for s in G.SHAPES for v in (0, 4096 | 8192)}
    assert sorted(golden.files) == sorted("%s/%s" % (name, k) for name, (route, _, _) in G.CASES.items() for k in G.REGIONS[route])


def test_shapes_cannot_skip_the_zero_fill_branches():
    assert G.SHAPES == [(2, 9, 6, 128, 128), (2, 9, 6, 640, 256)]
    for _, _, _, H, V in G.SHAPES:
        assert V % 512 != 0 and H % 512 != 0  # tiles past V in the forward pack, past H in the dHidden pack
        assert H % 128 == 0 and V % 128 == 0  # (what the routes take)
    assert G.SHAPES[1][3] > 512               # a second dHidden column pass


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(G.CASES))
def test_case_keeps_every_bit(engine, golden, name):
    for run in range(2):
        got = G.run_case(engine, name)
        assert sorted(got) == sorted(G.REGIONS[G.CASES[name][0]])
        for k, h in got.items():
            want = golden["%s/%s" % (name, k)]
            assert h.dtype == want.dtype and np.array_equal(h, want), "run %d: %s differs from the recorded bytes: %s != %s" % (run, k, h, want)
