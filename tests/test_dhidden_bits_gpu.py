"""The dHidden kernels of the two split routes (k_dhidden_x3<FIRST>; k_dhidden_x2<FIRST, PART>, k_dhidden_x2r) keep EVERY BIT of what the
library wrote before their producer set-up, G production, whole-line store addressing and epilogue became one toolkit over the piece
format (rnnt_amd/csrc/split_dhidden.hpp): per case, the SHA-256 of G's planes after the stages up to dHidden over a quiet-NaN workspace,
and the costs and the SHA-256 of the four gradients of the whole call, must equal tests/golden/dhidden_bits.npz (written by
tests/golden/make_golden_dhidden_bits.py, which also holds the cases and the code that runs them).  The cases reach every kernel form,
a second u block, k_dhidden_x2r at hp = 2, dead tiles and bf16x3's zero-fill branch; the tests of the case list need no GPU."""
import importlib.util
import os

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_dhidden_bits", os.path.join(_HERE, "golden", "make_golden_dhidden_bits.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

# case -> the kernel forms its H reaches, in launch order
FORMS = {
    "f16x2_2x9x17x768x128": ["k_dhidden_x2<true, false>", "k_dhidden_x2<false, true>"],
    "f16x2_2x9x17x1152x128": ["k_dhidden_x2<true, false>", "k_dhidden_x2<false, false>", "k_dhidden_x2r@hp=2"],
    "f16x2_2x9x17x640x128": ["k_dhidden_x2<true, false>", "k_dhidden_x2r@hp=1"],
    "f16x2_tiny_dead_tiles": ["k_dhidden_x2<true, true>"],
    "bf16x3_2x9x17x128x128": ["k_dhidden_x3<true>"],
    "bf16x3_2x9x17x1024x128": ["k_dhidden_x3<true>", "k_dhidden_x3<false>"],
    "bf16x3_2x17x6x640x128": ["k_dhidden_x3<true>", "k_dhidden_x3<false>"],
}


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
    from tests.x2_live_list_cases import TINY
    shapes = [("f16x2", (2, 9, 17, 768, 128)), ("f16x2", (2, 9, 17, 1152, 128)), ("f16x2", (2, 9, 17, 640, 128)),
              ("bf16x3", (2, 9, 17, 128, 128)), ("bf16x3", (2, 9, 17, 1024, 128)), ("bf16x3", (2, 17, 6, 640, 128))]
    assert {(r, tuple(s), seed) for r, s, seed in G.CASES.values()} == {(r, s, sum(s)) for r, s in shapes} | {("f16x2", tuple(TINY[:5]), TINY[5])}
    assert len(G.CASES) == 7
    assert sorted(golden.files) == sorted("%s/%s" % (name, k) for name in G.CASES for k in G.keys(name))


def test_cases_reach_every_kernel_form():
    assert sorted(FORMS) == sorted(G.CASES)
    for name, (route, (B, T, U, H, V), _) in G.CASES.items():
        assert G.kernel_forms(route, H) == FORMS[name], name
        assert H % 128 == 0 and V % 128 == 0  # (what the routes take)
    reached = {f.split("@")[0] for forms in FORMS.values() for f in forms}
    assert reached == {"k_dhidden_x3<true>", "k_dhidden_x3<false>", "k_dhidden_x2<true, true>", "k_dhidden_x2<true, false>",
                       "k_dhidden_x2<false, true>", "k_dhidden_x2<false, false>", "k_dhidden_x2r"}
    assert "k_dhidden_x2r@hp=2" in FORMS["f16x2_2x9x17x1152x128"]


def test_shapes_hold_the_tile_edges():
    two_u_blocks = [s for _, s, _ in G.CASES.values() if 16 < s[2] + 1 <= 32]
    assert len(two_u_blocks) == 5 and all((s[2] + 1) % 16 == 2 for s in two_u_blocks)  # the second u block: 2 of 16 columns
    assert {r for r, s, _ in G.CASES.values() if 16 < s[2] + 1} == {"f16x2", "bf16x3"}
    assert any(r == "f16x2" and s[3] % 512 == 128 and s[2] + 1 > 16 for r, s, _ in G.CASES.values())  # k_dhidden_x2r with two u blocks
    # bf16x3's zero-fill branch: three t tiles, the last with one row, and an utterance whose length ends before the last tile
    route, (B, T, U, H, V), seed = G.CASES["bf16x3_2x17x6x640x128"]
    assert (T + 7) // 8 == 3 and T % 8 == 1
    from tests.helpers import make_inputs
    lens = make_inputs(B, T, U, H, V, seed=seed, ragged=True)["logit_lens"]
    assert lens.min() <= 16 and lens.min() % 8 != 0 and lens.max() == T


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(G.CASES))
def test_case_keeps_every_bit(engine, golden, name):
    for run in range(2):
        got = G.run_case(engine, name)
        assert sorted(got) == sorted(G.keys(name))
        for k, h in got.items():
            want = golden["%s/%s" % (name, k)]
            assert h.dtype == want.dtype and np.array_equal(h, want), "run %d: %s differs from the recorded bytes: %s != %s" % (run, k, h, want)
