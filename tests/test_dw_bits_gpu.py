"""The dW GEMMs of the bf16 and bf16x3 routes (k_dw_bf16, k_dw_x3) keep EVERY BIT of what the library wrote before their tile decode,
operand sources, prologue DMA, fragment addressing, k-step pieces, live-range walk and slab store became one toolkit shared with the
f16x2 dW kernels (rnnt_amd/csrc/split_dw.hpp): per case, the SHA-256 of the split-K slabs of dW and db after the stages up to dW over a
quiet-NaN workspace, and the costs and the SHA-256 of the four gradients of the whole call, must equal tests/golden/dw_bits.npz (written
by tests/golden/make_golden_dw_bits.py, which also holds the cases and the code that runs them).  The host-only tests recompute
k_dw_table and the splits' shares and hold every case to what it is there for: splits of two live ranges with and without a gap, walks
longer than either ring, a lockstep that is on, empty shares, the block counts."""
import importlib.util
import os

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_dw_bits", os.path.join(_HERE, "golden", "make_golden_dw_bits.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

RING_STAGES = {"bf16": (4, 1), "bf16x3": (3, 2)}  # route -> (ring depth, ring stages per 32-cell granule)


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


def _walk(shape):
    B, T, U, H, V = shape
    lens = G.case_inputs("bf16_" + "x".join(map(str, shape)))["logit_lens"]
    n_split = G.dw_splits(B, T, H, V)
    return lens, n_split, G.split_ranges(lens, T, U + 1, n_split)


def test_recording_covers_exactly_the_cases(golden):
    shapes = [(3, 4, 95, 128, 128), (1, 2, 191, 512, 512), (2, 9, 6, 640, 384)]
    assert {(r, tuple(s), seed) for r, s, seed in G.CASES.values()} == {(r, s, sum(s)) for r in ("bf16", "bf16x3") for s in shapes}
    assert len(G.CASES) == 6
    assert sorted(golden.files) == sorted("%s/%s" % (name, k) for name in G.CASES for k in G.keys(name))
    for route, s, _ in G.CASES.values():  # both routes get the same inputs
        assert np.array_equal(G.case_inputs("%s_%s" % (route, "x".join(map(str, s))))["logit_lens"], _walk(s)[0])


def test_two_range_splits_touching_and_with_a_gap():
    shape = (3, 4, 95, 128, 128)
    lens, n_split, walk = _walk(shape)
    assert list(lens) == [4, 3, 2]  # stated by the case, not drawn
    assert G.dw_blocks(shape[3], shape[4]) == (1, 1) and n_split == 12  # one tile: min(256, B T) splits; one h block: two db tiles per wave (bf16x3)
    assert shape[4] < 256  # the v block is half empty
    first, before, nlive = G.dw_table(lens, shape[1], shape[2] + 1)
    assert (first, before, nlive) == ([0, 12, 24], [0, 12, 21], 27)  # 12 + 9 + 6 granules of 32 cells
    assert walk[5] == [(11, 1), (12, 1)]  # utterance 0's last granule and utterance 1's first: two ranges that touch
    assert walk[9] == [(20, 1), (24, 1)]  # utterance 1's last and utterance 2's first: granules 21, 22, 23 are dead
    for s, runs in enumerate(walk):
        if s not in (5, 9):
            assert len(runs) == 1 and 2 <= runs[0][1] <= 3, (s, runs)
    assert sum(n for runs in walk for _, n in runs) == nlive
    # 4-6 k-steps on bf16x3: more than its 3-stage ring
    assert all(RING_STAGES["bf16x3"][1] * runs[0][1] > RING_STAGES["bf16x3"][0] for s, runs in enumerate(walk) if s not in (5, 9))


def test_walk_longer_than_either_ring_with_the_lockstep_on():
    shape = (1, 2, 191, 512, 512)
    lens, n_split, walk = _walk(shape)
    n_vblk, n_hblk = G.dw_blocks(shape[3], shape[4])
    assert (n_vblk, n_hblk) == (2, 2) and n_split == 2
    assert 1 < n_vblk * n_hblk <= 16  # k_dw_bf16's lockstep is on
    assert walk == [[(0, 6)], [(6, 6)]]
    for route, (depth, per_granule) in RING_STAGES.items():
        assert per_granule * 6 > depth, route  # 6 stages on bf16, 12 k-steps on bf16x3
    assert n_hblk >= 2  # db comes from h blocks 0 and 1


def test_empty_shares_and_half_empty_blocks():
    shape = (2, 9, 6, 640, 384)
    lens, n_split, walk = _walk(shape)
    n_vblk, n_hblk = G.dw_blocks(shape[3], shape[4])
    assert (n_vblk, n_hblk) == (2, 3) and n_split == 18
    assert shape[3] % 256 == 128 and shape[4] % 256 == 128  # the last h block and the second v block are half empty; h block 2 carries no db
    nlive = G.dw_table(lens, shape[1], shape[2] + 1)[2]
    assert 1 <= nlive <= 4
    assert sum(1 for runs in walk if not runs) == n_split - nlive >= 14  # most shares are empty: their slabs must still hold zeros
    assert sum(n for runs in walk for _, n in runs) == nlive


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(G.CASES))
def test_case_keeps_every_bit(engine, golden, name):
    for run in range(2):
        got = G.run_case(engine, name)
        assert sorted(got) == sorted(G.keys(name))
        for k, h in got.items():
            want = golden["%s/%s" % (name, k)]
            assert h.dtype == want.dtype and np.array_equal(h, want), "run %d: %s differs from the recorded bytes: %s != %s" % (run, k, h, want)
