"""The shapes of tests/test_x2_live_list_gpu.py on the CPU, by the fp64 twin of the f16x2 flush rule: each leaves at least a quarter of
the dHidden tiles dead — work for the live-tile list — and leaves cells of dead tiles inside live 16-cell dW k-steps — work for
k_x2_dead_rows.  The shapes' condition, not a measurement."""
import pytest

from tests.x2_live_list_cases import LIST_CASES, facts


@pytest.mark.parametrize("name", sorted(LIST_CASES))
def test_cases_leave_dead_tiles_and_dead_rows_in_live_ksteps(name):
    lt, nt, lk, nk, rows = facts(name)
    print(f"{name}: live tiles {lt}/{nt}, live k-steps {lk}/{nk}, dead-tile cells in live k-steps {rows}")
    assert nt - lt >= 0.25 * nt
    assert rows > 0


def test_new_shapes_miss_the_tile_sizes():
    for name in ("t357", "t203"):
        B, T, U, H, V, seed, ragged, gs = LIST_CASES[name]
        assert T % 8 != 0 and (U + 1) % 16 != 0 and ragged and B > 1


def test_tiny_lattice_keeps_every_tile_inside_the_lengths():
    lt, nt, lk, nk, rows = facts("tiny")
    assert lt > 0 and lk > 0
