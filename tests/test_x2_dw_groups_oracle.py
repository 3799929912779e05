"""The shapes of tests/test_x2_dw_groups_gpu.py on the CPU, by the fp64 twin of the f16x2 flush rule: on each the 4-cell groups list fewer
rows than the 16-cell k-steps do, rows of dead dHidden tiles lie inside live groups (k_x2_dead_rows has work), and among them are a cell
count and a live-group count that are no multiple of 4 (a partly filled last group, a last k-step filled up with padding entries).  The
shapes' conditions, not a measurement."""
import pytest

from tests.x2_dw_group_cases import cells, group_facts
from tests.x2_live_list_cases import LIST_CASES, facts

NAMES = sorted(LIST_CASES)


@pytest.mark.parametrize("name", NAMES)
def test_groups_list_fewer_rows_than_ksteps_and_hold_dead_tile_rows(name):
    lg, ng, must, rows = group_facts(name)
    _, _, lk, nk, rows16 = facts(name)
    print(f"{name}: cells {cells(name)}, live groups {lg}/{ng} (must-live {must}), live k-steps {lk}/{nk}, "
          f"groups / (4 k-steps) {lg / (4.0 * lk):.3f}, dead-tile rows in live groups {rows} (in live k-steps {rows16})")
    assert ng == (cells(name) + 3) // 4
    assert must <= lg < 4 * lk
    assert 1 <= rows <= rows16


def test_some_cell_count_and_some_live_group_count_are_no_multiple_of_4():
    assert any(cells(n) % 4 for n in NAMES)
    assert any(group_facts(n)[0] % 4 for n in NAMES)


def test_tiny_has_fewer_ksteps_than_splits():
    """Nothing can be flushed on `tiny`: its live groups are the groups inside the lengths, its k-steps fewer than the dW GEMM's splits."""
    import os

    from rnnt_amd import engine
    from tests.x2_live_list_cases import TINY
    lg, ng, must, _ = group_facts("tiny")
    B, T, U, H, V = TINY[:5]
    assert lg == must and cells("tiny") % 4 and lg % 4
    if not os.path.exists(engine.LIB_PATH):  # (as tests/test_abi.py: the layout query needs no GPU)
        engine.build()
    assert (lg + 3) // 4 < engine.layout(B, T, U + 1, H, V, "f16x2").n_split
