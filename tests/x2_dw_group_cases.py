"""What the fp64 twin of the flush rule (tests/x2_flush_twin.py) says about the 4-cell groups of the f16x2 dW GEMM's walk
(rnnt_amd/csrc/x2.hip: grp_list, k_dw_x2, k_x2_dead_rows) on the shapes of tests/x2_live_list_cases.py.  A group is four consecutive
cells of the linear cell order [b][t][u]; four list entries make one k-step.  Shared by tests/test_x2_dw_groups_oracle.py (CPU: the
shapes' conditions) and tests/test_x2_dw_groups_gpu.py."""
import functools

import numpy as np

from tests.x2_flush_twin import twin
from tests.x2_live_list_cases import LIST_CASES, TINY, inputs


def _groups_of(flat):
    """Per group: any of its (up to four) cells is set."""
    n = (flat.size + 3) // 4
    f = np.zeros(n * 4, dtype=bool)
    f[:flat.size] = flat
    return f.reshape(n, 4).any(axis=1)


def group_facts_of(tw):
    """(live groups, groups, must-live groups, dead-tile rows inside live groups).  live = inside and not flushed; a group must be live
    when it holds a cell of inside & ~gamma_small (the set the device may never flag); the rows k_x2_dead_rows has to zero are the cells
    of dHidden tiles (8 t x 16 u) without a live cell that lie inside a live group."""
    live = tw["inside"] & ~tw["flush"]
    B, T, U1 = live.shape
    ntt, nub = (T + 7) // 8, (U1 + 15) // 16
    pad = np.zeros((B, ntt * 8, nub * 16), dtype=bool)
    pad[:, :T, :U1] = live
    tiles = pad.reshape(B, ntt, 8, nub, 16).any(axis=(2, 4))
    cell_tile_dead = ~np.repeat(np.repeat(tiles, 8, axis=1), 16, axis=2)[:, :T, :U1]
    grp = _groups_of(live.reshape(-1))
    must = _groups_of((tw["inside"] & ~tw["gamma_small"]).reshape(-1))
    in_live_group = np.repeat(grp, 4)[:live.size]
    return int(grp.sum()), int(grp.size), int(must.sum()), int((cell_tile_dead.reshape(-1) & in_live_group).sum())


@functools.lru_cache(maxsize=None)
def group_facts(name):
    case = TINY if name == "tiny" else LIST_CASES[name]
    return group_facts_of(twin(inputs(case), case[7]))


def cells(name):
    B, T, U = (TINY if name == "tiny" else LIST_CASES[name])[:3]
    return B * T * (U + 1)
