"""Shapes of the f16x2 live-tile-list tests (rnnt_amd/csrc/x2.hip: tile_list, k_x2_dead_rows, the reducers' tile flags) and what the
fp64 twin of the flush rule (tests/x2_flush_twin.py) says about them.  Shared by tests/test_x2_live_list_oracle.py (CPU: the shapes'
conditions) and tests/test_x2_live_list_gpu.py."""
import functools

import numpy as np

from tests.helpers import make_inputs
from tests.x2_flush_twin import CASES, live_fractions, twin

# (B, T, U, H, V, seed, ragged, grad_scale): the flush A/B cases (h640: the k_dhidden_x2r pass, h1024: a FIRST = false pass) and two
# whose T is no multiple of the tile's 8 rows and whose U + 1 is no multiple of its 16 columns
LIST_CASES = dict(CASES)
LIST_CASES["t357"] = (2, 357, 61, 128, 128, 31, True, 0.5)         # T % 8 = 5, U + 1 = 62
LIST_CASES["t203"] = (3, 203, 77, 128, 128, 33, True, 1.0 / 3.0)   # T % 8 = 3, U + 1 = 78
TINY = (2, 9, 4, 128, 128, 7, True, 0.5)  # nothing can be flushed


def inputs(case):
    B, T, U, H, V, seed, ragged, _ = case
    return make_inputs(B, T, U, H, V, seed, ragged=ragged)


def dead_rows_in_live_ksteps(tw):
    """Cells of dHidden tiles without a live cell that lie inside a live 16-cell dW k-step: the rows k_x2_dead_rows has to zero."""
    live = tw["inside"] & ~tw["flush"]
    B, T, U1 = live.shape
    ntt, nub = (T + 7) // 8, (U1 + 15) // 16
    pad = np.zeros((B, ntt * 8, nub * 16), dtype=bool)
    pad[:, :T, :U1] = live
    tiles = pad.reshape(B, ntt, 8, nub, 16).any(axis=(2, 4))
    cell_tile_dead = ~np.repeat(np.repeat(tiles, 8, axis=1), 16, axis=2)[:, :T, :U1]
    flat = live.reshape(-1)
    nks = (flat.size + 15) // 16
    fl = np.zeros(nks * 16, dtype=bool)
    fl[:flat.size] = flat
    ks_live = np.repeat(fl.reshape(nks, 16).any(axis=1), 16)[:flat.size]
    return int((cell_tile_dead.reshape(-1) & ks_live).sum())


@functools.lru_cache(maxsize=None)
def facts(name):
    """(live tiles, tiles, live k-steps, k-steps, dead-tile cells inside live k-steps) of a case, from the fp64 twin."""
    case = TINY if name == "tiny" else LIST_CASES[name]
    tw = twin(inputs(case), case[7])
    return live_fractions(tw) + (dead_rows_in_live_ksteps(tw),)
