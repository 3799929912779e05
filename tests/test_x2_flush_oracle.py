"""The f16x2 route's flush rule on the CPU, in fp64 (tests/x2_flush_twin.py): the bound is sound, a NaN flags nothing, and
the shapes the GPU A/B cases use (tests/test_x2_flush_skip_gpu.py) leave at least a quarter of the dHidden tiles dead."""
import numpy as np
import pytest

from tests.helpers import make_inputs
from tests.x2_flush_twin import CASES, g_scale_log2, live_fractions, twin


def test_g_scale_matches_the_host_rule():
    # engine.hip: frexpf(grad_scale) = m 2^e, m in [0.5, 1) -> g_scale = 2^(13 - e); the benchmark's 1/32 gives 2^17
    assert g_scale_log2(1.0 / 32.0) == 17
    assert [g_scale_log2(g) for g in (0.5, 1.0 / 3.0, 1.0, 0.125)] == [13, 14, 12, 15]


def test_twin_lattice_is_consistent():
    d = make_inputs(2, 40, 11, 128, 128, seed=3)
    tw = twin(d, 0.5)
    for b in range(2):
        Tb, Ub = int(d["logit_lens"][b]), int(d["target_lens"][b])
        end = tw["alpha"][b, Tb - 1, Ub] + tw["logp"][b, Tb - 1, Ub, -1]
        assert abs(end + tw["costs"][b]) < 1e-9 and abs(tw["beta"][b, 0, 0] + tw["costs"][b]) < 1e-9
        # occupancies of the arcs out of a node add up to the node's
        a = tw["s1"][b, :Tb, :Ub + 1]
        node = 2.0 ** a
        assert np.allclose(tw["sbse"][b, :Tb, :Ub + 1], node, rtol=1e-9, atol=1e-300)


@pytest.mark.parametrize("grad_scale", [1.0 / 32.0, 0.5, 1.0])
def test_flushed_cells_have_zero_planes_in_fp64(grad_scale):
    """Every entry of g_scale G of a flagged cell lies below 2^-26: fp16's round-to-nearest-even makes both pieces +-0."""
    d = make_inputs(2, 200, 50, 128, 128, seed=5, ragged=True)
    tw = twin(d, grad_scale)
    assert tw["flush"].any()
    B, T, U1, V = tw["logp"].shape
    gs = 2.0 ** tw["k"]
    worst = 0.0
    for b, t, u in zip(*np.nonzero(tw["flush"])):
        g = 2.0 ** tw["s1"][b, t, u] * np.exp(tw["logp"][b, t, u])  # grad_scale gamma p_v
        g[V - 1] -= tw["sb"][b, t, u]
        if u < int(d["target_lens"][b]):
            g[int(d["targets"][b, u])] -= tw["se"][b, t, u]
        worst = max(worst, float(np.abs(g).max()) * gs)
    assert worst < 2.0 ** -26
    # and the flagged cells lie inside the set the GPU test compares the device's flags with
    assert not (tw["flush"] & ~tw["gamma_small"]).any()


def test_nan_flags_nothing_in_its_utterance():
    d = make_inputs(2, 120, 40, 128, 128, seed=6, ragged=False)
    d["enc"][1, 3, 5] = np.nan
    tw = twin(d, 0.5)
    assert np.isnan(tw["costs"][1]) and not tw["flush"][1].any()
    assert np.isfinite(tw["costs"][0]) and tw["flush"][0].any()


def test_tiny_lattice_has_no_flushed_cell():
    tw = twin(make_inputs(2, 9, 4, 128, 128, seed=7), 0.5)
    assert not tw["flush"].any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_cases_leave_a_quarter_of_the_tiles_dead(name):
    B, T, U, H, V, seed, ragged, gs = CASES[name]
    tw = twin(make_inputs(B, T, U, H, V, seed, ragged=ragged), gs)
    lt, nt, lk, nk = live_fractions(tw)
    print(f"{name}: live tiles {lt}/{nt}, live k-steps {lk}/{nk}")
    assert nt - lt >= 0.25 * nt
