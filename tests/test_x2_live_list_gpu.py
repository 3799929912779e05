"""-m gpu: the f16x2 backward over its live-tile list (rnnt_amd/csrc/x2.hip "flush rule": tile_list, k_x2_dead_rows; joint_bwd.hip: the
reducers' tile flags).  k_dhidden_x2 runs the listed tiles only; a tile that is not listed writes no slab piece and no G row, so
  * the reducers must not read a dead tile's slab piece,
  * k_x2_dead_rows must zero every row of a dead tile that a live dW k-step reads,
  * no workgroup may read a list entry past the count:
each would show as a result that depends on what the workspace held before the call (0xFF bytes against zeros), or that differs from
RNNT_VARIANT_X2_NO_FLUSH_SKIP, from a second call, or from the same call cut into two at the dHidden stage.
The shapes (tests/x2_live_list_cases.py) are checked on the CPU (tests/test_x2_live_list_oracle.py) to leave >= 25 % of the tiles dead and
cells of dead tiles inside live k-steps."""
import pytest
import torch

from tests.helpers import oracle_fused
from tests.test_gpu_parity import _compare, _dev, _run_fused
from tests.x2_live_list_cases import LIST_CASES, TINY, facts, inputs

pytestmark = pytest.mark.gpu
X2 = "f16x2"
NAMES = sorted(LIST_CASES)
OUT = ("costs", "grad_enc", "grad_pred", "grad_W", "grad_bias")


@pytest.fixture(scope="module")
def e():
    import rnnt_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    rnnt_amd.engine.lib()
    return rnnt_amd.engine


def _run(e, g, V, gs, dtype=X2, variant=0, stage_mask=None, outs=None):
    outs = e.joint_loss_fwd_bwd(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"],
                                V - 1, gs, outs, dtype=dtype, variant=variant, stage_mask=stage_mask)
    torch.cuda.synchronize()
    return outs


def _counts(e, g, V):
    B, T, H = g["enc"].shape
    return e.x2_live_counts(g["enc"].device, B, T, g["pred"].shape[1], H, V)


def _fill_workspace(e, g, V, byte):
    """The whole workspace of the next f16x2 call of this shape (engine.workspace: one grow-only buffer per stream) filled with `byte`."""
    B, T, H = g["enc"].shape
    ws = e.workspace(g["enc"].device, e.layout(B, T, g["pred"].shape[1], H, V, X2).total)
    ws.fill_(byte)
    torch.cuda.synchronize()


def _assert_same(a, b, what):
    for k, x, y in zip(OUT, a, b):
        assert torch.equal(x, y), f"{what}: {k}"


_base = {}


def _case(e, name):
    """Inputs on the device, one whole default call and its device counts: computed once per case, never changed afterwards."""
    if name not in _base:
        case = LIST_CASES[name]
        g = _dev(inputs(case))
        outs = _run(e, g, case[4], case[7])
        _base[name] = (g, outs, _counts(e, g, case[4]))
    return _base[name]


@pytest.mark.parametrize("name", NAMES)
def test_result_does_not_depend_on_what_the_workspace_held(e, name):
    V, gs = LIST_CASES[name][4], LIST_CASES[name][7]
    g, base, _ = _case(e, name)
    _fill_workspace(e, g, V, 0xFF)
    poisoned = _run(e, g, V, gs)
    _fill_workspace(e, g, V, 0)
    zeroed = _run(e, g, V, gs)
    for o in poisoned:
        assert bool(torch.isfinite(o).all())
    _assert_same(poisoned, zeroed, "0xFF workspace against zeroed workspace")
    _assert_same(poisoned, base, "0xFF workspace against the first call")


@pytest.mark.parametrize("name", NAMES)
def test_list_is_exact_beside_the_variant(e, name):
    """costs / grad_enc / grad_pred: torch.equal.  grad_W / grad_bias: the existing bound (tests/test_x2_flush_skip_gpu.py),
    max |default - variant| <= max |variant - fp32 route|."""
    V, gs = LIST_CASES[name][4], LIST_CASES[name][7]
    g, new, c = _case(e, name)
    ref = _run(e, g, V, gs, variant=e.VARIANT_X2_NO_FLUSH_SKIP)
    cn = _counts(e, g, V)
    f32 = _run(e, g, V, gs, dtype="fp32")
    for k, a, b in zip(OUT[:3], new[:3], ref[:3]):
        assert torch.equal(a, b), k
    for k, a, b, x in zip(OUT[3:], new[3:], ref[3:], f32[3:]):
        diff, bound = float((a - b).abs().max()), float((b - x).abs().max())
        print(f"{name}: {k}: |default - variant| max {diff:.3e}, |variant - fp32 route| max {bound:.3e}")
        assert diff <= bound, k
    # counts: unchanged in meaning (the list's length is live_tiles); the twin's tile and k-step totals, >= 25 % of the tiles dead
    lt, nt, lk, nk, rows = facts(name)
    print(f"{name}: device counts {c}, with the variant bit {cn}; fp64 twin: live tiles {lt}/{nt}, dead-tile rows in live k-steps {rows}")
    assert c["tiles"] == cn["tiles"] == nt and c["ksteps"] == cn["ksteps"] == nk
    assert c["live_tiles"] < cn["live_tiles"] <= nt
    assert c["tiles"] - c["live_tiles"] >= 0.25 * c["tiles"]


@pytest.mark.parametrize("name", NAMES)
def test_stages_alone_and_repeat(e, name):
    """Stages up to dHidden (mask 31: k_x2_dead_rows and the list-indexed kernel) in one call, the reductions and dW (0xE0) in a
    second: bit-identical to one whole call; and a second whole call is bit-identical to the first."""
    V, gs = LIST_CASES[name][4], LIST_CASES[name][7]
    g, base, _ = _case(e, name)
    outs = e.alloc_fused_outputs(g["enc"], g["pred"], g["W"])
    for o in outs:
        o.fill_(float("nan"))
    _run(e, g, V, gs, stage_mask=31, outs=outs)
    _run(e, g, V, gs, stage_mask=0xE0, outs=outs)
    _assert_same(outs, base, "stage masks 31 + 0xE0 against one call")
    _assert_same(_run(e, g, V, gs), base, "second call against the first")


def test_lattice_too_small_to_flush_lists_every_tile_inside_the_lengths(e):
    B, T, U, H, V, seed, ragged, gs = TINY
    d = inputs(TINY)
    g = _dev(d)
    ref = _run(e, g, V, gs, variant=e.VARIANT_X2_NO_FLUSH_SKIP)
    cn = _counts(e, g, V)
    _fill_workspace(e, g, V, 0xFF)
    new = _run(e, g, V, gs)
    c = _counts(e, g, V)
    _assert_same(new, ref, "default against the variant")
    by_length = sum(((int(tb) + 7) // 8) * (int(ub) // 16 + 1) for tb, ub in zip(d["logit_lens"], d["target_lens"]))
    assert c == cn and c["live_tiles"] == by_length and c["live_tiles"] == facts("tiny")[0]


@pytest.mark.parametrize("route", ["bf16x3", "fp32"])
def test_routes_with_a_null_flag_pointer_keep_their_bar(route):
    """The reducers are shared: bf16x3 and fp32 hand them no tile flags and must sum every slab piece inside the lengths, as before."""
    import rnnt_amd
    d = inputs(LIST_CASES["t203"])
    _compare(_run_fused(rnnt_amd, d, route), oracle_fused(d))
