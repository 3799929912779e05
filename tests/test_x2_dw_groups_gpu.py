"""-m gpu: the f16x2 dW GEMM over its list of live 4-cell groups (rnnt_amd/csrc/x2.hip: grp_list, k_dw_x2, k_x2_dead_rows; the k-step pipeline: split_dw.hpp).  A k-step of
k_dw_x2 multiplies the 16 rows of four list entries, each DMA piece reads the four rows of one entry through a raw buffer of its own, and
the last k-step of the list is filled up with padding entries.  What could go wrong shows as
  * a count that disagrees with the fp64 twin's bounds or with the k-step / tile counts (which keep their meaning),
  * a result that differs from RNNT_VARIANT_X2_NO_FLUSH_SKIP (costs / grad_enc / grad_pred: any bit; grad_W / grad_bias: beyond the
    existing bound max |default - variant| <= max |variant - fp32 route|),
  * a result that depends on what the workspace held (the ring's read-ahead, the padding entries, a dead-tile row left unzeroed),
  * a result that differs between two calls, or between one call and the same call cut into two at the dHidden stage.
The shapes (tests/x2_live_list_cases.py) are checked on the CPU by tests/test_x2_dw_groups_oracle.py."""
import pytest
import torch

from tests.helpers import assert_close_grad
from tests.test_gpu_parity import _dev
from tests.x2_dw_group_cases import cells, group_facts
from tests.x2_live_list_cases import LIST_CASES, TINY, facts, inputs

pytestmark = pytest.mark.gpu
X2 = "f16x2"
CASES = dict(LIST_CASES, tiny=TINY)
NAMES = sorted(CASES)
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
    args = (g["enc"].device, B, T, g["pred"].shape[1], H, V)
    return dict(e.x2_live_counts(*args), **e.x2_live_group_counts(*args))


def _fill_workspace(e, g, V, byte):
    B, T, H = g["enc"].shape
    ws = e.workspace(g["enc"].device, e.layout(B, T, g["pred"].shape[1], H, V, X2).total)
    ws.fill_(byte)
    torch.cuda.synchronize()


def _assert_same(a, b, what):
    for k, x, y in zip(OUT, a, b):
        assert torch.equal(x, y), f"{what}: {k}"


_base = {}


def _case(e, name):
    """Inputs on the device, one whole default call and its device counts, then the NO_FLUSH_SKIP variant's results and counts and the
    fp32 route's results: computed once per case, never changed afterwards."""
    if name not in _base:
        case = CASES[name]
        g = _dev(inputs(case))
        V, gs = case[4], case[7]
        outs = _run(e, g, V, gs)
        c = _counts(e, g, V)
        ref = _run(e, g, V, gs, variant=e.VARIANT_X2_NO_FLUSH_SKIP)
        cn = _counts(e, g, V)
        f32 = _run(e, g, V, gs, dtype="fp32")
        _base[name] = (g, outs, c, ref, cn, f32)
    return _base[name]


@pytest.mark.parametrize("name", NAMES)
def test_counts(e, name):
    _, _, c, _, cn, _ = _case(e, name)
    lg, ng, must, rows = group_facts(name)
    lt, nt, lk, nk, _ = facts(name)
    print(f"{name}: device counts {c}, with the variant bit {cn}; fp64 twin: live groups {lg}/{ng}, must-live {must}, "
          f"dead-tile rows in live groups {rows}")
    assert c["groups"] == cn["groups"] == ng == (cells(name) + 3) // 4
    assert must <= c["live_groups"] <= 4 * c["live_ksteps"]
    assert c["live_groups"] <= cn["live_groups"] <= ng
    # slots 0-3: the same tiles and k-steps as the rule gave before the groups were listed beside them (twin's totals; its live counts
    # are what the device's lie around: a live k-step holds a live group and the reverse, a live tile holds a live cell)
    assert c["tiles"] == cn["tiles"] == nt and c["ksteps"] == cn["ksteps"] == nk
    assert (c["live_groups"] + 3) // 4 <= c["live_ksteps"] <= min(c["live_groups"], nk)
    assert 0 < c["live_tiles"] <= cn["live_tiles"] <= nt
    if name == "tiny":  # nothing can be flushed: the groups inside the lengths, with and without the variant bit
        assert c == cn and c["live_groups"] == lg == must and c["live_ksteps"] == lk and c["live_tiles"] == lt
    else:
        assert c["live_groups"] < 4 * c["live_ksteps"]
        assert c["live_groups"] < cn["live_groups"]


@pytest.mark.parametrize("name", NAMES)
def test_group_walk_is_exact_beside_the_variant(e, name):
    """costs / grad_enc / grad_pred: torch.equal.  grad_W / grad_bias: the existing bound (tests/test_x2_flush_skip_gpu.py),
    max |default - variant| <= max |variant - fp32 route|."""
    _, new, _, ref, _, f32 = _case(e, name)
    for k, a, b in zip(OUT[:3], new[:3], ref[:3]):
        assert torch.equal(a, b), k
    for k, a, b, x in zip(OUT[3:], new[3:], ref[3:], f32[3:]):
        diff, bound = float((a - b).abs().max()), float((b - x).abs().max())
        print(f"{name}: {k}: |default - variant| max {diff:.3e}, |variant - fp32 route| max {bound:.3e}")
        assert diff <= bound, k


@pytest.mark.parametrize("name", NAMES)
def test_result_does_not_depend_on_what_the_workspace_held(e, name):
    V, gs = CASES[name][4], CASES[name][7]
    g, base = _case(e, name)[:2]
    _fill_workspace(e, g, V, 0xFF)
    poisoned = _run(e, g, V, gs)
    _fill_workspace(e, g, V, 0)
    zeroed = _run(e, g, V, gs)
    for o in poisoned:
        assert bool(torch.isfinite(o).all())
    _assert_same(poisoned, zeroed, "0xFF workspace against zeroed workspace")
    _assert_same(poisoned, base, "0xFF workspace against the first call")


@pytest.mark.parametrize("name", NAMES)
def test_stages_alone_and_repeat(e, name):
    """Stages up to dHidden (mask 31: the lists, k_x2_dead_rows) in one call, the reductions and dW (0xE0) in a second: bit-identical to
    one whole call; and a second whole call is bit-identical to the first (h640: k_dw_x2m, which still walks the k-step list)."""
    V, gs = CASES[name][4], CASES[name][7]
    g, base = _case(e, name)[:2]
    outs = e.alloc_fused_outputs(g["enc"], g["pred"], g["W"])
    for o in outs:
        o.fill_(float("nan"))
    _run(e, g, V, gs, stage_mask=31, outs=outs)
    _run(e, g, V, gs, stage_mask=0xE0, outs=outs)
    _assert_same(outs, base, "stage masks 31 + 0xE0 against one call")
    _assert_same(_run(e, g, V, gs), base, "second call against the first")


@pytest.mark.parametrize("M,K,N", [(18, 256, 128), (130, 384, 128)])
def test_linear_backward_walks_the_identity_group_list(M, K, N):
    """rnnt_amd.linear on the f16x2 pipes: its dW is k_dw_x2 over the identity group list.  M = 18: rows % 4 = 2 (a group half of zero
    padding rows), two k-steps; M = 130 with K % 256 = 128 (the half-empty h block's form of the kernel).  dW / db against float64 torch
    at the bars of tests/test_linear_abi_gpu.py."""
    import rnnt_amd
    gen = torch.Generator(device="cuda").manual_seed(M + K + N)
    x = torch.randn(M, K, device="cuda", generator=gen)
    W = (torch.randn(N, K, device="cuda", generator=gen) / K ** 0.5).requires_grad_(True)
    b = torch.randn(N, device="cuda", generator=gen).requires_grad_(True)
    dy = torch.randn(M, N, device="cuda", generator=gen)
    rnnt_amd.linear(x, W, b, backend="x2").backward(dy)
    torch.cuda.synchronize()
    W64, b64 = W.detach().double().requires_grad_(True), b.detach().double().requires_grad_(True)
    (torch.nn.functional.linear(x.double(), W64, b64) * dy.double()).sum().backward()
    assert_close_grad("dW", W.grad.cpu().numpy(), W64.grad.cpu().numpy())
    assert_close_grad("db", b.grad.cpu().numpy(), b64.grad.cpu().numpy())
