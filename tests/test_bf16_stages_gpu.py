"""-m gpu: each kernel of the bf16 route (rnnt_amd/csrc/bf16.hip) against fp64 on the operands the device itself produced upstream,
through the comparators of tests/bf16_stage_cases.py (proved on the CPU by tests/test_bf16_stages_oracle.py).  Two engine calls per
case: stage_mask = 15 (producers, forward, lattice, coefficients) leaves hidden, the fp16 logits and the coefficients in the
workspace; the full pipeline then leaves G in place of the logits.  Every comparison prints `bf16-stage-parity: case stage worst
error / bar` (profiles/bf16_stage_parity.txt)."""
import numpy as np
import pytest
import torch

from tests.bf16_stage_cases import CASES, check_dhidden, check_dw, check_g, check_hidden, check_logits, dims, inside, make_case
from tests.helpers import assert_close_loss

pytestmark = pytest.mark.gpu
BF = "bf16"


@pytest.fixture(scope="module")
def amd():
    import rnnt_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    rnnt_amd.engine.lib()
    return rnnt_amd


def _dev(name, d):
    g = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    if CASES[name].get("permuted"):  # what the reference hands the joint: a (B,C,T)->(B,T,C) view (rnnt/model.py:27-28)
        g["enc"] = torch.from_numpy(np.ascontiguousarray(d["enc"].transpose(0, 2, 1))).cuda().permute(0, 2, 1)
        assert not g["enc"].is_contiguous()
    return g


def _run(e, g, V, gs, stage_mask=None):
    outs = e.joint_loss_fwd_bwd(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"], V - 1, gs,
                                dtype=BF, stage_mask=stage_mask)
    torch.cuda.synchronize()
    return outs


def _np64(t):
    return t.double().cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_each_stage_against_fp64_on_the_devices_operands(amd, name):
    e = amd.engine
    d, gs = make_case(name)
    B, T, U1, H, V = dims(d)
    cells = B * T * U1
    g = _dev(name, d)
    L = e.layout(B, T, U1, H, V, BF)

    def plane(off, cols, dtype):
        ws = e.workspace(g["enc"].device, L.total)
        return ws[off:off + cells * cols * dtype.itemsize].view(dtype).reshape(cells, cols).clone()

    def report(stage, ratio):
        print(f"bf16-stage-parity: {name} {stage} {ratio:.3f}")

    _run(e, g, V, gs, stage_mask=15)
    hidden_t = plane(L.hidden, H, torch.bfloat16)
    logits_t = plane(L.logits, V, torch.float16)
    coef = plane(L.coef, 4, torch.float32)
    costs, ge, gp, gW, gb = _run(e, g, V, gs)
    G_t = plane(L.logits, V, torch.bfloat16)
    assert torch.equal(plane(L.hidden, H, torch.bfloat16).view(torch.int16), hidden_t.view(torch.int16)), "hidden differs between the two calls"

    ins_t = torch.from_numpy(inside(d).reshape(-1)).cuda()
    hidden, logits, G = _np64(hidden_t), _np64(logits_t), _np64(G_t)
    report("hidden", check_hidden(hidden, d))
    report("logits", check_logits(logits, hidden, d))

    # the coefficients' exact parts: c1 = -inf exactly outside the lattices, the label of every emitting cell
    ins = inside(d)
    assert torch.equal(coef[:, 0] == float("-inf"), ~ins_t)
    y = np.full((B, T, U1), -1, dtype=np.int32)
    for b in range(B):
        Ub = int(d["target_lens"][b])
        y[b, :int(d["logit_lens"][b]), :Ub] = d["targets"][b, :Ub][None, :]
    assert np.array_equal(coef[:, 3].contiguous().view(torch.int32).cpu().numpy(), y.reshape(-1))

    # G: the yardstick is the fp32 route's standalone loss on the same (fp16) logits, rows outside the lattices zeroed for both
    lt = torch.where(ins_t[:, None], logits_t.float(), torch.zeros((), device="cuda")).reshape(B, T, U1, V).requires_grad_(True)
    amd.rnnt_loss(lt, g["targets"], g["logit_lens"], g["target_lens"], blank=-1, reduction="none").sum().backward()
    yard = _np64(lt.grad).reshape(cells, V) * gs
    ratio, costs64 = check_g(G, logits, d, gs, yard)
    report("G", ratio)
    assert_close_loss("costs", _np64(costs), costs64)

    re, rp = check_dhidden(_np64(ge), _np64(gp), G, hidden, d)
    report("grad_enc", re)
    report("grad_pred", rp)

    yard_W = _np64(G_t.float().T @ hidden_t.float())
    yard_b = _np64(G_t.float().sum(0))
    for k, r in check_dw(_np64(gW), _np64(gb), G, hidden, yard_W, yard_b).items():
        report({"W_bound": "grad_W", "b_bound": "grad_bias", "W_yard": "grad_W/fp32-yardstick", "b_yard": "grad_bias/fp32-yardstick"}[k], r)


def test_strided_enc_equals_its_contiguous_copy(amd):
    """The route's enc_sb / enc_st path: the full call on a permuted (B,H,T)->(B,T,H) view and on its contiguous copy, bit for bit."""
    e = amd.engine
    d, gs = make_case("permuted_enc")
    V = d["W"].shape[0]
    g = _dev("permuted_enc", d)
    a = [o.clone() for o in _run(e, g, V, gs)]
    g["enc"] = g["enc"].contiguous()
    b = _run(e, g, V, gs)
    for k, x, y in zip(("costs", "grad_enc", "grad_pred", "grad_W", "grad_bias"), a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), k
