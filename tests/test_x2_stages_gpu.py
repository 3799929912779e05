"""-m gpu: each kernel of the f16x2 route (rnnt_amd/csrc/x2.hip) against fp64 on the operand planes the device itself produced upstream,
through the comparators of tests/x2_stage_cases.py (proved on the CPU by tests/test_x2_stages_oracle.py).  Per case:
  1. stage_mask = 15 (producers, forward, lattice, coefficients) leaves the hidden planes, ep, the scales, the fp32 logits, the row
     statistics and the coefficients in the workspace;
  2. stage_mask = 31 with RNNT_VARIANT_X2_NO_FLUSH_SKIP leaves G's hi | mid planes of every cell a backward GEMM can read;
  3. the full pipeline with the variant bit and without: the four gradients of each, both held to the references of call 2's planes
     (the cells the default call skips hold exact zeros there).
Every comparison prints `x2-stage-parity: case stage worst error / bar` (profiles/x2_stage_parity.txt)."""
import numpy as np
import pytest
import torch

from tests.helpers import assert_close_loss
from tests.x2_stage_cases import (CASES, SH, check_dhidden, check_dw, check_ep, check_g, check_hidden, check_logits, check_scales, check_stats,
                                  dims, g_chunks, g_scale_of, inside, make_case, rows_alloc, seen, w_pieces)

pytestmark = pytest.mark.gpu
X2 = "f16x2"
GRADS = ("grad_enc", "grad_pred", "grad_W", "grad_bias")


@pytest.fixture(scope="module")
def amd():
    import rnnt_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    rnnt_amd.engine.lib()
    return rnnt_amd


def _case(name):
    return make_case(name, torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def _dev(name, d):
    g = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    if CASES[name].get("permuted"):  # what the reference hands the joint: a (B,C,T)->(B,T,C) view (rnnt/model.py:27-28)
        g["enc"] = torch.from_numpy(np.ascontiguousarray(d["enc"].transpose(0, 2, 1))).cuda().permute(0, 2, 1)
        assert not g["enc"].is_contiguous()
    return g


def _run(e, g, V, gs, stage_mask=None, variant=0):
    outs = e.joint_loss_fwd_bwd(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"], V - 1, gs,
                                dtype=X2, stage_mask=stage_mask, variant=variant)
    torch.cuda.synchronize()
    return outs


def _np64(t):
    return t.double().cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_each_stage_against_fp64_on_the_devices_planes(amd, name):
    e = amd.engine
    d, gs = _case(name)
    B, T, U1, H, V = dims(d)
    cells, ra, D = B * T * U1, rows_alloc(B * T * U1), T + U1 - 1
    g = _dev(name, d)
    L = e.layout(B, T, U1, H, V, X2)
    ins = inside(d).reshape(-1)
    ins_t = torch.from_numpy(ins).cuda()
    if name == "more_tiles_than_cus":  # a persistent forward workgroup takes a second tile
        assert (cells + 127) // 128 > torch.cuda.get_device_properties(g["W"].device).multi_processor_count

    def buf(off, n, dtype):
        ws = e.workspace(g["W"].device, L.total)
        return ws[off:off + n * dtype.itemsize].view(dtype).clone()

    def hidden_planes():
        return buf(L.hidden, 2 * ra * H, torch.float16).reshape(2, ra, H)

    def report(stage, ratio):
        print(f"x2-stage-parity: {name} {stage} {ratio:.3f}")

    # ---- call 1: everything up to the coefficients
    _run(e, g, V, gs, stage_mask=15)
    hid_t = hidden_planes()
    scales = buf(L.counters + 640, 2, torch.float32).cpu().numpy()
    ep_flag = int(buf(L.counters + 896, 1, torch.int32).item())
    E_t, P_t = buf(L.ep, B * T * H, torch.float32), buf(L.ep + B * T * H * 4, B * U1 * H, torch.float32)
    logits_t = buf(L.logits, cells * V, torch.float32).reshape(cells, V)
    stats = [buf(off, B * D * U1, torch.float32).cpu().numpy() for off in (L.denom_s, L.lpb_s, L.lpe_s)]
    coef1 = buf(L.coef, cells * 4, torch.float32).reshape(cells, 4)

    sW = check_scales(scales[0], scales[1], ep_flag, d, name == "exact_forward")
    report("ep", check_ep(E_t.cpu().numpy(), P_t.cpu().numpy(), d))
    hi, mid = _np64(hid_t[0]), _np64(hid_t[1])
    rs, rv = check_hidden(hi, mid, d, ep_flag)
    report("hidden-structure", rs)
    report("hidden", rv)

    # logits: the yardstick is a plain fp32 torch evaluation of the same three products on the same pieces
    wh, wm = (torch.from_numpy(x.astype(np.float32)).cuda() for x in w_pieces(d["W"], sW))
    ah, am = hid_t[0, :cells].float(), hid_t[1, :cells].float()
    yard_l = (ah @ wh.T + ah @ wm.T + am @ wh.T) * float(1.0 / (SH * sW)) + g["bias"]
    logits = _np64(logits_t)
    rl, ry = check_logits(logits, hi, mid, d, sW, yard=_np64(yard_l))
    report("logits", rl)
    report("logits/fp32-yardstick", ry)
    for k, r in zip(("denom_s", "lpb_s", "lpe_s"), check_stats(*stats, logits, d)):
        report(k, r)

    # the coefficients' exact parts: c1 = -inf outside the lattices, the label of every emitting cell
    assert not bool((coef1[:, 0] != float("-inf"))[~ins_t].any())
    y = np.full((B, T, U1), -1, dtype=np.int32)
    for b in range(B):
        Ub = int(d["target_lens"][b])
        y[b, :int(d["logit_lens"][b]), :Ub] = d["targets"][b, :Ub][None, :]
    live1 = (coef1[:, 0] != float("-inf")).cpu().numpy()
    assert np.array_equal(coef1[:, 3].contiguous().view(torch.int32).cpu().numpy()[live1], y.reshape(-1)[live1])
    flagged = torch.from_numpy(ins).cuda() & (coef1[:, 0] == float("-inf")) & (coef1[:, 1] == 0) & (coef1[:, 2] == 0)

    # ---- call 2: ... + dHidden with the flush rule off: G's planes
    _run(e, g, V, gs, stage_mask=31, variant=e.VARIANT_X2_NO_FLUSH_SKIP)
    planes_t = buf(L.logits, cells * V * 2, torch.float16).reshape(cells, 2 * V)
    assert torch.equal(hidden_planes().view(torch.int16), hid_t.view(torch.int16)), "hidden differs between the calls"
    coef2 = buf(L.coef, cells * 4, torch.float32).reshape(cells, 4)
    assert bool((coef2[:, 0] != float("-inf"))[ins_t].all()), "the variant bit left a lattice cell flagged"
    # soundness of the flush predicate: what the default call skips is exactly zero (a few cells far off the alignments are flagged
    # in several cases; flushed_band is the one built to have whole tiles of them)
    assert bool((planes_t[flagged] == 0).all()), "a cell the default call flags holds a non-zero G entry"
    assert name != "flushed_band" or bool(flagged.any())
    gh_t, gm_t = g_chunks(planes_t)
    gh, gm = _np64(gh_t), _np64(gm_t)
    # G: the yardstick is the fp32 route's standalone loss on the same logits, rows outside the lattices zeroed for both
    lt = torch.where(ins_t[:, None], logits_t, torch.zeros((), device="cuda")).reshape(B, T, U1, V).requires_grad_(True)
    amd.rnnt_loss(lt, g["targets"], g["logit_lens"], g["target_lens"], blank=-1, reduction="none").sum().backward()
    rg, costs64 = check_g(gh, gm, logits, d, gs, _np64(lt.grad).reshape(cells, V) * gs)
    report("G", rg)
    gh, gm = seen(gh, gm, d)

    # ---- call 3: the whole pipeline, flush rule off and on
    gsc = g_scale_of(gs)
    G32 = torch.where(ins_t[:, None], (gh_t.float() + gm_t.float()) * float(1.0 / gsc), torch.zeros((), device="cuda"))
    h32 = (ah + am) * float(1.0 / SH)
    yard_W, yard_b = _np64(G32.T @ h32), _np64(G32.sum(0))
    for call, variant in (("no-flush-skip", e.VARIANT_X2_NO_FLUSH_SKIP), ("default", 0)):
        costs, ge, gp, gW, gb = (_np64(o) for o in _run(e, g, V, gs, variant=variant))
        assert torch.equal(hidden_planes().view(torch.int16), hid_t.view(torch.int16)), "hidden differs between the calls"
        assert_close_loss("costs", costs, costs64)
        re, rp = check_dhidden(ge, gp, gh, gm, d, sW, gs)
        report(f"{call}:grad_enc", re)
        report(f"{call}:grad_pred", rp)
        for k, r in check_dw(gW, gb, gh, gm, hi[:cells], mid[:cells], gs, yard_W, yard_b).items():
            report(call + ":" + {"W_bound": "grad_W", "b_bound": "grad_bias", "W_yard": "grad_W/fp32-yardstick", "b_yard": "grad_bias/fp32-yardstick"}[k], r)
    if name == "flushed_band":  # the lists the default call walked really were shorter than by length
        c = e.x2_live_counts(g["W"].device, B, T, U1, H, V)
        assert 0 < c["live_tiles"] < c["tiles"], c


def test_strided_enc_equals_its_contiguous_copy(amd):
    """The route's enc_sb / enc_st path (k_x2_make_ep, the exact forward's loads, dHidden's epilogue): the full call on a permuted
    (B,H,T)->(B,T,H) view and on its contiguous copy, bit for bit."""
    e = amd.engine
    d, gs = _case("permuted_enc")
    V = d["W"].shape[0]
    g = _dev("permuted_enc", d)
    a = [o.clone() for o in _run(e, g, V, gs)]
    g["enc"] = g["enc"].contiguous()
    b = _run(e, g, V, gs)
    for k, x, y in zip(("costs",) + GRADS, a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), k
