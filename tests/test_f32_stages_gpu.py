"""-m gpu: each kernel of the fp32 route (joint_fwd.hip, joint_bwd.hip), of the bf16x3 route (x3.hip) and of the lattice stage they share
(lattice.hip) against fp64 on the operands the device itself produced upstream, through the comparators of tests/f32_stage_cases.py
(proved on the CPU by tests/test_f32_stages_oracle.py).  Per case a forward mask (fp32: 7, whose logits k_make_g has not yet
overwritten; bf16x3: 15), the forward-only entry, then the full pipeline; the bf16x3 cases run three ways — every stage on x3.hip, the
forward on the fp32 route's kernel + k_split_make_hidden, forward and dHidden on the fp32 route's kernels + k_split_g.  Every
comparison prints `f32-stage-parity: route[:variant] case stage worst error / bar` (profiles/fp32_stage_parity.txt,
profiles/x3_stage_parity.txt)."""
import numpy as np
import pytest
import torch

from tests.f32_stage_cases import (F32_CASES, U24, X3_CASES, YARD, _judge, barrier_sweep, chain_mm, chain_six, check_coef, check_dhidden_f32, check_dhidden_x3,
                                   check_dw_f32, check_dw_x3, check_g_f32, check_g_x3, check_hidden_f32, check_hidden_x3, check_lattice,
                                   check_logits_f32, check_logits_x3, check_stats, coef_dict, dims, fast_tanh_f32, g_chunks, gen_bu,
                                   inside, loss64, make_case, rows_alloc, split3, table_rows, tanh64, tile_cols, ulp_fp32, unskew)
from tests.helpers import assert_close_loss

pytestmark = pytest.mark.gpu
X3 = "bf16x3"
DW_NAMES = {"W_bound": "grad_W", "b_bound": "grad_bias", "W_yard": "grad_W/fp32-yardstick", "b_yard": "grad_bias/fp32-yardstick"}


@pytest.fixture(scope="module")
def amd():
    import rnnt_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    rnnt_amd.engine.lib()
    return rnnt_amd


def _n_cu():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _dev(spec, d):
    g = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    if spec.get("permuted"):  # what the reference hands the joint: a (B,C,T)->(B,T,C) view (rnnt/model.py:27-28)
        g["enc"] = torch.from_numpy(np.ascontiguousarray(d["enc"].transpose(0, 2, 1))).cuda().permute(0, 2, 1)
        assert not g["enc"].is_contiguous()
    return g


def _args(g, V):
    return g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"], V - 1


def _run(e, g, V, gs, route, stage_mask=None, variant=0):
    outs = e.joint_loss_fwd_bwd(*_args(g, V), gs, dtype=route, stage_mask=stage_mask, variant=variant)
    torch.cuda.synchronize()
    return outs


def _np64(t):
    return t.double().cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


class _Ws:
    """Reads of the fused workspace of one case (engine.layout / engine.workspace)."""

    def __init__(self, e, g, route, aux=False):
        B, T, H = g["enc"].shape
        self.e, self.dev, self.B, self.T, self.U1, self.H, self.V = e, g["W"].device, B, T, g["pred"].shape[1], H, g["W"].shape[0]
        self.L = e.layout(B, T, self.U1, H, self.V, route)
        self.cells, self.D = B * T * self.U1, T + self.U1 - 1
        self.need = self.L.total + (self.L.aux_bytes if aux else 0)  # what engine.joint_loss_fwd_bwd asks engine.workspace for

    def buf(self, off, n, dtype):
        ws = self.e.workspace(self.dev, self.need)
        return ws[off:off + n * dtype.itemsize].view(dtype).clone()

    def rows(self, off, cols, dtype):
        return self.buf(off, self.cells * cols, dtype).reshape(self.cells, cols)

    def skewed(self, off, dtype):
        return self.buf(off, self.B * self.D * self.U1, dtype).cpu().numpy()

    def loss_planes(self):
        L = self.L
        return dict(stats=[self.skewed(o, torch.float32) for o in (L.denom_s, L.lpb_s, L.lpe_s)],
                    alpha_s=self.skewed(L.alpha_s, torch.float64), beta_s=self.skewed(L.beta_s, torch.float64))

    def coef(self):
        c = self.rows(self.L.coef, 4, torch.float32)
        return c[:, :3].cpu().numpy(), c[:, 3].contiguous().view(torch.int32).cpu().numpy()


def _loss_checks(report, w, p, costs, logits, d, gs, coef, y):
    """The stages every route shares: statistics, the sweep, the costs, the coefficients."""
    B, T, U1 = w.B, w.T, w.U1
    for k, r in zip(("denom_s", "lpb_s", "lpe_s"), check_stats(*p["stats"], logits, d)):
        report(k, r)
    for k, r in zip(("alpha", "beta"), check_lattice(p["alpha_s"], p["beta_s"], costs.cpu().numpy(), p["stats"][1], p["stats"][2], d)):
        report(k, r)
    assert_close_loss("costs", _np64(costs), loss64(logits, d)[0])
    den, lpb, lpe = (unskew(x, B, T, U1) for x in p["stats"])
    lpe = np.where(np.arange(U1)[None, None, :] < d["target_lens"][:, None, None], lpe, 0.0)
    with np.errstate(invalid="ignore"):
        al, be = unskew(p["alpha_s"], B, T, U1), unskew(p["beta_s"], B, T, U1)
        for k, r in zip(("c1", "sb", "se"), check_coef(coef, y, al, be, den, lpb, lpe, d, gs)):
            report(k, r)


@pytest.mark.parametrize("name", list(F32_CASES))
def test_fp32_route_each_stage_against_fp64_on_the_devices_operands(amd, name):
    e = amd.engine
    d, gs = make_case("fp32", name, _n_cu())
    B, T, U1, H, V = dims(d)
    g = _dev(F32_CASES[name], d)
    w = _Ws(e, g, "fp32")
    L, cells = w.L, w.cells
    ins = inside(d).reshape(-1)
    ins_t = torch.from_numpy(ins).cuda()
    # the path the case is named for, where the engine shows it
    assert L.n_ublk == (U1 + gen_bu(T, U1) - 1) // gen_bu(T, U1)
    if name == "more_tiles_than_2_cus":
        assert B * ((T * U1 + 63) // 64) > 2 * _n_cu()
    if name == "barrier_sweep":
        assert barrier_sweep(U1, L.D)

    def report(stage, ratio):
        print(f"f32-stage-parity: fp32 {name} {stage} {ratio:.3f}")

    # ---- call 1: producers, forward, lattice (mask 15 would already run k_make_g over the logits where no tile kernel applies)
    costs1 = _run(e, g, V, gs, "fp32", stage_mask=7)[0].clone()
    hid_t = w.rows(L.hidden, H, torch.float32)
    logits_t = w.rows(L.logits, V, torch.float32)
    p = w.loss_planes()
    hidden, logits = _np64(hid_t), _np64(logits_t)
    report("hidden", check_hidden_f32(hidden, d))
    rl, ry = check_logits_f32(logits, hidden, d, yard=_np64(chain_mm(hid_t, g["W"].T, 2, first=g["bias"][None, :].expand(cells, V))))
    report("logits", rl)
    report("logits/fp32-yardstick", ry)

    # ---- the forward-only entry (no hidden written): the same costs, bit for bit
    cf = e.joint_loss_fwd(*_args(g, V), dtype="fp32")
    torch.cuda.synchronize()
    assert torch.equal(_bits(cf), _bits(costs1)), "joint_loss_fwd: costs differ from the training call's"

    # ---- call 2: the whole pipeline
    costs, ge, gp, gW, gb = _run(e, g, V, gs, "fp32")
    assert torch.equal(_bits(w.rows(L.hidden, H, torch.float32)), _bits(hid_t)), "hidden differs between the calls"
    assert torch.equal(_bits(costs), _bits(costs1)), "costs differ between the calls"
    coef, y = w.coef()
    _loss_checks(report, w, w.loss_planes(), costs, logits, d, gs, coef, y)
    G_t = w.rows(L.logits, V, torch.float32)
    report("G", check_g_f32(_np64(G_t), logits, coef_dict(coef, y), d, table_rows(d, 16)))
    G_t = torch.where(ins_t[:, None], G_t, torch.zeros((), device="cuda"))
    G = _np64(G_t)
    for k, r in zip(("grad_enc", "grad_pred"), check_dhidden_f32(_np64(ge), _np64(gp), G, hidden, d)):
        report(k, r)
    for k, r in check_dw_f32(_np64(gW), _np64(gb), G, hidden, _np64(G_t.T @ hid_t)).items():
        report(DW_NAMES[k], r)
    e.release_workspaces()


X3_VARIANTS = ("x3", "fp32-forward", "fp32-forward-and-dhidden")


@pytest.mark.parametrize("variant", X3_VARIANTS)
@pytest.mark.parametrize("name", list(X3_CASES))
def test_bf16x3_route_each_stage_against_fp64_on_the_devices_planes(amd, name, variant):
    e = amd.engine
    var = {"x3": 0, "fp32-forward": e.VARIANT_X3_FP32_FWD, "fp32-forward-and-dhidden": e.VARIANT_X3_FP32_FWD | e.VARIANT_X3_FP32_DH}[variant]
    fwd32, dh32 = bool(var & e.VARIANT_X3_FP32_FWD), bool(var & e.VARIANT_X3_FP32_DH)
    d, gs = make_case(X3, name, _n_cu())
    B, T, U1, H, V = dims(d)
    g = _dev(X3_CASES[name], d)
    w = _Ws(e, g, X3, aux=fwd32)
    L, cells, ra = w.L, w.cells, rows_alloc(w.cells)
    ins = inside(d).reshape(-1)
    ins_t = torch.from_numpy(ins).cuda()
    if name == "more_tiles_than_cus":
        assert (cells + 127) // 128 > _n_cu()
    if name == "fewer_ksteps_than_slabs":
        assert (cells + 15) // 16 < L.n_split
    if dh32 and name == "rows_past_a_live_end":
        assert tile_cols(H, V) > 0 and L.n_ublk == (U1 + 7) // 8

    def report(stage, ratio):
        print(f"f32-stage-parity: {X3}:{variant} {name} {stage} {ratio:.3f}")

    def hidden_planes():
        return w.buf(L.hidden, 3 * ra * H, torch.bfloat16).reshape(3, ra, H)

    def aux_hidden():
        return w.rows(L.aux, H, torch.float32)

    # ---- call 1: everything up to the coefficients
    costs1 = _run(e, g, V, gs, X3, stage_mask=15, variant=var)[0].clone()
    hid_t = hidden_planes()
    aux_t = aux_hidden() if fwd32 else None
    logits_t = w.rows(L.logits, V, torch.float32)
    p = w.loss_planes()
    coef, y = w.coef()
    planes, logits = _np64(hid_t), _np64(logits_t)
    report("hidden", check_hidden_x3(planes, d))
    if fwd32:  # the fp32 route's forward on its own fp32 hidden (k_split_make_hidden made the planes above)
        aux = _np64(aux_t)
        report("aux-hidden", check_hidden_f32(aux, d))
        rl, ry = check_logits_f32(logits, aux, d, yard=_np64(chain_mm(aux_t, g["W"].T, 2, first=g["bias"][None, :].expand(cells, V))))
        report("logits", rl)
        report("logits/fp32-yardstick", ry)
    else:
        wp_t = [torch.from_numpy(x.astype(np.float32)).cuda() for x in split3(d["W"])]
        a = [hid_t[i, :cells].float() for i in range(3)]
        yard = chain_six(a, [x.T for x in wp_t], first=g["bias"][None, :].expand(cells, V))
        for k, r in zip(("logits", "logits/fp32-yardstick", "logits/product-shares"), check_logits_x3(logits, planes, d, _np64(yard))):
            report(k, r)
    _loss_checks(report, w, p, costs1, logits, d, gs, coef, y)

    cf = e.joint_loss_fwd(*_args(g, V), dtype=X3)
    torch.cuda.synchronize()
    if not fwd32:  # (the forward-only entry runs the route's own forward)
        assert torch.equal(_bits(cf), _bits(costs1)), "joint_loss_fwd: costs differ from the training call's"

    # ---- call 2: the whole pipeline
    costs, ge, gp, gW, gb = _run(e, g, V, gs, X3, variant=var)
    assert torch.equal(_bits(hidden_planes()), _bits(hid_t)), "hidden planes differ between the calls"
    assert torch.equal(_bits(costs), _bits(costs1)), "costs differ between the calls"
    if fwd32:
        assert torch.equal(_bits(aux_hidden()), _bits(aux_t)), "fp32 hidden differs between the calls"
    gh_t, gm_t = g_chunks(w.rows(L.logits, 2 * V, torch.bfloat16))
    gl_t = w.rows(L.g_lo, V, torch.bfloat16)
    read = table_rows(d, 32) if dh32 else np.ones(cells, dtype=bool)
    report("G", check_g_x3(_np64(gh_t), _np64(gm_t), _np64(gl_t), logits, coef_dict(coef, y), d, read))
    gp3_t = [torch.where(ins_t[:, None], x.float(), torch.zeros((), device="cuda")) for x in (gh_t, gm_t, gl_t)]
    gp3 = tuple(_np64(x) for x in gp3_t)
    G32_t = gp3_t[0] + gp3_t[1] + gp3_t[2]  # exact: the fp32 value that was split
    rs = check_dhidden_f32(_np64(ge), _np64(gp), _np64(G32_t), _np64(aux_t), d) if dh32 else check_dhidden_x3(_np64(ge), _np64(gp), gp3, d)
    for k, r in zip(("grad_enc", "grad_pred"), rs):
        report(k, r)
    h32_t = hid_t[0, :cells].float() + hid_t[1, :cells].float() + hid_t[2, :cells].float()
    hp = tuple(planes[i, :cells] for i in range(3))
    for k, r in check_dw_x3(_np64(gW), _np64(gb), gp3, hp, _np64(G32_t.T @ h32_t)).items():
        report(DW_NAMES[k], r)
    e.release_workspaces()


DENSE = [(1, 1, 0, 4, 4), (2, 9, 4, 136, 36), (2, 11, 6, 128, 64), (1, 9, 5, 1024, 32), (2, 10, 7, 640, 32)]


@pytest.mark.parametrize("shape", DENSE, ids=lambda s: "x".join(map(str, s)))
def test_unfused_joint_forward_and_backward_per_entry(amd, shape):
    """rnnt_engine_joint_fwd (the logits-only forward kernels) and rnnt_engine_joint_bwd on a DENSE random G (the g_ready forms of the
    dHidden kernels, k_make_hidden, k_dw on every row): every entry against fp64 with the dot-product bars of tests/f32_stage_cases.py.
    The entries keep their hidden to themselves, so the references use tanh64 and the bars allow for the kernels' tanh, A = YARD x the
    fp32 numpy error of common.hpp's formula + an ulp: sum |w| A on a logit, 2 A + 2 U24 on the factor 1 - h^2, sum |g| A on dW."""
    from tests.helpers import make_inputs
    e = amd.engine
    B, T, U, H, V = shape
    U1 = U + 1
    d = make_inputs(B, T, U, H, V, seed=sum(shape), ragged=False)
    g = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    h64 = tanh64(d).reshape(-1, H)
    A = YARD * float(np.abs(fast_tanh_f32(d).astype(np.float64).reshape(-1, H) - h64).max()) + float(ulp_fp32(1.0))
    W, bias = d["W"].astype(np.float64), d["bias"].astype(np.float64)

    def report(stage, ratio):
        print(f"f32-stage-parity: fp32-unfused {'x'.join(map(str, shape))} {stage} {ratio:.3f}")

    logits = _np64(e.joint_fwd(g["enc"], g["pred"], g["W"], g["bias"])).reshape(-1, V)
    ref = h64 @ W.T + bias
    mag = np.abs(h64) @ np.abs(W).T + np.abs(bias)
    report("logits", _judge("logits", np.abs(logits - ref), (H + 1) * U24 * mag + 0.5 * ulp_fp32(ref) + A * np.abs(W).sum(1)[None, :]))

    G32 = np.random.default_rng(sum(shape)).standard_normal((B * T * U1, V)).astype(np.float32)
    ge, gp, gW, gb = (_np64(x) for x in e.joint_bwd(g["enc"], g["pred"], g["W"], torch.from_numpy(G32).cuda().reshape(B, T, U1, V)))
    G = G32.astype(np.float64)
    acc, macc = (G @ W).reshape(B, T, U1, H), (np.abs(G) @ np.abs(W)).reshape(B, T, U1, H)
    dt = (1.0 - h64 ** 2).reshape(B, T, U1, H)
    bar = lambda n, ax: ((V + n + 4) * U24 * macc * dt + (2 * A + 2 * U24) * macc).sum(ax)  # noqa: E731
    report("grad_enc", _judge("grad_enc", np.abs(ge - (acc * dt).sum(2)), bar(U1, 2)))
    report("grad_pred", _judge("grad_pred", np.abs(gp - (acc * dt).sum(1)), bar(T, 1)))
    cells = G.shape[0]
    report("grad_W", _judge("grad_W", np.abs(gW - G.T @ h64), (cells + 8) * U24 * (np.abs(G).T @ np.abs(h64)) + A * np.abs(G).sum(0)[:, None]))
    report("grad_bias", _judge("grad_bias", np.abs(gb - G.sum(0)), (cells + 8) * U24 * np.abs(G).sum(0)))
