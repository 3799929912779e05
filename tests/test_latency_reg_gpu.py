"""-m gpu: FastEmit and the delay penalty on every route against the float64 oracle of
tests/latency_reg_oracle.py; the new C entries at lambda = delta = 0 against the existing ones, bit for bit; the standalone loss
with clamp; the cost paths; the f16x2 G bound at large lambda (fused dHidden and the f32_dh fallback); NaN inputs; batch sharding;
RNNTModel's attributes and a regularised step captured as a HIP graph."""
import numpy as np
import pytest
import torch

import rnnt_amd
from rnnt_amd import engine
from tests import latency_reg_oracle as lro
from tests.helpers import (BF16_GRAD_RTOL, BF16_LOSS_RTOL, GRAD_RTOL, LOSS_RTOL, assert_close_grad, assert_close_loss,
                           make_inputs)

pytestmark = pytest.mark.gpu

ROUTES = ("fp32", "f16x2", "bf16x3", "bf16")
OPTIONS = {"fastemit": (0.5, 0.0), "delay": (0.0, 0.05), "both": (0.5, 0.05)}
GRADS = ("grad_enc", "grad_pred", "grad_W", "grad_bias")


def _dev(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def _case(kind, seed, B=4, T=23, U=9, H=128, V=128):
    d = make_inputs(B, T, U, H, V, seed=seed, ragged=(kind == "ragged"))
    if kind == "ragged":
        d["logit_lens"][-1] = 1   # a one-frame utterance
        d["target_lens"][-2] = 0  # one without labels
    return d


def _run(d, dtype, lam=0.0, dp=0.0, grad_scale=None, check_lengths=True):
    g = _dev(d)
    leaves = [g[k].requires_grad_(True) for k in ("enc", "pred", "W", "bias")]
    kw = {}
    if lam:
        kw["fastemit_lambda"] = lam
    if dp:
        kw["delay_penalty"] = dp
    loss, costs = rnnt_amd.joint_rnnt_loss(*leaves, g["targets"], g["logit_lens"], g["target_lens"], return_costs=True,
                                           grad_scale=grad_scale, check_lengths=check_lengths, dtype=dtype, **kw)
    loss.backward()
    torch.cuda.synchronize()
    out = dict(loss=loss.item(), costs=costs.cpu().numpy())
    for k, t in zip(GRADS, leaves):
        out[k] = t.grad.cpu().numpy()
    return out


def _compare(r, ref, bf16=False):
    lt, gt = (BF16_LOSS_RTOL, BF16_GRAD_RTOL) if bf16 else (LOSS_RTOL, GRAD_RTOL)
    assert_close_loss("costs", r["costs"], ref["costs"], rtol=lt)
    for k in GRADS:
        assert_close_grad(k, r[k], ref[k], rtol=gt)


def _engine_args(g, V, scale):
    return (g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"], V - 1, scale)


@pytest.mark.parametrize("kind", ["uniform", "ragged"])
@pytest.mark.parametrize("opt", sorted(OPTIONS))
@pytest.mark.parametrize("route", ROUTES)
def test_route_matches_the_oracle(route, opt, kind):
    lam, dp = OPTIONS[opt]
    d = _case(kind, seed=7 + len(opt) + len(kind))
    ref = lro.fused_bf16(d, lam, dp) if route == "bf16" else lro.fused(d, lam, dp)
    _compare(_run(d, route, lam, dp), ref, bf16=route == "bf16")
    plain = lro.fused(d)
    assert max(np.abs(ref[k] - plain[k]).max() / np.abs(plain[k]).max() for k in GRADS) > 10 * GRAD_RTOL


@pytest.mark.parametrize("route", ROUTES)
def test_zero_options_are_the_existing_entries_bit_for_bit(route):
    d = _case("ragged", seed=11)
    g = _dev(d)
    a = _engine_args(g, 128, 0.25)
    old = [o.clone() for o in engine.joint_loss_fwd_bwd(*a, dtype=route)]
    new = [o.clone() for o in engine.joint_loss_fwd_bwd_reg(*a, 0.0, 0.0, dtype=route)]
    for x, y in zip(old, new):
        assert torch.equal(x, y)
    assert torch.equal(engine.joint_loss_fwd(*a[:-1], dtype=route), engine.joint_loss_fwd_reg(*a[:-1], 0.0, dtype=route))
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((3, 9, 5, 12)).astype(np.float32)).cuda()
    t = torch.from_numpy(np.random.default_rng(3).integers(0, 11, (3, 4)).astype(np.int32)).cuda()
    ll, tl = torch.tensor([9, 1, 6], dtype=torch.int32).cuda(), torch.tensor([4, 2, 0], dtype=torch.int32).cuda()
    c0, g0 = engine.loss_fwd_bwd(x, t, ll, tl, 11, 0.3)
    c1, g1 = engine.loss_fwd_bwd_reg(x, t, ll, tl, 11, 0.3, 0.0, 0.0)
    assert torch.equal(c0, c1) and torch.equal(g0, g1)


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
def test_standalone_loss_with_options_and_clamp(reduction):
    rng = np.random.default_rng(5)
    B, T, U, V = 3, 13, 6, 20
    logits = (rng.standard_normal((B, T, U + 1, V)) * 2).astype(np.float32)
    targets = rng.integers(0, V - 1, (B, U)).astype(np.int32)
    ll, tl = np.array([13, 1, 9], dtype=np.int32), np.array([6, 3, 0], dtype=np.int32)
    lam, dp, clamp = 0.5, 0.05, 0.3
    x = torch.from_numpy(logits).cuda().requires_grad_(True)
    out = rnnt_amd.rnnt_loss(x, *(torch.from_numpy(a).cuda() for a in (targets, ll, tl)), clamp=clamp, reduction=reduction,
                             fastemit_lambda=lam, delay_penalty=dp)
    (out.sum() if reduction == "none" else out).backward()
    costs, G = lro.loss_and_grad(logits, targets, ll, tl, -1, lam, dp, clamp=clamp)
    want = {"none": costs, "mean": costs.mean(), "sum": costs.sum()}[reduction]
    assert_close_loss("loss", out.detach().cpu().numpy(), want)
    assert_close_grad("grad_logits", x.grad.cpu().numpy(), G * (1.0 / B if reduction == "mean" else 1.0))
    assert (np.abs(G) >= clamp).any()  # the clamp is active on the regularised gradient


@pytest.mark.parametrize("route", ROUTES)
def test_cost_paths(route):
    d = _case("ragged", seed=21)
    g = _dev(d)
    with torch.no_grad():
        _, c_ng = rnnt_amd.joint_rnnt_loss(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"],
                                           g["target_lens"], return_costs=True, dtype=route, delay_penalty=0.05)
    a = _engine_args(g, 128, 0.25)
    c_dp = engine.joint_loss_fwd_bwd_reg(*a, 0.0, 0.05, dtype=route)[0].clone()
    c_both = engine.joint_loss_fwd_bwd_reg(*a, 0.5, 0.05, dtype=route)[0].clone()
    c_fe = engine.joint_loss_fwd_bwd_reg(*a, 0.5, 0.0, dtype=route)[0].clone()
    c_plain = engine.joint_loss_fwd_bwd(*a, dtype=route)[0].clone()
    assert torch.equal(c_ng, c_dp)       # the no-grad path computes the fwd + bwd path's costs
    assert torch.equal(c_both, c_dp)     # lambda leaves the costs bit-identical
    assert torch.equal(c_fe, c_plain)
    ref = (lro.fused_bf16 if route == "bf16" else lro.fused)(d, 0.0, 0.05)
    assert_close_loss("costs", c_dp.cpu().numpy(), ref["costs"], rtol=BF16_LOSS_RTOL if route == "bf16" else LOSS_RTOL)


def test_f16x2_large_lambda_on_a_forced_label_path():
    """T = 1: the only path emits every label at frame 0, E = 1 on each label cell, and improbable labels put the label term
    of G at -(1 + lambda) grad_scale: 17 at lambda = 16, beyond the fp16 planes at a scale chosen for |G| <= grad_scale."""
    d = make_inputs(1, 1, 6, 128, 128, seed=3, ragged=False)
    d["bias"][d["targets"][0]] = -12.0
    lam = 16.0
    _, G = lro.loss_and_grad(lro.cpu_oracle.joint_fwd(d["enc"], d["pred"], d["W"], d["bias"]), d["targets"],
                             d["logit_lens"], d["target_lens"], -1, lam)
    assert np.abs(G).max() > 16.0
    r = _run(d, "f16x2", lam, grad_scale=1.0)
    for k in GRADS:
        assert np.isfinite(r[k]).all(), k
    _compare(r, lro.fused(d, lam, grad_scale=1.0))


def test_f16x2_f32_dh_fallback_shape():
    """A tile's logits rows beyond the 2 GiB buffer range of k_dhidden_x2 (x2_dhidden_ok: U1 = 1024, V = 74 752): the
    fp32 route's dHidden makes G and k_split_g<F16x2> splits it, with the same (1 + lambda) bound.  Against the exact-fp32 route."""
    B, T, U, H, V = 1, 2, 1023, 128, 74752
    assert (7 * (U + 1) + 16) * V * 4 >= 2 ** 31
    d = make_inputs(B, T, U, H, V, seed=9, ragged=False)
    # the fallback needs total + aux_bytes of workspace (include/rnnt_engine.h): grow this stream's grow-only buffer first
    L = engine.layout(B, T, U + 1, H, V, "f16x2")
    engine.workspace(torch.device("cuda", torch.cuda.current_device()), L.total + L.aux_bytes)
    r = _run(d, "f16x2", 16.0, 0.05, grad_scale=1.0)
    ref = _run(d, "fp32", 16.0, 0.05, grad_scale=1.0)
    engine.release_workspaces()
    _compare(r, ref)


def test_config2_f16x2_matches_the_exact_fp32_route():
    d = make_inputs(32, 1000, 200, 512, 1024, seed=2)
    r = _run(d, "f16x2", 0.01, 0.001)
    ref = _run(d, "fp32", 0.01, 0.001)
    engine.release_workspaces()
    _compare(r, ref)


@pytest.mark.parametrize("route", ROUTES)
def test_nan_row_poisons_only_its_utterance(route):
    d = _case("uniform", seed=31)
    d["enc"][1, 4, :] = np.nan
    g = _dev(d)
    a = _engine_args(g, 128, 0.25)
    c = engine.joint_loss_fwd_bwd_reg(*a, 0.5, 0.05, dtype=route)[0].cpu().numpy()
    c_ng = engine.joint_loss_fwd_reg(*a[:-1], 0.05, dtype=route).cpu().numpy()
    ref = (lro.fused_bf16 if route == "bf16" else lro.fused)(d, 0.5, 0.05)["costs"]
    for cc in (c, c_ng):
        assert np.isnan(cc[1])
        assert_close_loss("clean costs", np.delete(cc, 1), np.delete(ref, 1),
                          rtol=BF16_LOSS_RTOL if route == "bf16" else LOSS_RTOL)


@pytest.mark.parametrize("route", ["fp32", "f16x2"])
def test_half_batch_calls_sum_to_the_full_batch(route):
    d = _case("ragged", seed=41)
    B, lam, dp = 4, 0.5, 0.05
    full = _run(d, route, lam, dp, grad_scale=1.0 / B)
    parts = []
    for lo, hi in ((0, 2), (2, 4)):
        sub = {k: (v if k in ("W", "bias") else v[lo:hi]) for k, v in d.items()}
        parts.append(_run(sub, route, lam, dp, grad_scale=1.0 / B, check_lengths=False))
    assert_close_loss("costs", np.concatenate([p["costs"] for p in parts]), full["costs"])
    for k in ("grad_enc", "grad_pred"):
        assert_close_grad(k, np.concatenate([p[k] for p in parts]), full[k])
    for k in ("grad_W", "grad_bias"):
        assert_close_grad(k, parts[0][k] + parts[1][k], full[k])


class _Enc(torch.nn.Module):
    def forward(self, x):
        return x

    def calc_output_lens(self, lens):
        return lens


def _model(H=128, V=64, seed=0):
    torch.manual_seed(seed)
    return rnnt_amd.RNNTModel(torch.nn.Embedding(V, H), _Enc(), rnnt_amd.JointNetwork(-1, -1, H, V)).cuda()


def _batch(B=3, T=17, U=6, H=128, V=64, seed=1):
    gen = torch.Generator().manual_seed(seed)
    return dict(mel=torch.randn(B, H, T, generator=gen).cuda(), lens=torch.tensor([T, 11, 1]).cuda(),
                ids=torch.randint(0, V - 1, (B, U), generator=gen).cuda(), id_lens=torch.tensor([U, 0, 4]).cuda())


@pytest.mark.parametrize("lam,dp", [(0.0, 0.0), (0.5, 0.0), (0.0, 0.05), (0.5, 0.05)])
def test_model_attributes_reach_the_loss(lam, dp):
    V = 64
    model = _model(V=V)
    model.fastemit_lambda, model.delay_penalty = lam, dp
    b = _batch(V=V)
    loss = model(b["mel"], b["lens"], b["ids"], b["id_lens"], V - 1)
    loss.backward()
    got = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    start = torch.full((3, 1), V - 1, dtype=b["ids"].dtype, device="cuda")
    dec = model.predictor(torch.cat([start, b["ids"]], dim=1))
    kw = {k: v for k, v in (("fastemit_lambda", lam), ("delay_penalty", dp)) if v}
    loss2 = model.joint.fused_loss(b["mel"].permute(0, 2, 1), dec, b["ids"].int(), b["lens"].int(), b["id_lens"].int(),
                                   blank=-1, reduction="mean", **kw)
    loss2.backward()
    assert loss.item() == loss2.item()
    for n, p in model.named_parameters():
        assert torch.equal(got[n], p.grad), n


def test_regularised_step_as_a_hip_graph():
    V = 64
    model = _model(V=V, seed=3)
    model.check_lengths = False
    model.fastemit_lambda, model.delay_penalty = 0.5, 0.05
    b0, b1 = _batch(V=V, seed=7), _batch(V=V, seed=8)
    static = {k: v.clone() for k, v in b0.items()}
    params = list(model.parameters())

    def fwd_bwd():
        loss = model(static["mel"], static["lens"], static["ids"], static["id_lens"], V - 1)
        loss.backward()
        return loss

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            for p in params:
                p.grad = None
            fwd_bwd()
        s.synchronize()
        for p in params:
            p.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            static_loss = fwd_bwd()
    torch.cuda.current_stream().wait_stream(s)
    static_grads = [p.grad for p in params]
    for batch in (b1, b0):
        for k, v in batch.items():
            static[k].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        got_loss, got = static_loss.item(), [g.clone() for g in static_grads]
        for p in params:
            p.grad = None
        want_loss = fwd_bwd().item()
        torch.cuda.synchronize()
        assert got_loss == want_loss
        for (name, p), g in zip(model.named_parameters(), got):
            assert torch.equal(g, p.grad), name
        for p, g in zip(params, static_grads):
            p.grad = g
