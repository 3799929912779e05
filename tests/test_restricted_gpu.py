"""-m gpu: the alignment-restricted transducer loss on every route against the float64 oracle of
tests/restricted_oracle.py: windows around the Viterbi path on uniform and ragged batches; the chained sweep across a wave
boundary and the barrier sweep, both with unreachable cells inside the lattice; the identities (zero window = the aligned
path, wide window = the plain loss); restriction off = the existing calls bit for bit; FastEmit and the delay penalty on
the restricted lattice; the standalone loss with clamp and a blank inside the vocabulary; an infeasible utterance; NaN inputs;
the host checks; RNNTModel; a restricted step as a HIP graph; batch sharding; the f16x2 backward's live tiles."""
import functools

import numpy as np
import pytest
import torch

import rnnt_amd
from rnnt_amd import engine
from rnnt_amd.parallel import shard_utterances
from tests import align_oracle
from tests import latency_reg_oracle as lro
from tests import restricted_oracle as ro
from tests.helpers import (BF16_GRAD_RTOL, BF16_LOSS_RTOL, GRAD_RTOL, LOSS_RTOL, assert_close_grad, assert_close_loss,
                           make_inputs)

pytestmark = pytest.mark.gpu

ROUTES = ("fp32", "f16x2", "bf16x3", "bf16")
WINDOWS = ((0, 0), (2, 1), (0, 3))
GRADS = ("grad_enc", "grad_pred", "grad_W", "grad_bias")


def _dev(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _case(kind, seed=7, B=4, T=23, U=9, H=128, V=128):
    """(inputs, frames of the float64 Viterbi path): computed once, never changed afterwards."""
    d = make_inputs(B, T, U, H, V, seed=seed, ragged=(kind != "uniform"))
    if kind == "ragged":
        d["logit_lens"][-1] = 1   # a one-frame utterance
        d["target_lens"][-2] = 0  # one without labels
    _, frames = ro.viterbi_frames(d)
    return d, frames


@functools.lru_cache(maxsize=None)
def _ref(kind, window, bf16=False, lam=0.0, dp=0.0, **case):
    d, frames = _case(kind, **case)
    if bf16:
        return ro.fused_bf16(d, frames, *window, lam, dp)
    return ro.fused(d, frames, *window, lam, dp, want_occupancy=True)


@functools.lru_cache(maxsize=None)
def _plain_ref(kind, **case):
    return lro.fused(_case(kind, **case)[0])


def _run(d, dtype, frames=None, window=(0, 0), lam=0.0, dp=0.0, grad_scale=None, check_lengths=True):
    g = _dev(d)
    leaves = [g[k].requires_grad_(True) for k in ("enc", "pred", "W", "bias")]
    kw = {}
    if lam:
        kw["fastemit_lambda"] = lam
    if dp:
        kw["delay_penalty"] = dp
    if frames is not None:
        f = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames, dtype=np.int32)).cuda()
        kw.update(restrict_frames=f, restrict_left=window[0], restrict_right=window[1])
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


def _moved(ref, plain):
    return max(np.abs(ref[k] - plain[k]).max() / np.abs(plain[k]).max() for k in GRADS)


@pytest.mark.parametrize("kind", ["uniform", "ragged"])
@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "l%dr%d" % w)
@pytest.mark.parametrize("route", ROUTES)
def test_route_matches_the_oracle(route, window, kind):
    d, frames = _case(kind)
    ref = _ref(kind, window, bf16=route == "bf16")
    _compare(_run(d, route, frames, window), ref, bf16=route == "bf16")
    assert _moved(_ref(kind, window), _plain_ref(kind)) > 10 * GRAD_RTOL  # a call that restricted nothing cannot pass


WAVE = dict(seed=5, B=3, T=40, U=70)


@pytest.mark.parametrize("window", [(0, 0), (2, 1)], ids=lambda w: "l%dr%d" % w)
@pytest.mark.parametrize("route", ["fp32", "f16x2"])
def test_chained_sweep_across_a_wave_boundary(route, window):
    """U1 = 71: lattice columns 63 | 64 sit in two waves of the chained sweep, which hands -inf through its mailbox wherever the
    column is unreachable; T + U is no multiple of the sweep's prefetch block of 6, so the tail steps run too."""
    d, frames = _case("ragged", **WAVE)
    U1, D = d["pred"].shape[1], d["enc"].shape[1] + d["pred"].shape[1] - 1
    assert U1 == 71 and (d["enc"].shape[1] + U1 - 1) % 6 != 0 and ((U1 + 63) // 64 - 1) * D * 12 <= 64 * 1024
    ref = _ref("ragged", window, **WAVE)
    if window == (0, 0):
        occ, Tb = ref["occupancy"][0], int(d["logit_lens"][0])
        assert d["target_lens"][0] == 70 and all((occ[:Tb, u] == 0).mean() > 0.5 for u in (63, 64))
    _compare(_run(d, route, frames, window), ref)
    assert _moved(ref, _plain_ref("ragged", **WAVE)) > 10 * GRAD_RTOL


def test_barrier_sweep_on_a_restricted_lattice():
    """One long utterance whose mailboxes do not fit in LDS: launch_lattice takes the barrier sweep (k_lattice)."""
    T, U = 1700, 192
    NW, D = (U + 1 + 63) // 64, T + U
    assert (NW - 1) * D * 12 > 64 * 1024  # launch_lattice's test for the chained sweep fails
    d = make_inputs(1, T, U, 128, 128, seed=13, ragged=False)
    _, logits = ro._joint_fwd_numpy(d["enc"], d["pred"], d["W"], d["bias"])
    _, frames = ro.viterbi_frames(d, logits=logits)
    ref = ro.fused(d, frames, 2, 1, numpy_joint=True, want_occupancy=True)
    assert np.isfinite(ref["costs"]).all() and (ref["occupancy"][0] == 0).mean() > 0.5
    r = _run(d, "fp32", frames, (2, 1))
    engine.release_workspaces()
    _compare(r, ref)


@pytest.mark.parametrize("route", ROUTES)
def test_zero_window_around_the_engines_own_alignment(route):
    d, _ = _case("ragged")
    g = _dev(d)
    scores, frames = rnnt_amd.joint_rnnt_align(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"],
                                               g["target_lens"], dtype=route)
    r = _run(d, route, frames, (0, 0))
    assert_close_loss("costs", r["costs"], -scores.cpu().numpy().astype(np.float64))


@pytest.mark.parametrize("route", ROUTES)
def test_wide_window_is_the_plain_loss(route):
    d, frames = _case("ragged")
    T = d["enc"].shape[1]
    _compare(_run(d, route, frames, (T, T)), _run(d, route), bf16=route == "bf16")


def _model(H=128, V=64, seed=0):
    torch.manual_seed(seed)
    return rnnt_amd.RNNTModel(torch.nn.Embedding(V, H), _Enc(), rnnt_amd.JointNetwork(-1, -1, H, V)).cuda()


class _Enc(torch.nn.Module):
    def forward(self, x):
        return x

    def calc_output_lens(self, lens):
        return lens


def _batch(B=3, T=17, U=6, H=128, V=64, seed=1):
    gen = torch.Generator().manual_seed(seed)
    return dict(mel=torch.randn(B, H, T, generator=gen).cuda(), lens=torch.tensor([T, 11, 1]).cuda(),
                ids=torch.randint(0, V - 1, (B, U), generator=gen).cuda(), id_lens=torch.tensor([U, 0, 4]).cuda())


@pytest.mark.parametrize("route", ROUTES)
def test_off_is_off(route):
    """restrict_frames=None runs today's entries: bit-identical to the engine's existing calls."""
    d, _ = _case("ragged")
    g = _dev(d)
    B = d["enc"].shape[0]
    old = [o.clone() for o in engine.joint_loss_fwd_bwd(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"],
                                                        g["target_lens"], 127, 1.0 / B, dtype=route)]
    leaves = [g[k].clone().requires_grad_(True) for k in ("enc", "pred", "W", "bias")]
    loss, costs = rnnt_amd.joint_rnnt_loss(*leaves, g["targets"], g["logit_lens"], g["target_lens"], return_costs=True,
                                           dtype=route, restrict_frames=None, restrict_left=3, restrict_right=3)
    loss.backward()
    assert torch.equal(costs, old[0])
    for t, o in zip(leaves, old[1:]):
        assert torch.equal(t.grad, o)
    with torch.no_grad():
        _, c_ng = rnnt_amd.joint_rnnt_loss(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"],
                                           return_costs=True, dtype=route, restrict_frames=None)
    assert torch.equal(c_ng, engine.joint_loss_fwd(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"],
                                                   g["target_lens"], 127, dtype=route))
    # the standalone loss
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((3, 9, 5, 12)).astype(np.float32)).cuda()
    t = torch.from_numpy(np.random.default_rng(3).integers(0, 11, (3, 4)).astype(np.int32)).cuda()
    ll, tl = torch.tensor([9, 1, 6], dtype=torch.int32).cuda(), torch.tensor([4, 2, 0], dtype=torch.int32).cuda()
    c0, g0 = engine.loss_fwd_bwd(x, t, ll, tl, 11, 0.3)
    c0, g0 = c0.clone(), g0.clone()
    xr = x.clone().requires_grad_(True)
    c1 = rnnt_amd.rnnt_loss(xr, t, ll, tl, blank=11, clamp=0.3, reduction="none", restrict_frames=None)
    c1.sum().backward()
    assert torch.equal(c0, c1) and torch.equal(g0, xr.grad)
    # the model: the reference's five positional arguments, with and without the keyword
    V = 128  # (the bf16 route takes no padded vocabulary)
    model, b = _model(V=V), _batch(V=V)
    model.joint.compute_dtype = route
    model.restrict_left, model.restrict_right = 2, 1  # without frames they do nothing
    got = []
    for kw in ({}, dict(restrict_frames=None)):
        model.zero_grad(set_to_none=True)
        loss = model(b["mel"], b["lens"], b["ids"], b["id_lens"], V - 1, **kw)
        loss.backward()
        got.append([loss.detach().clone()] + [p.grad.clone() for p in model.parameters()])
    assert all(torch.equal(x, y) for x, y in zip(*got))


@pytest.mark.parametrize("kind", ["uniform", "ragged"])
@pytest.mark.parametrize("route", ROUTES)
def test_fastemit_and_delay_penalty_compose_with_the_restriction(route, kind):
    d, frames = _case(kind)
    ref = _ref(kind, (2, 1), bf16=route == "bf16", lam=0.5, dp=0.05)
    _compare(_run(d, route, frames, (2, 1), 0.5, 0.05), ref, bf16=route == "bf16")
    lat = (lro.fused_bf16 if route == "bf16" else lro.fused)(d, 0.5, 0.05)
    assert _moved(ref, lat) > 10 * (BF16_GRAD_RTOL if route == "bf16" else GRAD_RTOL)


@pytest.mark.parametrize("lam,dp", [(0.0, 0.0), (0.5, 0.05)])
@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
def test_standalone_loss_with_clamp_and_a_blank_inside_the_vocabulary(reduction, lam, dp):
    rng = np.random.default_rng(5)
    B, T, U, V, blank, clamp, window = 3, 13, 6, 20, 5, 0.3, (2, 1)
    logits = (rng.standard_normal((B, T, U + 1, V)) * 2).astype(np.float32)
    targets = rng.integers(0, V - 1, (B, U))
    targets = (targets + (targets >= blank)).astype(np.int32)  # every label but the blank
    ll, tl = np.array([13, 1, 9], dtype=np.int32), np.array([6, 3, 0], dtype=np.int32)
    _, frames, _ = align_oracle.viterbi_logits(logits, targets, ll, tl, blank)
    x = torch.from_numpy(logits).cuda().requires_grad_(True)
    out = rnnt_amd.rnnt_loss(x, *(torch.from_numpy(a).cuda() for a in (targets, ll, tl)), blank=blank, clamp=clamp,
                             reduction=reduction, fastemit_lambda=lam, delay_penalty=dp,
                             restrict_frames=torch.from_numpy(frames).cuda(), restrict_left=window[0], restrict_right=window[1])
    (out.sum() if reduction == "none" else out).backward()
    costs, G = ro.loss_and_grad(logits, targets, ll, tl, frames, *window, blank, lam, dp, clamp=clamp)
    want = {"none": costs, "mean": costs.mean(), "sum": costs.sum()}[reduction]
    assert_close_loss("loss", out.detach().cpu().numpy(), want)
    assert_close_grad("grad_logits", x.grad.cpu().numpy(), G * (1.0 / B if reduction == "mean" else 1.0))
    assert (np.abs(G) >= clamp).any()  # the clamp is active on the restricted gradient
    c0, G0 = lro.loss_and_grad(logits, targets, ll, tl, blank, lam, dp, clamp=clamp)
    assert np.abs(G - G0).max() > 10 * GRAD_RTOL * np.abs(G0).max() and (costs > c0).any()


@pytest.mark.parametrize("lam", [0.0, 0.5])
@pytest.mark.parametrize("route", ["fp32", "f16x2"])
def test_infeasible_utterance(route, lam):
    d, frames = _case("uniform")
    bad = frames.copy()
    bad[1, 3], bad[1, 4] = 15, 2  # label 4 of utterance 1 would have to come before label 3: no path survives
    window = (2, 1)
    ref = ro.fused(d, bad, *window, lam)
    assert ref["costs"][1] == np.inf and np.isfinite(np.delete(ref["costs"], 1)).all()
    r = _run(d, route, bad, window, lam, check_lengths=False)
    assert r["costs"][1] == np.inf
    assert (r["grad_enc"][1] == 0.0).all() and (r["grad_pred"][1] == 0.0).all()
    assert_close_loss("feasible costs", np.delete(r["costs"], 1), np.delete(ref["costs"], 1))
    for k in GRADS:
        assert np.isfinite(r[k]).all(), k
        assert_close_grad(k, r[k], ref[k])


@pytest.mark.parametrize("route", ROUTES)
def test_nan_row_poisons_only_its_utterance(route):
    d, frames = _case("uniform")
    d = dict(d, enc=d["enc"].copy())
    d["enc"][1, 4, :] = np.nan
    g = _dev(d)
    f = torch.from_numpy(frames).cuda()
    a = (g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"], 127)
    c = engine.joint_loss_fwd_bwd_restrict(*a, 0.25, 0.0, 0.0, f, 2, 1, dtype=route)[0].cpu().numpy()
    c_ng = engine.joint_loss_fwd_restrict(*a, 0.0, f, 2, 1, dtype=route).cpu().numpy()
    ref = _ref("uniform", (2, 1), bf16=route == "bf16")["costs"]
    for cc in (c, c_ng):
        assert np.isnan(cc[1])
        assert_close_loss("clean costs", np.delete(cc, 1), np.delete(ref, 1), rtol=BF16_LOSS_RTOL if route == "bf16" else LOSS_RTOL)


def test_host_checks():
    d, frames = _case("ragged")
    g = _dev(d)
    f = torch.from_numpy(frames).cuda()
    assert (frames[-2] == -1).all() and d["target_lens"][-2] == 0  # dead entries may hold anything: -1 here

    def call(fr, left=0, right=0, check_lengths=True):
        return rnnt_amd.joint_rnnt_loss(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"],
                                        dtype="fp32", check_lengths=check_lengths, restrict_frames=fr, restrict_left=left,
                                        restrict_right=right)

    assert torch.isfinite(call(f))  # a valid alignment is a surviving path
    Tb = int(d["logit_lens"][0])
    for u, v in ((0, -1), (int(d["target_lens"][0]) - 1, Tb)):
        bad = f.clone()
        bad[0, u] = v
        with pytest.raises(ValueError, match="outside"):
            call(bad)
    assert d["target_lens"][0] >= 3 and Tb >= 2
    bad = f.clone()
    bad[0, 1], bad[0, 2] = Tb - 1, 0  # in range, but label 2 before label 1
    with pytest.raises(ValueError, match="non-decreasing"):
        call(bad)
    assert torch.isinf(call(bad, check_lengths=False))  # unchecked: no error, and no path
    for kw in (dict(left=-1), dict(right=-1)):
        with pytest.raises(ValueError, match="restrict_"):
            call(f, **kw)
    with pytest.raises(RuntimeError, match="int32"):
        call(f.long())
    with pytest.raises(RuntimeError, match="shape"):
        call(f[:, :-1].contiguous())
    with pytest.raises(RuntimeError, match="contiguous"):
        call(torch.stack([f, f], dim=2)[:, :, 0])
    with pytest.raises(RuntimeError, match="HIP device"):
        call(f.cpu())
    lg = engine.joint_fwd(g["enc"], g["pred"], g["W"], g["bias"])
    with pytest.raises(ValueError, match="outside"):
        bad = f.clone()
        bad[0, 0] = -1
        rnnt_amd.rnnt_loss(lg, g["targets"], g["logit_lens"], g["target_lens"], restrict_frames=bad)


def test_model_passes_the_restriction_to_the_loss():
    V = 64
    model, b = _model(V=V), _batch(V=V)
    model.restrict_left, model.restrict_right = 2, 1
    _, frames = model.align(b["mel"], b["lens"], b["ids"], b["id_lens"], V - 1)
    loss = model(b["mel"], b["lens"], b["ids"], b["id_lens"], V - 1, restrict_frames=frames)
    loss.backward()
    got = {n: p.grad.clone() for n, p in model.named_parameters()}
    plain = model(b["mel"], b["lens"], b["ids"], b["id_lens"], V - 1)
    assert loss.item() > plain.item()  # fewer paths
    model.zero_grad(set_to_none=True)
    start = torch.full((3, 1), V - 1, dtype=b["ids"].dtype, device="cuda")
    dec = model.predictor(torch.cat([start, b["ids"]], dim=1))
    loss2 = rnnt_amd.joint_rnnt_loss(b["mel"].permute(0, 2, 1), dec, model.joint.joint_ln.weight, model.joint.joint_ln.bias,
                                     b["ids"].int(), b["lens"].int(), b["id_lens"].int(), restrict_frames=frames,
                                     restrict_left=2, restrict_right=1)
    loss2.backward()
    assert loss.item() == loss2.item()
    for n, p in model.named_parameters():
        assert torch.equal(got[n], p.grad), n


def test_restricted_step_as_a_hip_graph():
    V = 64
    model = _model(V=V, seed=3)
    model.check_lengths = False
    model.restrict_left, model.restrict_right = 2, 1
    b0, b1 = _batch(V=V, seed=7), _batch(V=V, seed=8)
    for b in (b0, b1):
        b["frames"] = model.align(b["mel"], b["lens"], b["ids"], b["id_lens"], V - 1)[1]
    static = {k: v.clone() for k, v in b0.items()}
    params = list(model.parameters())

    def fwd_bwd():
        loss = model(static["mel"], static["lens"], static["ids"], static["id_lens"], V - 1, restrict_frames=static["frames"])
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
        assert np.isfinite(got_loss) and got_loss == want_loss
        for (name, p), g in zip(model.named_parameters(), got):
            assert torch.equal(g, p.grad), name
        for p, g in zip(params, static_grads):
            p.grad = g


@pytest.mark.parametrize("route", ["fp32", "f16x2"])
def test_half_batch_calls_sum_to_the_full_batch(route):
    d, frames = _case("ragged")
    B, window, lam, dp = 4, (2, 1), 0.5, 0.05
    full = _run(d, route, frames, window, lam, dp, grad_scale=1.0 / B)
    keys = ("enc", "pred", "targets", "logit_lens", "target_lens")
    parts = []
    for rank in range(2):
        *per_utt, f = shard_utterances(2, rank, *(torch.from_numpy(d[k]) for k in keys), torch.from_numpy(frames))
        sub = dict(d, **{k: v.numpy() for k, v in zip(keys, per_utt)})
        assert f.shape[0] == 2 and f.is_contiguous()
        parts.append(_run(sub, route, f.numpy(), window, lam, dp, grad_scale=1.0 / B, check_lengths=False))
    assert_close_loss("costs", np.concatenate([p["costs"] for p in parts]), full["costs"])
    for k in ("grad_enc", "grad_pred"):
        assert_close_grad(k, np.concatenate([p[k] for p in parts]), full[k])
    for k in ("grad_W", "grad_bias"):
        assert_close_grad(k, parts[0][k] + parts[1][k], full[k])
    assert shard_utterances(2, 0, None, torch.from_numpy(frames))[0] is None  # an option that is off passes through


def test_f16x2_backward_skips_the_unreachable_tiles():
    """Dead cells carry the coefficients of a cell outside the lattice, so the f16x2 backward's live-tile list (8 t x 16 u tiles)
    holds no tile without a reachable cell."""
    d, frames = _case("ragged", **WAVE)
    B, T, H = d["enc"].shape
    U1, V = d["pred"].shape[1], d["W"].shape[0]
    dev = torch.device("cuda", torch.cuda.current_device())
    _run(d, "f16x2")
    plain = engine.x2_live_counts(dev, B, T, U1, H, V)
    _run(d, "f16x2", frames, (0, 0))
    narrow = engine.x2_live_counts(dev, B, T, U1, H, V)
    occ = _ref("ragged", (0, 0), **WAVE)["occupancy"] > 0
    nt, nu = (T + 7) // 8, (U1 + 15) // 16
    assert narrow["tiles"] == plain["tiles"] == B * nt * nu
    pad = np.zeros((B, nt * 8, nu * 16), dtype=bool)
    pad[:, :T, :U1] = occ
    reachable_tiles = int(pad.reshape(B, nt, 8, nu, 16).any(axis=(2, 4)).sum())
    assert 0 < narrow["live_tiles"] <= reachable_tiles < plain["live_tiles"]
    assert narrow["live_ksteps"] < plain["live_ksteps"]
