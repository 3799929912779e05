"""-m gpu: forced alignment on the device (rnnt_engine_align / rnnt_engine_joint_align) against the float64 oracle
of tests/align_oracle.py on every route, at the full config-2 lattice, on exact ties, single-path utterances, reruns, poisoned
workspaces, non-finite inputs, and through JointNetwork.align / RNNTModel.align."""
import numpy as np
import pytest
import torch

import rnnt_amd
from tests import align_oracle as ao
from tests.helpers import BF16_LOSS_RTOL_EXACT, LOSS_RTOL, DECODE_CASES, load_decode_case, make_inputs

pytestmark = pytest.mark.gpu

MARGIN = 1e-3  # frames must equal the oracle's where every decision on its path is won by more than this
ROUTES = ("fp32", "f16x2", "bf16x3", "bf16")


def _cuda(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def _oracle_logits(d):
    """float64 logits of the joint (reference rnnt/joint.py:32-39) from a make_inputs dict."""
    enc, pred = d["enc"].astype(np.float64), d["pred"].astype(np.float64)
    hidden = np.tanh(enc[:, :, None, :] + pred[:, None, :, :])
    return hidden @ d["W"].astype(np.float64).T + d["bias"].astype(np.float64)


def _ragged(B, T, U, H, V, seed):
    d = make_inputs(B, T, U, H, V, seed=seed)
    d["W"] *= 4.0  # logits spread over a few units: decisions on a path are rarely within the margin
    if B > 2:
        d["logit_lens"][-1] = 1  # a one-frame utterance
        d["target_lens"][-2] = 0  # one without labels
    return d


def _check_against_oracle(scores, frames, ref_scores, ref_frames, margins, tl, rtol=LOSS_RTOL, what=""):
    scores, frames = scores.cpu().numpy().astype(np.float64), frames.cpu().numpy()
    assert frames.shape == ref_frames.shape, (what, frames.shape, ref_frames.shape)
    rel = np.abs(scores - ref_scores) / np.maximum(np.abs(ref_scores), 1e-12)
    assert rel.max() <= rtol, (what, scores, ref_scores)
    counted = 0
    for b in range(len(scores)):
        Ub = int(tl[b])
        assert (frames[b, Ub:] == -1).all(), (what, b)
        f = frames[b, :Ub]
        assert Ub == 0 or (f.min() >= 0 and (np.diff(f) >= 0).all()), (what, b, f)
        if margins[b] > MARGIN:
            counted += 1
            assert (f == ref_frames[b, :Ub]).all(), (what, b, f, ref_frames[b, :Ub])
    return counted


@pytest.mark.parametrize("U", [0, 1, 63, 64, 200, 1023])
def test_both_entries_match_the_oracle(U):
    B, T, H, V = (5, 23, 64, 32) if U < 1000 else (3, 9, 32, 16)
    total = 0
    for seed in range(2):
        d = _ragged(B, T, U, H, V, seed=100 * U + seed)
        logits = _oracle_logits(d)
        ref = ao.viterbi_logits(logits, d["targets"], d["logit_lens"], d["target_lens"], V - 1)
        g = _cuda(d)
        lg32 = torch.from_numpy(logits.astype(np.float32)).cuda()
        # the materialised-logits entry, against the oracle on the same fp32 logits
        ref32 = ao.viterbi_logits(logits.astype(np.float32), d["targets"], d["logit_lens"], d["target_lens"], V - 1)
        s, f = rnnt_amd.rnnt_align(lg32, g["targets"], g["logit_lens"], g["target_lens"])
        total += _check_against_oracle(s, f, *ref32, d["target_lens"], what=("logits", U, seed))
        for route in ("fp32", "f16x2"):
            s, f = rnnt_amd.joint_rnnt_align(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"],
                                             g["target_lens"], dtype=route)
            total += _check_against_oracle(s, f, *ref, d["target_lens"], what=(route, U, seed))
    assert total >= 3 * 2 * B * 0.5  # the margin filter leaves most utterances in


@pytest.mark.parametrize("route", ROUTES)
def test_every_route(route):
    B, T, U, H, V = 4, 40, 17, 128, 256
    d = _ragged(B, T, U, H, V, seed=7)
    ref = ao.viterbi_logits(_oracle_logits(d), d["targets"], d["logit_lens"], d["target_lens"], V - 1)
    g = _cuda(d)
    s, f = rnnt_amd.joint_rnnt_align(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"],
                                     dtype=route)
    if route != "bf16":
        assert _check_against_oracle(s, f, *ref, d["target_lens"], what=route) >= B - 1
        return
    # bf16 operands: the bar of its loss tests against the unrounded oracle; the path it returns, rescored in float64, is
    # within that bar of the best one
    _check_against_oracle(s, f, ref[0], ref[1], np.zeros(B), d["target_lens"], rtol=BF16_LOSS_RTOL_EXACT, what=route)
    logits = _oracle_logits(d)
    for b in range(B):
        lpb, lpe = ao.lattice_logprobs(logits[b], d["targets"][b], V - 1)
        Tb, Ub = int(d["logit_lens"][b]), int(d["target_lens"][b])
        r = ao.rescore(lpb, lpe, f[b].cpu().numpy(), Tb, Ub)
        assert abs(r - ref[0][b]) <= BF16_LOSS_RTOL_EXACT * abs(ref[0][b]), (b, r, ref[0][b])


@pytest.mark.parametrize("route", ["f16x2", "fp32"])
def test_full_config2_lattice(route):
    """One utterance at config 2's T, U, H, V; oracle log-probs from float64 torch on the device."""
    T, U, H, V = 1000, 200, 512, 1024
    d = make_inputs(1, T, U, H, V, seed=2024)
    g = _cuda(d)
    s, f = rnnt_amd.joint_rnnt_align(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"],
                                     dtype=route)
    with torch.no_grad():
        enc, pred, W, bias = (g[k].double() for k in ("enc", "pred", "W", "bias"))
        lpb = torch.empty(T, U + 1, dtype=torch.float64, device="cuda")
        lpe = torch.zeros(T, U + 1, dtype=torch.float64, device="cuda")
        tg = g["targets"][0].long()
        for t0 in range(0, T, 100):  # 100 frames at a time: 1.6 GB of float64 logits per chunk
            lp = torch.log_softmax(torch.tanh(enc[0, t0:t0 + 100, None, :] + pred[0, None, :, :]) @ W.T + bias, dim=-1)
            lpb[t0:t0 + 100] = lp[..., V - 1]
            lpe[t0:t0 + 100, :U] = lp[:, :U, :].gather(-1, tg.view(1, U, 1).expand(lp.shape[0], U, 1))[..., 0]
            del lp
    lpb, lpe = lpb.cpu().numpy(), lpe.cpu().numpy()
    best, ref_frames, margin = ao.viterbi(lpb, lpe, T, U)
    got = ao.rescore(lpb, lpe, f[0].cpu().numpy(), T, U)
    assert abs(got - best) <= LOSS_RTOL * abs(best), (got, best)
    assert abs(float(s[0]) - best) <= LOSS_RTOL * abs(best), (float(s[0]), best)
    assert abs(got - float(s[0])) <= LOSS_RTOL * abs(best), (got, float(s[0]))
    if margin > MARGIN:
        assert (f[0].cpu().numpy() == ref_frames).all()


@pytest.mark.parametrize("route", ["f16x2", "fp32", "bf16x3"])
def test_exact_ties_emit_every_label_at_frame_zero(route):
    B, T, U, H, V = 3, 30, 12, 128, 128
    d = _ragged(B, T, U, H, V, seed=5)
    d["W"][:] = 0.0
    d["bias"][:] = 0.0
    g = _cuda(d)
    s, f = rnnt_amd.joint_rnnt_align(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"],
                                     dtype=route)
    f = f.cpu().numpy()
    for b in range(B):
        Ub = int(d["target_lens"][b])
        assert (f[b, :Ub] == 0).all() and (f[b, Ub:] == -1).all(), (b, f[b])
        n = int(d["logit_lens"][b]) + Ub
        assert float(s[b]) == pytest.approx(-n * np.log(V), rel=1e-6)


@pytest.mark.parametrize("route", ["f16x2", "fp32"])
def test_single_path_scores_equal_minus_the_loss(route):
    B, T, U, H, V = 6, 31, 9, 128, 128
    d = make_inputs(B, T, U, H, V, seed=11)
    d["logit_lens"] = np.array([T, 1, 1, 12, 20, 5], dtype=np.int32)
    d["target_lens"] = np.array([U, 0, U, 0, 4, U], dtype=np.int32)
    single = (d["logit_lens"] == 1) | (d["target_lens"] == 0)
    g = _cuda(d)
    with torch.no_grad():
        _, costs = rnnt_amd.joint_rnnt_loss(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"],
                                            g["target_lens"], return_costs=True, dtype=route)
    s, _ = rnnt_amd.joint_rnnt_align(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"],
                                     dtype=route)
    s, c = s.cpu().numpy().astype(np.float64), costs.cpu().numpy().astype(np.float64)
    tol = LOSS_RTOL * np.abs(c)
    assert (np.abs(s[single] + c[single]) <= tol[single]).all(), (s, -c)
    assert (s <= -c + tol).all(), (s, -c)
    assert (s[~single] < -c[~single]).all()  # more than one path: the best is strictly below the sum


@pytest.mark.parametrize("route", ["f16x2", "fp32"])
def test_reruns_and_poisoned_workspaces_are_bit_identical(route):
    B, T, U, H, V = 4, 50, 70, 128, 128
    d = _ragged(B, T, U, H, V, seed=21)
    g = _cuda(d)
    args = (g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"])
    s0, f0 = rnnt_amd.joint_rnnt_align(*args, dtype=route)
    s1, f1 = rnnt_amd.joint_rnnt_align(*args, dtype=route)
    lg = torch.from_numpy(_oracle_logits(d).astype(np.float32)).cuda()
    ls0, lf0 = rnnt_amd.rnnt_align(lg, g["targets"], g["logit_lens"], g["target_lens"])
    for pattern in (-1, 0x7FA00000, 0x7F800000):  # quiet NaN, signalling NaN, +inf in every word
        ws = rnnt_amd.engine.workspace(torch.device("cuda", 0), 1)
        ws.view(torch.int32)[: ws.numel() // 4].fill_(pattern)
        s2, f2 = rnnt_amd.joint_rnnt_align(*args, dtype=route)
        ws.view(torch.int32)[: ws.numel() // 4].fill_(pattern)
        ls2, lf2 = rnnt_amd.rnnt_align(lg, g["targets"], g["logit_lens"], g["target_lens"])
        assert torch.equal(s0.view(torch.int32), s2.view(torch.int32)) and torch.equal(f0, f2), pattern
        assert torch.equal(ls0.view(torch.int32), ls2.view(torch.int32)) and torch.equal(lf0, lf2), pattern
    assert torch.equal(s0.view(torch.int32), s1.view(torch.int32)) and torch.equal(f0, f1)
    assert torch.isfinite(s0).all() and torch.isfinite(ls0).all()


@pytest.mark.parametrize("route", ["fp32", "f16x2"])
def test_nan_in_one_utterance(route):
    B, T, U, H, V = 3, 20, 8, 128, 128
    d = make_inputs(B, T, U, H, V, seed=33, ragged=False)
    g = _cuda(d)
    args = lambda e: (e, g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"])  # noqa: E731
    s0, f0 = rnnt_amd.joint_rnnt_align(*args(g["enc"]), dtype=route)
    enc = g["enc"].clone()
    enc[1, 4, 7] = float("nan")
    s, f = rnnt_amd.joint_rnnt_align(*args(enc), dtype=route)
    assert torch.isnan(s[1]) and (f[1] == -1).all(), (s, f[1])
    for b in (0, 2):
        assert torch.equal(s[b].view(torch.int32), s0[b].view(torch.int32)) and torch.equal(f[b], f0[b]), b
    # the materialised-logits entry: a NaN logit in one cell of utterance 0's lattice
    lg = torch.from_numpy(_oracle_logits(d).astype(np.float32)).cuda()
    ls0, lf0 = rnnt_amd.rnnt_align(lg, g["targets"], g["logit_lens"], g["target_lens"])
    lg[0, 3, 2, 5] = float("nan")
    ls, lf = rnnt_amd.rnnt_align(lg, g["targets"], g["logit_lens"], g["target_lens"])
    assert torch.isnan(ls[0]) and (lf[0] == -1).all()
    assert torch.equal(ls[1:], ls0[1:]) and torch.equal(lf[1:], lf0[1:])


class _Enc(torch.nn.Module):
    """Encoder output handed over as is, with a frame-count rule like the reference's strided encoder."""

    def forward(self, x):
        return x

    def calc_output_lens(self, lens):
        return lens


@pytest.mark.parametrize("name", ["decode_small", "decode_small_proj", "decode_ref_widths", "decode_ref_widths_proj"])
def test_model_align_equals_joint_align(golden_dir, name):
    from tests.stream_models import load_into
    spec = DECODE_CASES[name]
    c = load_decode_case(golden_dir, name)
    pred = rnnt_amd.ConvPredictor(spec["V"], spec["O"], spec["E"], 0.3)
    joint = rnnt_amd.JointNetwork(spec["fa"], spec["ft"], spec["H"], spec["V"])
    load_into(pred, c["pred_sd"])
    load_into(joint, c["joint_sd"])
    model = rnnt_amd.RNNTModel(pred, _Enc(), joint).cuda().eval()
    T, C = c["frames"].shape
    rng = np.random.default_rng(len(name))
    B, U = 3, 12
    mel = torch.from_numpy(np.stack([c["frames"].T] * B)).cuda()  # (N, C, L)
    mel[1] = mel[1].roll(5, dims=1)
    lens = torch.tensor([T, T - 7, T // 2], device="cuda")
    ids = torch.from_numpy(rng.integers(0, spec["V"] - 1, (B, U))).cuda()
    id_lens = torch.tensor([U, 5, 0], device="cuda")
    blank = spec["V"] - 1
    s, f = model.align(mel, lens, ids, id_lens, blank)
    assert s.shape == (B,) and f.shape == (B, U) and f.dtype == torch.int32
    with torch.no_grad():
        text = model.predictor(torch.cat([torch.full((B, 1), blank, device="cuda", dtype=ids.dtype), ids], dim=1))
        s2, f2 = joint.align(mel.permute(0, 2, 1), text, ids.int(), lens.int(), id_lens.int())
    assert torch.equal(s.view(torch.int32), s2.view(torch.int32)) and torch.equal(f, f2)
    assert torch.isfinite(s).all()
    for b in range(B):
        Ub = int(id_lens[b])
        fb = f[b].cpu().numpy()
        assert (fb[Ub:] == -1).all() and (Ub == 0 or (fb[:Ub].min() >= 0 and fb[:Ub].max() < int(lens[b])))
        assert (np.diff(fb[:Ub]) >= 0).all()
    # the same alignment from the loss's own lattice: the best path never beats the sum over paths
    with torch.no_grad():
        _, costs = joint.fused_loss(mel.permute(0, 2, 1), text, ids.int(), lens.int(), id_lens.int(), return_costs=True)
    assert (s.double() <= -costs.double() + LOSS_RTOL * costs.double().abs()).all()
