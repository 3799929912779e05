"""GPU tests of rnnt_amd.AudioEncoder's training path (backend "engine" with grad mode on: rnnt_engine_encoder_train_fwd / _bwd through
a torch.autograd.Function) against the gradients recorded from the reference's module in float64 (tests/golden/encoder_train_*.npz).
The bar is the forward file's: for every parameter tensor, max|g - g64| <= 4 x the reference's OWN recorded fp32 error for that
tensor; the bias of a conv that feeds an instance norm has an exactly zero gradient and is held to M 2^-24 sum|dy| per channel.  Both
numbers are printed (profiles/encoder_train_parity.txt holds a run's).  The output is held to the forward's bar."""
import numpy as np
import pytest
import torch

from tests import encoder_train_cases as C
from tests.encoder_cases import e2e_case, fixture, out64

pytestmark = pytest.mark.gpu
FACTOR = 4.0


def _engine(case, regime="auto"):
    enc = C.small_train_encoder(case).cuda()
    enc.backend, enc.conv_regime = "engine", regime
    return enc


def _step(enc, mel, G, keep_masks=None):
    enc.zero_grad()
    out = enc(mel, keep_masks=keep_masks) if keep_masks is not None else enc(mel)
    (out * G).sum().backward()
    return out.detach(), {k: p.grad.detach().clone() for k, p in enc.named_parameters()}


def _np(grads):
    return {k: v.cpu().numpy() for k, v in grads.items()}


@pytest.mark.parametrize("case", C.TRAIN_CASES)
@pytest.mark.parametrize("N", (3, 1))
@pytest.mark.parametrize("regime", ("auto", "many_rows"))
def test_gradients_of_the_recorded_cases(case, N, regime):
    fx, enc = C.train_fixture(case, N), _engine(case, regime)
    ref = fixture(C.norm_of(case))
    mel = torch.from_numpy(ref["mel"])[:N].cuda()
    out, got = _step(enc, mel, torch.from_numpy(fx["G"]).cuda())
    assert enc.last_backend == "engine" and enc.last_saved_bytes > 0
    if case == "instance_affine_la2":
        la = C.lookahead_out()
        want, ref_err = (la["out32"].astype(np.float64) + la["out64_corr"])[:N], float(la["err_out"])
    else:
        want, ref_err = out64(ref)[:N], float(ref["err_whole"])
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - want).max())
    print(f"encoder train parity {case} N={N} ({regime}) output: engine max|y - fp64| = {err:.3e}, reference fp32 error = {ref_err:.3e}, "
          f"bar = {FACTOR * ref_err:.3e}")
    assert out.shape == want.shape and err <= FACTOR * ref_err
    assert out.permute(0, 2, 1).is_contiguous()
    C.check_grads(f"{case} N={N} ({regime})", fx, _np(got), C.bias_rows(enc, N, mel.shape[2]).__getitem__)


def test_no_grad_lookahead_runs_on_the_engine():
    enc = _engine("instance_affine_la2")
    la = C.lookahead_out()
    mel = torch.from_numpy(fixture("instance_affine")["mel"]).cuda()
    with torch.no_grad():
        y = enc(mel)
    assert enc.last_backend == "engine"
    err = float(np.abs(y.cpu().numpy().astype(np.float64) - (la["out32"].astype(np.float64) + la["out64_corr"])).max())
    print(f"encoder parity look-ahead forward: engine max|y - fp64| = {err:.3e}, reference fp32 error = {float(la['err_out']):.3e}")
    assert err <= FACTOR * float(la["err_out"])
    enc.backend = "auto"
    with torch.no_grad():
        enc(mel[:1, :, :20])
    assert enc.last_backend == "torch"  # "auto" keeps look-ahead modules on torch


def _dropout_encoders(p=0.5):
    out = []
    for dtype in (torch.float32, torch.float64):
        enc = C.small_train_encoder("instance_affine").to(dtype).train()
        for m in enc.blocks:
            if hasattr(m, "dropout"):
                m.dropout.p = p
        out.append(enc)
    return out


def _mask_shapes(enc, N, L):
    rows, _ = enc._lengths(L, None)
    inside = {id(c) for m in enc.blocks if hasattr(m, "convs") for c in m.convs}
    return [(N, r[2], c.conv.out_channels) for c, r in zip(enc._causal_convs(), rows) if id(c) in inside]


def test_dropout_with_explicit_masks_against_the_torch_path_in_float64():
    """p = 0.5, the same masks on every path.  Bar per tensor: 4 x the fp32 torch path's own error on this case; for the exactly zero
    bias gradients in front of the instance norms: M 2^-24 sum|dy| from the float64 run (a hook on the conv's output)."""
    enc32, enc64 = _dropout_encoders()
    fx = fixture("instance_affine")
    mel = torch.from_numpy(fx["mel"])
    g = torch.Generator().manual_seed(11)
    masks = [(torch.rand(s, generator=g) >= 0.5).to(torch.uint8) for s in _mask_shapes(enc32, 3, 101)]
    G = torch.randn(3, 36, 50, generator=g)
    dyabs, handles = {}, []
    names = {id(m): n for n, m in enc64.named_modules()}
    for m in enc64.modules():
        if isinstance(m, torch.nn.Conv1d) and m is not enc64.blocks[-1]:
            handles.append(m.register_full_backward_hook(
                lambda mod, gi, go: dyabs.__setitem__(names[id(mod)] + ".bias", go[0].abs().sum(dim=(0, 2)).numpy())))
    o64, g64 = _step(enc64, mel.double(), G.double(), masks)
    for h in handles:
        h.remove()
    o32, g32 = _step(enc32, mel, G, masks)
    eng = C.small_train_encoder("instance_affine").cuda().train()
    for m in eng.blocks:
        if hasattr(m, "dropout"):
            m.dropout.p = 0.5
    eng.backend = "engine"
    oe, ge = _step(eng, mel.cuda(), G.cuda(), [m.cuda() for m in masks])
    assert eng.last_backend == "engine"
    e_ref, e = float((o32.double() - o64).abs().max()), float((oe.cpu().double() - o64).abs().max())
    print(f"encoder train dropout output: engine {e:.3e}, torch fp32 {e_ref:.3e}")
    assert e <= FACTOR * e_ref
    rows = C.bias_rows(enc32, 3, 101)
    bad = []
    for k in g64:
        d = (ge[k].cpu().double() - g64[k]).abs()
        if k in dyabs:
            bound = torch.from_numpy(rows[k] * 2.0 ** -24 * dyabs[k])
            print(f"encoder train dropout {k}: exactly zero; engine max|g| = {float(d.max()):.3e}, bound >= {float(bound.min()):.3e}")
            ok = bool((d <= bound).all())
        else:
            ref = float((g32[k].double() - g64[k]).abs().max())
            print(f"encoder train dropout {k}: engine max|g - g64| = {float(d.max()):.3e}, torch fp32 = {ref:.3e}, bar = {FACTOR * ref:.3e}")
            ok = float(d.max()) <= FACTOR * ref
        if not ok:
            bad.append(k)
    assert not bad, bad


def test_drawn_masks_follow_the_seed_and_keep_the_right_fraction():
    eng = C.small_train_encoder("instance_affine").cuda().train()
    for m in eng.blocks:
        if hasattr(m, "dropout"):
            m.dropout.p = 0.25
    eng.backend = "engine"
    mel = torch.from_numpy(fixture("instance_affine")["mel"]).cuda()
    outs = []
    for seed in (5, 5, 6):
        torch.manual_seed(seed)
        y = eng(mel)
        masks = [m for m in y.grad_fn.call[4] if m is not None]
        assert len(masks) == 5 and all(m.dtype == torch.uint8 and m.is_cuda for m in masks)
        n = sum(m.numel() for m in masks)
        kept = sum(int(m.sum()) for m in masks)
        assert abs(kept - 0.75 * n) <= 5.0 * (n * 0.75 * 0.25) ** 0.5, (kept, n)
        outs.append(y.detach().clone())
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    eng.eval()
    assert all(m is None for m in eng(mel).grad_fn.call[4])  # eval(): nothing is drawn


def test_identical_calls_give_identical_bits():
    enc = _engine("instance_affine")
    mel = torch.from_numpy(fixture("instance_affine")["mel"]).cuda()
    G = torch.from_numpy(C.train_fixture("instance_affine", 3)["G"]).cuda()
    (a, ga), (b, gb) = _step(enc, mel, G), _step(enc, mel, G)
    assert torch.equal(a, b) and all(torch.equal(ga[k], gb[k]) for k in ga)


def test_an_optimizer_step_rebuilds_both_packed_tables():
    """After one rnnt_amd.optim.AdamW step the next forward and backward agree with the torch path on the new weights (a stale forward table
    would show in the output, a stale transposed table in the gradients of every layer in front of it)."""
    import rnnt_amd
    enc = _engine("batch")
    mel = torch.from_numpy(fixture("batch")["mel"]).cuda()
    G = torch.from_numpy(C.train_fixture("batch", 3)["G"]).cuda()
    opt = rnnt_amd.optim.AdamW(enc.parameters(), lr=0.05)
    y0, g0 = _step(enc, mel, G)
    table = enc._train_packed
    opt.step()
    y1, g1 = _step(enc, mel, G)
    assert enc._train_packed is not table and enc.last_backend == "engine"
    enc.backend = "torch"
    yt, gt = _step(enc, mel, G)
    assert (y1 - y0).abs().max().item() > 0.05
    assert (y1 - yt).abs().max().item() <= 1e-4 * max(1.0, yt.abs().max().item())
    for k in gt:  # (AdamW at lr 0.05 moves every weight by about 0.05: a stale table is wrong in the first digit)
        assert (g1[k] - gt[k]).abs().max().item() <= 1e-3 * max(1.0, gt[k].abs().max().item()), k
    assert max((g1[k] - g0[k]).abs().max().item() for k in gt) > 1e-2
    enc.repack()
    assert enc._train_packed is None and enc._cache is None


def test_refusals_raise_and_launch_nothing():
    enc = _engine("batch")
    mel = torch.from_numpy(fixture("batch")["mel"]).cuda()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="requires grad"):
        enc(mel.clone().requires_grad_())
    enc.train()  # batch norm on batch statistics
    with pytest.raises(RuntimeError, match="batch statistics"):
        enc(mel)
    enc.eval()
    with pytest.raises(RuntimeError, match="fp32"):
        enc.double()(mel.double())
    enc.float()
    with pytest.raises(RuntimeError, match="grad mode"):
        enc.streaming_forward(mel[:, :, :20], [s.cuda() for s in enc.streaming_init_state(3)])
    assert enc.last_saved_bytes is None  # no training forward ran
    enc.backend = "auto"
    assert enc(mel).requires_grad and enc.last_backend == "torch"  # "auto" keeps grad-mode calls on torch
    frozen = _engine("batch").train()
    for m in frozen.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.eval()
    assert frozen(mel).requires_grad and frozen.last_backend == "engine"  # train() with frozen batch norms is the supported mode


def test_one_training_step_end_to_end():
    """A small RNNTModel (engine ConvPredictor and joint) with the encoder on "engine" against the same model with the encoder on
    "torch": loss and encoder gradients within 4 x the torch-encoder step's own error against a float64 CPU copy of the step."""
    from oracle import torch_check
    from tests.stream_models import cpu_model, engine_model
    spec, enc, mel1, pred_sd, joint_sd = e2e_case()
    g = torch.Generator().manual_seed(21)
    mel = torch.cat([mel1, torch.randn(1, 9, 101, generator=g)])
    mel_lens = torch.tensor([101, 90])
    U = 6
    ids = torch.randint(0, spec["V"] - 1, (2, U), generator=g)
    id_lens = torch.tensor([U, U - 2])
    blank = spec["V"] - 1
    import copy
    ref = cpu_model(spec, pred_sd, joint_sd, encoder=copy.deepcopy(enc)).double()
    start = torch.full((2, 1), blank, dtype=ids.dtype)
    audio = ref.encoder(mel.double()).permute(0, 2, 1)
    text = ref.predictor(torch.cat([start, ids], dim=1))
    a, t = ref.joint._project(audio, text)
    logits = torch_check.joint_torch(a, t, ref.joint.joint_ln.weight, ref.joint.joint_ln.bias)
    loss64 = torch_check.rnnt_loss_torch(logits, ids, ref.encoder.calc_output_lens(mel_lens), id_lens, blank=-1, reduction="mean")[0]
    loss64.backward()
    g64 = {k: p.grad for k, p in ref.encoder.named_parameters()}
    got = {}
    for backend in ("torch", "engine"):
        model = engine_model(spec, pred_sd, joint_sd, encoder=copy.deepcopy(enc))
        model.encoder.backend = backend
        loss = model(mel.cuda(), mel_lens.cuda(), ids.cuda(), id_lens.cuda(), blank)
        loss.backward()
        assert model.encoder.last_backend == backend
        got[backend] = (float(loss), {k: p.grad.cpu().double() for k, p in model.encoder.named_parameters()})
    e_ref, e = abs(got["torch"][0] - float(loss64)), abs(got["engine"][0] - float(loss64))
    print(f"encoder train end to end loss: engine encoder {e:.3e}, torch encoder {e_ref:.3e} from {float(loss64):.6f}")
    assert e <= FACTOR * e_ref
    bad = []
    for k in g64:
        e_ref = float((got["torch"][1][k] - g64[k]).abs().max())
        e = float((got["engine"][1][k] - g64[k]).abs().max())
        print(f"encoder train end to end {k}: engine encoder {e:.3e}, torch encoder {e_ref:.3e}, bar = {FACTOR * e_ref:.3e}")
        if not e <= FACTOR * e_ref:
            bad.append((k, e, e_ref))
    assert not bad, bad
