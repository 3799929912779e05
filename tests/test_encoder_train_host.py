"""CPU tests around the encoder's training path: the torch path (the engine path's oracle) against the gradients recorded from the
reference (tests/golden/encoder_train_*.npz), explicit keep masks, the dispatch rules that need no GPU, and the layer cases' float64
numpy oracle against torch's autograd."""
import numpy as np
import pytest
import torch

import rnnt_amd
from tests import encoder_train_cases as C
from tests.encoder_cases import fixture, out64


def _run(enc, mel, G, keep_masks=None):
    enc.zero_grad()
    out = enc(mel, keep_masks=keep_masks) if keep_masks is not None else enc(mel)
    (out * G).sum().backward()
    return out.detach(), {k: p.grad.detach().cpu().numpy() for k, p in enc.named_parameters()}


def _ones(enc, N, L):
    rows, _ = enc._lengths(L, None)
    convs = enc._causal_convs()
    inside = {id(c) for m in enc.blocks if hasattr(m, "convs") for c in m.convs}
    return [torch.ones((N, r[2], c.conv.out_channels), dtype=torch.uint8) for c, r in zip(convs, rows) if id(c) in inside]


@pytest.mark.parametrize("case", C.TRAIN_CASES)
@pytest.mark.parametrize("N", (3, 1))
def test_torch_path_fp32_gives_the_recorded_gradients(case, N):
    """With keep masks handed over (all ones: the module is in eval(), so nothing is dropped or scaled)."""
    fx, enc = C.train_fixture(case, N), C.small_train_encoder(case)
    mel = torch.from_numpy(fixture(C.norm_of(case))["mel"])[:N]
    out, got = _run(enc, mel, torch.from_numpy(fx["G"]), _ones(enc, N, mel.shape[2]))
    assert enc.last_backend == "torch"
    C.check_grads(f"torch path {case} N={N}", fx, got, C.bias_rows(enc, N, mel.shape[2]).__getitem__, printer=lambda s: None)
    if case == "instance_affine_la2":
        ref = C.lookahead_out()
        want = (ref["out32"].astype(np.float64) + ref["out64_corr"])[:N]
        assert out.shape == want.shape and np.abs(out.numpy() - want).max() <= 4 * float(ref["err_out"])


@pytest.mark.parametrize("case", ("batch", "instance_affine_la2"))
def test_torch_path_float64_gives_the_recorded_float64_gradients(case):
    fx, enc = C.train_fixture(case, 3), C.small_train_encoder(case).double()
    mel = torch.from_numpy(fixture(C.norm_of(case))["mel"]).double()
    _, got = _run(enc, mel, torch.from_numpy(fx["G"]).double())
    want = C.grads64(fx)
    for k in want:  # g32 + float32(g64 - g32) carries g64 to 2^-24 of the correction
        assert np.abs(got[k] - want[k]).max() <= 1e-9 + 2.0 ** -23 * np.abs(fx["g64_corr/" + k]).max(), k


def test_explicit_keep_masks_replace_the_draw_on_the_torch_path():
    enc = C.small_train_encoder("instance_affine").train()
    for m in enc.blocks:
        if hasattr(m, "dropout"):
            m.dropout.p = 0.5
    mel = torch.from_numpy(fixture("instance_affine")["mel"])
    g = torch.Generator().manual_seed(3)
    masks = [(torch.rand(k.shape, generator=g) >= 0.5).to(torch.uint8) for k in _ones(enc, 3, 101)]
    G = torch.randn(3, 36, 50, generator=g)
    a, ga = _run(enc, mel, G, masks)
    b, gb = _run(enc, mel, G, masks)
    assert torch.equal(a, b) and all(np.array_equal(ga[k], gb[k]) for k in ga)  # nothing is drawn
    enc64 = C.small_train_encoder("instance_affine").double().train()
    for m in enc64.blocks:
        if hasattr(m, "dropout"):
            m.dropout.p = 0.5
    c, _ = _run(enc64, mel.double(), G.double(), masks)
    assert (a.double() - c).abs().max().item() < 1e-3 and (a - _run(enc, mel, G)[0]).abs().max().item() > 1e-2  # ... unlike a drawn call
    flipped = [1 - m for m in masks]
    assert (a - _run(enc, mel, G, flipped)[0]).abs().max().item() > 1e-2
    with pytest.raises(ValueError):
        enc(mel, keep_masks=masks[:-1])
    enc.eval()
    assert torch.equal(enc(mel, keep_masks=masks), enc(mel))  # dropout inactive: the masks are not applied


def test_flat_names_lookahead_and_blocks_with_lookahead_run_nowhere():
    enc = C.small_train_encoder("instance_affine_la2")
    assert "look-ahead" in enc._flat()
    assert isinstance(enc._flat(allow_lookahead=True), list)
    blocks = [rnnt_amd.JasperBlock(5, 12, 20, 0.1, 2, "instance_affine", additional_context=2)]
    inside = rnnt_amd.AudioEncoder(input_features=9, prologue_kernel_size=5, blocks=blocks, epilogue_features=28, epilogue_kernel_size=7,
                                   output_features=36, norm_type="instance_affine").eval()
    assert "look-ahead" in inside._flat()
    assert "inside a JasperBlock" in inside._flat(allow_lookahead=True)
    with pytest.raises(RuntimeError), torch.no_grad():  # the torch path (like the reference) cannot add the residual branch there
        inside(torch.zeros(1, 9, 101))


def test_auto_with_grad_stays_on_torch_and_engine_names_why_it_cannot_run():
    enc = C.small_train_encoder("batch")
    mel = torch.from_numpy(fixture("batch")["mel"])
    enc.backend = "auto"
    assert enc(mel).requires_grad and enc.last_backend == "torch"
    enc.backend = "engine"
    with pytest.raises(RuntimeError, match="fp32 on a HIP device"):
        enc(mel)
    with pytest.raises(RuntimeError, match="requires grad"):
        enc(mel.clone().requires_grad_())
    import copy
    twin = copy.deepcopy(enc)
    assert twin._train_packed is None and twin._cache is None


@pytest.mark.parametrize("name,kind", C.case_ids())
def test_the_layer_oracle_is_torch_autograd_in_float64(name, kind):
    case, want, (out_bar, bars) = C.prepared(name, kind)
    out, grads = C.torch_train(case, torch.float64)
    assert np.abs(out - want.out).max() <= 1e-11 * max(1.0, np.abs(want.out).max())
    for l, g, w, b in zip(case.layers, grads, want.grads, bars):
        for k in C.GRAD_KEYS:
            assert (g[k] is None) == (w[k] is None), (name, k)
            if w[k] is not None:
                assert np.abs(g[k] - w[k]).max() <= 1e-11 * max(1.0, np.abs(w[k]).max()), (name, k)
                assert np.all(np.asarray(b[k]) > 0)
        if C.zero_bias(l):
            assert np.abs(w["b"]).max() <= 1e-12 * max(1.0, w["dyabs"].max())  # exactly zero up to float64 rounding
