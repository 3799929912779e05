"""GPU tests of rnnt_amd.AudioEncoder's engine path (rnnt_amd/csrc/encoder.hip) against the float64 outputs recorded from the reference's
module (tests/golden/encoder_*.npz).  The bar of every comparison is 4 x the reference's OWN recorded fp32 error for that case (a
different summation order and split-K over otherwise the same exact-fp32 arithmetic); both numbers are printed
(profiles/encoder_parity.txt holds a run's)."""
import numpy as np
import pytest
import torch

from tests.encoder_cases import (NORM_TYPES, e2e_case, fixture, loaded_small_encoder, out64, reference_width_encoder, running, stream_all)

pytestmark = pytest.mark.gpu
FACTOR = 4.0


def _engine(norm_type, regime="auto"):
    enc = loaded_small_encoder(norm_type).cuda()
    enc.backend, enc.conv_regime = "engine", regime
    return enc


def _check(label, got, want64, ref_err):
    err = float(np.abs(got.detach().cpu().numpy().astype(np.float64) - want64).max())
    print(f"encoder parity {label}: engine max|y - fp64| = {err:.3e}, reference fp32 error = {ref_err:.3e}, bar = {FACTOR * ref_err:.3e}")
    assert got.shape == want64.shape
    assert err <= FACTOR * ref_err, (label, err, ref_err)


@pytest.mark.parametrize("norm_type", NORM_TYPES)
@pytest.mark.parametrize("N", (3, 1))
def test_whole_utterance_forward(norm_type, N):
    fx, enc = fixture(norm_type), _engine(norm_type)
    mel = torch.from_numpy(fx["mel"])[:N].cuda()
    with torch.no_grad():
        y = enc(mel)
    assert enc.last_backend == "engine"
    _check(f"{norm_type} forward N={N}", y, out64(fx)[:N], float(fx["err_whole"]))
    assert y.shape == (N, 36, 50) and y.permute(0, 2, 1).is_contiguous()  # RNNTModel's permute gives (N, L, C) without a copy


@pytest.mark.parametrize("norm_type", NORM_TYPES)
@pytest.mark.parametrize("regime", ("auto", "many_rows"))
def test_streamed_chunkings(norm_type, regime):
    fx, enc = fixture(norm_type), _engine(norm_type, regime)
    mel = torch.from_numpy(fx["mel"])[:1].cuda()
    names = running(fx) if regime == "auto" else ["whole", "halves"]
    for name in names:
        y, state, lens0 = stream_all(enc, mel, fx["chunks_" + name].tolist())
        assert enc.last_backend == "engine"
        _check(f"{norm_type} streamed {name} ({regime})", y, out64(fx, name), float(fx["err_" + name]))
        assert [list(s.shape) for s in state] == fx["state_shapes_" + name].tolist()
        assert lens0 == fx["state0_lens_" + name].tolist()
        assert all(s.is_contiguous() and s.device.type == "cuda" for s in state)
        assert len({s.untyped_storage().data_ptr() for s in state}) == 1  # a push's new states are views of one buffer


@pytest.mark.parametrize("norm_type", ("batch", "instance_affine"))
def test_streamed_batch_of_three_against_the_torch_path_in_float64(norm_type):
    """The fixtures stream utterance 0 only; N = 3 (state indexed per batch entry) against this module's torch path in float64, bar 4 x
    the torch path's fp32 error."""
    fx = fixture(norm_type)
    chunks = [7] * 14 + [3] if norm_type == "batch" else [50, 51]
    mel = torch.from_numpy(fx["mel"])
    ref32 = loaded_small_encoder(norm_type)
    ref64 = loaded_small_encoder(norm_type).double()
    want, st64, _ = stream_all(ref64, mel.double(), chunks)
    y32, _, _ = stream_all(ref32, mel, chunks)
    ref_err = float((y32.double() - want).abs().max())
    y, state, _ = stream_all(_engine(norm_type), mel.cuda(), chunks)
    _check(f"{norm_type} streamed N=3", y, want.numpy(), ref_err)
    for a, b in zip(state, st64):  # a state is a copy of input frames
        assert a.shape == b.shape and (a.cpu().double() - b).abs().max().item() <= FACTOR * ref_err


@pytest.mark.parametrize("norm_type", NORM_TYPES)
@pytest.mark.parametrize("first", ("engine", "torch"))
def test_switching_path_mid_stream(norm_type, first):
    fx = fixture(norm_type)
    name, k = ("sevens", 6) if norm_type == "batch" else ("halves", 1)
    chunks = fx["chunks_" + name].tolist()
    enc = loaded_small_encoder(norm_type).cuda()
    mel = torch.from_numpy(fx["mel"])[:1].cuda()
    enc.backend = first
    y1, state, _ = stream_all(enc, mel[:, :, :sum(chunks[:k])], chunks[:k])
    assert enc.last_backend == first
    enc.backend = "torch" if first == "engine" else "engine"
    y2, state, _ = stream_all(enc, mel[:, :, sum(chunks[:k]):], chunks[k:], state)
    assert enc.last_backend == enc.backend
    _check(f"{norm_type} {name}: {first} for {k} chunks, then the other path", torch.cat([y1, y2], dim=2), out64(fx, name),
           float(fx["err_" + name]))
    assert [list(s.shape) for s in state] == fx["state_shapes_" + name].tolist()


def test_identical_calls_give_identical_bits():
    fx = fixture("instance_affine")
    mel = torch.from_numpy(fx["mel"]).cuda()
    for regime in ("auto", "many_rows"):
        enc = _engine("instance_affine", regime)
        with torch.no_grad():
            a, b = enc(mel), enc(mel)
        assert torch.equal(a, b)
        (ya, sa, _), (yb, sb, _) = stream_all(enc, mel[:1], [50, 51]), stream_all(enc, mel[:1], [50, 51])
        assert torch.equal(ya, yb) and all(torch.equal(p, q) for p, q in zip(sa, sb))


@pytest.mark.parametrize("norm_type", NORM_TYPES)
@torch.no_grad()
def test_valueerror_cases_leave_the_state_untouched(norm_type):
    fx, enc = fixture(norm_type), _engine(norm_type)
    mel = torch.from_numpy(fx["mel"])[:1].cuda()
    state = [s.cuda() for s in enc.streaming_init_state(1)]
    _, state, _ = stream_all(enc, mel, [9], state)
    before = [s.clone() for s in state]
    bad = [0] if norm_type == "batch" else [0, 2]  # 4 + 2 frames: one output frame, which instance norm refuses
    assert state[0].shape[2] == 4
    for k in bad:
        with pytest.raises(ValueError):
            enc.streaming_forward(mel[:, :, 9:9 + k], state)
        assert all(torch.equal(a, b) for a, b in zip(state, before))
    with pytest.raises(ValueError):
        enc(mel[:, :, :1])
    y, _ = enc.streaming_forward(mel[:, :, 9:13], state)  # the stream goes on
    assert y.shape == (1, 36, 2)


def test_weight_version_rebuilds_the_packed_tables():
    fx, enc = fixture("batch"), _engine("batch")
    mel = torch.from_numpy(fx["mel"]).cuda()
    with torch.no_grad():
        y0 = enc(mel).clone()
        packed0 = enc._cache[2]
        assert enc(mel) is not None and enc._cache[2] is packed0  # nothing changed: no repack
        enc.blocks[3].convs[1].conv.weight.mul_(1.5)  # an optimizer step's in-place update bumps _version
        enc.blocks[-1].bias.add_(0.25)               # (read through its pointer every call)
        y1 = enc(mel)
        assert enc._cache[2] is not packed0
        enc.backend = "torch"
        want = enc(mel)
    assert (y1 - y0).abs().max().item() > 0.1
    assert (y1 - want).abs().max().item() <= 1e-5


@pytest.fixture(scope="module")
def ref_width_case():
    """basic_sp_convjs.yaml's widths, 120 mel frames, whole and streamed [50, 50, 20]: this module's torch path on the CPU in float64
    (the reference) and in fp32 (its error sets the bar), computed once."""
    enc = reference_width_encoder("instance_affine", seed=3)
    mel = torch.randn(1, 201, 120, generator=torch.Generator().manual_seed(5))
    enc64 = reference_width_encoder("instance_affine", seed=3).double()
    chunks = [50, 50, 20]
    with torch.no_grad():
        w64, w32 = enc64(mel.double()), enc(mel)
    s64, _, _ = stream_all(enc64, mel.double(), chunks)
    s32, _, _ = stream_all(enc, mel, chunks)
    return enc, mel, chunks, w64, float((w32.double() - w64).abs().max()), s64, float((s32.double() - s64).abs().max())


@pytest.mark.parametrize("regime", ("auto", "many_rows"))
def test_reference_widths(ref_width_case, regime):
    """Tile edges at C = 201 / 256 / 384 / 512, k = 29, dilation 2, which the small config cannot reach."""
    enc, mel, chunks, w64, w_err, s64, s_err = ref_width_case
    enc = enc.cuda()
    enc.backend, enc.conv_regime = "engine", regime
    try:
        with torch.no_grad():
            y = enc(mel.cuda())
        _check(f"reference widths forward ({regime})", y, w64.numpy(), w_err)
        ys, _, _ = stream_all(enc, mel.cuda(), chunks)
        _check(f"reference widths streamed [50, 50, 20] ({regime})", ys, s64.numpy(), s_err)
    finally:
        enc.backend, enc.conv_regime = "auto", "auto"
        enc.cpu()
        enc.repack()


def test_mel_to_tokens_end_to_end():
    """GreedyStream.push(mel_chunk) and greedy_decode(mel) with the engine encoder give the torch-path model's tokens, on device paths."""
    from oracle import decode_oracle
    from tests.stream_models import engine_model
    spec, enc, mel, pred_sd, joint_sd = e2e_case()
    with torch.no_grad():
        frames = enc(mel)[0].T.numpy()
    ref, margins = decode_oracle.greedy_decode(frames, pred_sd, joint_sd, max_length=60)
    assert margins.min() >= 1e-3 and 10 < len(ref) < 59  # the decode fixtures' MIN_MARGIN; the utterance ends by its frames
    model = engine_model(spec, pred_sd, joint_sd, encoder=enc)
    mel = mel.cuda()
    lens = torch.tensor([mel.shape[2]], device="cuda")
    got = {}
    for backend in ("torch", "engine"):
        model.encoder.backend = backend
        whole = model.greedy_decode(mel, lens, max_length=60)
        assert model.encoder.last_backend == backend
        s = model.greedy_stream(max_length=60)
        streamed = s.push(mel[..., :50]) + s.push(mel[..., 50:])
        assert s.last_path == "persistent" and model.encoder.last_backend == backend
        got[backend] = (whole, streamed)
    assert got["torch"][0] == got["torch"][1] == ref
    assert got["engine"] == got["torch"]
    model.encoder.backend = "auto"
    assert model.greedy_decode(mel, lens, max_length=60) == ref and model.encoder.last_backend == "engine"
    import rnnt_amd.encoder as E
    with torch.no_grad():  # "auto" leaves calls of more than ENGINE_AUTO_MAX_ROWS output rows to the torch path
        model.encoder(torch.cat([mel, mel], dim=2))
        assert 2 * 50 > E.ENGINE_AUTO_MAX_ROWS and model.encoder.last_backend == "torch"


@torch.no_grad()
def test_deepcopy_and_save_after_an_engine_call():
    """The engine cache (ctypes descriptors, packed weights) is not module state: an EMA twin or a whole-module checkpoint of an encoder
    that has run on the engine works, and the twin packs its own weights."""
    import copy
    import io
    fx, enc = fixture("instance_affine"), _engine("instance_affine")
    mel = torch.from_numpy(fx["mel"]).cuda()
    y = enc(mel)
    assert enc._cache is not None
    twin = copy.deepcopy(enc)
    torch.save(enc, io.BytesIO())
    assert twin._cache is None and enc._cache is not None
    twin.blocks[-1].bias.add_(1.0)  # its own parameters, its own packed tables
    assert torch.equal(enc(mel), y) and (twin(mel) - y - 1.0).abs().max().item() < 1e-5 and twin.last_backend == "engine"
    assert twin._cache[2].data_ptr() != enc._cache[2].data_ptr()


@torch.no_grad()
def test_wrong_feature_count_never_reaches_the_kernels():
    enc = _engine("batch")
    mel = torch.from_numpy(fixture("batch")["mel"]).cuda()
    state = [s.cuda() for s in enc.streaming_init_state(3)]
    for bad in (mel[:, :5], torch.cat([mel, mel], dim=1)):
        with pytest.raises(ValueError):
            enc(bad)
        with pytest.raises(ValueError):
            enc.streaming_forward(bad[:, :, :20], state)
    assert all(float(s.abs().max()) == 0.0 for s in state)


@torch.no_grad()
def test_auto_keeps_only_weight_streaming_shapes_on_the_engine():
    """64 output rows either way; 16 x (12 + 4) = 256 frames into the epilogue is beyond the weight-streaming kernel, so "auto" takes
    the torch path there instead of the MFMA conv."""
    enc = loaded_small_encoder("batch").cuda()
    g = torch.Generator().manual_seed(3)
    for N, L, want in ((8, 16, "engine"), (16, 8, "torch")):
        mel = torch.randn(N, 9, L, generator=g).cuda()
        state = [s.cuda() for s in enc.streaming_init_state(N)]
        enc.backend = "auto"
        y, _ = enc.streaming_forward(mel, state)
        assert enc.last_backend == want, (N, L)
        enc.backend = "torch"
        ref, _ = enc.streaming_forward(mel, state)
        assert (y - ref).abs().max().item() <= 1e-5
