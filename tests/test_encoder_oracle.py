"""CPU tests of rnnt_amd.AudioEncoder's torch path against numbers recorded from the reference's own rnnt.jasper.AudioEncoder
(tests/golden/make_golden_encoder.py): state-dict keys, forward, calc_output_lens, streaming with every recorded chunking (the
growing prologue state included), the cases in which the reference raises, from_module."""
import numpy as np
import pytest
import torch

from tests.encoder_cases import NORM_TYPES, fixture, loaded_small_encoder, running, small_encoder, state_dict_of, stream_all

TOL = 1e-6  # the torch calls are the reference's: equality is expected


@pytest.mark.parametrize("norm_type", NORM_TYPES)
def test_reference_state_dict_loads_strictly(norm_type):
    enc = small_encoder(norm_type)
    sd = state_dict_of(fixture(norm_type))
    assert set(enc.state_dict()) == set(sd)
    res = enc.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert "blocks.0.conv.weight" in sd and "blocks.3.convs.0.conv.weight" in sd and "blocks.3.residual_conv.weight" in sd
    if norm_type != "instance":
        assert "blocks.3.norms.1.weight" in sd and "blocks.3.residual_norm.bias" in sd


@pytest.mark.parametrize("norm_type", NORM_TYPES)
def test_forward_and_output_lens_match_the_reference(norm_type):
    fx, enc = fixture(norm_type), loaded_small_encoder(norm_type)
    with torch.no_grad():
        y = enc(torch.from_numpy(fx["mel"]))
    assert enc.last_backend == "torch"
    assert y.shape == fx["out32"].shape
    assert np.abs(y.numpy() - fx["out32"]).max() <= TOL
    assert enc.calc_output_lens(torch.from_numpy(fx["lens"])).tolist() == fx["out_lens"].tolist()
    assert [tuple(s.shape) for s in enc.streaming_init_state(3)] == [(3, 9, 3), (3, 12, 4), (3, 20, 4), (3, 20, 6), (3, 24, 6),
                                                                      (3, 24, 6), (3, 24, 12)]
    assert all(s.device.type == "cpu" for s in enc.streaming_init_state(2))


@pytest.mark.parametrize("norm_type", NORM_TYPES)
def test_streamed_outputs_and_states_match_the_reference(norm_type):
    fx, enc = fixture(norm_type), loaded_small_encoder(norm_type)
    mel = torch.from_numpy(fx["mel"])[:1]
    assert running(fx)
    for name in running(fx):
        y, state, lens0 = stream_all(enc, mel, fx["chunks_" + name].tolist())
        assert np.abs(y.numpy() - fx["stream32_" + name]).max() <= TOL, name
        assert [list(s.shape) for s in state] == fx["state_shapes_" + name].tolist(), name
        assert lens0 == fx["state0_lens_" + name].tolist(), name  # the strided prologue's state grows and shrinks
    if norm_type == "batch":
        assert sorted(set(fx["state0_lens_sevens"].tolist())) == [3, 4]


@pytest.mark.parametrize("norm_type", NORM_TYPES)
def test_where_the_reference_raises_valueerror_and_state_untouched(norm_type):
    fx, enc = fixture(norm_type), loaded_small_encoder(norm_type)
    mel = torch.from_numpy(fx["mel"])[:1]
    assert set(fx["raising"].tolist()) == (set() if norm_type == "batch" else {"sevens", "twos", "ragged"})
    for name in fx["raising"].tolist():
        chunks, at = fx["chunks_" + name].tolist(), int(fx["raise_at_" + name])
        _, state, _ = stream_all(enc, mel, chunks[:at]) if at else (None, enc.streaming_init_state(1), None)
        before = [s.clone() for s in state]
        t = sum(chunks[:at])
        with pytest.raises(ValueError):
            enc.streaming_forward(mel[:, :, t:t + chunks[at]], state)
        assert all(torch.equal(a, b) for a, b in zip(state, before)), name
    # a chunk too short for one prologue frame, the empty chunk included: any norm type
    state = enc.streaming_init_state(1)
    before = [s.clone() for s in state]
    for k in (0, 1):  # 3 frames of state + 1 < 5
        with pytest.raises(ValueError):
            enc.streaming_forward(mel[:, :, :k], state)
    assert all(torch.equal(a, b) for a, b in zip(state, before))
    with pytest.raises(ValueError):
        enc(mel[:, :, :1])  # a whole "utterance" shorter than the stride


def test_seven_frame_chunk_on_the_strided_prologue():
    """A 7-frame chunk on the k = 5, s = 2 prologue from the initial 3-frame state gives (3 + 7 - 5) // 2 + 1 = 3 frames and leaves
    10 - 6 = 4 frames; the next 7-frame chunk gives 4 frames and a 3-long state."""
    enc = loaded_small_encoder("batch")
    mel = torch.from_numpy(fixture("batch")["mel"])[:1]
    state = enc.streaming_init_state(1)
    y, state = enc.streaming_forward(mel[:, :, :7], state)
    assert y.shape[2] == 3 and state[0].shape[2] == 4
    y, state = enc.streaming_forward(mel[:, :, 7:14], state)
    assert y.shape[2] == 4 and state[0].shape[2] == 3


def test_batch_norm_streams_exactly_and_instance_norm_does_not():
    fx = fixture("batch")
    for name in running(fx):
        assert float(fx["stream_vs_whole_" + name]) < 1e-12, name
    enc = loaded_small_encoder("batch")
    mel = torch.from_numpy(fx["mel"])
    with torch.no_grad():
        whole = enc(mel)
    y, _, _ = stream_all(enc, mel, [50, 51])
    assert (y - whole).abs().max().item() <= 4 * float(fx["err_whole"]) + 1e-6
    for nt in ("instance", "instance_affine"):
        assert float(fixture(nt)["stream_vs_whole_halves"]) > 1e-2  # the chunk's statistics: nobody "fixes" this


def test_from_module_shares_parameters():
    import rnnt_amd
    src = loaded_small_encoder("instance_affine")
    enc = rnnt_amd.AudioEncoder.from_module(src)
    assert rnnt_amd.AudioEncoder.from_module(enc) is enc
    a, b = dict(src.named_parameters()), dict(enc.named_parameters())
    assert set(a) == set(b) and len(a) > 10
    assert all(a[k].data_ptr() == b[k].data_ptr() and a[k] is b[k] for k in a)
    assert set(enc.state_dict()) == set(src.state_dict())
    fx = fixture("instance_affine")
    with torch.no_grad():
        y = enc(torch.from_numpy(fx["mel"]))
    assert np.abs(y.numpy() - fx["out32"]).max() <= TOL

    class Lookalike(torch.nn.Module):  # duck typing: only the attribute layout counts
        def __init__(self, blocks):
            super().__init__()
            self.blocks = blocks
    enc2 = rnnt_amd.AudioEncoder.from_module(Lookalike(src.blocks).eval())
    y2, _, _ = stream_all(enc2, torch.from_numpy(fx["mel"])[:1], [50, 51])
    assert np.abs(y2.numpy() - fx["stream32_halves"]).max() <= TOL
    with pytest.raises(TypeError):
        rnnt_amd.AudioEncoder.from_module(torch.nn.Linear(2, 2))


def test_backend_switch_and_train_mode_stay_on_torch():
    enc = loaded_small_encoder("batch")
    mel = torch.from_numpy(fixture("batch")["mel"])
    enc.backend = "engine"
    with torch.no_grad(), pytest.raises(RuntimeError, match="engine path does not apply"):
        enc(mel)  # CPU tensors
    enc.backend = "auto"
    enc.train()
    y = enc(mel)  # autograd through the torch path
    y.sum().backward()
    assert enc.last_backend == "torch" and enc.blocks[0].conv.weight.grad is not None
    import rnnt_amd
    blk = rnnt_amd.JasperBlock(5, 12, 20, 0.1, 2, "batch", additional_context=2)
    assert blk.convs[0].left_padding == 2 and blk.convs[0].padding == 4
    with pytest.raises(ValueError):
        rnnt_amd.encoder.CausalConv1d(4, 4, 3, 1, 1, additional_context=3)
