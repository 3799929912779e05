"""CPU tests of rnnt_amd.AudioEncoder's host logic: inputs refused before any path runs, the engine cache kept out of copies and
pickles, and which modules / shapes backend "auto" leaves to the torch path."""
import copy
import ctypes
import io
import pickle

import pytest
import torch

import rnnt_amd
from rnnt_amd import encoder as E
from tests.encoder_cases import fixture, loaded_small_encoder, small_encoder


def test_wrong_feature_count_is_refused_before_any_path():
    """The engine reads channels by its layer list, so a mel with another feature count must never reach it: ValueError from
    forward and streaming_forward on every backend, state untouched."""
    enc = loaded_small_encoder("batch")
    mel = torch.from_numpy(fixture("batch")["mel"])
    state = enc.streaming_init_state(3)
    before = [s.clone() for s in state]
    for backend in ("auto", "torch", "engine"):
        enc.backend = backend
        for bad in (mel[:, :8], torch.cat([mel, mel], dim=1), mel[0], mel[:0]):
            with torch.no_grad(), pytest.raises(ValueError):
                enc(bad)
            with torch.no_grad(), pytest.raises(ValueError):
                enc.streaming_forward(bad, state)
    assert all(torch.equal(a, b) for a, b in zip(state, before))


def test_engine_cache_stays_out_of_deepcopy_pickle_and_torch_save():
    """After an engine call the module holds ctypes descriptors (raw pointers) and the packed weights; neither is module state."""
    enc = loaded_small_encoder("instance_affine")
    arr = (E._Layer * 2)()  # what _prepared leaves behind, without a device
    assert pytest.raises(ValueError, pickle.dumps, arr)
    enc._cache_key, enc._cache = ("key",), ([], arr, torch.zeros(4), [0])
    twin = copy.deepcopy(enc)
    assert twin._cache is None and twin._cache_key is None and enc._cache is not None
    assert all(a is not b and torch.equal(a, b) for a, b in zip(enc.parameters(), twin.parameters()))
    back = pickle.loads(pickle.dumps(enc))
    assert back._cache is None and set(back.state_dict()) == set(enc.state_dict())
    buf = io.BytesIO()
    torch.save(enc, buf)
    model = rnnt_amd.RNNTModel(torch.nn.Identity(), enc, torch.nn.Identity())
    assert copy.deepcopy(model).encoder._cache is None
    mel = torch.from_numpy(fixture("instance_affine")["mel"])
    with torch.no_grad():
        assert torch.equal(twin(mel), enc(mel))


def _flat_reason(**kw):
    args = dict(input_features=9, prologue_kernel_size=5, prologue_stride=2, blocks=[rnnt_amd.JasperBlock(5, 12, 20, 0.1, 2, "batch")],
                epilogue_features=28, epilogue_kernel_size=7, epilogue_dilation=2, output_features=36, norm_type="batch")
    args.update(kw)
    return rnnt_amd.AudioEncoder(**args)._flat()


def test_modules_the_engine_refuses_are_left_to_torch():
    """_flat() names why (a string): backend "auto" then takes the torch path instead of meeting RNNT_ERR_UNSUPPORTED in the C ABI."""
    assert isinstance(_flat_reason(), list)
    assert "stride > 64" in _flat_reason(prologue_kernel_size=80, prologue_stride=65)
    assert "4096" in _flat_reason(epilogue_kernel_size=3, epilogue_dilation=1400)
    assert "look-ahead" in _flat_reason(blocks=[rnnt_amd.JasperBlock(5, 12, 20, 0.1, 2, "batch", additional_context=1)])
    enc = small_encoder("batch")
    enc.blocks[1] = torch.nn.BatchNorm1d(12, track_running_stats=False)
    assert "norm" in enc._flat()


def test_auto_routes_on_the_weight_streaming_kernels_own_conditions():
    """rows = [(frames in, state frames, frames out, next state)] per causal conv: "auto" keeps a call on the engine only if every layer
    has N * frames out <= 64 AND N * (state + input frames) <= 224, the C side's test for k_enc_conv_few."""
    enc = loaded_small_encoder("batch")

    def over(N, L, state_lens=None):
        rows, _ = enc._lengths(L, state_lens)
        return any(N * r[2] > E.ENGINE_AUTO_MAX_ROWS or N * (r[0] + r[1]) > E.ENGINE_AUTO_MAX_FRAMES for r in rows)
    init = [s.shape[2] for s in enc.streaming_init_state(1)]
    assert not over(1, 101) and not over(1, 50, init)
    assert over(1, 202)              # 100 rows
    assert not over(8, 16, init)     # 64 rows; the epilogue reads 8 * (12 + 8) = 160 frames
    assert over(16, 8, init)         # 64 rows again, but the epilogue reads 16 * (12 + 4) = 256 frames: the MFMA kernel on the C side
    assert E.ENGINE_AUTO_MAX_ROWS == 64 and E.ENGINE_AUTO_MAX_FRAMES == 224
