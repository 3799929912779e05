"""CPU: the C entries of the latency regularisers are exported and bound; a negative, NaN or infinite lambda
or delta is refused with RNNT_ERR_INVALID_ARG and a message before anything is enqueued (no device is needed: nothing is
launched); the Python layer raises ValueError for the same values; RNNTModel carries the two options as attributes and hands
them to the loss only when they are non-zero."""
import ctypes
import inspect

import pytest
import torch

import rnnt_amd
from rnnt_amd import engine

NEW = ("rnnt_engine_loss_fwd_bwd_reg", "rnnt_engine_joint_loss_fwd_bwd_reg", "rnnt_engine_joint_loss_fwd_reg")
BAD = (-1.0, -1e-30, float("nan"), float("inf"), -float("inf"))


@pytest.fixture(scope="module")
def lib():
    return engine.lib()


def _err(lib):
    return lib.rnnt_engine_last_error().decode()


def _loss(lib, lam, dp, logits=16):
    B, T, U1, V = 2, 5, 3, 8
    n = ctypes.c_size_t(0)
    assert lib.rnnt_engine_loss_workspace_bytes(B, T, U1, V, 0, ctypes.byref(n)) == 0
    return lib.rnnt_engine_loss_fwd_bwd_reg(logits, 16, 16, 16, B, T, U1, V, 7, ctypes.c_float(-1), ctypes.c_float(lam),
                                            ctypes.c_float(dp), 0, 16, 16, 256, n, None)


def _joint_args(lib, enc=16):
    B, T, U1, H, V = 2, 5, 3, 128, 128
    n = ctypes.c_size_t(0)
    assert lib.rnnt_engine_workspace_bytes(B, T, U1, H, V, 0, ctypes.byref(n)) == 0
    return (enc, (ctypes.c_int64 * 3)(T * H, H, 1), 16, 16, 16, 16, 16, 16, B, T, U1, H, V, V - 1), n


def _joint(lib, lam, dp, enc=16):
    head, n = _joint_args(lib, enc)
    return lib.rnnt_engine_joint_loss_fwd_bwd_reg(*head, ctypes.c_float(-1), ctypes.c_float(0.5), ctypes.c_float(lam),
                                                  ctypes.c_float(dp), 0, 16, 16, 16, 16, 16, 256, n, None)


def _joint_fwd(lib, dp, enc=16):
    head, n = _joint_args(lib, enc)
    return lib.rnnt_engine_joint_loss_fwd_reg(*head, ctypes.c_float(dp), 0, 16, 256, n, None)


def test_new_entries_are_exported_and_bound(lib):
    for name in NEW:
        assert hasattr(lib, name) and name in engine.EXPORTS
        assert len(getattr(lib, name).argtypes) == len(engine.SIGNATURES[name])
    assert lib.rnnt_engine_version() == 4  # callers detect the feature by symbol


@pytest.mark.parametrize("bad", BAD)
def test_bad_options_are_refused_before_any_work(lib, bad):
    assert _loss(lib, bad, 0.0) == -1 and "fastemit_lambda" in _err(lib)
    assert _loss(lib, 0.0, bad) == -1 and "delay_penalty" in _err(lib)
    assert _joint(lib, bad, 0.0) == -1 and "fastemit_lambda" in _err(lib)
    assert _joint(lib, 0.0, bad) == -1 and "delay_penalty" in _err(lib)
    assert _joint_fwd(lib, bad) == -1 and "delay_penalty" in _err(lib)


def test_good_options_reach_the_usual_checks(lib):
    # valid options pass on to the counterpart's own argument checks (here: a null pointer, refused before any launch)
    assert _loss(lib, 0.5, 0.01, logits=None) == -1 and "null pointer" in _err(lib)
    assert _joint(lib, 0.5, 0.01, enc=None) == -1 and "null pointer" in _err(lib)
    assert _joint_fwd(lib, 0.01, enc=None) == -1 and "null pointer" in _err(lib)


@pytest.mark.parametrize("bad", BAD + ("x", None))
def test_python_layer_raises_value_error(bad):
    logits = torch.zeros(2, 5, 3, 8)
    targets = torch.zeros(2, 2, dtype=torch.int32)
    ll = torch.full((2,), 5, dtype=torch.int32)
    tl = torch.full((2,), 2, dtype=torch.int32)
    enc, pred, W, bias = torch.zeros(2, 5, 16), torch.zeros(2, 3, 16), torch.zeros(8, 16), torch.zeros(8)
    for kw in ({"fastemit_lambda": bad}, {"delay_penalty": bad}):
        with pytest.raises(ValueError):
            rnnt_amd.rnnt_loss(logits, targets, ll, tl, **kw)
        with pytest.raises(ValueError):
            rnnt_amd.joint_rnnt_loss(enc, pred, W, bias, targets, ll, tl, **kw)
        with pytest.raises(ValueError):
            engine.check_reg(kw.get("fastemit_lambda", 0.0), kw.get("delay_penalty", 0.0))


def test_model_options_are_attributes_passed_only_when_set():
    class Enc(torch.nn.Module):
        def forward(self, x):
            return x

        def calc_output_lens(self, lens):
            return lens

    H, V = 8, 6
    model = rnnt_amd.RNNTModel(torch.nn.Embedding(V, H), Enc(), rnnt_amd.JointNetwork(-1, -1, H, V))
    assert model.fastemit_lambda == 0.0 and model.delay_penalty == 0.0
    assert list(inspect.signature(model.forward).parameters) == [
        "mel_features", "mel_feature_lens", "input_ids", "input_id_lens", "blank_idx"]
    seen = []
    model.joint.fused_loss = lambda *a, **kw: seen.append(kw) or torch.zeros(())
    args = (torch.zeros(2, H, 4), torch.full((2,), 4), torch.zeros(2, 3, dtype=torch.long), torch.full((2,), 3), V - 1)
    model(*args)
    assert "fastemit_lambda" not in seen[-1] and "delay_penalty" not in seen[-1]
    model.fastemit_lambda = 0.01
    model(*args)
    assert seen[-1]["fastemit_lambda"] == 0.01 and "delay_penalty" not in seen[-1]
    model.delay_penalty = 0.002
    model(*args)
    assert seen[-1]["fastemit_lambda"] == 0.01 and seen[-1]["delay_penalty"] == 0.002
