"""CPU: argument checks of rnnt_engine_align / rnnt_engine_joint_align — every refusal is a code and a message, returned before
anything is enqueued (no device is needed: nothing is launched) — and the Python-level argument errors of rnnt_align /
joint_rnnt_align, which must be rnnt_loss's / joint_rnnt_loss's."""
import ctypes

import pytest
import torch

import rnnt_amd
from rnnt_amd import engine


@pytest.fixture(scope="module")
def lib():
    L = engine.lib()
    assert hasattr(L, "rnnt_engine_align") and hasattr(L, "rnnt_engine_joint_align")
    return L


def _loss_ws(lib, B, T, U1, V):
    n = ctypes.c_size_t(0)
    assert lib.rnnt_engine_loss_workspace_bytes(B, T, U1, V, 0, ctypes.byref(n)) == 0
    return n.value


def _align(lib, logits=16, targets=16, ll=16, tl=16, B=2, T=5, U1=3, V=8, blank=7, scores=16, frames=16, ws=256,
           ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = _loss_ws(lib, B, T, U1, V) if U1 <= 1024 and V % 4 == 0 and B > 0 else 1 << 40
    return lib.rnnt_engine_align(logits, targets, ll, tl, B, T, U1, V, blank, scores, frames, ws, ctypes.c_size_t(ws_bytes), None)


def _joint(lib, enc=16, pred=16, W=16, bias=16, B=2, T=5, U1=3, H=128, V=128, blank=127, dtype=0, scores=16, frames=16,
           ws=256, ws_bytes=None):
    strides = (ctypes.c_int64 * 3)(T * H, H, 1)
    if ws_bytes is None:
        n = ctypes.c_size_t(0)
        ws_bytes = n.value if lib.rnnt_engine_workspace_bytes(B, T, U1, H, V, dtype, ctypes.byref(n)) == 0 else 1 << 40
    return lib.rnnt_engine_joint_align(enc, strides, pred, W, bias, 16, 16, 16, B, T, U1, H, V, blank, dtype, scores, frames,
                                       ws, ctypes.c_size_t(ws_bytes), None)


def _err(lib):
    lib.rnnt_engine_last_error.restype = ctypes.c_char_p
    return lib.rnnt_engine_last_error().decode()


def test_version_is_4(lib):
    assert lib.rnnt_engine_version() == 4


@pytest.mark.parametrize("arg", ["logits", "targets", "ll", "tl", "scores", "frames", "ws"])
def test_align_null_pointers(lib, arg):
    assert _align(lib, **{arg: None}) == -1
    assert "null pointer" in _err(lib)


def test_align_refusals(lib):
    assert _align(lib, blank=8) == -1 and "blank=8" in _err(lib)
    assert _align(lib, blank=-1) == -1 and "blank=-1" in _err(lib)
    need = _loss_ws(lib, 2, 5, 3, 8)
    assert _align(lib, ws_bytes=need - 1) == -3 and "workspace" in _err(lib)
    assert _align(lib, U1=1025) == -2 and "1024" in _err(lib)
    assert _align(lib, V=10, blank=3) == -2 and "multiple of 4" in _err(lib)
    assert _align(lib, B=0) == -1 and "non-positive" in _err(lib)
    assert _align(lib, logits=8) == -1 and "aligned" in _err(lib)
    assert _align(lib, ws=128) == -1 and "aligned" in _err(lib)


def test_align_needs_no_more_than_the_loss_workspace(lib):
    # the largest U1 the kernels cover: refusing the loss's own size would make a caller allocate a second buffer
    for (B, T, U1, V) in ((1, 1, 1, 4), (32, 1000, 201, 1024), (2, 7, 1024, 8)):
        need = _loss_ws(lib, B, T, U1, V)
        assert _align(lib, B=B, T=T, U1=U1, V=V, blank=0, ws_bytes=need - 256) == -3


@pytest.mark.parametrize("arg", ["enc", "pred", "W", "bias", "scores", "frames", "ws"])
def test_joint_align_null_pointers(lib, arg):
    assert _joint(lib, **{arg: None}) == -1
    assert "null pointer" in _err(lib)


def test_joint_align_refusals(lib):
    assert _joint(lib, dtype=7) == -2 and "dtype 7" in _err(lib)
    assert _joint(lib, blank=128) == -1 and "blank=128" in _err(lib)
    assert _joint(lib, U1=1025) == -2 and "1024" in _err(lib)
    assert _joint(lib, V=130, blank=0) == -2 and "multiple of 4" in _err(lib)
    for dtype in (engine.DTYPE_BF16, engine.DTYPE_F32_BF16X3, engine.DTYPE_F32_F16X2):
        assert _joint(lib, H=96, dtype=dtype) == -2 and "H % 128 == 0" in _err(lib)
        assert _joint(lib, V=132, blank=0, dtype=dtype) == -2 and "V % 128 == 0" in _err(lib)
    for dtype in (0, 1, 2, 3):
        n = ctypes.c_size_t(0)
        assert lib.rnnt_engine_workspace_bytes(2, 5, 3, 128, 128, dtype, ctypes.byref(n)) == 0
        assert _joint(lib, dtype=dtype, ws_bytes=n.value - 1) == -3 and "workspace" in _err(lib)


def _cpu_inputs(B=2, T=5, U=2, V=8):
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(B, T, U + 1, V, generator=g)
    targets = torch.randint(0, V - 1, (B, U), generator=g, dtype=torch.int32)
    return logits, targets, torch.full((B,), T, dtype=torch.int32), torch.full((B,), U, dtype=torch.int32)


def _bad_cases():
    lg, tg, ll, tl = _cpu_inputs()
    return {
        "targets_int64": (lg, tg.long(), ll, tl, -1),
        "lengths_int64": (lg, tg, ll.long(), tl, -1),
        "targets_1d": (lg, tg[0], ll, tl, -1),
        "blank_range": (lg, tg, ll, tl, 8),
        "batch_mismatch": (lg, tg[:1], ll, tl, -1),
        "targets_width": (lg, tg[:, :1], ll, tl, -1),
        "input_length": (lg, tg, ll - 1, tl, -1),
        "output_length": (lg, tg, ll, tl - 1, -1),
        "logits_3d": (lg[0], tg, ll, tl, -1),
        "logits_f64": (lg.double(), tg, ll, tl, -1),
        "logits_noncontig": (lg.transpose(1, 2), tg, ll, tl, -1),
    }


@pytest.mark.parametrize("case", list(_bad_cases()))
def test_rnnt_align_raises_what_rnnt_loss_raises(case):
    args = _bad_cases()[case]
    with pytest.raises(Exception) as want:
        rnnt_amd.rnnt_loss(*args[:4], blank=args[4])
    with pytest.raises(type(want.value)) as got:
        rnnt_amd.rnnt_align(*args[:4], blank=args[4])
    assert str(got.value) == str(want.value)


def test_joint_align_raises_what_joint_loss_raises():
    B, T, U, H, V = 2, 5, 2, 16, 8
    enc, pred = torch.randn(B, T, H), torch.randn(B, U + 1, H)
    W, bias = torch.randn(V, H), torch.randn(V)
    _, tg, ll, tl = _cpu_inputs(B, T, U, V)
    cases = [(enc, pred, W, bias, tg.long(), ll, tl), (enc, pred[:, :, :8], W, bias, tg, ll, tl),
             (enc.double(), pred, W, bias, tg, ll, tl), (enc[0], pred, W, bias, tg, ll, tl), (enc, pred, W, bias, tg, ll - 1, tl)]
    for args in cases:
        with pytest.raises(Exception) as want:
            rnnt_amd.joint_rnnt_loss(*args)
        with pytest.raises(type(want.value)) as got:
            rnnt_amd.joint_rnnt_align(*args)
        assert str(got.value) == str(want.value)


def test_cpu_tensors_are_rejected():
    lg, tg, ll, tl = _cpu_inputs()
    with pytest.raises(RuntimeError, match="HIP device"):
        rnnt_amd.rnnt_align(lg, tg, ll, tl)
    B, T, U, H, V = 2, 5, 2, 16, 8
    with pytest.raises(RuntimeError, match="HIP device"):
        rnnt_amd.joint_rnnt_align(torch.randn(B, T, H), torch.randn(B, U + 1, H), torch.randn(V, H), torch.randn(V), tg, ll, tl,
                                  dtype="fp32")
