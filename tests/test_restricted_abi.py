"""CPU: the C ABI of the alignment-restricted loss — rnnt_engine_loss_fwd_bwd_restrict,
rnnt_engine_joint_loss_fwd_bwd_restrict, rnnt_engine_joint_loss_fwd_restrict: the symbols exist with the declared signatures,
every refusal is a code and a message returned before anything is enqueued (no device is needed), the existing entries keep
theirs; and the Python-level argument errors of rnnt_loss / joint_rnnt_loss that need no device."""
import ctypes
import os
import re

import pytest
import torch

import rnnt_amd
from rnnt_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rnnt_engine_loss_fwd_bwd_restrict", "rnnt_engine_joint_loss_fwd_bwd_restrict", "rnnt_engine_joint_loss_fwd_restrict")


@pytest.fixture(scope="module")
def lib():
    L = engine.lib()
    for n in NAMES:
        assert hasattr(L, n), n
    return L


def _err(lib):
    lib.rnnt_engine_last_error.restype = ctypes.c_char_p
    return lib.rnnt_engine_last_error().decode()


def _kinds(name):
    """The argument kinds of a prototype of include/rnnt_engine.h, in engine.SIGNATURES's letters."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnnt_engine.h")).read(), flags=re.S)
    args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
    out = ""
    for a in args.split(","):
        a = " ".join(a.split())
        if "*" in a or "[" in a:
            out += "p"
        elif a.startswith("size_t"):
            out += "z"
        elif a.startswith("float"):
            out += "f"
        elif a.startswith("int64_t"):
            out += "q"
        else:
            assert a.startswith("int "), a
            out += "i"
    return out


def test_signatures_are_the_reg_entries_plus_frames_and_two_buffers():
    for name in NAMES:
        got = _kinds(name)
        assert engine.SIGNATURES[name] == got and name in engine.EXPORTS
        reg = _kinds(name.replace("_restrict", "_reg"))
        assert engine.SIGNATURES[name.replace("_restrict", "_reg")] == reg  # the existing entry keeps its signature
        k = reg.rindex("f") + 1  # behind lambda / delta
        assert got == reg[:k] + "pii" + reg[k:]


def _loss(lib, logits=16, frames=16, left=0, right=0, lam=0.0, dp=0.0, B=2, T=5, U1=3, V=8, blank=7, costs=16, ws=256):
    n = ctypes.c_size_t(0)
    if lib.rnnt_engine_loss_workspace_bytes(B, T, U1, V, 0, ctypes.byref(n)) != 0:
        n.value = 1 << 40  # a shape the size query refuses: the entry must refuse it too
    return lib.rnnt_engine_loss_fwd_bwd_restrict(logits, 16, 16, 16, B, T, U1, V, blank, ctypes.c_float(-1.0), ctypes.c_float(lam),
                                                 ctypes.c_float(dp), frames, left, right, 0, costs, None, ws,
                                                 ctypes.c_size_t(n.value), None)


def _joint(lib, bwd, enc=16, frames=16, left=0, right=0, lam=0.0, dp=0.0, B=2, T=5, U1=3, H=128, V=128, blank=127, dtype=0,
           ws_bytes=None):
    strides = (ctypes.c_int64 * 3)(T * H, H, 1)
    if ws_bytes is None:
        n = ctypes.c_size_t(0)
        ws_bytes = n.value if lib.rnnt_engine_workspace_bytes(B, T, U1, H, V, dtype, ctypes.byref(n)) == 0 else 1 << 40
    head = (enc, strides, 16, 16, 16, 16, 16, 16, B, T, U1, H, V, blank)
    if bwd:
        return lib.rnnt_engine_joint_loss_fwd_bwd_restrict(*head, ctypes.c_float(-1.0), ctypes.c_float(0.5), ctypes.c_float(lam),
                                                           ctypes.c_float(dp), frames, left, right, dtype, 16, 16, 16, 16, 16,
                                                           256, ctypes.c_size_t(ws_bytes), None)
    return lib.rnnt_engine_joint_loss_fwd_restrict(*head, ctypes.c_float(dp), frames, left, right, dtype, 16, 256,
                                                   ctypes.c_size_t(ws_bytes), None)


def _calls(lib):
    return (lambda **kw: _loss(lib, **kw), lambda **kw: _joint(lib, True, **kw), lambda **kw: _joint(lib, False, **kw))


def test_null_frames_is_an_argument_error(lib):
    for call in _calls(lib):
        assert call(frames=None) == -1 and "restrict_frames" in _err(lib) and "null pointer" in _err(lib)


@pytest.mark.parametrize("left,right", [(-1, 0), (0, -1), (-2 ** 31, 3)])
def test_negative_buffers_are_an_argument_error(lib, left, right):
    for call in _calls(lib):
        assert call(left=left, right=right) == -1 and "must be >= 0" in _err(lib)


def test_the_existing_refusals_still_apply(lib):
    for call in _calls(lib):
        assert call(dp=-1.0) == -1 and "delay_penalty" in _err(lib)
        assert call(dp=float("nan")) == -1 and "delay_penalty" in _err(lib)
        assert call(blank=-1) == -1 and "blank=-1" in _err(lib)
        assert call(U1=1025) == -2 and "1024" in _err(lib)
    for call in _calls(lib)[:2]:
        assert call(lam=float("inf")) == -1 and "fastemit_lambda" in _err(lib)
    assert _loss(lib, logits=None) == -1 and "null pointer" in _err(lib)
    assert _loss(lib, ws=128) == -1 and "aligned" in _err(lib)
    for bwd in (True, False):
        assert _joint(lib, bwd, enc=None) == -1 and "null pointer" in _err(lib)
        assert _joint(lib, bwd, dtype=7) == -2 and "dtype 7" in _err(lib)
        for dtype in (0, 1, 2, 3):
            n = ctypes.c_size_t(0)
            assert lib.rnnt_engine_workspace_bytes(2, 5, 3, 128, 128, dtype, ctypes.byref(n)) == 0
            assert _joint(lib, bwd, dtype=dtype, ws_bytes=n.value - 1) == -3 and "workspace" in _err(lib)  # the same workspace


def test_version_is_unchanged(lib):
    assert lib.rnnt_engine_version() == 4


# ---- the operators' argument errors that come before any device work
def _cpu_inputs(B=2, T=5, U=2, V=8):
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(B, T, U + 1, V, generator=g)
    targets = torch.randint(0, V - 1, (B, U), generator=g, dtype=torch.int32)
    return logits, targets, torch.full((B,), T, dtype=torch.int32), torch.full((B,), U, dtype=torch.int32)


def test_operators_reject_bad_restrictions_on_the_host():
    lg, tg, ll, tl = _cpu_inputs()
    fr = torch.zeros(2, 2, dtype=torch.int32)
    B, T, U, H, V = 2, 5, 2, 16, 8
    joint = (torch.randn(B, T, H), torch.randn(B, U + 1, H), torch.randn(V, H), torch.randn(V), tg, ll, tl)
    for call in (lambda **kw: rnnt_amd.rnnt_loss(lg, tg, ll, tl, **kw), lambda **kw: rnnt_amd.joint_rnnt_loss(*joint, **kw)):
        with pytest.raises(RuntimeError, match="int32"):
            call(restrict_frames=fr.long())
        with pytest.raises(RuntimeError, match=r"shape \[B, U\]"):
            call(restrict_frames=fr[:, :1].contiguous())
        with pytest.raises(RuntimeError, match=r"shape \[B, U\]"):
            call(restrict_frames=fr[0])
        with pytest.raises(RuntimeError, match="contiguous"):
            call(restrict_frames=torch.zeros(2, 4, dtype=torch.int32)[:, ::2])
        with pytest.raises(RuntimeError, match="HIP device"):
            call(restrict_frames=fr)  # a CPU tensor: no CPU path
        with pytest.raises(RuntimeError, match="tensor"):
            call(restrict_frames=[[0, 0], [0, 0]])


@pytest.mark.parametrize("bad", [-1, 1.0, True, None, 2 ** 31])
def test_buffers_must_be_ints_that_are_not_negative(bad):
    lg, tg, ll, tl = _cpu_inputs()
    fr = torch.zeros(2, 2, dtype=torch.int32)
    for kw in (dict(restrict_left=bad), dict(restrict_right=bad)):
        with pytest.raises(ValueError, match="restrict_"):  # (before the tensor checks: no device needed)
            rnnt_amd.rnnt_loss(lg, tg, ll, tl, restrict_frames=fr, **kw)


def test_shard_utterances_slices_every_per_utterance_tensor():
    from rnnt_amd.parallel import shard_bounds, shard_utterances
    B = 5
    enc, frames, lens = torch.randn(B, 7, 4), torch.arange(B * 3, dtype=torch.int32).view(B, 3), torch.arange(B, dtype=torch.int32)
    got = [shard_utterances(2, r, enc, None, frames, lens) for r in range(2)]
    for r, (e, none, f, n) in enumerate(got):
        lo, hi = shard_bounds(B, 2, r)
        assert none is None and torch.equal(e, enc[lo:hi]) and torch.equal(f, frames[lo:hi]) and torch.equal(n, lens[lo:hi])
        assert f.is_contiguous()
    assert torch.equal(torch.cat([g[2] for g in got]), frames)
    with pytest.raises(RuntimeError, match="leading dimension"):
        shard_utterances(2, 0, enc, frames[:4])
