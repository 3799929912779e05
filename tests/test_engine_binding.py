"""Which C entry each loss / alignment wrapper of rnnt_amd.engine reaches, and with which arguments at which positions —
on the CPU, against a stand-in library that records its calls.  The table of expected entries and positions is written out
here from include/rnnt_engine.h; it is not derived from the binding.  (The decode family's loops need events and a device:
the GPU suite walks them.)"""
import contextlib
import ctypes

import pytest
import torch

from rnnt_amd import engine

B, T, U1, H, V = 2, 3, 2, 4, 4
BLANK, SCALE, CLAMP, FE, DP, LEFT, RIGHT = 1, 0.125, 0.75, 0.25, 0.5, 3, 5
DTYPE, CODE = "bf16x3", 2
WS_BYTES, AUX_BYTES = 64, 32


class _Lib:
    """Every entry records (name, args) and returns 0; a size query writes WS_BYTES, the layout query AUX_BYTES, through its byref."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            if name.endswith("_bytes"):
                args[-1]._obj.value = WS_BYTES
            elif name == "rnnt_engine_workspace_layout":
                args[-1]._obj.aux_bytes = AUX_BYTES
            return 0
        return entry


@pytest.fixture
def fake(monkeypatch):
    lib = _Lib()
    lib.workspaces = []

    def workspace(dev, nbytes):
        lib.workspaces.append(nbytes)
        return torch.empty(nbytes, dtype=torch.uint8)

    monkeypatch.setattr(engine, "_lib", lib)
    monkeypatch.setattr(engine, "_require_cuda", lambda *tensors: tensors[0].device)
    monkeypatch.setattr(engine, "workspace", workspace)
    monkeypatch.setattr(engine, "_stream", lambda dev: ctypes.c_void_p(0))
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    return lib


def _fused():
    return (torch.zeros(B, T, H), torch.zeros(B, U1, H), torch.zeros(V, H), torch.zeros(V),
            torch.zeros(B, U1 - 1, dtype=torch.int32), torch.full((B,), T, dtype=torch.int32),
            torch.full((B,), U1 - 1, dtype=torch.int32), BLANK)


def _unfused():
    return (torch.zeros(B, T, U1, V), torch.zeros(B, U1 - 1, dtype=torch.int32), torch.full((B,), T, dtype=torch.int32),
            torch.full((B,), U1 - 1, dtype=torch.int32), BLANK)


def _frames():
    return torch.zeros(B, U1 - 1, dtype=torch.int32)


def _val(a):
    return getattr(a, "value", a)


DIMS5 = {8: B, 9: T, 10: U1, 11: H, 12: V, 13: BLANK}  # the fused entries: after the eight pointers
DIMS4 = {4: B, 5: T, 6: U1, 7: V, 8: BLANK}            # the entries on materialised logits: after the four pointers

# name of the call -> (the call, its size query, the C entry it must reach, {position: value} in that entry's argument list)
CASES = {
    "joint_loss_fwd_bwd": (
        lambda: engine.joint_loss_fwd_bwd(*_fused(), SCALE, dtype=DTYPE),
        "rnnt_engine_workspace_bytes", "rnnt_engine_joint_loss_fwd_bwd", {**DIMS5, 14: -1.0, 15: SCALE, 16: CODE}),
    "joint_loss_fwd_bwd_reg": (
        lambda: engine.joint_loss_fwd_bwd_reg(*_fused(), SCALE, FE, DP, dtype=DTYPE),
        "rnnt_engine_workspace_bytes", "rnnt_engine_joint_loss_fwd_bwd_reg", {**DIMS5, 14: -1.0, 15: SCALE, 16: FE, 17: DP, 18: CODE}),
    "joint_loss_fwd_bwd_reg, both zero": (  # still the _reg entry: it runs the f16x2 route without its flush rule
        lambda: engine.joint_loss_fwd_bwd_reg(*_fused(), SCALE, 0.0, 0.0, dtype=DTYPE),
        "rnnt_engine_workspace_bytes", "rnnt_engine_joint_loss_fwd_bwd_reg", {**DIMS5, 14: -1.0, 15: SCALE, 16: 0.0, 17: 0.0, 18: CODE}),
    "joint_loss_fwd_bwd_restrict": (
        lambda: engine.joint_loss_fwd_bwd_restrict(*_fused(), SCALE, FE, DP, _frames(), LEFT, RIGHT, dtype=DTYPE),
        "rnnt_engine_workspace_bytes", "rnnt_engine_joint_loss_fwd_bwd_restrict",
        {**DIMS5, 14: -1.0, 15: SCALE, 16: FE, 17: DP, 19: LEFT, 20: RIGHT, 21: CODE}),
    "joint_loss_fwd": (
        lambda: engine.joint_loss_fwd(*_fused(), dtype=DTYPE),
        "rnnt_engine_workspace_bytes", "rnnt_engine_joint_loss_fwd", {**DIMS5, 14: CODE}),
    "joint_loss_fwd_reg": (
        lambda: engine.joint_loss_fwd_reg(*_fused(), DP, dtype=DTYPE),
        "rnnt_engine_workspace_bytes", "rnnt_engine_joint_loss_fwd_reg", {**DIMS5, 14: DP, 15: CODE}),
    "joint_loss_fwd_restrict": (
        lambda: engine.joint_loss_fwd_restrict(*_fused(), DP, _frames(), LEFT, RIGHT, dtype=DTYPE),
        "rnnt_engine_workspace_bytes", "rnnt_engine_joint_loss_fwd_restrict", {**DIMS5, 14: DP, 16: LEFT, 17: RIGHT, 18: CODE}),
    "joint_align": (
        lambda: engine.joint_align(*_fused(), dtype=DTYPE),
        "rnnt_engine_workspace_bytes", "rnnt_engine_joint_align", {**DIMS5, 14: CODE}),
    "loss_fwd_bwd": (
        lambda: engine.loss_fwd_bwd(*_unfused(), CLAMP),
        "rnnt_engine_loss_workspace_bytes", "rnnt_engine_loss_fwd_bwd", {**DIMS4, 9: CLAMP, 10: 0}),
    "loss_fwd_bwd_reg": (
        lambda: engine.loss_fwd_bwd_reg(*_unfused(), CLAMP, FE, DP),
        "rnnt_engine_loss_workspace_bytes", "rnnt_engine_loss_fwd_bwd_reg", {**DIMS4, 9: CLAMP, 10: FE, 11: DP, 12: 0}),
    "loss_fwd_bwd_restrict": (
        lambda: engine.loss_fwd_bwd_restrict(*_unfused(), CLAMP, FE, DP, _frames(), LEFT, RIGHT),
        "rnnt_engine_loss_workspace_bytes", "rnnt_engine_loss_fwd_bwd_restrict",
        {**DIMS4, 9: CLAMP, 10: FE, 11: DP, 13: LEFT, 14: RIGHT, 15: 0}),
    "align": (
        lambda: engine.align(*_unfused()),
        "rnnt_engine_loss_workspace_bytes", "rnnt_engine_align", DIMS4),
    "joint_loss_fwd_bwd, stage": (
        lambda: engine.joint_loss_fwd_bwd(*_fused(), SCALE, stage=6, dtype=DTYPE),
        "rnnt_engine_workspace_bytes", "rnnt_engine_run_stage",
        {0: 6, **{k + 1: v for k, v in DIMS5.items()}, 15: -1.0, 16: SCALE, 17: CODE}),
    "joint_loss_fwd_bwd, stage_mask": (
        lambda: engine.joint_loss_fwd_bwd(*_fused(), SCALE, dtype=DTYPE, stage_mask=engine.STAGES_FORWARD),
        "rnnt_engine_workspace_bytes", "rnnt_engine_run_stages",
        {0: 7, 1: 0, **{k + 2: v for k, v in DIMS5.items()}, 16: -1.0, 17: SCALE, 18: CODE}),
    "joint_loss_fwd_bwd, variant": (
        lambda: engine.joint_loss_fwd_bwd(*_fused(), SCALE, dtype=DTYPE, variant=engine.VARIANT_SEPARATE_G),
        "rnnt_engine_workspace_bytes", "rnnt_engine_run_stages",
        {0: 255, 1: 32, **{k + 2: v for k, v in DIMS5.items()}, 16: -1.0, 17: SCALE, 18: CODE}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_wrapper_reaches_its_entry_with_its_arguments_in_place(fake, case):
    call, query, entry, at = CASES[case]
    out = call()
    # one size query, then the entry: no other call into the library
    assert [name for name, _ in fake.calls] == [query, entry]
    assert fake.workspaces == [WS_BYTES]
    args = fake.calls[-1][1]
    assert len(args) == len(engine.SIGNATURES[entry])
    for pos, want in at.items():
        assert _val(args[pos]) == want, f"{entry}: argument {pos} is {_val(args[pos])!r}, not {want!r}"
    assert _val(args[-2]) == WS_BYTES  # the workspace's size, before the stream
    if "fwd_bwd" in entry or "run_stage" in entry:
        if case.startswith("joint"):
            assert [tuple(o.shape) for o in out] == [(B,), (B, T, H), (B, U1, H), (V, H), (V,)]
        else:
            assert tuple(out[0].shape) == (B,) and tuple(out[1].shape) == (B, T, U1, V)
    elif "align" in entry:
        assert tuple(out[0].shape) == (B,) and tuple(out[1].shape) == (B, U1 - 1) and out[1].dtype == torch.int32
    else:
        assert tuple(out.shape) == (B,)


def test_fp32_substitution_variant_adds_the_aux_bytes_with_one_layout_query(fake):
    engine.joint_loss_fwd_bwd(*_fused(), SCALE, dtype=DTYPE, variant=engine.VARIANT_X3_FP32_FWD)
    assert [name for name, _ in fake.calls] == ["rnnt_engine_workspace_bytes", "rnnt_engine_workspace_layout", "rnnt_engine_run_stages"]
    assert fake.workspaces == [WS_BYTES + AUX_BYTES]
    args = fake.calls[-1][1]
    assert len(args) == len(engine.SIGNATURES["rnnt_engine_run_stages"])
    assert (_val(args[0]), _val(args[1])) == (255, engine.VARIANT_X3_FP32_FWD)


def test_caller_outputs_and_want_grad_are_passed_through(fake):
    outs = (torch.zeros(B), torch.zeros(B, T, H), torch.zeros(B, U1, H), torch.zeros(V, H), torch.zeros(V))
    assert engine.joint_loss_fwd_bwd(*_fused(), SCALE, outs, dtype=DTYPE) is outs
    assert [_val(a) for a in fake.calls[-1][1][17:22]] == [o.data_ptr() for o in outs]
    assert engine.joint_loss_fwd_bwd_reg(*_fused(), SCALE, FE, DP, outs, dtype=DTYPE) is outs
    assert [_val(a) for a in fake.calls[-1][1][19:24]] == [o.data_ptr() for o in outs]
    assert engine.joint_loss_fwd_bwd_restrict(*_fused(), SCALE, FE, DP, _frames(), LEFT, RIGHT, outs, dtype=DTYPE) is outs
    assert [_val(a) for a in fake.calls[-1][1][22:27]] == [o.data_ptr() for o in outs]
    costs, grad = engine.loss_fwd_bwd(*_unfused(), CLAMP, want_grad=False)
    assert grad is None and _val(fake.calls[-1][1][12]) in (0, None)  # a NULL gradient pointer


def test_first_error_reported_is_the_regulariser_then_the_tensors_then_the_window(fake):
    enc, pred, W, bias, targets, ll, tl, blank = _fused()
    with pytest.raises(ValueError, match="fastemit_lambda"):
        engine.joint_loss_fwd_bwd_restrict(enc.double(), pred, W, bias, targets, ll, tl, blank, SCALE, -1.0, DP, _frames(), -1, RIGHT,
                                           dtype=DTYPE)
    with pytest.raises(RuntimeError, match="enc must be torch.float32"):
        engine.joint_loss_fwd_bwd_restrict(enc.double(), pred, W, bias, targets, ll, tl, blank, SCALE, FE, DP, _frames(), -1, RIGHT,
                                           dtype=DTYPE)
    with pytest.raises(ValueError, match="delay_penalty"):
        engine.joint_loss_fwd_restrict(enc.double(), pred, W, bias, targets, ll, tl, blank, float("nan"), _frames(), LEFT, -1, dtype=DTYPE)
    with pytest.raises(ValueError, match="restrict_right"):
        engine.joint_loss_fwd_restrict(enc, pred, W, bias, targets, ll, tl, blank, DP, _frames(), LEFT, -1, dtype="no such route")
    with pytest.raises(ValueError, match="unsupported compute dtype"):
        engine.joint_loss_fwd_restrict(enc, pred, W, bias, targets, ll, tl, blank, DP, _frames(), LEFT, RIGHT, dtype="no such route")
    assert fake.calls == []
