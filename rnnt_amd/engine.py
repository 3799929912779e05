"""ctypes binding of librnnt_engine.so (include/rnnt_engine.h) for torch tensors.

PyTorch is plumbing here: it owns device memory and the HIP stream; every compute call goes
through the C ABI.  There is NO fallback: if the library is missing or a call fails, a
RuntimeError is raised.
"""
import ctypes
import math
import os
import subprocess
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
# RNNT_ENGINE_LIB: another BUILD of the same engine (a diagnostic -DRNNT_ABLATE / -DRNNT_STAMPS library of
# tools/exp_*.py, an A/B candidate).  Still the HIP engine and nothing else: a missing file raises.
LIB_PATH = os.environ.get("RNNT_ENGINE_LIB") or os.path.join(_CSRC, "librnnt_engine.so")

DTYPE_F32 = 0
DTYPE_BF16 = 1  # bf16 GEMM operands, fp32 accumulate, fp16 logits (workspace), fp32/fp64 loss; fp32 tensors at the boundary
DTYPE_F32_BF16X3 = 2  # fp32-accurate products as six bf16 MFMA products of 3-way split operands (x3.hip)
DTYPE_F32_F16X2 = 3  # fp32-class products as three fp16 MFMA products of scaled, 2-way split operands (x2.hip): half the bf16x3 route's matrix work
# The arithmetic the product ships (JointNetwork.compute_dtype, the default of rnnt_amd.joint_rnnt_loss and of bench.py).  The low-level
# entry points joint_loss_fwd_bwd / joint_loss_fwd take `dtype` as a REQUIRED keyword.
DEFAULT_DTYPE = "f16x2"
_DTYPES = {"fp32": DTYPE_F32, "f32": DTYPE_F32, "float32": DTYPE_F32, DTYPE_F32: DTYPE_F32,
           "bf16": DTYPE_BF16, "bfloat16": DTYPE_BF16, DTYPE_BF16: DTYPE_BF16,
           "bf16x3": DTYPE_F32_BF16X3, "f32_bf16x3": DTYPE_F32_BF16X3, DTYPE_F32_BF16X3: DTYPE_F32_BF16X3,
           "f16x2": DTYPE_F32_F16X2, "f32_f16x2": DTYPE_F32_F16X2, DTYPE_F32_F16X2: DTYPE_F32_F16X2}


class _Int32:
    """argtypes entry for a C `int`: ctypes' own c_int wraps silently (2**31 -> -2**31) and a dimension
    that does not fit must raise, as must a float where a dimension is expected."""

    @classmethod
    def from_param(cls, v):
        if isinstance(v, ctypes.c_int):
            return v
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"rnnt_engine: C int argument needs a Python int, got {type(v).__name__} ({v!r})")
        if not -2 ** 31 <= v < 2 ** 31:
            raise OverflowError(f"rnnt_engine: {v} does not fit a C int")
        return ctypes.c_int(v)


# Argument kinds of every entry point of include/rnnt_engine.h, in declaration order (i = int,
# q = int64_t, z = size_t, f = float, d = double, p = any pointer).  tests/test_abi.py re-derives this
# table from the header, so a prototype change that is not mirrored here fails on the CPU.
_KINDS = {"i": _Int32, "q": ctypes.c_int64, "z": ctypes.c_size_t, "f": ctypes.c_float,
          "d": ctypes.c_double, "p": ctypes.c_void_p}
SIGNATURES = {
    "rnnt_engine_version": "",
    "rnnt_engine_set_flags": "i",
    "rnnt_engine_set_debug": "p",
    "rnnt_engine_debug_query": "i",
    "rnnt_engine_last_error": "",
    "rnnt_engine_workspace_bytes": "iiiiiip",
    "rnnt_engine_loss_workspace_bytes": "iiiiip",
    "rnnt_engine_joint_fwd_workspace_bytes": "iiiiiip",
    "rnnt_engine_joint_fwd": "pppppiiiiiippzp",
    "rnnt_engine_loss_fwd_bwd": "ppppiiiiifipppzp",
    "rnnt_engine_joint_loss_fwd_bwd": "ppppppppiiiiiiffippppppzp",
    "rnnt_engine_joint_loss_fwd": "ppppppppiiiiiiippzp",
    "rnnt_engine_loss_fwd_bwd_reg": "ppppiiiiifffipppzp",
    "rnnt_engine_joint_loss_fwd_bwd_reg": "ppppppppiiiiiiffffippppppzp",
    "rnnt_engine_joint_loss_fwd_reg": "ppppppppiiiiiifippzp",
    "rnnt_engine_loss_fwd_bwd_restrict": "ppppiiiiifffpiiipppzp",
    "rnnt_engine_joint_loss_fwd_bwd_restrict": "ppppppppiiiiiiffffpiiippppppzp",
    "rnnt_engine_joint_loss_fwd_restrict": "ppppppppiiiiiifpiiippzp",
    "rnnt_engine_align": "ppppiiiiipppzp",
    "rnnt_engine_joint_align": "ppppppppiiiiiiipppzp",
    "rnnt_engine_ctc_workspace_bytes": "iiiip",
    "rnnt_engine_ctc_loss_fwd_bwd": "ppppiiiiippppzp",
    "rnnt_engine_ctc_greedy_decode": "ppiiiippp",
    "rnnt_engine_joint_bwd_workspace_bytes": "iiiiiip",
    "rnnt_engine_joint_bwd": "pppppiiiiiipppppzp",
    "rnnt_engine_greedy_scan_workspace_bytes": "iiip",
    "rnnt_engine_greedy_scan": "pqqpppiiiiippzp",
    "rnnt_engine_greedy_decode_workspace_bytes": "iiiiip",
    "rnnt_engine_greedy_decode": "pqipiiiffppppiiiiiiiippppzp",
    "rnnt_engine_greedy_decode_lstm_workspace_bytes": "iiiiiiiiiiip",
    "rnnt_engine_greedy_decode_lstm": "pqipiipiiiiiifffppppiiiiiiiipppppzp",
    "rnnt_engine_greedy_stream_lstm_bytes": "iiiiiiiiiip",
    "rnnt_engine_greedy_stream_lstm_init": "iiiiiipzp",
    "rnnt_engine_greedy_stream_lstm_push_workspace_bytes": "iiiiiiiiiiip",
    "rnnt_engine_greedy_stream_lstm_push": "pqipiipiiiiiifffppppiiiiiiiippipzpzp",
    "rnnt_engine_greedy_decode_persistent_workspace_bytes": "iiiiiiip",
    "rnnt_engine_greedy_decode_persistent": "pqipiiiffppppiiiiipppppzp",
    "rnnt_engine_greedy_decode_tables_bytes": "iiiiip",
    "rnnt_engine_greedy_decode_build_tables": "piiifppipzp",
    "rnnt_engine_greedy_stream_init": "pip",
    "rnnt_engine_greedy_stream_decode_workspace_bytes": "iiiiiiiiiip",
    "rnnt_engine_greedy_stream_decode": "pqipiiiffppppiiiiipipppzp",
    "rnnt_engine_beam_decode_workspace_bytes": "iiiiiiiip",
    "rnnt_engine_beam_decode": "pqipiiiffppppiiiiiipiipppppzp",
    "rnnt_engine_beam_decode_batch_workspace_bytes": "iiiiiiiiip",
    "rnnt_engine_beam_decode_batch": "pqipiipiiiffppppiiiiiipiipppppzp",
    "rnnt_engine_beam_decode_lstm_workspace_bytes": "iiiiiiiiiiiip",
    "rnnt_engine_beam_decode_lstm": "pqipiipiiiiiifffppppiiiiiiiipppppzp",
    "rnnt_engine_beam_decode_ctx_workspace_bytes": "iiiiiiiip",
    "rnnt_engine_beam_decode_ctx": "pqipiiiffppppiiiiiipiipppppzpp",
    "rnnt_engine_beam_decode_batch_ctx_workspace_bytes": "iiiiiiiiip",
    "rnnt_engine_beam_decode_batch_ctx": "pqipiipiiiffppppiiiiiipiipppppzpp",
    "rnnt_engine_beam_stream_bytes": "iiiiiiiiip",
    "rnnt_engine_beam_stream_init": "iiiiiiiiiiipppzp",
    "rnnt_engine_beam_stream_push": "pqipiipiiiffppppiiiiiipiipppppzp",
    "rnnt_engine_grad_norm_workspace_bytes": "ipp",
    "rnnt_engine_grad_norm": "ippppzp",
    "rnnt_engine_adamw_step": "ipppppdddddqpfip",
    "rnnt_engine_adamw_step_dev": "ippppppddddpppfip",
    "rnnt_engine_conv_predictor_saved_bytes": "iiiiip",
    "rnnt_engine_conv_predictor_fwd": "piiiiipppfffppzp",
    "rnnt_engine_conv_predictor_bwd": "piiiiipppfpppzp",
    "rnnt_engine_lstm_predictor_saved_bytes": "iiiiiiiip",
    "rnnt_engine_lstm_predictor_workspace_bytes": "iiiiiiiiip",
    "rnnt_engine_lstm_predictor_fwd": "piiiiiiiipppffffpppzpzp",
    "rnnt_engine_lstm_predictor_bwd": "piiiiiiiippffffpppzpzp",
    "rnnt_engine_linear_fwd": "pqppiiipp",
    "rnnt_engine_linear_bwd_workspace_bytes": "iiip",
    "rnnt_engine_linear_bwd": "pqppiiippppzp",
    "rnnt_engine_linear_x2_workspace_bytes": "iiiip",
    "rnnt_engine_linear_x2_fwd": "pqppiiippzp",
    "rnnt_engine_linear_x2_bwd": "pqppiiippppzp",
    "rnnt_engine_encoder_packed_bytes": "pip",
    "rnnt_engine_encoder_pack": "pipzp",
    "rnnt_engine_encoder_workspace_bytes": "piiiipp",
    "rnnt_engine_encoder_fwd": "pipppiiippzp",
    "rnnt_engine_encoder_stream_push": "pipppiippppippzp",
    "rnnt_engine_encoder_train_packed_bytes": "pip",
    "rnnt_engine_encoder_train_pack": "pipzp",
    "rnnt_engine_encoder_train_saved_bytes": "piiipp",
    "rnnt_engine_encoder_train_workspace_bytes": "piiiipp",
    "rnnt_engine_encoder_train_fwd": "pipppiipppippzpzp",
    "rnnt_engine_encoder_train_bwd": "pipppiipppppzppzp",
    "rnnt_engine_featurizer_basis_bytes": "pp",
    "rnnt_engine_featurizer_pack": "pppzp",
    "rnnt_engine_featurizer_workspace_bytes": "piip",
    "rnnt_engine_featurizer_fwd": "ppppqiipippppipzp",
    "rnnt_engine_featurizer_stream_push": "ppppipqiiippppipipzp",
    "rnnt_engine_allreduce": "pzpp",
    "rnnt_engine_workspace_layout": "iiiiiip",
    "rnnt_engine_run_stage": "ippppppppiiiiiiffippppppzp",
    "rnnt_engine_run_stages": "iippppppppiiiiiiffippppppzp",
}


def dtype_code(dtype):
    if isinstance(dtype, torch.dtype):
        dtype = {torch.float32: "fp32", torch.bfloat16: "bf16"}.get(dtype, dtype)
    try:
        return _DTYPES[dtype]
    except (KeyError, TypeError):
        raise ValueError(f"rnnt_amd: unsupported compute dtype {dtype!r} (fp32, bf16, bf16x3 or f16x2)") from None
_lock = threading.Lock()
_lib = None
_workspaces = {}
_captured = {}  # (device, stream) -> workspace a captured HIP graph points into: never freed or replaced

EXPORTS = (
    "rnnt_engine_version", "rnnt_engine_last_error", "rnnt_engine_workspace_bytes",
    "rnnt_engine_loss_workspace_bytes", "rnnt_engine_joint_fwd_workspace_bytes",
    "rnnt_engine_joint_fwd", "rnnt_engine_loss_fwd_bwd", "rnnt_engine_joint_loss_fwd_bwd",
    "rnnt_engine_workspace_layout", "rnnt_engine_run_stage",
    "rnnt_engine_greedy_scan_workspace_bytes", "rnnt_engine_greedy_scan",
    "rnnt_engine_greedy_decode_workspace_bytes", "rnnt_engine_greedy_decode",
    "rnnt_engine_greedy_decode_persistent_workspace_bytes", "rnnt_engine_greedy_decode_persistent",
    "rnnt_engine_greedy_decode_tables_bytes", "rnnt_engine_greedy_decode_build_tables",
    "rnnt_engine_greedy_stream_init", "rnnt_engine_greedy_stream_decode_workspace_bytes", "rnnt_engine_greedy_stream_decode",
    "rnnt_engine_beam_decode_workspace_bytes", "rnnt_engine_beam_decode",
    "rnnt_engine_beam_decode_batch_workspace_bytes", "rnnt_engine_beam_decode_batch",
    "rnnt_engine_beam_stream_bytes", "rnnt_engine_beam_stream_init", "rnnt_engine_beam_stream_push",
    "rnnt_engine_beam_decode_ctx_workspace_bytes", "rnnt_engine_beam_decode_ctx",
    "rnnt_engine_beam_decode_batch_ctx_workspace_bytes", "rnnt_engine_beam_decode_batch_ctx",
    "rnnt_engine_joint_loss_fwd", "rnnt_engine_run_stages",
    "rnnt_engine_joint_bwd_workspace_bytes", "rnnt_engine_joint_bwd",
    "rnnt_engine_grad_norm_workspace_bytes", "rnnt_engine_grad_norm", "rnnt_engine_adamw_step",
    "rnnt_engine_adamw_step_dev",
    "rnnt_engine_conv_predictor_saved_bytes", "rnnt_engine_conv_predictor_fwd",
    "rnnt_engine_conv_predictor_bwd", "rnnt_engine_linear_fwd", "rnnt_engine_linear_bwd_workspace_bytes",
    "rnnt_engine_linear_bwd", "rnnt_engine_allreduce",
    "rnnt_engine_linear_x2_workspace_bytes", "rnnt_engine_linear_x2_fwd", "rnnt_engine_linear_x2_bwd",
    "rnnt_engine_align", "rnnt_engine_joint_align",
    "rnnt_engine_loss_fwd_bwd_reg", "rnnt_engine_joint_loss_fwd_bwd_reg", "rnnt_engine_joint_loss_fwd_reg",
    "rnnt_engine_loss_fwd_bwd_restrict", "rnnt_engine_joint_loss_fwd_bwd_restrict", "rnnt_engine_joint_loss_fwd_restrict",
    "rnnt_engine_encoder_packed_bytes", "rnnt_engine_encoder_pack", "rnnt_engine_encoder_workspace_bytes",
    "rnnt_engine_encoder_fwd", "rnnt_engine_encoder_stream_push",
    "rnnt_engine_encoder_train_packed_bytes", "rnnt_engine_encoder_train_pack", "rnnt_engine_encoder_train_saved_bytes",
    "rnnt_engine_encoder_train_workspace_bytes", "rnnt_engine_encoder_train_fwd", "rnnt_engine_encoder_train_bwd",
    "rnnt_engine_featurizer_basis_bytes", "rnnt_engine_featurizer_pack", "rnnt_engine_featurizer_workspace_bytes",
    "rnnt_engine_featurizer_fwd", "rnnt_engine_featurizer_stream_push",
    "rnnt_engine_lstm_predictor_saved_bytes", "rnnt_engine_lstm_predictor_workspace_bytes",
    "rnnt_engine_lstm_predictor_fwd", "rnnt_engine_lstm_predictor_bwd",
    "rnnt_engine_greedy_decode_lstm_workspace_bytes", "rnnt_engine_greedy_decode_lstm",
    "rnnt_engine_beam_decode_lstm_workspace_bytes", "rnnt_engine_beam_decode_lstm",
    "rnnt_engine_greedy_stream_lstm_bytes", "rnnt_engine_greedy_stream_lstm_init",
    "rnnt_engine_greedy_stream_lstm_push_workspace_bytes", "rnnt_engine_greedy_stream_lstm_push",
    "rnnt_engine_ctc_workspace_bytes", "rnnt_engine_ctc_loss_fwd_bwd", "rnnt_engine_ctc_greedy_decode",
)

# per-call kernel variants (include/rnnt_engine.h RNNT_VARIANT_*): bit-identical results
VARIANT_SEPARATE_G = 32
VARIANT_SEPARATE_HIDDEN = 64
VARIANT_FWD_LDS_RING = 128
VARIANT_FWD_ONE_WG_PER_TILE = 256
VARIANT_X2_NO_FLUSH_SKIP = 512  # f16x2 route: no cell flushed (costs / grad_enc / grad_pred bit-identical; grad_W / grad_bias: summation order)
VARIANT_X3_FP32_FWD = 4096  # bf16x3 route: this stage on the fp32 route's kernel (isolation checks; not bit-identical)
VARIANT_X3_FP32_DH = 8192
# bits 14 and up are reserved (include/rnnt_engine.h): librnnt_engine.so refuses every one of them with RNNT_ERR_UNSUPPORTED
VARIANT_LAB_MASK = 0x7FFFC000
STAGES_ALL = 255
STAGES_FORWARD = 7  # operand producers + joint-forward GEMM + lattice sweep: costs only


class WsLayout(ctypes.Structure):
    _fields_ = [(n, ctypes.c_size_t) for n in (
        "logits", "hidden", "denom_s", "lpb_s", "lpe_s", "alpha_s", "beta_s", "coef", "wpack",
        "enc_copy", "slab_enc", "slab_pred", "slab_w", "slab_b", "counters", "total", "rows_pad")] + [
        (n, ctypes.c_int) for n in ("n_ublk", "n_ttile", "n_split", "D")] + [
        (n, ctypes.c_size_t) for n in ("g_lo", "aux", "aux_bytes", "ep", "x2_live")]


def build(force: bool = False) -> str:
    """Compile librnnt_engine.so for gfx950 with hipcc (rnnt_amd/csrc/Makefile)."""
    cmd = ["make", "-C", _CSRC, "-j4", "-s", "librnnt_engine.so"]
    if force:
        cmd.insert(1, "-B")
    subprocess.check_call(cmd)
    return LIB_PATH


def lib():
    """Load the engine; raises RuntimeError (never falls back) when it is missing."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    f"rnnt_amd: HIP engine {LIB_PATH} is missing; build it with "
                    "`python -c 'import __graft_entry__ as g; g.build()'` "
                    "(hipcc --offload-arch=gfx950). There is no CPU/torch fallback.")
            L = ctypes.CDLL(LIB_PATH)
            for name in EXPORTS:
                if not hasattr(L, name):
                    raise RuntimeError(f"rnnt_amd: {LIB_PATH} does not export {name}")
            for name, kinds in SIGNATURES.items():  # typed bindings: a wrong kind or an int beyond 2^31 raises
                fn = getattr(L, name)
                fn.argtypes = [_KINDS[k] for k in kinds]
                fn.restype = ctypes.c_int
            L.rnnt_engine_last_error.restype = ctypes.c_char_p
            L.rnnt_engine_set_debug.restype = None
            _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        msg = lib().rnnt_engine_last_error().decode()
        if rc == -1:
            raise ValueError(f"rnnt_engine: {msg}")
        raise RuntimeError(f"rnnt_engine error {rc}: {msg}")


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _nonempty(targets):
    """U = 0 (no labels) gives an empty [B,0] tensor whose data_ptr is NULL; the ABI wants a
    valid pointer, the kernels never dereference it in that case."""
    if targets.numel() == 0:
        return torch.zeros(1, dtype=torch.int32, device=targets.device)
    return targets


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require_cuda(*tensors):
    dev = tensors[0].device
    for t in tensors:
        if t is None:
            continue
        if t.device.type != "cuda":
            raise RuntimeError(
                "rnnt_amd: tensors must live on a HIP device (got %s); the engine has no CPU path"
                % t.device)
        if t.device != dev:
            raise RuntimeError("rnnt_amd: all tensors must be on the same device")
    return dev


def _require_dtype(dtype, **tensors):
    """The C side reinterprets every pointer: a wrong element type would be read past its
    allocation.  Raise instead."""
    for name, t in tensors.items():
        if t is not None and t.dtype != dtype:
            raise RuntimeError(f"rnnt_amd: {name} must be {dtype} (got {t.dtype})")


def _require_contiguous(**tensors):
    for name, t in tensors.items():
        if t is not None and not t.is_contiguous():
            raise RuntimeError(f"rnnt_amd: {name} must be contiguous")


def workspace(device, nbytes):
    """Grow-only scratch buffer per (device, stream): work enqueued on two streams of one device
    never shares scratch memory (torch owns the memory; 256-byte aligned).

    HIP graphs: a call captured by `torch.cuda.graph` has this buffer's address baked into its
    kernel arguments.  A buffer handed out during a capture is therefore PINNED: it is never
    replaced (growth on that stream raises instead of freeing memory a graph still replays into)
    and `release_workspaces()` keeps it alive — INTEGRATION.md "HIP graphs"."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (device.type, idx, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    capturing = torch.cuda.is_current_stream_capturing()
    if ws is None or ws.numel() < nbytes:
        if key in _captured:
            raise RuntimeError(
                f"rnnt_amd: this stream's workspace ({ws.numel()} B) is baked into a captured HIP graph and the "
                f"call needs {int(nbytes)} B; warm up with the largest shapes before capturing "
                "(rnnt_amd.engine.workspace)")
        _workspaces.pop(key, None)
        ws = None
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    if capturing:
        _captured[key] = ws
    return ws


def release_workspaces():
    """Drop the cached scratch buffers — except those a captured HIP graph points into — and hand their memory back to
    the driver (torch's caching allocator would otherwise keep a freed 145 GB segment that small tensors then settle in:
    the next, larger workspace — config 4 on the bf16x3 route needs 212 GB of the 288 — could not be allocated beside it)."""
    dropped = False
    for key in list(_workspaces):
        if key not in _captured:
            del _workspaces[key]
            dropped = True
    if dropped and torch.cuda.is_initialized():
        torch.cuda.empty_cache()


def layout(B, T, U1, H, V, dtype="fp32"):
    L = WsLayout()
    _check(lib().rnnt_engine_workspace_layout(B, T, U1, H, V, dtype_code(dtype), ctypes.byref(L)))
    return L


def x2_live_counts(device, B, T, U1, H, V):
    """Device-side counts of the last f16x2 fused call of these dims on the current stream (rnnt_engine_ws_layout.x2_live):
    dict(live_ksteps, ksteps, live_tiles, tiles) — the 16-cell dW k-steps the call walked of those that hold a cell, the
    dHidden tiles (8 t x 16 u) it ran of all.  Synchronises."""
    L = layout(B, T, U1, H, V, "f16x2")
    ws = workspace(device, L.total)
    c = ws[L.x2_live:L.x2_live + 16].view(torch.int32).cpu().tolist()
    return dict(live_ksteps=c[0], ksteps=c[1], live_tiles=c[2], tiles=c[3])


def x2_live_group_counts(device, B, T, U1, H, V):
    """Beside x2_live_counts, the 4-cell groups (linear cell index // 4) of the dW GEMM's walk: dict(live_groups, groups) — the
    groups the last f16x2 fused call of these dims listed of those that hold a cell (four list entries make a k-step).  Synchronises."""
    L = layout(B, T, U1, H, V, "f16x2")
    ws = workspace(device, L.total)
    c = ws[L.x2_live + 16:L.x2_live + 24].view(torch.int32).cpu().tolist()
    return dict(live_groups=c[0], groups=c[1])


def workspace_bytes(B, T, U1, H, V, dtype="fp32"):
    n = ctypes.c_size_t(0)
    _check(lib().rnnt_engine_workspace_bytes(B, T, U1, H, V, dtype_code(dtype), ctypes.byref(n)))
    return n.value


def _strides3(t):
    return (ctypes.c_int64 * 3)(*t.stride())


def joint_fwd(enc, pred, W, bias):
    """logits[B,T,U1,V] = tanh(enc[:, :, None] + pred[:, None]) @ W.T + bias on the GPU
    (reference rnnt/joint.py:32-39).  `enc` may be a non-contiguous (B,T,H) view."""
    dev = _require_cuda(enc, pred, W, bias)
    _require_dtype(torch.float32, enc=enc, pred=pred, W=W, bias=bias)
    B, T, H = enc.shape
    U1 = pred.shape[1]
    V = W.shape[0]
    pred, W, bias = pred.contiguous(), W.contiguous(), bias.contiguous()
    with torch.cuda.device(dev):
        logits = torch.empty((B, T, U1, V), dtype=torch.float32, device=dev)
        n = ctypes.c_size_t(0)
        _check(lib().rnnt_engine_joint_fwd_workspace_bytes(B, T, U1, H, V, DTYPE_F32, ctypes.byref(n)))
        ws = workspace(dev, n.value)
        _check(lib().rnnt_engine_joint_fwd(_p(enc), _strides3(enc), _p(pred), _p(W), _p(bias), B, T, U1,
                                           H, V, DTYPE_F32, _p(logits), _p(ws),
                                           ctypes.c_size_t(ws.numel()), _stream(dev)))
    return logits


def joint_bwd(enc, pred, W, grad_logits):
    """Backward of joint_fwd on the engine (C ABI rnnt_engine_joint_bwd; autograd of reference
    rnnt/joint.py:32-39): (grad_enc, grad_pred, grad_W, grad_bias) for an upstream gradient
    `grad_logits` [B,T,U1,V]."""
    dev = _require_cuda(enc, pred, W, grad_logits)
    _require_dtype(torch.float32, enc=enc, pred=pred, W=W, grad_logits=grad_logits)
    B, T, H = enc.shape
    U1 = pred.shape[1]
    V = W.shape[0]
    if tuple(grad_logits.shape) != (B, T, U1, V):
        raise RuntimeError("rnnt_amd.joint_bwd: grad_logits must be [B,T,U1,V]")
    pred, W, grad_logits = pred.contiguous(), W.contiguous(), grad_logits.contiguous()
    with torch.cuda.device(dev):
        ge = torch.empty((B, T, H), dtype=torch.float32, device=dev)
        gp = torch.empty((B, U1, H), dtype=torch.float32, device=dev)
        gW = torch.empty((V, H), dtype=torch.float32, device=dev)
        gb = torch.empty(V, dtype=torch.float32, device=dev)
        n = ctypes.c_size_t(0)
        _check(lib().rnnt_engine_joint_bwd_workspace_bytes(B, T, U1, H, V, DTYPE_F32, ctypes.byref(n)))
        ws = workspace(dev, n.value)
        _check(lib().rnnt_engine_joint_bwd(_p(enc), _strides3(enc), _p(pred), _p(W), _p(grad_logits), B, T,
                                           U1, H, V, DTYPE_F32, _p(ge), _p(gp), _p(gW), _p(gb), _p(ws),
                                           ctypes.c_size_t(ws.numel()), _stream(dev)))
    return ge, gp, gW, gb


def check_reg(fastemit_lambda, delay_penalty):
    """FastEmit's lambda and the delay penalty's delta as floats; ValueError unless both are finite and >= 0
    (the C entries answer RNNT_ERR_INVALID_ARG for the same values)."""
    out = []
    for name, v in (("fastemit_lambda", fastemit_lambda), ("delay_penalty", delay_penalty)):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"rnnt_amd: {name} must be a finite number >= 0 (got {v!r})") from None
        if not (math.isfinite(f) and f >= 0.0):
            raise ValueError(f"rnnt_amd: {name} must be finite and >= 0 (got {v!r})")
        out.append(f)
    return tuple(out)


def check_restrict(restrict_frames, restrict_left, restrict_right, B, U, dev=None):
    """The alignment restriction's arguments: frames int32 [B,U], contiguous, on the HIP device (`dev`: the
    other tensors' device); the two buffers as ints >= 0.  No synchronisation: the entries are not read here."""
    for name, v in (("restrict_left", restrict_left), ("restrict_right", restrict_right)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"rnnt_amd: {name} must be an int >= 0 (got {v!r})")
        if not 0 <= v < 2 ** 31:
            raise ValueError(f"rnnt_amd: {name} must be >= 0 and fit a C int (got {v!r})")
    if not isinstance(restrict_frames, torch.Tensor):
        raise RuntimeError("restrict_frames must be a tensor")
    if restrict_frames.dtype != torch.int32:
        raise RuntimeError("restrict_frames must be int32 type")
    if restrict_frames.dim() != 2 or tuple(restrict_frames.shape) != (B, U):
        raise RuntimeError("restrict_frames must have shape [B, U] (max target length), as targets")
    if not restrict_frames.is_contiguous():
        raise RuntimeError("restrict_frames must be contiguous")
    _require_cuda(restrict_frames)
    if dev is not None and restrict_frames.device != dev:
        raise RuntimeError("restrict_frames must be on the device of the other tensors")
    return restrict_left, restrict_right


def loss_fwd_bwd(logits, targets, logit_lens, target_lens, blank, clamp=-1.0, want_grad=True):
    """Per-utterance costs and d(sum costs)/d logits (reference rnnt/model.py:35-41)."""
    return _loss_fwd_bwd(logits, targets, logit_lens, target_lens, blank, clamp, want_grad)


def loss_fwd_bwd_reg(logits, targets, logit_lens, target_lens, blank, clamp, fastemit_lambda, delay_penalty,
                     want_grad=True):
    """loss_fwd_bwd with FastEmit and the delay penalty (C ABI rnnt_engine_loss_fwd_bwd_reg); `clamp`
    applies to the regularised gradient."""
    return _loss_fwd_bwd(logits, targets, logit_lens, target_lens, blank, clamp, want_grad, (fastemit_lambda, delay_penalty))


def loss_fwd_bwd_restrict(logits, targets, logit_lens, target_lens, blank, clamp, fastemit_lambda, delay_penalty,
                          restrict_frames, restrict_left, restrict_right, want_grad=True):
    """loss_fwd_bwd_reg on the lattice restricted to restrict_frames[b,u] - restrict_left <= t <= restrict_frames[b,u] +
    restrict_right for label u (C ABI rnnt_engine_loss_fwd_bwd_restrict)."""
    return _loss_fwd_bwd(logits, targets, logit_lens, target_lens, blank, clamp, want_grad, (fastemit_lambda, delay_penalty),
                         (restrict_frames, restrict_left, restrict_right))


def _check_logits_inputs(logits, targets, logit_lens, target_lens):
    dev = _require_cuda(logits, targets, logit_lens, target_lens)
    _require_dtype(torch.float32, logits=logits)
    _require_dtype(torch.int32, targets=targets, logit_lens=logit_lens, target_lens=target_lens)
    _require_contiguous(logits=logits, targets=targets, logit_lens=logit_lens, target_lens=target_lens)
    return dev


def _call_on_logits(entry, logits, targets, logit_lens, target_lens, blank, mid, outs):
    """One entry on materialised logits [B,T,U1,V] (rnnt_engine_loss_fwd_bwd*, rnnt_engine_align: one workspace serves them all):
    the four input pointers, the dimensions and `blank`, the entry's own arguments `mid`, the output pointers, the workspace."""
    dev = logits.device
    B, T, U1, V = logits.shape
    targets = _nonempty(targets)
    n = ctypes.c_size_t(0)
    _check(lib().rnnt_engine_loss_workspace_bytes(B, T, U1, V, DTYPE_F32, ctypes.byref(n)))
    ws = workspace(dev, n.value)
    _check(getattr(lib(), entry)(_p(logits), _p(targets), _p(logit_lens), _p(target_lens), B, T, U1, V, int(blank), *mid,
                                 *[_p(o) for o in outs], _p(ws), ctypes.c_size_t(ws.numel()), _stream(dev)))


def _loss_fwd_bwd(logits, targets, logit_lens, target_lens, blank, clamp, want_grad, reg=None, restrict=None):
    """The three loss_fwd_bwd* entries: `reg` (fastemit_lambda, delay_penalty) or None, `restrict` (frames, left, right) or None
    (only with `reg`); each optional group is appended where its entry declares it."""
    if restrict is not None:
        B, _, U1, _ = logits.shape
        restrict = (restrict[0],) + check_restrict(*restrict, B, U1 - 1, logits.device)
    if reg is not None:
        reg = check_reg(*reg)
    dev = _check_logits_inputs(logits, targets, logit_lens, target_lens)
    with torch.cuda.device(dev):
        costs = torch.empty(logits.shape[0], dtype=torch.float32, device=dev)
        grad = torch.empty_like(logits) if want_grad else None
        suffix, mid = "", [ctypes.c_float(clamp)]
        if reg is not None:
            suffix = "_reg"
            mid += [ctypes.c_float(reg[0]), ctypes.c_float(reg[1])]
        if restrict is not None:
            suffix = "_restrict"
            frames = _nonempty(restrict[0])
            mid += [_p(frames), restrict[1], restrict[2]]
        _call_on_logits("rnnt_engine_loss_fwd_bwd" + suffix, logits, targets, logit_lens, target_lens, blank, mid + [DTYPE_F32],
                        (costs, grad))
    return costs, grad


def alloc_fused_outputs(enc, pred, W):
    dev = enc.device
    B, T, H = enc.shape
    return (torch.empty(B, dtype=torch.float32, device=dev),
            torch.empty((B, T, H), dtype=torch.float32, device=dev),
            torch.empty(pred.shape, dtype=torch.float32, device=dev),
            torch.empty(W.shape, dtype=torch.float32, device=dev),
            torch.empty(W.shape[0], dtype=torch.float32, device=dev))


def _check_fused_inputs(enc, pred, W, bias, targets, logit_lens, target_lens):
    dev = _require_cuda(enc, pred, W, bias, targets, logit_lens, target_lens)
    _require_dtype(torch.float32, enc=enc, pred=pred, W=W, bias=bias)
    _require_dtype(torch.int32, targets=targets, logit_lens=logit_lens, target_lens=target_lens)
    _require_contiguous(pred=pred, W=W, bias=bias, targets=targets, logit_lens=logit_lens,
                        target_lens=target_lens)
    if enc.dim() != 3 or pred.dim() != 3 or W.dim() != 2 or bias.dim() != 1:
        raise RuntimeError("rnnt_amd: enc [B,T,H], pred [B,U1,H], W [V,H], bias [V] expected")
    B, T, H = enc.shape
    if pred.shape[0] != B or pred.shape[2] != H or W.shape[1] != H or bias.shape[0] != W.shape[0]:
        raise RuntimeError("rnnt_amd: enc / pred / W / bias shape mismatch")
    if logit_lens.shape[0] != B or target_lens.shape[0] != B:
        raise RuntimeError("rnnt_amd: length tensors must have B entries")
    if targets.numel() and tuple(targets.shape) != (B, pred.shape[1] - 1):
        raise RuntimeError("rnnt_amd: targets must be [B, U1-1]")
    return dev


def _frames_out(B, U1, dev):
    """frames [B, U1-1] int32 and the buffer behind it (never empty: U1 == 1 still hands the ABI a valid pointer)."""
    buf = torch.empty(max(B * (U1 - 1), 1), dtype=torch.int32, device=dev)
    return buf[:B * (U1 - 1)].view(B, U1 - 1), buf


def _fused(enc, pred, W, bias, targets, logit_lens, target_lens, blank, dtype, grad_scale=None, reg=None, restrict=None,
           outs=None, stage=None, stage_mask=None, variant=0, align=False):
    """Every fused entry (rnnt_engine_joint_loss_fwd*, rnnt_engine_run_stage[s], rnnt_engine_joint_align): validation, outputs,
    workspace and the argument list, once.  `grad_scale` None: costs only (the forward kernels); `reg` (fastemit_lambda,
    delay_penalty) or None — a costs-only entry takes the delay penalty alone, FastEmit changes no cost; `restrict` (frames, left,
    right) or None (only with `reg`); `stage` / `stage_mask` / `variant` as joint_loss_fwd_bwd's; `align`: the best path instead of
    the loss.  Each optional group is appended where its entry declares it.  Returns the tuple of output tensors."""
    if reg is not None:
        reg = check_reg(*reg)
    dev = _check_fused_inputs(enc, pred, W, bias, targets, logit_lens, target_lens)
    B, T, H = enc.shape
    U1 = pred.shape[1]
    V = W.shape[0]
    if restrict is not None:
        restrict = (restrict[0],) + check_restrict(*restrict, B, U1 - 1, dev)
    targets = _nonempty(targets)
    with torch.cuda.device(dev):
        if align:
            scores = torch.empty(B, dtype=torch.float32, device=dev)
            frames, fbuf = _frames_out(B, U1, dev)
            outs = (scores, fbuf)
        elif grad_scale is None:
            outs = (torch.empty(B, dtype=torch.float32, device=dev),)
        elif outs is None:
            outs = alloc_fused_outputs(enc, pred, W)
        else:
            _require_cuda(enc, *outs)
            _require_dtype(torch.float32, **{f"outs[{i}]": o for i, o in enumerate(outs)})
            _require_contiguous(**{f"outs[{i}]": o for i, o in enumerate(outs)})
        code = dtype_code(dtype)
        need = workspace_bytes(B, T, U1, H, V, code)
        if variant & (VARIANT_X3_FP32_FWD | VARIANT_X3_FP32_DH):
            need += layout(B, T, U1, H, V, code).aux_bytes  # fp32 hidden + W pack of the substituted stages
        ws = workspace(dev, need)
        args = []
        if align:
            entry = "rnnt_engine_joint_align"
        elif stage_mask is not None or variant:
            entry, args = "rnnt_engine_run_stages", [STAGES_ALL if stage_mask is None else int(stage_mask), int(variant)]
        elif stage is not None:
            entry, args = "rnnt_engine_run_stage", [int(stage)]
        else:
            entry = ("rnnt_engine_joint_loss_fwd" + ("_bwd" if grad_scale is not None else "")
                     + ("_restrict" if restrict is not None else "_reg" if reg is not None else ""))
        args += [_p(enc), _strides3(enc), _p(pred), _p(W), _p(bias), _p(targets), _p(logit_lens), _p(target_lens),
                 B, T, U1, H, V, int(blank)]
        if grad_scale is not None:
            args += [ctypes.c_float(-1.0), ctypes.c_float(grad_scale)]  # (clamp: none on the fused path)
        if reg is not None:
            args += [ctypes.c_float(f) for f in (reg if grad_scale is not None else reg[1:])]
        if restrict is not None:
            window = _nonempty(restrict[0])
            args += [_p(window), restrict[1], restrict[2]]
        _check(getattr(lib(), entry)(*args, code, *[_p(o) for o in outs], _p(ws), ctypes.c_size_t(ws.numel()), _stream(dev)))
    return (outs[0], frames) if align else outs


def joint_loss_fwd_bwd(enc, pred, W, bias, targets, logit_lens, target_lens, blank, grad_scale,
                       outs=None, stage=None, *, dtype, stage_mask=None, variant=0):
    """Fused joint + transducer loss forward AND backward (one C-ABI call).  `dtype` is REQUIRED (no default: a caller
    that forgets it must not silently run a route other than the one it means; DEFAULT_DTYPE is what the product ships).
    Returns (costs[B], grad_enc, grad_pred, grad_W, grad_bias); gradients are those of
    grad_scale * sum_b costs[b].  `stage` (0..7) runs a single pipeline stage (bench aid);
    `stage_mask` / `variant` run any subset of stages with per-call kernel variants (VARIANT_*).
    `dtype` "bf16": the three GEMMs take bf16-rounded operands (tensors stay fp32)."""
    return _fused(enc, pred, W, bias, targets, logit_lens, target_lens, blank, dtype, grad_scale, outs=outs, stage=stage,
                  stage_mask=stage_mask, variant=variant)


def joint_loss_fwd_bwd_reg(enc, pred, W, bias, targets, logit_lens, target_lens, blank, grad_scale, fastemit_lambda,
                           delay_penalty, outs=None, *, dtype):
    """joint_loss_fwd_bwd with FastEmit and the delay penalty (C ABI rnnt_engine_joint_loss_fwd_bwd_reg):
    costs are the penalised -log P' (lambda does not change them), gradients those of grad_scale * the regularised loss."""
    return _fused(enc, pred, W, bias, targets, logit_lens, target_lens, blank, dtype, grad_scale, (fastemit_lambda, delay_penalty),
                  outs=outs)


def joint_loss_fwd_bwd_restrict(enc, pred, W, bias, targets, logit_lens, target_lens, blank, grad_scale, fastemit_lambda,
                                delay_penalty, restrict_frames, restrict_left, restrict_right, outs=None, *, dtype):
    """joint_loss_fwd_bwd_reg on the restricted lattice (C ABI rnnt_engine_joint_loss_fwd_bwd_restrict): label u
    of utterance b is emitted only at frames restrict_frames[b,u] - restrict_left .. restrict_frames[b,u] + restrict_right.  An
    utterance without a surviving path has cost +inf and zero gradient contributions."""
    return _fused(enc, pred, W, bias, targets, logit_lens, target_lens, blank, dtype, grad_scale, (fastemit_lambda, delay_penalty),
                  (restrict_frames, restrict_left, restrict_right), outs=outs)


def joint_loss_fwd_restrict(enc, pred, W, bias, targets, logit_lens, target_lens, blank, delay_penalty, restrict_frames,
                            restrict_left, restrict_right, *, dtype):
    """joint_loss_fwd_reg on the restricted lattice (C ABI rnnt_engine_joint_loss_fwd_restrict): costs only, forward kernels only."""
    return _fused(enc, pred, W, bias, targets, logit_lens, target_lens, blank, dtype, None, (0.0, delay_penalty),
                  (restrict_frames, restrict_left, restrict_right))[0]


def joint_loss_fwd_reg(enc, pred, W, bias, targets, logit_lens, target_lens, blank, delay_penalty, *, dtype):
    """joint_loss_fwd with the delay penalty (C ABI rnnt_engine_joint_loss_fwd_reg): the penalised costs, forward kernels
    only (FastEmit changes no cost)."""
    return _fused(enc, pred, W, bias, targets, logit_lens, target_lens, blank, dtype, None, (0.0, delay_penalty))[0]


def joint_loss_fwd(enc, pred, W, bias, targets, logit_lens, target_lens, blank, *, dtype):
    """Costs only (C ABI rnnt_engine_joint_loss_fwd): the fused path's forward — joint GEMM with
    the log-softmax in its epilogue, lattice sweep — and none of the backward kernels or gradient
    buffers.  What RNNTModel.forward costs under torch.no_grad()."""
    return _fused(enc, pred, W, bias, targets, logit_lens, target_lens, blank, dtype)[0]


def align(logits, targets, logit_lens, target_lens, blank):
    """Best alignment on materialised logits [B,T,U1,V] (C ABI rnnt_engine_align): (scores [B] fp32, frames [B,U1-1] int32).
    Workspace: the loss entry's (loss_fwd_bwd's buffer serves both)."""
    dev = _check_logits_inputs(logits, targets, logit_lens, target_lens)
    B, _, U1, _ = logits.shape
    with torch.cuda.device(dev):
        scores = torch.empty(B, dtype=torch.float32, device=dev)
        frames, fbuf = _frames_out(B, U1, dev)
        _call_on_logits("rnnt_engine_align", logits, targets, logit_lens, target_lens, blank, [], (scores, fbuf))
    return scores, frames


def joint_align(enc, pred, W, bias, targets, logit_lens, target_lens, blank, *, dtype):
    """Fused joint + best alignment (C ABI rnnt_engine_joint_align): the joint-forward GEMM of the loss, then the Viterbi sweep
    and the backtrace.  (scores [B] fp32, frames [B,U1-1] int32); workspace: the fused loss entry's."""
    return _fused(enc, pred, W, bias, targets, logit_lens, target_lens, blank, dtype, align=True)


CTC_MAX_U = 1023  # rnnt_engine_ctc_loss_fwd_bwd: two lattice states per lane of a 1024-thread workgroup


def ctc_loss_fwd_bwd(logits, targets, logit_lens, target_lens, blank, cost_weights=None, want_grad=True):
    """CTC loss on logits [N,T,V] (C ABI rnnt_engine_ctc_loss_fwd_bwd): (costs [N] fp32, d sum_n cost_weights[n]
    costs[n] / d logits or None).  targets [N,U] int32, U <= CTC_MAX_U, V % 4 == 0."""
    dev = _check_logits_inputs(logits, targets, logit_lens, target_lens)
    if cost_weights is not None:
        _require_cuda(logits, cost_weights)
        _require_dtype(torch.float32, cost_weights=cost_weights)
        _require_contiguous(cost_weights=cost_weights)
    N, T, V = logits.shape
    U = targets.shape[1]
    targets = _nonempty(targets)
    with torch.cuda.device(dev):
        n = ctypes.c_size_t(0)
        _check(lib().rnnt_engine_ctc_workspace_bytes(N, T, U, V, ctypes.byref(n)))
        ws = workspace(dev, n.value)
        costs = torch.empty(N, dtype=torch.float32, device=dev)
        grad = torch.empty_like(logits) if want_grad else None
        _check(lib().rnnt_engine_ctc_loss_fwd_bwd(_p(logits), _p(targets), _p(logit_lens), _p(target_lens), N, T, U, V, int(blank),
                                                  _p(cost_weights), _p(costs), _p(grad), _p(ws), ctypes.c_size_t(ws.numel()),
                                                  _stream(dev)))
    return costs, grad


def ctc_greedy_decode(logits, logit_lens, blank):
    """CTC greedy decode of logits [N,T,V] (C ABI rnnt_engine_ctc_greedy_decode): (tokens [N,T] int32 whose row n starts with
    utterance n's labels, counts [N] int32).  Enqueues only."""
    dev = _require_cuda(logits, logit_lens)
    _require_dtype(torch.float32, logits=logits)
    _require_dtype(torch.int32, logit_lens=logit_lens)
    _require_contiguous(logits=logits, logit_lens=logit_lens)
    N, T, V = logits.shape
    with torch.cuda.device(dev):
        tokens = torch.empty((N, T), dtype=torch.int32, device=dev)
        counts = torch.empty(N, dtype=torch.int32, device=dev)
        _check(lib().rnnt_engine_ctc_greedy_decode(_p(logits), _p(logit_lens), N, T, V, int(blank), _p(tokens), _p(counts),
                                                   _stream(dev)))
    return tokens, counts


def _rows(x):
    """[.., K] -> a [M, K] view with unit k-stride and a row stride that is a multiple of 4 floats
    (copying when the caller's layout does not allow 16-byte row loads, e.g. the permuted encoder view)."""
    K = x.shape[-1]
    x2 = x.reshape(-1, K) if x.is_contiguous() else x.contiguous().view(-1, K)
    if x2.stride(1) != 1 or x2.stride(0) % 4 != 0 or x2.data_ptr() % 16 != 0:
        x2 = x2.contiguous()
    return x2


# Work (rows x in-features x out-features) from which "auto" runs a projection on the f16x2 pipes (rnnt_engine_linear_x2_*: three GEMMs at ~3x
# the fp32 matrix rate around ~12 small launches, a ~0.26 ms floor for forward + backward).  Measured, forward + backward
# (tools/bench_linear.py, profiles/r05_f_linear_bench.txt; engine f16x2 / library / engine fp32-MFMA): 32 000 x 1024 x 1024: 0.94 / 1.45 / 2.38 ms;
# 12 864 x 1024 x 1024: 0.53 / 0.66 / 0.98; 6 432 x 1024 x 1024: 0.29 / 0.38 / 0.55; 32 000 x 512 x 1024: 0.69 / 0.85 / 1.33;
# 8 000 x 512 x 1024: 0.26 / 0.22 / 0.36; 808 x 1024 x 1024: 0.26 / 0.15 / 0.22 — the crossover with rocBLAS / hipBLASLt lies near 5e9.
LINEAR_X2_MIN_MKN = 5_500_000_000


def linear_x2_preferred(M, K, N):
    """"auto": the f16x2 kernels take the shape (K, N multiples of 128) and the GEMM is large enough for them to beat the library."""
    return K % 128 == 0 and N % 128 == 0 and M * K * N >= LINEAR_X2_MIN_MKN


def _linear_x2(M, K, N, backend):
    if backend == "x2":
        if K % 128 or N % 128:
            raise RuntimeError("rnnt_amd.linear: the f16x2 kernels need K % 128 == 0 and N % 128 == 0")
        return True
    return backend == "auto" and linear_x2_preferred(M, K, N)


def linear_fwd(x, W, bias, backend="auto"):
    """y = x W^T + b (reference rnnt/joint.py:26-30).  backend "x2": rnnt_engine_linear_x2_fwd (f16x2 matrix pipes), "fp32":
    rnnt_engine_linear_fwd (fp32-MFMA small-GEMM kernels), "auto": x2 from LINEAR_X2_MIN_MKN (rows x K x N) when the shape allows it."""
    dev = _require_cuda(x, W, bias)
    _require_dtype(torch.float32, x=x, W=W, bias=bias)
    N, K = W.shape
    if x.shape[-1] != K or bias.shape != (N,):
        raise RuntimeError("rnnt_amd.linear: x [..,K], W [N,K], bias [N] expected")
    x2 = _rows(x)
    M = x2.shape[0]
    W, bias = W.contiguous(), bias.contiguous()
    if _linear_x2(M, K, N, backend):
        with torch.cuda.device(dev):
            y = torch.empty((M, N), dtype=torch.float32, device=dev)
            n = ctypes.c_size_t(0)
            _check(lib().rnnt_engine_linear_x2_workspace_bytes(M, K, N, 0, ctypes.byref(n)))
            ws = workspace(dev, n.value)
            _check(lib().rnnt_engine_linear_x2_fwd(_p(x2), ctypes.c_int64(x2.stride(0)), _p(W), _p(bias), M, K, N, _p(y), _p(ws),
                                                   ctypes.c_size_t(ws.numel()), _stream(dev)))
        return y.view(*x.shape[:-1], N)
    with torch.cuda.device(dev):
        y = torch.empty((M, N), dtype=torch.float32, device=dev)
        _check(lib().rnnt_engine_linear_fwd(_p(x2), ctypes.c_int64(x2.stride(0)), _p(W), _p(bias), M, K, N,
                                            _p(y), _stream(dev)))
    return y.view(*x.shape[:-1], N)


def linear_bwd(x, W, dy, need_dx=True, backend="auto"):
    """(dx, dW, db) of linear_fwd (C ABI rnnt_engine_linear_x2_bwd / rnnt_engine_linear_bwd, chosen as in linear_fwd)."""
    dev = _require_cuda(x, W, dy)
    _require_dtype(torch.float32, x=x, W=W, dy=dy)
    N, K = W.shape
    x2 = _rows(x)
    M = x2.shape[0]
    dy2 = dy.reshape(M, N).contiguous()
    W = W.contiguous()
    with torch.cuda.device(dev):
        dW = torch.empty((N, K), dtype=torch.float32, device=dev)
        db = torch.empty(N, dtype=torch.float32, device=dev)
        dx = torch.empty((M, K), dtype=torch.float32, device=dev) if need_dx else None
        n = ctypes.c_size_t(0)
        if _linear_x2(M, K, N, backend):
            _check(lib().rnnt_engine_linear_x2_workspace_bytes(M, K, N, 1, ctypes.byref(n)))
            ws = workspace(dev, n.value)
            _check(lib().rnnt_engine_linear_x2_bwd(_p(x2), ctypes.c_int64(x2.stride(0)), _p(W), _p(dy2), M, K, N,
                                                   _p(dx), _p(dW), _p(db), _p(ws), ctypes.c_size_t(ws.numel()), _stream(dev)))
            return (dx.view(x.shape) if need_dx else None), dW, db
        _check(lib().rnnt_engine_linear_bwd_workspace_bytes(M, K, N, ctypes.byref(n)))
        ws = workspace(dev, n.value)
        _check(lib().rnnt_engine_linear_bwd(_p(x2), ctypes.c_int64(x2.stride(0)), _p(W), _p(dy2), M, K, N,
                                            _p(dx), _p(dW), _p(db), _p(ws), ctypes.c_size_t(ws.numel()),
                                            _stream(dev)))
    return (dx.view(x.shape) if need_dx else None), dW, db


GREEDY_SCAN_MAX_FRAMES = 128


def greedy_scan(enc, pred, W, bias, t0, nframes, blank):
    """Greedy-decode scan (C ABI rnnt_engine_greedy_scan; reference rnnt/model.py:108-125 inner
    loop): frames t0 .. t0+nframes-1 of `enc` [T,H] (any strides) against ONE predictor state
    `pred` [H].  Returns an int32 device tensor [2+nframes]: first non-blank frame (t0+nframes if
    none), its token, then the argmax of every frame.  No host synchronisation."""
    dev = _require_cuda(enc, pred, W, bias)
    if enc.dim() != 2 or pred.dim() != 1 or enc.shape[1] != pred.shape[0] or W.shape[1] != pred.shape[0]:
        raise RuntimeError("greedy_scan: enc [T,H], pred [H], W [V,H] expected")
    _require_dtype(torch.float32, enc=enc, pred=pred, W=W, bias=bias)
    T, H = enc.shape
    V = W.shape[0]
    nframes = int(nframes)
    if t0 < 0 or nframes < 1 or t0 + nframes > T:
        raise ValueError(f"greedy_scan: frames [{t0}, {t0 + nframes}) outside [0, {T})")
    with torch.cuda.device(dev):
        n = ctypes.c_size_t(0)
        _check(lib().rnnt_engine_greedy_scan_workspace_bytes(nframes, H, V, ctypes.byref(n)))
        ws = workspace(dev, n.value)
        out = torch.empty(2 + nframes, dtype=torch.int32, device=dev)
        _check(lib().rnnt_engine_greedy_scan(_p(enc), ctypes.c_int64(enc.stride(0)), ctypes.c_int64(enc.stride(1)),
                                             _p(pred.contiguous()), _p(W.contiguous()), _p(bias.contiguous()),
                                             int(t0), nframes, H, V, int(blank), _p(out), _p(ws),
                                             ctypes.c_size_t(ws.numel()), _stream(dev)))
    return out


def _eps_pair(ln_eps):
    """`ln_eps` of the decode entry points: one float (both LayerNorms of the ConvPredictor) or (input_layer_norm.eps, output_layer_norm.eps)."""
    if isinstance(ln_eps, (tuple, list)):
        return float(ln_eps[0]), float(ln_eps[1])
    return float(ln_eps), float(ln_eps)


class _PredParams(ctypes.Structure):  # include/rnnt_engine.h: rnnt_conv_predictor_params
    _fields_ = [(n, ctypes.c_void_p) for n in (
        "embedding", "ln_in_w", "ln_in_b", "conv1_w", "conv1_b", "conv2_w", "conv2_b", "linear_w",
        "linear_b", "ln_out_w", "ln_out_b")]


class _DecodeModel:
    """What every decode entry is told about the model, checked once: the tensors (fp32, contiguous, on one HIP device; `frames` [n,H]
    with unit column stride), the sizes, the predictor's struct and the run of arguments the C entries share.  greedy_decode_tables
    has no frames and no joint: it passes `H` instead."""

    def __init__(self, frames, pred_params, ln_eps, text_W, text_b, W=None, bias=None, H=None):
        params = [t.contiguous() for t in pred_params]
        self.dev = _require_cuda(*[t for t in (frames, W, bias) if t is not None], *params)
        _require_dtype(torch.float32, frames=frames, W=W, bias=bias, **{f"param{i}": t for i, t in enumerate(params)})
        if frames is not None and (frames.dim() != 2 or frames.stride(1) != 1):
            frames = frames.contiguous()
        if W is not None:
            W, bias = W.contiguous(), bias.contiguous()
        if text_W is not None:
            _require_cuda(text_W, text_b)
            _require_dtype(torch.float32, text_W=text_W, text_b=text_b)
            text_W, text_b = text_W.contiguous(), text_b.contiguous()
        self.frames, self.params, self.text_W, self.text_b, self.W, self.bias = frames, params, text_W, text_b, W, bias
        self.S, self.E = params[0].shape
        self.O = params[7].shape[0]
        self.H = int(H) if frames is None else frames.shape[1]
        self.V = None if W is None else W.shape[0]
        self.has_text = 1 if text_W is not None else 0
        self.sizes = (self.S, self.E, self.O, self.H, self.V, self.has_text)  # as the *_workspace_bytes queries take them
        self.eps = _eps_pair(ln_eps)
        self.struct = _PredParams(*[t.data_ptr() for t in params])
        self.keep = (frames, params, W, bias, text_W, text_b)  # what a launch reads: alive until the caller has synchronised

    def args(self, blank, max_length, max_per_frame):
        """predictor struct, S, E, O, the two eps, text_ln, joint_ln, H, V, blank, max_length, max_per_frame: in every decode entry."""
        return (ctypes.byref(self.struct), self.S, self.E, self.O, ctypes.c_float(self.eps[0]), ctypes.c_float(self.eps[1]),
                _p(self.text_W), _p(self.text_b), _p(self.W), _p(self.bias), self.H, self.V, int(blank), int(max_length),
                int(max_per_frame))


def _supported(entry, *ints):
    """Whether the size query `entry` takes these sizes: the C ABI's own answer, no device work."""
    n = ctypes.c_size_t(0)
    return getattr(lib(), entry)(*[int(v) for v in ints], ctypes.byref(n)) == 0


def _enqueue_rounds(launch, bound, chunk, in_flight=None, wait_at_limit=False):
    """The decode loops' enqueueing: `launch(it, first, flag)` enqueues `it` <= `chunk` rounds (`first`: 1 on the first call) until the
    device has raised the end flag in a pinned host word (polled, never waited for) or `bound` rounds are enqueued.  `in_flight` None:
    no events; else the host waits for the oldest chunk's completion event once more than `in_flight` chunks are ahead of the device —
    with `wait_at_limit`, once `in_flight` are.  The wait comes before the flag is read again, so a short push ends after the chunk that
    served it.  Returns the flag's tensor (to be kept alive until the caller has synchronised)."""
    flag = torch.zeros(1, dtype=torch.int32).pin_memory()
    flag_p = ctypes.c_void_p(flag.data_ptr())
    limit = None if in_flight is None else max(1, int(in_flight)) + (0 if wait_at_limit else 1)
    pending = []
    done = 0
    while done < bound and (done == 0 or int(flag[0]) == 0):
        it = min(chunk, bound - done)
        launch(it, 1 if done == 0 else 0, flag_p)
        done += it
        if limit is not None:
            ev = torch.cuda.Event()
            ev.record()
            pending.append(ev)
            if len(pending) >= limit:
                pending.pop(0).synchronize()
    return flag


def _pack_rows(frames_list, counts):
    """The entries with frames packed into one [rows, H] tensor, and [(first row, count)] of every entry (None / count 0 included)."""
    live = [f for f, k in zip(frames_list, counts) if k > 0]
    table, at = [], 0
    for k in counts:
        table.append((at, k))
        at += k
    return (live[0] if len(live) == 1 else torch.cat(live, 0)), table


def _rows_table(table, dev):
    """_pack_rows' table on the device: the call's one small host-to-device copy."""
    return torch.tensor(table, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)


# ---- the greedy loops' state words (include/rnnt_engine.h RNNT_DECODE_*): rnnt_engine_greedy_decode, _lstm and _persistent
DECODE_STATE_WORDS = 8
DECODE_T, DECODE_EMITTED, DECODE_NTOK, DECODE_DONE, DECODE_NEWTOK, DECODE_ITERATIONS = 0, 1, 2, 3, 4, 5
DECODE_SETTLED = DECODE_WORKGROUPS = 6  # the LSTM loop's "settled", the persistent loop's workgroup count
DECODE_CODE = 7  # the persistent loop: != 0 = not a decode
DECODE_LABELS = DECODE_STATE_WORDS + 1  # state | tokens read as one list: the labels start after the state words and the leading blank


def greedy_decode_persistent_supported(T, S, E, O, H, V, has_text):
    """Whether rnnt_engine_greedy_decode_persistent takes these sizes (else: greedy_decode_loop's kernel-per-layer chain)."""
    return _supported("rnnt_engine_greedy_decode_persistent_workspace_bytes", T, S, E, O, H, V, bool(has_text))


def greedy_decode_tables(pred_params, ln_eps, text_W, text_b, H):
    """The model's part of the persistent decode's memory (C ABI rnnt_engine_greedy_decode_build_tables): conv2's weight pack, conv1 as
    three tap tables over the symbols, joint.text_ln folded into the predictor's linear layer — a function of the parameters only.  Returns a
    device buffer to pass as `tables=` to greedy_decode_persistent for every utterance decoded with THESE parameter values (build again after
    the weights change); enqueued on the current stream, no synchronisation."""
    m = _DecodeModel(None, pred_params, ln_eps, text_W, text_b, H=H)
    with torch.cuda.device(m.dev):
        n = ctypes.c_size_t(0)
        _check(lib().rnnt_engine_greedy_decode_tables_bytes(m.S, m.E, m.O, m.H, m.has_text, ctypes.byref(n)))
        tables = torch.empty(n.value, dtype=torch.uint8, device=m.dev)
        _check(lib().rnnt_engine_greedy_decode_build_tables(ctypes.byref(m.struct), m.S, m.E, m.O, ctypes.c_float(m.eps[0]), _p(m.text_W),
                                                            _p(m.text_b), m.H, _p(tables), ctypes.c_size_t(n.value), _stream(m.dev)))
        tables._keepalive = (m.params, m.text_W, m.text_b)
    return tables


def greedy_decode_persistent(frames, pred_params, ln_eps, text_W, text_b, W, bias, blank, max_length, max_per_frame=10, tables=None):
    """Device-resident greedy decode of one utterance as ONE persistent launch (C ABI rnnt_engine_greedy_decode_persistent;
    reference rnnt/model.py:108-125 with the stateless ConvPredictor).  Arguments as greedy_decode_loop.  Returns (state int32[8],
    tokens int32[max_length]) device tensors WITHOUT synchronising: after one synchronisation tokens[1 : 1 + state[DECODE_NTOK]] are the
    decoded ids; state[DECODE_CODE] != 0 means the loop gave up on a hand-off (check_decode_state raises).  `tables`: greedy_decode_tables(...) of
    the same parameters (else they are rebuilt inside this call, ~0.13 ms)."""
    m = _DecodeModel(frames, pred_params, ln_eps, text_W, text_b, W, bias)
    T = m.frames.shape[0]
    with torch.cuda.device(m.dev):
        n = ctypes.c_size_t(0)
        _check(lib().rnnt_engine_greedy_decode_persistent_workspace_bytes(T, *m.sizes, ctypes.byref(n)))
        ws = workspace(m.dev, n.value)
        both = torch.empty(DECODE_STATE_WORDS + int(max_length), dtype=torch.int32, device=m.dev)  # state | tokens: ONE device-to-host copy reads the whole result
        state, tokens = both[:DECODE_STATE_WORDS], both[DECODE_STATE_WORDS:]
        _check(lib().rnnt_engine_greedy_decode_persistent(
            _p(m.frames), ctypes.c_int64(m.frames.stride(0)), T, *m.args(blank, max_length, max_per_frame),
            _p(tables), None, _p(state), _p(tokens), _p(ws), ctypes.c_size_t(ws.numel()), _stream(m.dev)))
        state._keepalive = (*m.keep, tables)  # until the caller has synchronised
        state._with_tokens = both
    return state, tokens


DECODE_RANGE_CODES = (10, 11)  # decode.hip DP_CODE_FRAME_RANGE / DP_CODE_TEXT_RANGE


def check_decode_state(state_list):
    """After the synchronisation: raise if the persistent loop did not decode — state[DECODE_CODE]: the hand-off that never arrived, or 10 / 11: an
    audio frame / a text vector with an entry beyond +-30 (or non-finite), where tanh(e + p) = 1 - 2 / (1 + exp 2e exp 2p) is not exact
    (greedy_decode_loop takes tanh of the sum and has no such limit)."""
    code = state_list[DECODE_CODE]
    if code in DECODE_RANGE_CODES:
        raise RuntimeError(f"rnnt_engine: the persistent greedy decode met an {'audio frame' if code == 10 else 'text vector'} "
                           "entry beyond +-30 (or non-finite): use greedy_decode_loop for this utterance")
    if code != 0:
        raise RuntimeError(f"rnnt_engine: the persistent greedy decode gave up waiting for hand-off {code} "
                           f"(iteration {state_list[DECODE_ITERATIONS]}, {state_list[DECODE_WORKGROUPS]} workgroups): are all of its workgroups resident?")


def greedy_decode_loop(frames, pred_params, ln_eps, text_W, text_b, W, bias, blank, max_length,
                       max_per_frame=10, scan_frames=64, chunk=8):
    """Device-resident greedy decode of one utterance (C ABI rnnt_engine_greedy_decode; reference
    rnnt/model.py:108-125 with the stateless ConvPredictor).  `frames` [T,H] fp32 audio frames (after audio_ln),
    `pred_params` the 11 ConvPredictor parameter tensors in rnnt_conv_predictor_params order, `text_W` / `text_b`
    joint.text_ln's parameters or None.  Iterations are enqueued `chunk` at a time until the device has raised the
    end-of-loop flag in a pinned host word (polled, never waited for) or the loop's upper bound is reached.
    Returns (state int32[8], tokens int32[max_length]) device tensors WITHOUT synchronising: after one
    synchronisation tokens[1 : 1 + state[DECODE_NTOK]] are the decoded ids."""
    m = _DecodeModel(frames, pred_params, ln_eps, text_W, text_b, W, bias)
    T = m.frames.shape[0]
    scan_frames, chunk = int(scan_frames), max(1, int(chunk))
    bound = int(max_length) + (T + scan_frames - 1) // scan_frames + 1
    with torch.cuda.device(m.dev):
        n = ctypes.c_size_t(0)
        _check(lib().rnnt_engine_greedy_decode_workspace_bytes(m.H, m.V, m.E, m.O, scan_frames, ctypes.byref(n)))
        ws = workspace(m.dev, n.value)
        state = torch.empty(DECODE_STATE_WORDS, dtype=torch.int32, device=m.dev)
        tokens = torch.empty(int(max_length), dtype=torch.int32, device=m.dev)
        head = (_p(m.frames), ctypes.c_int64(m.frames.stride(0)), T, *m.args(blank, max_length, max_per_frame), scan_frames)
        tail = (_p(state), _p(tokens), _p(ws), ctypes.c_size_t(ws.numel()), _stream(m.dev))
        flag = _enqueue_rounds(lambda it, first, flag: _check(lib().rnnt_engine_greedy_decode(*head, it, first, flag, *tail)),
                               bound, chunk)
        state._keepalive = (flag, *m.keep)  # until the caller has synchronised
    return state, tokens


# ---- greedy decode with the LSTMPredictor, n_utt utterances in lockstep (DESIGN.md §4p "Device decode")
LSTM_DECODE_MAX = 32  # rnnt_engine_greedy_decode_lstm: 1 <= n_utt <= 32, the rows of one tile of every product


def greedy_decode_lstm_supported(n_utt, S, E, Hd, O, L, layer_norm, H, V, has_text, scan_frames=32):
    """Whether rnnt_engine_greedy_decode_lstm takes these sizes (no device work)."""
    return _supported("rnnt_engine_greedy_decode_lstm_workspace_bytes", n_utt, S, E, Hd, O, L, bool(layer_norm), H, V, bool(has_text),
                      scan_frames)


def greedy_decode_lstm(frames_list, lstm_params, text_W, text_b, W, bias, blank, max_length, max_per_frame=10, scan_frames=32, chunk=8,
                       want_state=True):
    """Device-resident greedy decode of 1 .. 32 utterances of one LSTMPredictor model, advanced in lockstep (C ABI
    rnnt_engine_greedy_decode_lstm; reference rnnt/model.py:45-87).  `frames_list`: [T_u, H] fp32 frame tensors (audio_ln applied), packed
    here into one buffer; the table of first rows and lengths is the call's one small host-to-device copy.  `lstm_params`:
    LSTMPredictor._decode_bundle() = (the parameter tensors in rnnt_lstm_predictor_params order, (L, Hd, layer_norm), the three eps).
    The other arguments and the enqueueing (chunks of iterations until the device raises the pinned end flag — when ALL utterances have
    ended) as greedy_decode_loop.  Returns (state int32[N, 8], tokens int32[N, max_length], state_out float32[L, 2, N, Hd] or None, text
    float32[N, H]: the joint's text input after each utterance's last label, a view of the stream's workspace valid until the next engine
    call on it) device tensors WITHOUT synchronising: afterwards tokens[u, 1 : 1 + state[u, DECODE_NTOK]] are utterance u's ids, bit for bit
    what it gives decoded alone."""
    from .lstm_predictor import _struct
    frames_list = list(frames_list)
    lens = [int(f.shape[0]) for f in frames_list]
    if not lens or min(lens) < 1:
        raise ValueError("greedy_decode_lstm: no utterance, or an utterance without frames")
    params, (L, Hd, layer_norm), eps = lstm_params
    params = [t.contiguous() for t in params]
    packed, table = _pack_rows(frames_list, lens)
    if packed.dim() != 2 or packed.stride(1) != 1:
        packed = packed.contiguous()
    joint = [t.contiguous() for t in (W, bias)] + ([text_W.contiguous(), text_b.contiguous()] if text_W is not None else [])
    dev = _require_cuda(packed, *joint, *params)
    _require_dtype(torch.float32, frames=packed, **{f"joint{i}": t for i, t in enumerate(joint)}, **{f"param{i}": t for i, t in enumerate(params)})
    N, H, V = len(lens), packed.shape[1], joint[0].shape[0]
    S, E = params[0].shape
    O = params[3].shape[0]
    max_length, scan_frames, chunk = int(max_length), int(scan_frames), max(1, int(chunk))
    bound = max_length + (max(lens) + scan_frames - 1) // max(1, scan_frames) + 1
    with torch.cuda.device(dev):
        n = ctypes.c_size_t(0)
        _check(lib().rnnt_engine_greedy_decode_lstm_workspace_bytes(N, S, E, Hd, O, L, int(bool(layer_norm)), H, V, int(len(joint) == 4),
                                                                    scan_frames, ctypes.byref(n)))
        ws = workspace(dev, n.value)
        utt = _rows_table(table, dev)
        state = torch.empty(N, DECODE_STATE_WORDS, dtype=torch.int32, device=dev)  # (a single row's stride is whatever torch says: the row is contiguous)
        tokens = torch.empty(N, max_length, dtype=torch.int32, device=dev)
        state_out = torch.empty(L, 2, N, Hd, dtype=torch.float32, device=dev) if want_state else None
        st, arr = _struct(params, L, layer_norm)
        head = (_p(packed), ctypes.c_int64(packed.stride(0) if packed.shape[0] > 1 else H), packed.shape[0], _p(utt), N, max(lens),
                ctypes.byref(st), S, E, Hd, O, L,
                int(bool(layer_norm)), *[ctypes.c_float(e) for e in eps], _p(joint[2]) if len(joint) == 4 else None,
                _p(joint[3]) if len(joint) == 4 else None, _p(joint[0]), _p(joint[1]), H, V, int(blank), max_length, int(max_per_frame),
                scan_frames)
        tail = (_p(state), _p(tokens), _p(state_out), _p(ws), ctypes.c_size_t(ws.numel()), _stream(dev))
        flag = _enqueue_rounds(lambda it, first, flag: _check(lib().rnnt_engine_greedy_decode_lstm(*head, it, first, flag, *tail)),
                               bound, chunk)
        state._keepalive = (flag, utt, packed, params, joint, arr)  # until the caller has synchronised
        text = ws[:N * H * 4].view(torch.float32).view(N, H)
    return state, tokens, state_out, text


# ---- streaming greedy decode with the LSTMPredictor, 1 .. 32 streams in lockstep (include/rnnt_engine.h RNNT_LSTM_STREAM_*; DESIGN.md §4p
# "Device stream")
LSTM_STREAM_MAX = 32  # rnnt_engine_greedy_stream_lstm_*: 1 <= n_streams <= 32
LSTM_STREAM_STATE_WORDS = 16
(LSTM_STREAM_T, LSTM_STREAM_EMITTED, LSTM_STREAM_LABELS, LSTM_STREAM_PAUSED, LSTM_STREAM_NEWTOK, LSTM_STREAM_PUSH_ITERATIONS,
 LSTM_STREAM_AT_REST, LSTM_STREAM_DONE, LSTM_STREAM_FRAMES, LSTM_STREAM_NEWEST, LSTM_STREAM_PUSH_LABELS, LSTM_STREAM_BASE) = range(12)


def greedy_stream_lstm_bytes(n_streams, S, E, Hd, O, L, layer_norm, H, V, has_text):
    """Bytes of the persistent block of `n_streams` LSTM greedy streams (C ABI rnnt_engine_greedy_stream_lstm_bytes; no device work)."""
    n = ctypes.c_size_t(0)
    _check(lib().rnnt_engine_greedy_stream_lstm_bytes(int(n_streams), int(S), int(E), int(Hd), int(O), int(L), int(bool(layer_norm)), int(H),
                                                      int(V), int(bool(has_text)), ctypes.byref(n)))
    return n.value


def greedy_stream_lstm_supported(n_streams, S, E, Hd, O, L, layer_norm, H, V, has_text, scan_frames=32):
    """Whether rnnt_engine_greedy_stream_lstm_push takes these sizes (no device work)."""
    return _supported("rnnt_engine_greedy_stream_lstm_push_workspace_bytes", n_streams, S, E, Hd, O, L, bool(layer_norm), H, V, bool(has_text),
                      scan_frames)


def greedy_stream_lstm_views(block, n_streams, L, Hd, H):
    """The three sections of a group's block (uint8, as greedy_stream_lstm_bytes sized it) as views: state int32[n, 16], the LSTM state
    float32[L, 2, n, Hd] and the text vectors float32[n, H] — each section a multiple of 256 bytes."""
    n = int(n_streams)
    cuts, at = [], 0
    for nbytes in (4 * n * LSTM_STREAM_STATE_WORDS, 4 * L * 2 * n * Hd, 4 * n * H):
        cuts.append((at, at + nbytes))
        at += (nbytes + 255) & ~255
    (a0, a1), (b0, b1), (c0, c1) = cuts
    return (block[a0:a1].view(torch.int32).view(n, LSTM_STREAM_STATE_WORDS), block[b0:b1].view(torch.float32).view(L, 2, n, Hd),
            block[c0:c1].view(torch.float32).view(n, H))


def greedy_stream_lstm_init(block, n_streams, L, Hd, H, blank, index=None):
    """Start every stream of a group (index None) or stream `index` alone (C ABI rnnt_engine_greedy_stream_lstm_init): `block`
    uint8[greedy_stream_lstm_bytes(...)] on the device.  Enqueued on the current stream, no synchronisation."""
    dev = _require_cuda(block)
    _require_dtype(torch.uint8, block=block)
    _require_contiguous(block=block)
    with torch.cuda.device(dev):
        _check(lib().rnnt_engine_greedy_stream_lstm_init(int(n_streams), int(Hd), int(L), int(H), int(blank), -1 if index is None else int(index),
                                                         _p(block), ctypes.c_size_t(block.numel()), _stream(dev)))


def greedy_stream_lstm_push(frames_list, lstm_params, text_W, text_b, W, bias, blank, max_length, max_per_frame, scan_frames, block,
                            out_tokens, chunk=8, in_flight=2):
    """Enqueue one push of a group of LSTM greedy streams (C ABI rnnt_engine_greedy_stream_lstm_push; DESIGN.md §4p "Device stream"):
    `frames_list` holds one entry per stream, a [k_u, H] fp32 frame tensor (audio_ln applied) or None / k_u = 0 for a stream that sits
    the push out; they are packed here and the table of first rows and counts is the push's one small host-to-device copy.
    `lstm_params` as greedy_decode_lstm's, `max_length` 0 = unbounded, `block` the group's persistent block (greedy_stream_lstm_init),
    `out_tokens` int32[n, stride] with stride >= the largest count * max_per_frame.  Iterations are enqueued in chunks until the device
    has raised the pinned flag (all streams at rest; polled, never waited for): chunks of `chunk` iterations, fewer for a push of few
    frames, at most `in_flight` of them ahead of the device.  No synchronisation: afterwards, with state = greedy_stream_lstm_views(block,
    ...)[0], out_tokens[u, :state[u, LSTM_STREAM_PUSH_LABELS]] are the labels this push gave stream u (if it got frames and was not done)
    and state[u, LSTM_STREAM_FRAMES] its frames consumed.  A push without any frame enqueues nothing."""
    from .lstm_predictor import _struct
    n = int(out_tokens.shape[0])
    frames_list = list(frames_list)
    if len(frames_list) != n:
        raise ValueError(f"greedy_stream_lstm_push: {len(frames_list)} entries for {n} streams")
    counts = [0 if f is None else int(f.shape[0]) for f in frames_list]
    if not any(counts):
        return
    max_count = max(counts)
    params, (L, Hd, layer_norm), eps = lstm_params
    params = [t.contiguous() for t in params]
    packed, rows = _pack_rows(frames_list, counts)
    if packed.dim() != 2 or packed.stride(1) != 1:
        packed = packed.contiguous()
    joint = [t.contiguous() for t in (W, bias)] + ([text_W.contiguous(), text_b.contiguous()] if text_W is not None else [])
    dev = _require_cuda(packed, block, out_tokens, *joint, *params)
    _require_dtype(torch.float32, frames=packed, **{f"joint{i}": t for i, t in enumerate(joint)}, **{f"param{i}": t for i, t in enumerate(params)})
    _require_dtype(torch.int32, out_tokens=out_tokens)
    _require_dtype(torch.uint8, block=block)
    _require_contiguous(block=block, out_tokens=out_tokens)
    H, V = packed.shape[1], joint[0].shape[0]
    S, E = params[0].shape
    O = params[3].shape[0]
    max_length, max_per_frame, scan_frames = int(max_length), int(max_per_frame), int(scan_frames)
    bound = max_count * max(1, max_per_frame) + (max_count + scan_frames - 1) // max(1, scan_frames) + 1
    with torch.cuda.device(dev):
        nb = ctypes.c_size_t(0)
        _check(lib().rnnt_engine_greedy_stream_lstm_push_workspace_bytes(n, S, E, Hd, O, L, int(bool(layer_norm)), H, V, int(len(joint) == 4),
                                                                         scan_frames, ctypes.byref(nb)))
        ws = workspace(dev, nb.value)
        table = _rows_table(rows, dev)
        st, arr = _struct(params, L, layer_norm)
        head = (_p(packed), ctypes.c_int64(packed.stride(0) if packed.shape[0] > 1 else H), packed.shape[0], _p(table), n, max_count,
                ctypes.byref(st), S, E, Hd, O, L, int(bool(layer_norm)), *[ctypes.c_float(e) for e in eps],
                _p(joint[2]) if len(joint) == 4 else None, _p(joint[3]) if len(joint) == 4 else None, _p(joint[0]), _p(joint[1]), H, V,
                int(blank), max_length, max_per_frame, scan_frames)
        tail = (_p(out_tokens), int(out_tokens.shape[1]), _p(block), ctypes.c_size_t(block.numel()), _p(ws), ctypes.c_size_t(ws.numel()),
                _stream(dev))
        # chunks sized to the push (a 1-frame push needs one iteration, two if it emits a label), and the wait as soon as `in_flight`
        # chunks are out, before the flag is read again: a short push ends after the chunk that served it
        flag = _enqueue_rounds(lambda it, first, flag: _check(lib().rnnt_engine_greedy_stream_lstm_push(*head, it, first, flag, *tail)),
                               bound, min(max(1, int(chunk)), 2 * max_count + 1), in_flight, wait_at_limit=True)
        out_tokens._keepalive = (flag, table, packed, params, joint, arr)  # until the caller has synchronised


# ---- streaming greedy decode (include/rnnt_engine.h RNNT_STREAM_*)
STREAM_STATE_WORDS = 16
STREAM_FRAMES, STREAM_EMITTED, STREAM_LABELS, STREAM_DONE, STREAM_TOKENS = 0, 1, 2, 3, 4
STREAM_PUSH_LABELS, STREAM_PUSH_ITERATIONS, STREAM_STATUS = 11, 12, 13


def greedy_stream_init(state, blank):
    """Write the initial stream state into `state` (int32 device tensor of >= STREAM_STATE_WORDS entries) on the current stream."""
    dev = _require_cuda(state)
    _require_dtype(torch.int32, state=state)
    if state.numel() < STREAM_STATE_WORDS or not state.is_contiguous():
        raise RuntimeError(f"greedy_stream_init: a contiguous int32 block of {STREAM_STATE_WORDS} words expected")
    with torch.cuda.device(dev):
        _check(lib().rnnt_engine_greedy_stream_init(_p(state), int(blank), _stream(dev)))


def greedy_stream_supported(n, S, E, O, H, V, has_text, max_length, max_per_frame):
    """Whether a push of n frames can take the persistent launch (rnnt_engine_greedy_stream_decode with persistent = 1); no device work.
    max_length 0 or None: unbounded."""
    return _supported("rnnt_engine_greedy_stream_decode_workspace_bytes", n, S, E, O, H, V, bool(has_text), max_length or 0,
                      max_per_frame, 1)


def greedy_stream_decode(frames, pred_params, ln_eps, text_W, text_b, W, bias, blank, max_length, max_per_frame, tables, persistent,
                         state, out_tokens):
    """Enqueue one push of a stream (C ABI rnnt_engine_greedy_stream_decode): `frames` [n, H] fp32 (audio_ln applied), `state` the
    stream's int32 block (greedy_stream_init), `out_tokens` int32 with room for the push's labels (n * max_per_frame, or fewer when
    max_length leaves fewer); max_length 0 / None = unbounded.  No synchronisation: afterwards state[STREAM_STATUS] == 0 means the push
    decoded and out_tokens[:state[STREAM_PUSH_LABELS]] are its labels; non-zero (persistent only) means nothing changed — redo the push
    with persistent=False."""
    m = _DecodeModel(frames, pred_params, ln_eps, text_W, text_b, W, bias)
    _require_cuda(m.frames, state, out_tokens)
    _require_dtype(torch.int32, state=state, out_tokens=out_tokens)
    _require_contiguous(state=state, out_tokens=out_tokens)
    n = m.frames.shape[0]
    ml, mpf, persistent = int(max_length or 0), int(max_per_frame), 1 if persistent else 0
    cap = n * mpf if ml == 0 else min(n * mpf, ml - 1)
    if state.numel() < STREAM_STATE_WORDS or out_tokens.numel() < cap:
        raise RuntimeError(f"greedy_stream_decode: state needs {STREAM_STATE_WORDS} words, out_tokens {cap} (got {state.numel()}, {out_tokens.numel()})")
    with torch.cuda.device(m.dev):
        q = ctypes.c_size_t(0)
        _check(lib().rnnt_engine_greedy_stream_decode_workspace_bytes(n, *m.sizes, ml, mpf, persistent, ctypes.byref(q)))
        ws = workspace(m.dev, q.value)
        _check(lib().rnnt_engine_greedy_stream_decode(
            _p(m.frames) if n > 0 else None, ctypes.c_int64(m.frames.stride(0)), n, *m.args(blank, ml, mpf), _p(tables), persistent,
            _p(state), _p(out_tokens), _p(ws), ctypes.c_size_t(ws.numel()), _stream(m.dev)))
        state._keepalive = (*m.keep, tables)  # until the caller has synchronised


BEAM_MAX = 16  # rnnt_engine_beam_decode: 1 <= beam <= 16 (the slots are the M = 16 rows of every product)
BEAM_CONTEXT_MAX_NODES = 65536  # include/rnnt_engine.h RNNT_BEAM_CONTEXT_MAX_NODES


class _BeamContext(ctypes.Structure):  # include/rnnt_engine.h: rnnt_beam_context
    _fields_ = [("n_nodes", ctypes.c_int32), ("n_children", ctypes.c_int32), ("score", ctypes.c_double)] + [
        (n, ctypes.c_void_p) for n in ("child_off", "child_tok", "child_node", "fail_link", "depth", "terminal")]


def _beam_context(context, dev):
    """`context` (None, or the dict of ContextGraph.device_tables: int32 tensors on the search's device and n_nodes, n_children, score)
    -> (the rnnt_beam_context to pass, the tensors to keep alive)."""
    if context is None:
        return None, ()
    arrays = [context[n] for n in ("child_off", "child_tok", "child_node", "fail_link", "depth", "terminal")]
    n_nodes, n_children = int(context["n_nodes"]), int(context["n_children"])
    for name, t, need in zip(("child_off", "child_tok", "child_node", "fail_link", "depth", "terminal"), arrays,
                             (n_nodes + 1, n_children, n_children, n_nodes, n_nodes, n_nodes)):
        if t.dtype != torch.int32 or t.device != dev or not t.is_contiguous() or t.numel() < max(need, 1):
            raise RuntimeError(f"beam context: {name} must be a contiguous int32 tensor of >= {max(need, 1)} entries on {dev}")
    return _BeamContext(n_nodes, n_children, float(context["score"]), *[t.data_ptr() for t in arrays]), tuple(arrays)


def beam_decode_supported(S, E, O, H, V, has_text, max_length, beam):
    """Whether rnnt_engine_beam_decode takes these sizes (no device work)."""
    return _supported("rnnt_engine_beam_decode_workspace_bytes", S, E, O, H, V, bool(has_text), max_length, beam)


def beam_decode(frames, pred_params, ln_eps, text_W, text_b, W, bias, blank, max_length, beam, max_per_frame=10, tables=None,
                chunk=32, in_flight=2, context=None):
    """Frame-synchronous beam search of one utterance on the device (C ABI rnnt_engine_beam_decode).  Arguments as
    greedy_decode_loop, plus `beam` (1 .. 16) and `tables` (greedy_decode_tables(...) of the same parameters, or None: rebuilt inside).
    Rounds are enqueued `chunk` at a time until the device has raised the end flag in a pinned host word (polled, never waited for);
    at most `in_flight` chunks are ahead of the device (the host waits for the oldest one's completion event), so the rounds enqueued
    after the end stay few.  Returns (state int32[32], tokens int32[beam, max_length], scores float64[beam]) device tensors WITHOUT a
    final synchronisation: afterwards entry j < state[2] is tokens[j, 1 : 1 + state[8 + j]] with log-probability scores[j], best first.
    `context` (ContextGraph.device_tables(device)): the search biased by a phrase list (C ABI rnnt_engine_beam_decode_ctx; DESIGN.md §4h
    "Context") — the scores are then INTERNAL and the order is theirs: the caller finalises (ContextGraph.finalise)."""
    m = _DecodeModel(frames, pred_params, ln_eps, text_W, text_b, W, bias)
    T = m.frames.shape[0]
    beam, max_length, max_per_frame = int(beam), int(max_length), int(max_per_frame)
    with torch.cuda.device(m.dev):
        n = ctypes.c_size_t(0)
        cx, cx_keep = _beam_context(context, m.dev)
        cx_arg = () if cx is None else (ctypes.byref(cx),)  # the _ctx entries take it before the stream
        query = lib().rnnt_engine_beam_decode_workspace_bytes if cx is None else lib().rnnt_engine_beam_decode_ctx_workspace_bytes
        _check(query(*m.sizes, max_length, beam, ctypes.byref(n)))
        ws = workspace(m.dev, n.value)
        state = torch.empty(32, dtype=torch.int32, device=m.dev)
        tokens = torch.empty(beam, max_length, dtype=torch.int32, device=m.dev)
        scores = torch.empty(beam, dtype=torch.float64, device=m.dev)
        fn = lib().rnnt_engine_beam_decode if cx is None else lib().rnnt_engine_beam_decode_ctx
        head = (_p(m.frames), ctypes.c_int64(m.frames.stride(0)), T, *m.args(blank, max_length, max_per_frame), beam, _p(tables))
        tail = (_p(state), _p(tokens), _p(scores), _p(ws), ctypes.c_size_t(ws.numel()), *cx_arg, _stream(m.dev))
        flag = _enqueue_rounds(lambda it, first, flag: _check(fn(*head, it, first, flag, *tail)),
                               T * max(1, max_per_frame) + 1, max(1, int(chunk)), in_flight)
        state._keepalive = (flag, *m.keep, tables, cx_keep)  # until the caller has synchronised
    return state, tokens, scores


BEAM_BATCH_MAX = 64  # rnnt_engine_beam_decode_batch: 1 <= n_utt <= 64


def beam_decode_batch_supported(S, E, O, H, V, has_text, max_length, beam, n_utt):
    """Whether rnnt_engine_beam_decode_batch takes these sizes (no device work)."""
    return _supported("rnnt_engine_beam_decode_batch_workspace_bytes", S, E, O, H, V, bool(has_text), max_length, beam, n_utt)


def beam_decode_batch(frames_list, pred_params, ln_eps, text_W, text_b, W, bias, blank, max_length, beam, max_per_frame=10, tables=None,
                      chunk=32, in_flight=2, context=None):
    """The beam search of beam_decode for SEVERAL utterances of one model, advanced in lockstep on the device (C ABI
    rnnt_engine_beam_decode_batch; DESIGN.md §4h "Batched"): `frames_list` holds 1 .. 64 [T_u, H] fp32 frame tensors (audio_ln applied),
    packed here into one buffer; the table of first rows and lengths is the call's one small host-to-device copy.  The other arguments
    and the enqueueing (chunks of rounds, the pinned end flag — raised when ALL searches have ended —, `in_flight`) as beam_decode.
    Returns (state int32[N, 32], tokens int32[N, beam, max_length], scores float64[N, beam]) device tensors WITHOUT a final
    synchronisation; row u of each is what beam_decode returns for frames_list[u] alone, bit for bit.  `context` as beam_decode's: ONE
    graph biases every utterance of the batch (C ABI rnnt_engine_beam_decode_batch_ctx)."""
    frames_list = list(frames_list)
    if not frames_list:
        raise ValueError("beam_decode_batch: no utterance")
    lens = [int(f.shape[0]) for f in frames_list]
    if min(lens) < 1:
        raise ValueError("beam_decode_batch: an utterance without frames")
    packed, table = _pack_rows(frames_list, lens)
    m = _DecodeModel(packed, pred_params, ln_eps, text_W, text_b, W, bias)
    N = len(lens)
    beam, max_length, max_per_frame = int(beam), int(max_length), int(max_per_frame)
    with torch.cuda.device(m.dev):
        n = ctypes.c_size_t(0)
        cx, cx_keep = _beam_context(context, m.dev)
        cx_arg = () if cx is None else (ctypes.byref(cx),)  # the _ctx entries take it before the stream
        query = lib().rnnt_engine_beam_decode_batch_workspace_bytes if cx is None else lib().rnnt_engine_beam_decode_batch_ctx_workspace_bytes
        _check(query(*m.sizes, max_length, beam, N, ctypes.byref(n)))
        ws = workspace(m.dev, n.value)
        utt = _rows_table(table, m.dev)
        state = torch.empty(N, 32, dtype=torch.int32, device=m.dev)
        tokens = torch.empty(N, beam, max_length, dtype=torch.int32, device=m.dev)
        scores = torch.empty(N, beam, dtype=torch.float64, device=m.dev)
        fn = lib().rnnt_engine_beam_decode_batch if cx is None else lib().rnnt_engine_beam_decode_batch_ctx
        head = (_p(m.frames), ctypes.c_int64(m.frames.stride(0)), m.frames.shape[0], _p(utt), N, max(lens),
                *m.args(blank, max_length, max_per_frame), beam, _p(tables))
        tail = (_p(state), _p(tokens), _p(scores), _p(ws), ctypes.c_size_t(ws.numel()), *cx_arg, _stream(m.dev))
        flag = _enqueue_rounds(lambda it, first, flag: _check(fn(*head, it, first, flag, *tail)),
                               max(lens) * max(1, max_per_frame) + 1, max(1, int(chunk)), in_flight)
        state._keepalive = (flag, utt, *m.keep, tables, cx_keep)  # until the caller has synchronised
    return state, tokens, scores


# ---- beam search with the LSTMPredictor, n_utt utterances in lockstep (DESIGN.md §4h "LSTM")
BEAM_LSTM_MAX = 32  # rnnt_engine_beam_decode_lstm: 1 <= n_utt <= 32 (16 slots each: two utterances to a 32-row tile)


def beam_decode_lstm_supported(n_utt, S, E, Hd, O, L, layer_norm, H, V, has_text, max_length, beam):
    """Whether rnnt_engine_beam_decode_lstm takes these sizes (no device work)."""
    return _supported("rnnt_engine_beam_decode_lstm_workspace_bytes", n_utt, S, E, Hd, O, L, bool(layer_norm), H, V, bool(has_text),
                      max_length, beam)


def beam_decode_lstm(frames_list, lstm_params, text_W, text_b, W, bias, blank, max_length, beam, max_per_frame=10, chunk=32, in_flight=2):
    """The beam search of beam_decode_batch for 1 .. 32 utterances of one LSTMPredictor model (C ABI rnnt_engine_beam_decode_lstm;
    DESIGN.md §4h "LSTM").  `frames_list` and the enqueueing as beam_decode_batch's, `lstm_params` = LSTMPredictor._decode_bundle() as
    greedy_decode_lstm's.  Returns (state int32[N, 32], tokens int32[N, beam, max_length], scores float64[N, beam]) device tensors WITHOUT
    a final synchronisation; row u of each is, bit for bit, what the call gives for frames_list[u] alone."""
    from .lstm_predictor import _struct
    frames_list = list(frames_list)
    lens = [int(f.shape[0]) for f in frames_list]
    if not lens or min(lens) < 1:
        raise ValueError("beam_decode_lstm: no utterance, or an utterance without frames")
    params, (L, Hd, layer_norm), eps = lstm_params
    params = [t.contiguous() for t in params]
    packed, table = _pack_rows(frames_list, lens)
    if packed.dim() != 2 or packed.stride(1) != 1:
        packed = packed.contiguous()
    joint = [t.contiguous() for t in (W, bias)] + ([text_W.contiguous(), text_b.contiguous()] if text_W is not None else [])
    dev = _require_cuda(packed, *joint, *params)
    _require_dtype(torch.float32, frames=packed, **{f"joint{i}": t for i, t in enumerate(joint)}, **{f"param{i}": t for i, t in enumerate(params)})
    N, H, V = len(lens), packed.shape[1], joint[0].shape[0]
    S, E = params[0].shape
    O = params[3].shape[0]
    beam, max_length, max_per_frame = int(beam), int(max_length), int(max_per_frame)
    with torch.cuda.device(dev):
        n = ctypes.c_size_t(0)
        _check(lib().rnnt_engine_beam_decode_lstm_workspace_bytes(N, S, E, Hd, O, L, int(bool(layer_norm)), H, V, int(len(joint) == 4),
                                                                  max_length, beam, ctypes.byref(n)))
        ws = workspace(dev, n.value)
        utt = _rows_table(table, dev)
        state = torch.empty(N, 32, dtype=torch.int32, device=dev)
        tokens = torch.empty(N, beam, max_length, dtype=torch.int32, device=dev)
        scores = torch.empty(N, beam, dtype=torch.float64, device=dev)
        st, arr = _struct(params, L, layer_norm)
        head = (_p(packed), ctypes.c_int64(packed.stride(0) if packed.shape[0] > 1 else H), packed.shape[0], _p(utt), N, max(lens),
                ctypes.byref(st), S, E, Hd, O, L,
                int(bool(layer_norm)), *[ctypes.c_float(e) for e in eps], _p(joint[2]) if len(joint) == 4 else None,
                _p(joint[3]) if len(joint) == 4 else None, _p(joint[0]), _p(joint[1]), H, V, int(blank), max_length, max_per_frame, beam)
        tail = (_p(state), _p(tokens), _p(scores), _p(ws), ctypes.c_size_t(ws.numel()), _stream(dev))
        flag = _enqueue_rounds(lambda it, first, flag: _check(lib().rnnt_engine_beam_decode_lstm(*head, it, first, flag, *tail)),
                               max(lens) * max(1, max_per_frame) + 1, max(1, int(chunk)), in_flight)
        state._keepalive = (flag, utt, packed, params, joint, arr)  # until the caller has synchronised
    return state, tokens, scores


# ---- streaming beam search (include/rnnt_engine.h RNNT_BEAM_STREAM_*)
BEAM_STREAM_MAX = 64  # rnnt_engine_beam_stream_*: 1 <= n_streams <= 64
BEAM_STREAM_FRAMES, BEAM_STREAM_AT_REST, BEAM_STREAM_BASE = 0, 24, 25


def beam_stream_bytes(S, E, O, H, V, has_text, max_length, beam, n_streams):
    """Bytes of the persistent block of `n_streams` beam streams (C ABI rnnt_engine_beam_stream_bytes; no device work)."""
    n = ctypes.c_size_t(0)
    _check(lib().rnnt_engine_beam_stream_bytes(int(S), int(E), int(O), int(H), int(V), int(bool(has_text)), int(max_length), int(beam),
                                               int(n_streams), ctypes.byref(n)))
    return n.value


def beam_stream_supported(S, E, O, H, V, has_text, max_length, beam, n_streams=1):
    """Whether rnnt_engine_beam_stream_push takes these sizes (no device work)."""
    return _supported("rnnt_engine_beam_stream_bytes", S, E, O, H, V, bool(has_text), max_length, beam, n_streams)


def beam_stream_init(sizes, max_length, beam, blank, state, scores, block, index=None):
    """Start every stream of a group (index None) or stream `index` alone (C ABI rnnt_engine_beam_stream_init): `sizes` =
    (S, E, O, H, V, has_text), `state` int32[n, 32], `scores` float64[n, beam], `block` uint8[beam_stream_bytes(...)], all on one
    device.  Enqueued on the current stream, no synchronisation."""
    dev = _require_cuda(state, scores, block)
    _require_dtype(torch.int32, state=state)
    _require_dtype(torch.float64, scores=scores)
    _require_dtype(torch.uint8, block=block)
    _require_contiguous(state=state, scores=scores, block=block)
    S, E, O, H, V, has_text = sizes
    n, beam = int(state.shape[0]), int(beam)
    if state.shape != (n, 32) or scores.shape != (n, beam):
        raise RuntimeError(f"beam_stream_init: state [n, 32] and scores [n, {beam}] expected, got {tuple(state.shape)}, {tuple(scores.shape)}")
    with torch.cuda.device(dev):
        _check(lib().rnnt_engine_beam_stream_init(int(S), int(E), int(O), int(H), int(V), int(bool(has_text)), int(max_length), beam, int(blank), n,
                                                  -1 if index is None else int(index), _p(state), _p(scores), _p(block),
                                                  ctypes.c_size_t(block.numel()), _stream(dev)))


def beam_stream_push(frames_list, pred_params, ln_eps, text_W, text_b, W, bias, blank, max_length, beam, max_per_frame, tables,
                     state, tokens, scores, block, chunk=32, in_flight=2):
    """Enqueue one push of a group of beam streams (C ABI rnnt_engine_beam_stream_push): `frames_list` holds one entry per
    stream, a [k_u, H] fp32 frame tensor (audio_ln applied) or None / k_u = 0 for a stream that sits the push out; they are packed here
    and the table of first rows and counts is the push's one small host-to-device copy.  `state` int32[n, 32], `tokens`
    int32[n, beam, max_length], `scores` float64[n, beam] and `block` are the group's persistent tensors (beam_stream_init); `tables`
    greedy_decode_tables(...) of the same parameters.  Rounds are enqueued in chunks until the device has raised the pinned flag (all
    streams at rest; polled, never waited for): chunks of `chunk` rounds, fewer for a push of few frames (2 * frames + 1), at most
    `in_flight` of them ahead of the device.  No synchronisation: afterwards entry j < state[u, 2] of stream u is tokens[u, j, 1 : 1 + state[u, 8 + j]] with
    log-probability scores[u, j], best first, and state[u, BEAM_STREAM_FRAMES] its frames consumed.  A push without any frame enqueues
    nothing."""
    n = int(state.shape[0])
    frames_list = list(frames_list)
    if len(frames_list) != n:
        raise ValueError(f"beam_stream_push: {len(frames_list)} entries for {n} streams")
    counts = [0 if f is None else int(f.shape[0]) for f in frames_list]
    if not any(counts):
        return
    max_count = max(counts)
    packed, rows = _pack_rows(frames_list, counts)
    m = _DecodeModel(packed, pred_params, ln_eps, text_W, text_b, W, bias)
    _require_cuda(m.frames, state, tokens, scores, block, tables)
    _require_dtype(torch.int32, state=state, tokens=tokens)
    _require_dtype(torch.float64, scores=scores)
    _require_contiguous(state=state, tokens=tokens, scores=scores, block=block)
    beam, max_length, max_per_frame = int(beam), int(max_length), int(max_per_frame)
    if state.shape != (n, 32) or tokens.shape != (n, beam, max_length) or scores.shape != (n, beam):
        raise RuntimeError(f"beam_stream_push: state [{n}, 32], tokens [{n}, {beam}, {max_length}], scores [{n}, {beam}] expected")
    with torch.cuda.device(m.dev):
        table = _rows_table(rows, m.dev)
        head = (_p(m.frames), ctypes.c_int64(m.frames.stride(0)), m.frames.shape[0], _p(table), n, max_count,
                *m.args(blank, max_length, max_per_frame), beam, _p(tables))
        tail = (_p(state), _p(tokens), _p(scores), _p(block), ctypes.c_size_t(block.numel()), _stream(m.dev))
        # chunks sized to the push: a 1-frame push enqueues 3 rounds at a time, not `chunk`; and the wait as soon as `in_flight` chunks
        # are out (before the flag is read again: a short push ends after the chunk that served it)
        flag = _enqueue_rounds(lambda it, first, flag: _check(lib().rnnt_engine_beam_stream_push(*head, it, first, flag, *tail)),
                               max_count * max(1, max_per_frame) + 1, min(max(1, int(chunk)), 2 * max_count + 1), in_flight,
                               wait_at_limit=True)
        state._keepalive = (flag, table, *m.keep, tables)  # until the caller has synchronised
