"""AudioEncoder / JasperBlock with the constructor arguments, attribute layout and state-dict keys of the reference
(rnnt/jasper.py, rnnt/causalconv.py) whose INFERENCE forward — whole utterances and streaming pushes — runs on the HIP
engine (C ABI rnnt_engine_encoder_*; rnnt_amd/csrc/encoder.hip).

    encoder:
      _target_: rnnt_amd.AudioEncoder                 # was rnnt.jasper.AudioEncoder
      blocks:
        - _target_: rnnt_amd.JasperBlock              # was rnnt.jasper.JasperBlock

or, for a model that is already built (the reference's own rnnt.jasper.AudioEncoder included):

    model.encoder = rnnt_amd.AudioEncoder.from_module(model.encoder)     # shares the Parameters

One definition, two paths.  The torch path is the module stated in plain torch: it trains through autograd, runs on the
CPU, in float64, streams with look-ahead (`additional_context`), and it is the oracle of the engine path.  The engine path
is taken by backend "auto" when gradients are off, the module is in eval(), input and parameters are fp32 tensors on a HIP
device and no conv has look-ahead; `backend` ("auto" | "torch" | "engine") forces either, "engine" raises where it does not
apply.  Only backend "engine" goes further: whole-utterance calls with look-ahead, and — with grad mode on — TRAINING on
the engine (C ABI rnnt_engine_encoder_train_*): a forward that keeps what the backward reads and a backward
for every parameter, through a torch.autograd.Function.  The training path takes instance norm and batch norm on its
running statistics (the BatchNorm1d modules in eval()), draws one uint8 keep mask per sub-block while a block's dropout is
active, and refuses inputs that require grad, batch statistics and streamed pushes.  "auto" keeps grad-mode calls on torch.

Definition.  A causal conv (kernel k, stride s, dilation d, P = (k-1)d - s + 1) reads X~ = P zeros (whole utterance) or the
carried state (streaming) followed by the input; it gives (len(X~) - d(k-1) - 1) // s + 1 frames and leaves X~ from frame
out*s on as the next state — P frames plus the stride remainder, so the strided prologue's state length varies from push to
push.  Every length is host arithmetic on the chunk length; nothing is read back from the device.  Instance norm takes its
statistics over the frames of the call: a streamed instance-norm encoder depends on the chunking, exactly as the
reference's does.  Where the reference cannot run — a chunk too short for one prologue frame, instance norm over a single
frame — ValueError is raised before anything is launched and the state is left as it was.
"""
import ctypes

import torch

from . import engine

NORM_NONE, NORM_BATCH, NORM_INSTANCE = 0, 1, 2  # include/rnnt_engine.h RNNT_ENC_NORM_*
ROLE_PLAIN, ROLE_FIRST, ROLE_LAST, ROLE_RESIDUAL, ROLE_FINAL = 0, 1, 2, 4, 8  # RNNT_ENC_ROLE_*
REGIME_AUTO, REGIME_MANY_ROWS = 0, 1  # RNNT_ENC_REGIME_*
MAX_LAYERS = 64  # RNNT_ENC_MAX_LAYERS
# backend "auto" hands calls of more than this many output rows (N x output frames) to the torch path.  64 = the rows the engine's
# weight-streaming kernel covers; measured at the reference's widths (tools/bench_encoder.py, profiles/encoder_bench.txt) its pushes of
# 1 and 25 rows take 0.43x and 0.45x the torch path's time.  The one many-row shape timed (500 rows, N = 1) takes 0.75x on the MFMA
# conv, but a single point does not carry a rule for every batch and length, so those shapes stay on torch until measured.
# backend "engine" ignores the threshold.
ENGINE_AUTO_MAX_ROWS = 64
# ... and, of those, only calls whose every layer also stays within this many frames of state + input (N x len): the second
# condition of the weight-streaming kernel (encoder.hip ENC_FEW_FRAMES).  Together the two are exactly the C side's test for that
# kernel, so "auto" never runs the MFMA conv.  The threshold rests on three measured
# shapes only (1, 25 and 500 rows at N = 1); nothing between 25 and 500 rows, and no batched push, has been timed.
ENGINE_AUTO_MAX_FRAMES = 224


class _Layer(ctypes.Structure):  # include/rnnt_engine.h: rnnt_encoder_layer
    _fields_ = [(n, ctypes.c_int) for n in ("cin", "cout", "taps", "stride", "dilation", "norm", "role")] + [
        ("eps", ctypes.c_float)] + [(n, ctypes.c_void_p) for n in ("weight", "bias", "gamma", "beta", "mean", "var")]


class _Grads(ctypes.Structure):  # include/rnnt_engine.h: rnnt_encoder_grads
    _fields_ = [(n, ctypes.c_void_p) for n in ("weight", "bias", "gamma", "beta")]


def _make_norm(norm_type, channels):
    if norm_type == "batch":
        return torch.nn.BatchNorm1d(channels)
    if norm_type == "instance":
        return torch.nn.InstanceNorm1d(channels, track_running_stats=False)
    if norm_type == "instance_affine":
        return torch.nn.InstanceNorm1d(channels, track_running_stats=False, affine=True)
    raise ValueError(f"norm_type {norm_type!r}: 'batch', 'instance' or 'instance_affine'")


class CausalConv1d(torch.nn.Module):
    """The encoder's conv: `self.conv` under the reference's name, any stride / dilation / look-ahead (the predictor's
    CausalConv1d refuses those).  Its own methods are the torch path."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, dilation, additional_context: int = 0):
        super().__init__()
        self.conv = torch.nn.Conv1d(in_channels, out_channels, kernel_size, stride, dilation=dilation)
        self.padding = (kernel_size - 1) * dilation - stride + 1
        if additional_context < 0:
            raise ValueError("additional_context must be non-negative")
        if additional_context > self.padding:
            raise ValueError("additional_context can't be greater than the padding")
        self.additional_context = additional_context
        self.left_padding = self.padding - additional_context

    def forward(self, x):
        return self.conv(torch.nn.functional.pad(x, (self.left_padding, 0)))

    def streaming_forward(self, x, state):
        xt = torch.cat((state, x), dim=2)
        y = self.conv(xt)
        return y, xt[:, :, y.shape[2] * self.conv.stride[0]:]


class JasperBlock(torch.nn.Module):
    """num_sub_blocks x (conv -> norm -> GELU -> dropout); residual_norm(residual_conv(input)) joins before the last GELU."""

    def __init__(self, kernel_size, in_channels, out_channels, dropout, num_sub_blocks, norm_type="batch", additional_context: int = 0):
        super().__init__()
        self.convs = torch.nn.ModuleList()
        self.norms = torch.nn.ModuleList()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.num_sub_blocks = num_sub_blocks
        for i in range(num_sub_blocks):
            self.convs.append(CausalConv1d(in_channels if i == 0 else out_channels, out_channels, kernel_size, 1, 1,
                                           additional_context=additional_context))
            self.norms.append(_make_norm(norm_type, out_channels))
        self.residual_conv = torch.nn.Conv1d(in_channels, out_channels, 1)
        self.residual_norm = _make_norm(norm_type, out_channels)
        self.dropout = torch.nn.Dropout(dropout)

    def forward(self, x, keep_masks=None):
        return _block_torch(self, x, None, keep_masks)[0]

    def streaming_forward(self, x, states):
        return _block_torch(self, x, states)


def _drops(blk):
    """The block's drop probability while its dropout is active (train() mode and p > 0), else 0."""
    d = getattr(blk, "dropout", None)
    return float(d.p) if isinstance(d, torch.nn.Dropout) and d.training and d.p > 0 else 0.0


def _block_torch(blk, x, states, keeps=None):
    """keeps: one keep mask (N, frames, channels) per sub-block, time-major like the engine's activations, used in place of
    drawing while the block's dropout is active."""
    res = blk.residual_norm(blk.residual_conv(x))
    new_states = []
    last = len(blk.convs) - 1
    p = _drops(blk)
    for i, (conv, norm) in enumerate(zip(blk.convs, blk.norms)):
        if states is None:
            x = conv(x)
        else:
            x, st = conv.streaming_forward(x, states[i])
            new_states.append(st)
        x = norm(x)
        if i == last:
            x = x + res
        x = torch.nn.functional.gelu(x)
        if keeps is not None and p > 0:
            x = x * keeps[i].permute(0, 2, 1).to(x.dtype) / (1.0 - p)
        else:
            x = blk.dropout(x)
    return x, new_states


def _is_causal(m):
    return isinstance(getattr(m, "conv", None), torch.nn.Conv1d) and hasattr(m, "left_padding")


def _has_lookahead(holder):
    conv = holder.conv
    return (getattr(holder, "additional_context", 0) != 0 or
            holder.left_padding != (conv.kernel_size[0] - 1) * conv.dilation[0] - conv.stride[0] + 1)


def _is_block(m):
    return all(hasattr(m, a) for a in ("convs", "norms", "residual_conv", "residual_norm"))


def _norm_kind(m):
    """(kind, usable by the engine in eval mode) of a norm module."""
    if isinstance(m, torch.nn.BatchNorm1d):
        return NORM_BATCH, m.running_mean is not None and m.running_var is not None
    if isinstance(m, torch.nn.InstanceNorm1d):
        return NORM_INSTANCE, not m.track_running_stats
    return None, False


class _EncoderTrainFn(torch.autograd.Function):
    """rnnt_engine_encoder_train_fwd / _train_bwd.  Behind the bookkeeping arguments come the parameters, per layer
    of the list: conv weight, conv bias and, where the norm is affine, norm weight and bias.  The `saved` block, the keep masks
    and the packed tables of the forward are held for the backward; the input gets no gradient."""

    @staticmethod
    def forward(ctx, enc, prep, packed, x, masks, drop, L_out, *params):
        flat, arr = prep[0], prep[1]
        dev, nl = x.device, len(flat)
        N, _, L = x.shape
        regime = {"auto": REGIME_AUTO, "many_rows": REGIME_MANY_ROWS}[enc.conv_regime]
        lead = (ctypes.c_int32 * nl)(*[0 if h is None else h.left_padding for h, _, _, _ in flat])
        keep = (ctypes.c_void_p * nl)(*[None if m is None else m.data_ptr() for m in masks])
        p = (ctypes.c_float * nl)(*drop)
        strides = (ctypes.c_int64 * 3)(*x.stride())
        lib = engine.lib()
        n = ctypes.c_size_t(0)
        with torch.cuda.device(dev):
            engine._check(lib.rnnt_engine_encoder_train_saved_bytes(arr, nl, N, L, lead, ctypes.byref(n)))
            saved = torch.empty(max(256, int(n.value)), dtype=torch.uint8, device=dev)
            engine._check(lib.rnnt_engine_encoder_train_workspace_bytes(arr, nl, N, L, regime, lead, ctypes.byref(n)))
            ws = engine.workspace(dev, n.value)
            out = torch.empty((N, L_out, flat[-1][1].out_channels), dtype=torch.float32, device=dev)
            engine._check(lib.rnnt_engine_encoder_train_fwd(arr, nl, engine._p(packed), engine._p(x), strides, N, L, lead, keep, p, regime,
                                                            engine._p(out), engine._p(saved), ctypes.c_size_t(saved.numel()),
                                                            engine._p(ws), ctypes.c_size_t(ws.numel()), engine._stream(dev)))
        ctx.call = (flat, arr, packed, x, masks, lead, keep, p, strides, regime, saved, params)
        enc.last_saved_bytes = int(saved.numel())
        return out.permute(0, 2, 1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        flat, arr, packed, x, masks, lead, keep, p, strides, regime, saved, params = ctx.call
        dev, nl = x.device, len(flat)
        N, _, L = x.shape
        dout = grad_out.to(torch.float32).permute(0, 2, 1).contiguous()  # time-major once, like `out`
        grads, out, k = (_Grads * nl)(), [], 0
        needs = ctx.needs_input_grad[7:]
        for G, (_, _, norm, _) in zip(grads, flat):
            names = ("weight", "bias") + (("gamma", "beta") if norm is not None and norm.weight is not None else ())
            for name in names:
                g = torch.empty(params[k].shape, dtype=torch.float32, device=dev) if needs[k] else None
                if g is not None:
                    setattr(G, name, g.data_ptr())
                out.append(g)
                k += 1
        lib = engine.lib()
        n = ctypes.c_size_t(0)
        with torch.cuda.device(dev):
            engine._check(lib.rnnt_engine_encoder_train_workspace_bytes(arr, nl, N, L, regime, lead, ctypes.byref(n)))
            ws = engine.workspace(dev, n.value)
            engine._check(lib.rnnt_engine_encoder_train_bwd(arr, nl, engine._p(packed), engine._p(x), strides, N, L, lead, keep, p,
                                                            engine._p(dout), engine._p(saved), ctypes.c_size_t(saved.numel()), grads,
                                                            engine._p(ws), ctypes.c_size_t(ws.numel()), engine._stream(dev)))
        return (None,) * 7 + tuple(out)


class AudioEncoder(torch.nn.Module):
    """(N, input_features, L) mel features -> (N, output_features, ~L / prologue_stride)."""

    backend = "auto"       # "auto" | "torch" | "engine"
    conv_regime = "auto"   # "auto" | "many_rows": force the engine's MFMA GEMM on every layer (tests)

    def __init__(self, input_features: int = 80, prologue_kernel_size: int = 11, prologue_stride: int = 2, prologue_dilation: int = 1,
                 blocks=(), epilogue_features: int = 896, epilogue_kernel_size: int = 29, epilogue_stride: int = 1,
                 epilogue_dilation: int = 2, output_features: int = 1024, norm_type="batch"):
        super().__init__()
        blocks = list(blocks)
        self.blocks = torch.nn.Sequential()
        self.prologue_stride = prologue_stride
        self.epilogue_stride = epilogue_stride
        first = blocks[0].in_channels if blocks else epilogue_features
        self.blocks.append(CausalConv1d(input_features, first, prologue_kernel_size, prologue_stride, prologue_dilation))
        self.blocks.append(_make_norm(norm_type, first))
        self.blocks.append(torch.nn.GELU())
        self.blocks.extend(blocks)
        last = blocks[-1].out_channels if blocks else first
        self.blocks.append(CausalConv1d(last, epilogue_features, epilogue_kernel_size, epilogue_stride, epilogue_dilation))
        self.blocks.append(_make_norm(norm_type, epilogue_features))
        self.blocks.append(torch.nn.GELU())
        self.blocks.append(torch.nn.Conv1d(epilogue_features, output_features, kernel_size=1, stride=1, dilation=1))
        self._reset_cache()

    @classmethod
    def from_module(cls, enc):
        """Wrap an encoder that is already built — anything with the reference's layout (`blocks`: conv holders with `.conv` and
        `.left_padding`, Jasper blocks with `convs` / `norms` / `residual_conv` / `residual_norm`, norms, GELUs, the final Conv1d).
        The wrapper holds the SAME `blocks` container, so every Parameter and buffer is shared, not copied."""
        if isinstance(enc, cls):
            return enc
        if not isinstance(getattr(enc, "blocks", None), torch.nn.Sequential):
            raise TypeError(f"AudioEncoder.from_module: {type(enc).__name__} has no `blocks` Sequential")
        self = cls.__new__(cls)
        torch.nn.Module.__init__(self)
        self.blocks = enc.blocks
        self.prologue_stride = getattr(enc, "prologue_stride", None)
        self.epilogue_stride = getattr(enc, "epilogue_stride", None)
        self.train(enc.training)
        self._reset_cache()
        return self

    def _reset_cache(self):
        self._cache_key = None
        self._cache = None  # (layer list, ctypes layer array, packed weights, layer index of each causal conv, has look-ahead)
        self._train_packed = None  # the training path's two tables (rnnt_engine_encoder_train_pack), under the same key
        self.last_backend = None  # "engine" | "torch": the path of the last call
        self.last_saved_bytes = None  # bytes the last engine training forward kept for its backward

    # ------------------------------------------------------------------------------------------------- structure
    def _causal_convs(self):
        """The convs that carry streaming state, in state order."""
        out = []
        for m in self.blocks:
            if _is_causal(m):
                out.append(m)
            elif _is_block(m):
                out.extend(m.convs)
        return out

    def _flat(self, allow_lookahead=False):
        """The module as the engine's layer list: (conv holder or None, Conv1d, norm or None, role) in execution order, or a string
        saying why the engine cannot take it.  Look-ahead is a reason unless `allow_lookahead` (whole-utterance calls under
        backend "engine" carry it as each layer's `left_padding`)."""
        mods = list(self.blocks)
        out, i = [], 0
        while i < len(mods):
            m = mods[i]
            if _is_causal(m):
                if i + 2 >= len(mods) or not isinstance(mods[i + 2], torch.nn.GELU):
                    return "a causal conv outside a block is not followed by norm and GELU"
                out.append((m, m.conv, mods[i + 1], ROLE_PLAIN))
                i += 3
            elif _is_block(m):
                n = len(m.convs)
                if n < 1 or len(m.norms) != n:
                    return "a block without sub-blocks"
                out.append((None, m.residual_conv, m.residual_norm, ROLE_RESIDUAL))
                for k, (c, nm) in enumerate(zip(m.convs, m.norms)):
                    if not _is_causal(c):
                        return "a block's conv is not a causal conv holder"
                    out.append((c, c.conv, nm, (ROLE_FIRST if k == 0 else 0) | (ROLE_LAST if k == n - 1 else 0)))
                i += 1
            elif isinstance(m, torch.nn.Conv1d) and i == len(mods) - 1:
                out.append((None, m, None, ROLE_FINAL))
                i += 1
            else:
                return f"unexpected module {type(m).__name__} at blocks.{i}"
        if not out or out[-1][3] != ROLE_FINAL:
            return "the module does not end in the output 1x1 conv"
        if len(out) > MAX_LAYERS:
            return f"more than {MAX_LAYERS} layers"
        for holder, conv, norm, role in out:
            if conv.padding != (0,) or conv.groups != 1 or conv.bias is None or conv.padding_mode != "zeros":
                return "a conv with padding, groups or no bias"
            if holder is None and (conv.kernel_size[0] != 1 or conv.stride[0] != 1):
                return "a residual / output conv that is not 1x1"
            if holder is not None and _has_lookahead(holder):
                if not allow_lookahead:
                    return "look-ahead (additional_context != 0)"
                if role != ROLE_PLAIN or any(holder is c for m in mods if _is_block(m) for c in m.convs):
                    # (the torch path raises there as well, and so does the reference: x + residual on unequal lengths)
                    return "look-ahead inside a JasperBlock: its sub-blocks lose frames, its residual branch keeps the input's length"
            if role not in (ROLE_PLAIN, ROLE_RESIDUAL, ROLE_FINAL) and conv.stride[0] != 1:
                return "a strided conv inside a block"
            # the limits of rnnt_engine_encoder_* (RNNT_ERR_UNSUPPORTED there: such a module stays on the torch path)
            if conv.kernel_size[0] * conv.dilation[0] > 4096 or conv.stride[0] > 64 or max(conv.in_channels, conv.out_channels) > 65536:
                return "kernel_size * dilation > 4096, stride > 64 or more than 65536 channels"
            if holder is not None and holder.left_padding < 0:
                return "a stride beyond the kernel's span (negative padding)"
            if norm is not None and not _norm_kind(norm)[1]:
                return f"norm {type(norm).__name__} (batch norm with running statistics, or instance norm without)"
        return out

    # ------------------------------------------------------------------------------------------------- host arithmetic
    def _lengths(self, L, state_lens):
        """Frames through the module for an input of L frames: [(frames in, state frames, frames out, next state frames)] per causal
        conv, and the output length.  state_lens None: whole utterance (left_padding zeros).  Raises ValueError where the reference
        cannot run: too few frames for an output frame, instance norm over one frame."""
        rows, si = [], 0

        def conv_len(h, L):
            nonlocal si
            k, s, d = h.conv.kernel_size[0], h.conv.stride[0], h.conv.dilation[0]
            slen = h.left_padding if state_lens is None else state_lens[si]
            si += 1
            Lt = slen + L
            if Lt < d * (k - 1) + 1:
                raise ValueError(f"AudioEncoder: {L} input frames (+ {slen} of state) are too short for one output frame of a conv with "
                                 f"kernel {k}, stride {s}, dilation {d}")
            out = (Lt - d * (k - 1) - 1) // s + 1
            rows.append((L, slen, out, Lt - out * s))
            return out

        def norm_len(nm, L):
            if isinstance(nm, torch.nn.InstanceNorm1d) and not nm.track_running_stats and L == 1:
                raise ValueError("AudioEncoder: instance norm over a single output frame (torch: Expected more than 1 spatial element); "
                                 "push a longer chunk")

        if L < 1:
            raise ValueError("AudioEncoder: empty input (a chunk must give the prologue at least one output frame)")
        for m in self.blocks:
            if _is_causal(m):
                L = conv_len(m, L)
            elif _is_block(m):
                norm_len(m.residual_norm, L)
                for c, nm in zip(m.convs, m.norms):
                    L = conv_len(c, L)
                    norm_len(nm, L)
            else:
                norm_len(m, L)
        return rows, L

    def calc_output_lens(self, input_lens):
        out = input_lens.clone()
        for h in self._causal_convs():
            k, s, d = h.conv.kernel_size[0], h.conv.stride[0], h.conv.dilation[0]
            out = (out + h.left_padding - d * (k - 1) - 1) // s + 1
        return out

    def streaming_init_state(self, batch_size):
        """The reference's list of (N, C_in, P) zero tensors on the CPU, one per causal conv."""
        return [torch.zeros(batch_size, h.conv.in_channels, (h.conv.kernel_size[0] - 1) * h.conv.dilation[0] - h.conv.stride[0] + 1)
                for h in self._causal_convs()]

    # ------------------------------------------------------------------------------------------------- dispatch
    def _check_input(self, x):
        if x.dim() != 3:
            raise ValueError(f"AudioEncoder takes (N, features, L), got {tuple(x.shape)}")
        cin = self.blocks[0].conv.in_channels if len(self.blocks) and _is_causal(self.blocks[0]) else None
        if cin is not None and x.shape[1] != cin:  # the engine reads channels by the layer list: never launch on another count
            raise ValueError(f"AudioEncoder takes (N, {cin}, L) features, got {tuple(x.shape)}")
        if x.shape[0] < 1:
            raise ValueError("AudioEncoder: empty batch")

    def __getstate__(self):
        """copy.deepcopy / pickle / torch.save(module): the engine cache (ctypes descriptors with raw pointers, the packed weights) is
        not part of the module's state; a copy builds its own on first engine use."""
        state = dict(self.__dict__)
        state["_cache_key"] = state["_cache"] = state["_train_packed"] = None
        return state

    def _use_engine(self, x, rows, streaming=False):
        """The prepared engine state (layer list, descriptors, packed weights) when the engine path applies to this call, else None;
        backend "engine" raises with the reason instead.  With grad mode on the engine path is the training path (saved forward and
        backward) and only backend "engine" takes it."""
        if self.backend not in ("auto", "torch", "engine"):
            raise ValueError(f"AudioEncoder.backend {self.backend!r}: 'auto', 'torch' or 'engine'")
        if self.backend == "torch":
            return None
        why = None
        grad = torch.is_grad_enabled()
        if grad and (self.backend == "auto" or streaming):
            why = "grad mode is on"  # ("auto" keeps training on the torch path; a streamed push has no engine backward)
        elif grad and x.requires_grad:
            why = "the input requires grad (the engine's backward stops at the parameters)"
        elif not grad and self.training:
            why = "the module is in train() mode"
        elif x.device.type != "cuda" or x.dtype != torch.float32:
            why = f"input is {x.dtype} on {x.device} (needs fp32 on a HIP device)"
        elif any(x.shape[0] * r[2] > 2 ** 20 or x.shape[0] * (r[0] + r[1]) > 2 ** 28 or r[1] > 2 ** 20 for r in rows):
            why = "a layer of more than 2^20 output rows or 2^28 frames of state + input"  # (the C side's limits, with room)
        elif self.backend == "auto" and any(x.shape[0] * r[2] > ENGINE_AUTO_MAX_ROWS or
                                            x.shape[0] * (r[0] + r[1]) > ENGINE_AUTO_MAX_FRAMES for r in rows):
            why = (f"more than ENGINE_AUTO_MAX_ROWS = {ENGINE_AUTO_MAX_ROWS} output rows or ENGINE_AUTO_MAX_FRAMES = "
                   f"{ENGINE_AUTO_MAX_FRAMES} frames of state + input in a layer")
        else:
            prep = self._prepared(x.device)
            if isinstance(prep, str):
                why = prep
            elif prep[4] and (self.backend == "auto" or streaming):
                why = "look-ahead (additional_context != 0)"
            elif grad and any(isinstance(nm, torch.nn.BatchNorm1d) and nm.training for _, _, nm, _ in prep[0]):
                why = "batch norm on batch statistics (a BatchNorm1d in train() mode; the engine trains through running statistics)"
        if why is not None:
            if self.backend == "engine":
                raise RuntimeError(f"AudioEncoder(backend='engine'): the engine path does not apply: {why}")
            return None
        return prep

    def forward(self, x, keep_masks=None):
        """`keep_masks` (test aid): one uint8 keep mask (N, frames, channels) — time-major, like the engine's activations — per
        sub-block of every JasperBlock, in execution order, used instead of drawing while that block's dropout is active."""
        self._check_input(x)
        rows, L_out = self._lengths(x.shape[2], None)  # raises before anything is launched
        if keep_masks is not None:
            keep_masks = list(keep_masks)
            want, si = [], 0
            for m in self.blocks:
                if _is_causal(m):
                    si += 1
                elif _is_block(m):
                    for c in m.convs:
                        want.append((x.shape[0], rows[si][2], c.conv.out_channels))
                        si += 1
            if [tuple(k.shape) for k in keep_masks] != want:
                raise ValueError(f"AudioEncoder: keep_masks of shapes {[tuple(k.shape) for k in keep_masks]}, the blocks' layers give {want}")
        prep = self._use_engine(x, rows)
        if prep is None:
            self.last_backend = "torch"
            return self._torch_forward(x, keep_masks)
        self.last_backend = "engine"
        if torch.is_grad_enabled():
            return self._engine_train(prep, x, keep_masks, rows, L_out)
        if prep[4]:  # look-ahead: the push entry with left_padding zero frames of state per conv; the states it leaves are dropped
            state = [torch.zeros((x.shape[0], h.conv.in_channels, h.left_padding), dtype=torch.float32, device=x.device)
                     for h in self._causal_convs()]
            return self._engine_call(prep, x, state, rows, L_out)[0]
        return self._engine_call(prep, x, None, rows, L_out)[0]

    def _torch_forward(self, x, keep_masks):
        if keep_masks is None:
            return self.blocks(x)
        at = 0
        for m in self.blocks:
            if _is_block(m):
                x = _block_torch(m, x, None, keep_masks[at:at + len(m.convs)])[0]
                at += len(m.convs)
            else:
                x = m(x)
        return x

    def streaming_forward(self, x, state):
        self._check_input(x)
        n_state = len(self._cache[3]) if self._cache is not None else len(self._causal_convs())
        if len(state) != n_state:
            raise ValueError(f"AudioEncoder.streaming_forward: {len(state)} state tensors for {n_state} causal convs")
        rows, L_out = self._lengths(x.shape[2], [int(s.shape[2]) for s in state])  # raises with `state` untouched
        prep = self._use_engine(x, rows, streaming=True)
        if prep is None:
            self.last_backend = "torch"
            return self._stream_torch(x, state)
        self.last_backend = "engine"
        return self._engine_call(prep, x, state, rows, L_out)

    def _stream_torch(self, x, state):
        si, new = 0, []
        for m in self.blocks:
            if _is_causal(m):
                x, st = m.streaming_forward(x, state[si])
                new.append(st)
                si += 1
            elif _is_block(m):
                n = len(m.convs)
                x, sts = m.streaming_forward(x, state[si:si + n])
                new.extend(sts)
                si += n
            else:
                x = m(x)
        return x, new

    # ------------------------------------------------------------------------------------------------- engine path
    def repack(self):
        """Drop the packed weights and the cached layer list; the next engine call builds them again.  Needed only after the weights
        were written through raw pointers that no version counter sees (a replayed HIP graph of an optimizer step), or after a
        block's own module lists were edited in place."""
        self._cache_key = None
        self._cache = None
        self._train_packed = None

    def _prepared(self, dev):
        """(layer list, ctypes layer array, packed weights, [layer index of each causal conv]) — or why the engine cannot take the
        module.  Built on first use; the weights are packed again whenever a conv weight's storage or `_version` changed (an
        optimizer step, load_state_dict, .to()); the other parameters are read through their pointers on every call."""
        struct = tuple(map(id, self.blocks))
        flat = self._cache[0] if self._cache is not None and self._cache_key[0] == struct else self._flat(allow_lookahead=True)
        if isinstance(flat, str):
            return flat
        key = []
        for _, conv, norm, _ in flat:
            key.append((conv.weight.data_ptr(), conv.weight._version, conv.bias.data_ptr()))
            if norm is not None:
                key.append(tuple(0 if t is None else t.data_ptr() for t in (norm.weight, norm.bias, norm.running_mean, norm.running_var)))
        key = (struct, dev, tuple(key))
        if key == self._cache_key:
            return self._cache
        for p in list(self.parameters()) + list(self.buffers()):
            if p.is_floating_point() and (p.device != dev or p.dtype != torch.float32):
                return "a parameter is not fp32 on the input's device"
        arr = (_Layer * len(flat))()
        for L, (_, conv, norm, role) in zip(arr, flat):
            L.cin, L.cout, L.taps = conv.in_channels, conv.out_channels, conv.kernel_size[0]
            L.stride, L.dilation, L.role = conv.stride[0], conv.dilation[0], role
            L.norm, L.eps = NORM_NONE, 0.0
            engine._require_contiguous(weight=conv.weight, bias=conv.bias)
            L.weight, L.bias = conv.weight.data_ptr(), conv.bias.data_ptr()
            if norm is not None:
                L.norm, L.eps = _norm_kind(norm)[0], float(norm.eps)
                ptr = lambda t: None if t is None else t.data_ptr()
                L.gamma, L.beta = ptr(norm.weight), ptr(norm.bias)
                if L.norm == NORM_BATCH:
                    L.mean, L.var = ptr(norm.running_mean), ptr(norm.running_var)
        causal = [i for i, (holder, _, _, _) in enumerate(flat) if holder is not None]
        lookahead = any(holder is not None and _has_lookahead(holder) for holder, _, _, _ in flat)
        # the packed tables (entry 2: inference; _train_packed: training) are built by the first call that reads them (_packed)
        self._cache_key, self._cache, self._train_packed = key, [flat, arr, None, causal, lookahead], None
        return self._cache

    def _packed(self, prep, dev, train=False):
        """The inference tables (rnnt_engine_encoder_pack) or the training path's two (rnnt_engine_encoder_train_pack) of the
        prepared state, packed on first use; _prepared drops both when a conv weight's `_version` or storage changed."""
        have = self._train_packed if train else prep[2]
        if have is not None:
            return have
        flat, arr = prep[0], prep[1]
        lib = engine.lib()
        size, pack = ((lib.rnnt_engine_encoder_train_packed_bytes, lib.rnnt_engine_encoder_train_pack) if train else
                      (lib.rnnt_engine_encoder_packed_bytes, lib.rnnt_engine_encoder_pack))
        n = ctypes.c_size_t(0)
        with torch.cuda.device(dev):
            engine._check(size(arr, len(flat), ctypes.byref(n)))
            packed = torch.empty(int(n.value), dtype=torch.uint8, device=dev)
            engine._check(pack(arr, len(flat), engine._p(packed), ctypes.c_size_t(packed.numel()), engine._stream(dev)))
        if train:
            self._train_packed = packed
        else:
            prep[2] = packed
        return packed

    def _engine_train(self, prep, x, keep_masks, rows, L_out):
        """The training path: draws the keep masks (or takes the given ones) and runs _EncoderTrainFn over the parameters."""
        flat = prep[0]
        dev = x.device
        drop, sub = [], []  # per layer of the list: its block's drop probability while that dropout is active; is a sub-block
        for m in self.blocks:
            if _is_block(m):
                drop += [0.0] + [_drops(m)] * len(m.convs)
                sub += [False] + [True] * len(m.convs)
            elif _is_causal(m) or isinstance(m, torch.nn.Conv1d):
                drop.append(0.0)
                sub.append(False)
        assert len(drop) == len(flat)
        row_of = {li: si for si, li in enumerate(prep[3])}
        masks, k = [None] * len(flat), 0
        for i, (_, conv, _, _) in enumerate(flat):
            if not sub[i]:
                continue
            if drop[i] > 0.0:
                if keep_masks is not None:
                    masks[i] = keep_masks[k].to(device=dev, dtype=torch.uint8).contiguous()
                else:
                    shape = (x.shape[0], rows[row_of[i]][2], conv.out_channels)
                    masks[i] = (torch.rand(shape, device=dev) >= drop[i]).to(torch.uint8)
            k += 1
        params = []
        for _, conv, norm, _ in flat:
            params += [conv.weight, conv.bias]
            if norm is not None and norm.weight is not None:
                params += [norm.weight, norm.bias]
        return _EncoderTrainFn.apply(self, prep, self._packed(prep, dev, train=True), x, masks, drop, L_out, *params)

    def _engine_call(self, prep, x, state, rows, L_out):
        flat, arr, _, causal, _ = prep
        dev = x.device
        packed = self._packed(prep, dev)
        N, _, L = x.shape
        nl = len(flat)
        regime = {"auto": REGIME_AUTO, "many_rows": REGIME_MANY_ROWS}[self.conv_regime]
        lib = engine.lib()
        with torch.cuda.device(dev):
            out = torch.empty((N, L_out, flat[-1][1].out_channels), dtype=torch.float32, device=dev)
            strides = (ctypes.c_int64 * 3)(*x.stride())
            lens_in = None
            if state is not None:
                lens_in, lens_out = (ctypes.c_int32 * nl)(), (ctypes.c_int32 * nl)()
                ptr_in, ptr_out = (ctypes.c_void_p * nl)(), (ctypes.c_void_p * nl)()
                # every new state of the push is a view of one buffer
                sizes = [N * flat[li][1].in_channels * r[3] for li, r in zip(causal, rows)]
                flat_state = torch.empty(max(1, sum(sizes)), dtype=torch.float32, device=dev)
                base, new_state, keep, off = flat_state.data_ptr(), [], [], 0
                for si, li in enumerate(causal):
                    cin, s = flat[li][1].in_channels, state[si]
                    if s.shape[0] != N or s.shape[1] != cin:
                        raise ValueError(f"AudioEncoder.streaming_forward: state {si} is {tuple(s.shape)}, the conv takes ({N}, {cin}, len)")
                    if s.device != dev or s.dtype != torch.float32:
                        raise RuntimeError("AudioEncoder.streaming_forward: the state must be fp32 on the input's device")
                    if not s.is_contiguous():
                        s = s.contiguous()
                        keep.append(s)
                    new_state.append(flat_state[off:off + sizes[si]].view(N, cin, rows[si][3]))
                    lens_in[li], lens_out[li] = rows[si][1], rows[si][3]
                    ptr_in[li] = s.data_ptr() if rows[si][1] else None
                    ptr_out[li] = base + 4 * off if sizes[si] else None
                    off += sizes[si]
            n = ctypes.c_size_t(0)
            engine._check(lib.rnnt_engine_encoder_workspace_bytes(arr, nl, N, L, regime, lens_in, ctypes.byref(n)))
            ws = engine.workspace(dev, n.value)
            if state is None:
                engine._check(lib.rnnt_engine_encoder_fwd(arr, nl, engine._p(packed), engine._p(x), strides, N, L, regime, engine._p(out),
                                                          engine._p(ws), ctypes.c_size_t(ws.numel()), engine._stream(dev)))
                return out.permute(0, 2, 1), None
            engine._check(lib.rnnt_engine_encoder_stream_push(arr, nl, engine._p(packed), engine._p(x), strides, N, L, ptr_in, lens_in,
                                                              ptr_out, lens_out, regime, engine._p(out), engine._p(ws),
                                                              ctypes.c_size_t(ws.numel()), engine._stream(dev)))
            return out.permute(0, 2, 1), new_state
