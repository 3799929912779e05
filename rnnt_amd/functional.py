"""Autograd-facing operators of the engine.

  rnnt_loss(...)        drop-in for torchaudio.functional.rnnt_loss as the reference calls it
                        (rnnt/model.py:35-41): same argument names, checks and error types.
  joint_logits(...)     the T x U joint expansion of reference rnnt/joint.py:32-39.
  joint_rnnt_loss(...)  the fused hot path: joint + loss, forward and backward in ONE engine
                        call; the (B,T,U+1,V) logits never leave the engine's workspace.
  fastemit_lambda / delay_penalty (both loss operators): FastEmit and the delay penalty, the
                        latency regularisers of streaming transducers.
  restrict_frames / restrict_left / restrict_right (both loss operators): the alignment-restricted
                        loss, "Ar-RNN-T" (DESIGN.md §4n): label u only within a window of frames around
                        a reference alignment, e.g. the `frames` of rnnt_align / joint_rnnt_align.
  rnnt_align(...), joint_rnnt_align(...)
                        forced alignment on the same lattice: the best path's
                        log-probability and the frame of every label; no autograd.
  ctc_loss(...), ctc_greedy_decode(...)
                        the CTC auxiliary head's loss and frame-wise decode on logits [N,T,V].
Every operator runs on the HIP engine; CPU tensors are rejected (no fallback).  The two CTC operators alone
also have a `backend="torch"` path with the same semantics (any device, float64): it is their oracle's carrier.
"""
import torch

from . import engine

_PAD_NEG = -1.0e30  # bias of padded vocabulary columns: exp() underflows to exactly 0
# bf16x3 route (pads V to a multiple of 128, so a lane's whole column group can be padding): -1e30 next to
# itself loses the softmax's max subtraction to fp32 rounding (ulp(1.44e30) = 7.6e22 -> exp2 overflows);
# -1e4 still underflows to exactly 0 against any real logit (> -9.9e3) and subtracts from itself exactly
_PAD_NEG_WIDE = -1.0e4


def _check_loss_args(T, U1, V, B, targets, logit_lengths, target_lengths, blank, reduction,
                     check_lengths):
    if reduction not in ("none", "mean", "sum"):
        raise ValueError('reduction should be one of "none", "mean", or "sum"')
    if blank < 0:
        blank = V + blank
    if not 0 <= blank < V:
        raise RuntimeError("blank must be within [0, logits.shape[-1])")
    if targets.dim() != 2:
        raise RuntimeError("targets must have 2 dimensions")
    if logit_lengths.dim() != 1 or target_lengths.dim() != 1:
        raise RuntimeError("logit_lengths and target_lengths must have 1 dimension")
    if targets.dtype != torch.int32:
        raise RuntimeError("targets must be int32 type")
    if logit_lengths.dtype != torch.int32 or target_lengths.dtype != torch.int32:
        raise RuntimeError("logit_lengths and target_lengths must be int32 type")
    if not (targets.is_contiguous() and logit_lengths.is_contiguous()
            and target_lengths.is_contiguous()):
        raise RuntimeError("targets, logit_lengths and target_lengths must be contiguous")
    if logit_lengths.shape[0] != B or target_lengths.shape[0] != B or targets.shape[0] != B:
        raise RuntimeError("batch dimension mismatch between logits, targets and lengths")
    if targets.shape[1] != U1 - 1:
        raise RuntimeError("targets must have max target length + 1 == logits.shape[2]")
    if check_lengths:
        # same host-side checks torchaudio performs (they synchronise, as torchaudio's do)
        if int(logit_lengths.max()) != T:
            raise RuntimeError("input length mismatch")
        if int(target_lengths.max()) + 1 != U1:
            raise RuntimeError("output length mismatch")
        if int(logit_lengths.min()) < 1 or int(target_lengths.min()) < 0:
            raise RuntimeError("lengths must be positive")
    return blank


def _check_restrict_args(restrict_frames, restrict_left, restrict_right, B, U, logit_lengths, target_lengths, check_lengths):
    """The alignment restriction's arguments -> (left, right).  Tensor and buffer checks always; under
    `check_lengths` (which synchronises already) the live entries too: for u < target_lengths[b], 0 <= frames[b,u] <=
    logit_lengths[b] - 1 and non-decreasing in u — such an alignment is itself a surviving path, so every cost is finite."""
    left, right = engine.check_restrict(restrict_frames, restrict_left, restrict_right, B, U)
    if check_lengths and U > 0:
        live = torch.arange(U, device=restrict_frames.device)[None, :] < target_lengths[:, None]
        f = restrict_frames.long()
        in_range = (f >= 0) & (f <= logit_lengths.long()[:, None] - 1)
        ordered = torch.ones_like(live)
        ordered[:, 1:] = f[:, 1:] >= f[:, :-1]
        if bool((live & ~in_range).any()):
            raise ValueError("restrict_frames: a live entry lies outside [0, logit_lengths[b] - 1]")
        if bool((live & ~ordered).any()):
            raise ValueError("restrict_frames: the live entries of an utterance must be non-decreasing")
    return left, right


class _RNNTLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, logit_lengths, target_lengths, blank, clamp, fastemit_lambda=0.0,
                delay_penalty=0.0, restrict=None):
        reg = (fastemit_lambda, delay_penalty) if restrict is not None or fastemit_lambda or delay_penalty else None
        costs, grad = engine._loss_fwd_bwd(logits, targets, logit_lengths, target_lengths, blank, clamp, ctx.needs_input_grad[0],
                                           reg, restrict)
        ctx.save_for_backward(grad)
        return costs

    @staticmethod
    def backward(ctx, grad_costs):
        (grad,) = ctx.saved_tensors
        if grad is None:
            return None, None, None, None, None, None, None, None, None
        return grad * grad_costs.view(-1, 1, 1, 1), None, None, None, None, None, None, None, None


def rnnt_loss(logits, targets, logit_lengths, target_lengths, blank=-1, clamp=-1, reduction="mean",
              fused_log_softmax=True, check_lengths=True, fastemit_lambda=0.0, delay_penalty=0.0,
              restrict_frames=None, restrict_left=0, restrict_right=0):
    """Transducer loss on materialised logits [B,T,U+1,V] (reference rnnt/model.py:35-41).
    `fastemit_lambda` / `delay_penalty` (finite, >= 0): FastEmit adds lambda E (p_k - [k = y]) to the
    gradient of every label cell and leaves the costs unchanged; the delay penalty runs the lattice on
    lp_emit + delta ((T_b - 1) / 2 - t) and returns the penalised costs.  `clamp` applies to the regularised gradient.
    `restrict_frames` (int32 [B,U] on the device, e.g. rnnt_align's frames; None: no restriction) with `restrict_left` /
    `restrict_right` (ints >= 0, in frames): label u of utterance b is emitted only at frames
    restrict_frames[b,u] - restrict_left .. restrict_frames[b,u] + restrict_right; costs and gradients are those of the
    paths that remain (an utterance without one: cost +inf, zero gradient).  Entries at u >= target_lengths[b] are ignored;
    under `check_lengths` the live ones must lie in [0, logit_lengths[b] - 1] and not decrease (ValueError)."""
    fastemit_lambda, delay_penalty = engine.check_reg(fastemit_lambda, delay_penalty)
    if not fused_log_softmax:
        raise NotImplementedError("rnnt_amd.rnnt_loss only implements fused_log_softmax=True")
    if logits.dim() != 4:
        raise RuntimeError("logits must have 4 dimensions")
    if logits.dtype != torch.float32:
        raise RuntimeError("logits must be float32 type")
    if not logits.is_contiguous():
        raise RuntimeError("logits must be contiguous")
    B, T, U1, V = logits.shape
    blank = _check_loss_args(T, U1, V, B, targets, logit_lengths, target_lengths, blank, reduction,
                             check_lengths)
    restrict = None
    if restrict_frames is not None:
        restrict = (restrict_frames,) + _check_restrict_args(restrict_frames, restrict_left, restrict_right, B, U1 - 1,
                                                             logit_lengths, target_lengths, check_lengths)
    if V % 4 != 0:
        pad = 4 - V % 4
        logits = torch.nn.functional.pad(logits, (0, pad), value=_PAD_NEG)
    costs = _RNNTLoss.apply(logits, targets, logit_lengths, target_lengths, blank, float(clamp), fastemit_lambda,
                            delay_penalty, restrict)
    if reduction == "mean":
        return costs.mean()
    if reduction == "sum":
        return costs.sum()
    return costs


# ---- CTC auxiliary head
def _ctc_check_args(logits, targets, logit_lengths, target_lengths, blank, check_lengths):
    if logits.dim() != 3:
        raise RuntimeError("logits must have 3 dimensions [N, T, V]")
    N, T, V = logits.shape
    if N < 1 or T < 1 or V < 1:
        raise RuntimeError("logits must not be empty")
    if blank < 0:
        blank = V + blank
    if not 0 <= blank < V:
        raise RuntimeError("blank must be within [0, logits.shape[-1])")
    if targets is not None:
        if targets.dim() != 2 or targets.shape[0] != N:
            raise RuntimeError("targets must be [N, U]")
        if target_lengths.dim() != 1 or target_lengths.shape[0] != N:
            raise RuntimeError("target_lengths must be [N]")
        if targets.dtype != torch.int32 or target_lengths.dtype != torch.int32:
            raise RuntimeError("targets and target_lengths must be int32 type")
    if logit_lengths.dim() != 1 or logit_lengths.shape[0] != N:
        raise RuntimeError("logit_lengths must be [N]")
    if logit_lengths.dtype != torch.int32:
        raise RuntimeError("logit_lengths must be int32 type")
    if check_lengths:  # (host-side: these synchronise, as rnnt_loss's do)
        if int(logit_lengths.min()) < 1 or int(logit_lengths.max()) > T:
            raise RuntimeError("logit_lengths must lie in [1, T]")
        if targets is not None and (int(target_lengths.min()) < 0 or int(target_lengths.max()) > targets.shape[1]):
            raise RuntimeError("target_lengths must lie in [0, U]")
    return blank


def _ctc_infeasible(targets, logit_lengths, target_lengths, T):
    """[N] bool: no frame labelling of T_n frames collapses to the utterance's labels, T_n < U_n + (adjacent equal labels); the
    lengths clamped as the kernels clamp them."""
    N, U = targets.shape
    Tn = logit_lengths.long().clamp(1, T)
    Un = target_lengths.long().clamp(0, U)
    if U < 2:
        return Tn < Un
    pair_live = torch.arange(1, U, device=targets.device)[None, :] < Un[:, None]
    repeats = ((targets[:, 1:] == targets[:, :-1]) & pair_live).sum(dim=1)
    return Tn < Un + repeats


def _ctc_costs_torch(logits, targets, logit_lengths, target_lengths, blank):
    """Per-utterance CTC costs by log_softmax + torch.nn.functional.ctc_loss with the engine's conventions: +inf (and, through
    the `where`, an exactly zero gradient) for an utterance without a valid path, frames t >= T_n and labels u >= U_n ignored
    whatever they hold.  Any device, float32 or float64."""
    N, T, V = logits.shape
    Tn = logit_lengths.long().clamp(1, T)
    Un = target_lengths.long().clamp(0, targets.shape[1])
    dead = torch.arange(T, device=logits.device)[None, :] >= Tn[:, None]
    lp = torch.log_softmax(logits.masked_fill(dead[:, :, None], 0.0), dim=-1).transpose(0, 1)
    tg = targets.long().clamp(0, V - 1)
    if tg.shape[1] == 0:
        tg = tg.new_zeros((N, 1))
    costs = torch.nn.functional.ctc_loss(lp, tg, Tn, Un, blank=blank, reduction="none", zero_infinity=True)
    return torch.where(_ctc_infeasible(tg[:, :targets.shape[1]], Tn, Un, T), costs.new_full((), float("inf")), costs)


class _CTCLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, logit_lengths, target_lengths, blank):
        costs, grad = engine.ctc_loss_fwd_bwd(logits, targets, logit_lengths, target_lengths, blank,
                                              want_grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(grad)
        return costs

    @staticmethod
    def backward(ctx, grad_costs):
        (grad,) = ctx.saved_tensors
        if grad is None:
            return None, None, None, None, None
        return grad * grad_costs.view(-1, 1, 1), None, None, None, None


def _ctc_backend(backend, logits, U, what):
    if backend not in ("auto", "engine", "torch"):
        raise ValueError('backend should be one of "auto", "engine", or "torch"')
    refusal = None
    if not logits.is_cuda:
        refusal = "the engine has no CPU path"
    elif logits.dtype != torch.float32:
        refusal = f"the engine takes float32 logits (got {logits.dtype})"
    elif U > engine.CTC_MAX_U:
        refusal = f"U={U} exceeds the engine's {engine.CTC_MAX_U} labels"
    if backend == "engine" and refusal is not None:
        raise RuntimeError(f"rnnt_amd.{what}(backend=\"engine\"): {refusal}")
    return "torch" if backend == "torch" or refusal is not None else "engine"


def ctc_loss(logits, targets, logit_lengths, target_lengths, blank=-1, reduction="mean", zero_infinity=False,
             check_lengths=True, backend="auto"):
    """CTC loss of logits [N,T,V] (batch first, log-softmax fused) against targets [N,U] int32; lengths int32 [N].
    `reduction`: "none" (the per-utterance costs -log P), "sum", or "mean" = the MEAN OF THE PER-UTTERANCE COSTS, as rnnt_loss
    defines it here, so that (1 - w) rnnt + w ctc mixes like for like — NOT torch.nn.functional.ctc_loss's mean, which divides
    each cost by its target length first.  An utterance no frame labelling can produce (T_n < U_n + its adjacent equal labels)
    has cost +inf and an exactly zero gradient (the alignment-restricted loss's convention); `zero_infinity` also sets that cost
    to 0.  Frames t >= logit_lengths[n] and labels u >= target_lengths[n] are ignored whatever they hold.
    `backend`: "engine" = rnnt_engine_ctc_loss_fwd_bwd (float32 HIP tensors, U <= 1023; raises otherwise),
    "torch" = log_softmax + torch.nn.functional.ctc_loss with the same semantics (any device, float64 too), "auto" = the engine
    where it runs.  Differentiable once, in the logits."""
    if reduction not in ("none", "mean", "sum"):
        raise ValueError('reduction should be one of "none", "mean", or "sum"')
    blank = _ctc_check_args(logits, targets, logit_lengths, target_lengths, blank, check_lengths)
    if _ctc_backend(backend, logits, targets.shape[1], "ctc_loss") == "engine":
        V = logits.shape[-1]
        x = logits.contiguous()
        if V % 4 != 0:
            x = torch.nn.functional.pad(x, (0, 4 - V % 4), value=_PAD_NEG)
        costs = _CTCLoss.apply(x, targets.contiguous(), logit_lengths.contiguous(), target_lengths.contiguous(), blank)
    else:
        costs = _ctc_costs_torch(logits, targets, logit_lengths, target_lengths, blank)
    if zero_infinity:
        costs = torch.where(costs == float("inf"), torch.zeros_like(costs), costs)
    if reduction == "mean":
        return costs.mean()
    if reduction == "sum":
        return costs.sum()
    return costs


def _ctc_collapse(frames, blank):
    out, prev = [], None
    for tok in frames:
        if tok != blank and tok != prev:
            out.append(tok)
        prev = tok
    return out


@torch.no_grad()
def ctc_greedy_decode(logits, logit_lengths, blank=-1, backend="auto"):
    """CTC greedy decode of logits [N,T,V]: per frame t < logit_lengths[n] the argmax (lowest index on ties), then frames equal
    to their predecessor and blanks are dropped.  Returns a list of N token lists; ONE host synchronisation per call.
    `backend` as ctc_loss's: "engine" = rnnt_engine_ctc_greedy_decode (two launches for the whole batch), "torch" = argmax on
    the tensors' device and the collapse on the host."""
    blank = _ctc_check_args(logits, None, logit_lengths, None, blank, False)
    N, T, V = logits.shape
    if _ctc_backend(backend, logits, 0, "ctc_greedy_decode") == "engine":
        x = logits.detach().contiguous()
        if V % 4 != 0:
            x = torch.nn.functional.pad(x, (0, 4 - V % 4), value=_PAD_NEG)
        tokens, counts = engine.ctc_greedy_decode(x, logit_lengths.contiguous(), blank)
        host = torch.cat((counts[:, None], tokens), dim=1).tolist()  # the call's one synchronisation
        return [row[1:1 + row[0]] for row in host]
    best = torch.cat((logit_lengths.long().clamp(1, T)[:, None], logits.argmax(dim=-1)), dim=1).tolist()
    return [_ctc_collapse(row[1:1 + row[0]], blank) for row in best]


def _pad_hv(enc, pred, W, bias, mult=4):
    """Zero-pad H and V to multiples of `mult` (engine requirement: 4 on the fp32 route, 128 on the
    bf16x3 route); padded vocabulary rows get bias -1e30 so they carry zero probability and zero
    gradient, padded hidden columns are tanh(0) = 0 against zero weights."""
    H, V = W.shape[1], W.shape[0]
    ph, pv = (-H) % mult, (-V) % mult
    if ph:
        enc = torch.nn.functional.pad(enc, (0, ph))
        pred = torch.nn.functional.pad(pred, (0, ph))
        W = torch.nn.functional.pad(W, (0, ph))
    if pv:
        W = torch.nn.functional.pad(W, (0, 0, 0, pv))
        bias = torch.nn.functional.pad(bias, (0, pv), value=_PAD_NEG if mult <= 4 else _PAD_NEG_WIDE)
    return enc, pred, W, bias, H, V


class _JointLogits(torch.autograd.Function):
    """Unfused joint: forward and backward both on the engine (rnnt_engine_joint_fwd /
    rnnt_engine_joint_bwd).  The backward is reached when a caller keeps the (B,T,U+1,V) logits and
    the loss as two calls — e.g. a maintainer who swaps only rnnt/joint.py — and differentiates
    through them; the training hot path is _JointRNNTLoss."""

    @staticmethod
    def forward(ctx, enc, pred, W, bias):
        ctx.save_for_backward(enc, pred, W)
        return engine.joint_fwd(enc, pred, W, bias)

    @staticmethod
    def backward(ctx, G):
        enc, pred, W = ctx.saved_tensors
        return engine.joint_bwd(enc, pred, W, G)


def joint_logits(enc, pred, W, bias):
    """logits = tanh(enc.unsqueeze(2) + pred.unsqueeze(1)) @ W.T + bias."""
    if any(t.dtype != torch.float32 for t in (enc, pred, W, bias)):
        raise RuntimeError("rnnt_amd.joint_logits: float32 inputs required")
    enc_p, pred_p, W_p, bias_p, H, V = _pad_hv(enc, pred, W, bias)
    out = _JointLogits.apply(enc_p, pred_p, W_p, bias_p)
    return out[..., :V] if out.shape[-1] != V else out


class _Linear(torch.autograd.Function):
    """y = x W^T + b on the engine (rnnt_engine_linear_x2_* on the f16x2 pipes from engine.LINEAR_X2_MIN_MKN of work, the fp32-MFMA
    small-GEMM kernels rnnt_engine_linear_* below): the joint's optional input projections audio_ln / text_ln (reference
    rnnt/joint.py:8-12,26-30)."""

    @staticmethod
    def forward(ctx, x, W, bias, backend):
        ctx.save_for_backward(x, W)
        ctx.backend = backend
        return engine.linear_fwd(x, W, bias, backend=backend)

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        dx, dW, db = engine.linear_bwd(x, W, dy, need_dx=ctx.needs_input_grad[0], backend=ctx.backend)
        return dx, dW, db, None


def linear(x, W, bias, backend="auto"):
    """torch.nn.functional.linear(x, W, bias) for [.., K] fp32 HIP tensors with K % 4 == 0 and
    N % 4 == 0, forward and backward on the engine.  A permuted (N,C,L)->(N,L,C) encoder view
    (reference rnnt/model.py:28) is gathered into rows once (the transposing copy the joint needs
    anyway)."""
    if x.dtype != torch.float32 or W.dtype != torch.float32 or bias.dtype != torch.float32:
        raise RuntimeError("rnnt_amd.linear: float32 tensors required")
    return _Linear.apply(x, W, bias, backend)


class _JointRNNTLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, pred, W, bias, targets, logit_lengths, target_lengths, blank, scale,
                dtype, need_grad=True, fastemit_lambda=0.0, delay_penalty=0.0, restrict=None):
        # need_grad False (torch.no_grad() / nothing requires grad): forward kernels only, and FastEmit changes no cost.  The
        # regularised entries only where a regulariser is set (or the lattice is restricted): the plain ones keep the f16x2 flush rule
        regularised = (fastemit_lambda or delay_penalty) if need_grad else delay_penalty
        costs, *grads = engine._fused(enc, pred.contiguous(), W.contiguous(), bias.contiguous(), targets, logit_lengths,
                                      target_lengths, blank, dtype, scale if need_grad else None,
                                      (fastemit_lambda, delay_penalty) if restrict is not None or regularised else None, restrict)
        if need_grad:
            ctx.save_for_backward(*grads)
            ctx.scale = scale
        ctx.mark_non_differentiable(costs)
        return costs.sum() * scale, costs

    @staticmethod
    def backward(ctx, grad_loss, _grad_costs):
        ge, gp, gW, gb = ctx.saved_tensors
        return (ge * grad_loss, gp * grad_loss, gW * grad_loss, gb * grad_loss,
                None, None, None, None, None, None, None, None, None, None)


def joint_rnnt_loss(enc, pred, W, bias, targets, logit_lengths, target_lengths, blank=-1,
                    reduction="mean", check_lengths=True, return_costs=False, grad_scale=None,
                    dtype=engine.DEFAULT_DTYPE, fastemit_lambda=0.0, delay_penalty=0.0,
                    restrict_frames=None, restrict_left=0, restrict_right=0):
    """Fused replacement of
        logits = joint(enc, pred)                      # reference rnnt/model.py:32
        loss = torchaudio.functional.rnnt_loss(logits, targets, ..., blank, clamp=-1, reduction)
    (rnnt/model.py:35-41) including everything loss.backward() (rnnt/train.py:134) sends to
    enc, pred, W and bias.  enc [B,T,H] (any strides), pred [B,U+1,H], W [V,H], bias [V].
    `grad_scale` overrides the reduction factor (1/B_global when the batch is sharded).
    `dtype` defaults to engine.DEFAULT_DTYPE — the arithmetic RNNTModel.forward ships ("f16x2": fp32-class, 22-bit operands,
    three fp16 MFMA products per fp32 product); "fp32" = exact fp32 products.
    `dtype="bf16"` (BASELINE config 3): tensors stay fp32, the three GEMMs run on bf16-rounded
    operands with fp32 accumulation; needs H % 128 == 0, V % 128 == 0.
    `dtype="bf16x3"`: fp32-accurate results (same 1e-4 bar as "fp32") from the bf16 matrix pipes — operands
    split three ways, six bf16 products per fp32 product (include/rnnt_engine.h RNNT_DTYPE_F32_BF16X3);
    any H, V (zero-padded to multiples of 128 here).
    `fastemit_lambda` / `delay_penalty` (finite, >= 0): the latency regularisers, as rnnt_loss takes them;
    both are per utterance and FastEmit is linear in `grad_scale`, so sharded calls still sum to the full batch's gradients.
    `restrict_frames` / `restrict_left` / `restrict_right`: the alignment-restricted loss, as rnnt_loss takes it;
    `restrict_frames` is what joint_rnnt_align returns as `frames`.  Per utterance as well: shards sum to the full batch."""
    fastemit_lambda, delay_penalty = engine.check_reg(fastemit_lambda, delay_penalty)
    if reduction not in ("mean", "sum"):
        if reduction == "none":
            raise NotImplementedError(
                'joint_rnnt_loss supports reduction "mean" and "sum"; use joint_logits + rnnt_loss '
                'for reduction="none"')
        raise ValueError('reduction should be one of "none", "mean", or "sum"')
    if enc.dim() != 3 or pred.dim() != 3:
        raise RuntimeError("enc and pred must have 3 dimensions")
    if any(t.dtype != torch.float32 for t in (enc, pred, W, bias)):
        raise RuntimeError("enc, pred, W and bias must be float32 type")
    B, T, _ = enc.shape
    U1 = pred.shape[1]
    V = W.shape[0]
    if pred.shape[0] != B or pred.shape[2] != enc.shape[2] or W.shape[1] != enc.shape[2]:
        raise RuntimeError("enc / pred / W shape mismatch")
    blank = _check_loss_args(T, U1, V, B, targets, logit_lengths, target_lengths, blank, reduction,
                             check_lengths)
    code = engine.dtype_code(dtype)
    if code == engine.DTYPE_BF16:  # no host-side padding on this route: the C side validates
        enc_p, pred_p, W_p, bias_p = enc, pred, W, bias
    else:
        enc_p, pred_p, W_p, bias_p, H, V = _pad_hv(enc, pred, W, bias, 128 if code in (engine.DTYPE_F32_BF16X3, engine.DTYPE_F32_F16X2) else 4)
    scale = float(grad_scale) if grad_scale is not None else (1.0 / B if reduction == "mean" else 1.0)
    # validation / eval (reference rnnt/train.py:170-201 runs the model under no_grad): costs only
    need_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (enc, pred, W, bias))
    restrict = None
    if restrict_frames is not None:
        restrict = (restrict_frames,) + _check_restrict_args(restrict_frames, restrict_left, restrict_right, B, U1 - 1,
                                                             logit_lengths, target_lengths, check_lengths)
    loss, costs = _JointRNNTLoss.apply(enc_p, pred_p, W_p, bias_p, targets, logit_lengths,
                                       target_lengths, blank, scale, code, need_grad, fastemit_lambda, delay_penalty, restrict)
    return (loss, costs) if return_costs else loss


def _align_checks(T, U1, V, B, targets, logit_lengths, target_lengths, blank, check_lengths):
    return _check_loss_args(T, U1, V, B, targets, logit_lengths, target_lengths, blank, "mean", check_lengths)


def rnnt_align(logits, targets, logit_lengths, target_lengths, blank=-1, check_lengths=True):
    """Forced alignment on materialised logits [B,T,U+1,V]: the best path through the lattice rnnt_loss sums
    over.  Returns (scores [B] float32: the best path's log-probability, frames [B,U] int32: the frame at which label u is
    emitted, -1 for u >= target_lengths[b]).  Same argument checks and errors as rnnt_loss; no autograd; enqueues only
    (apart from the check_lengths host checks)."""
    if logits.dim() != 4:
        raise RuntimeError("logits must have 4 dimensions")
    if logits.dtype != torch.float32:
        raise RuntimeError("logits must be float32 type")
    if not logits.is_contiguous():
        raise RuntimeError("logits must be contiguous")
    B, T, U1, V = logits.shape
    blank = _align_checks(T, U1, V, B, targets, logit_lengths, target_lengths, blank, check_lengths)
    logits = logits.detach()
    if V % 4 != 0:
        logits = torch.nn.functional.pad(logits, (0, 4 - V % 4), value=_PAD_NEG)
    return engine.align(logits, targets, logit_lengths, target_lengths, blank)


def joint_rnnt_align(enc, pred, W, bias, targets, logit_lengths, target_lengths, blank=-1,
                     dtype=engine.DEFAULT_DTYPE, check_lengths=True):
    """Forced alignment of the fused path: the joint GEMM of joint_rnnt_loss on the same route, with H and V
    padded exactly as there, then the best path through the lattice.  Returns (scores [B] float32, frames [B,U] int32) as
    rnnt_align does; the (B,T,U+1,V) logits never leave the engine's workspace.  No autograd."""
    if enc.dim() != 3 or pred.dim() != 3:
        raise RuntimeError("enc and pred must have 3 dimensions")
    if any(t.dtype != torch.float32 for t in (enc, pred, W, bias)):
        raise RuntimeError("enc, pred, W and bias must be float32 type")
    B, T, _ = enc.shape
    U1 = pred.shape[1]
    V = W.shape[0]
    if pred.shape[0] != B or pred.shape[2] != enc.shape[2] or W.shape[1] != enc.shape[2]:
        raise RuntimeError("enc / pred / W shape mismatch")
    blank = _align_checks(T, U1, V, B, targets, logit_lengths, target_lengths, blank, check_lengths)
    code = engine.dtype_code(dtype)
    enc, pred, W, bias = enc.detach(), pred.detach(), W.detach(), bias.detach()
    if code != engine.DTYPE_BF16:  # bf16: no host-side padding, the C side validates (as joint_rnnt_loss)
        enc, pred, W, bias, _, _ = _pad_hv(enc, pred, W, bias, 128 if code in (engine.DTYPE_F32_BF16X3, engine.DTYPE_F32_F16X2) else 4)
    return engine.joint_align(enc, pred.contiguous(), W.contiguous(), bias.contiguous(), targets, logit_lengths,
                              target_lengths, blank, dtype=code)
