"""JointNetwork with the constructor, attribute names and state-dict keys of the reference
(rnnt/joint.py:4-55) whose batch `forward` runs on the HIP engine.

`forward` (the T x U expansion used in training, reference joint.py:25-39) calls the engine's
joint GEMM; `fused_loss` is the entry RNNTModel uses so that the logits are never
materialised outside the engine; `single_forward` (decode/export, joint.py:44-55) is not on
the hot path and stays as plain torch ops so TorchScript/ONNX export keeps working.
"""
import torch

from . import functional as F_amd
from .engine import DEFAULT_DTYPE as engine_default_dtype


class JointNetwork(torch.nn.Module):
    def __init__(self, audio_features: int, text_features: int, hidden_features: int,
                 num_classes: int):
        super().__init__()
        # optional input projections exist only when the feature sizes are given, exactly as
        # the reference decides it (joint.py:8-12); hasattr() is the switch at call time.
        if audio_features > 0:
            self.audio_ln = torch.nn.Linear(audio_features, hidden_features)
        if text_features > 0:
            self.text_ln = torch.nn.Linear(text_features, hidden_features)
        self.activation = torch.tanh
        self.joint_ln = torch.nn.Linear(hidden_features, num_classes)
        self.blank_idx = num_classes - 1

    # The optional input projections are plain GEMMs ([B*T, Fa] x [Fa, H]: 32 000 rows at the headline config).
    # "auto" (default since round 5): from engine.LINEAR_X2_MIN_MKN rows x in x out (6 432 rows at 1024 x 1024; feature sizes multiples of 128) they run on the
    # ENGINE — rnnt_engine_linear_x2_fwd / _bwd: the joint forward's pipeline as a plain GEMM on the f16x2 matrix pipes for y and dx,
    # the joint's dW kernel for dW / db (tools/bench_linear.py: ahead of rocBLAS / hipBLASLt's fp32 GEMM there) — and through
    # torch.nn.functional.linear (the library GEMM, ahead of any engine kernel at a few hundred rows) below;
    # "engine": always the engine (f16x2 pipes where the shape allows, else the fp32-MFMA small-GEMM kernels rnnt_engine_linear_*);
    # "library": always torch.
    projection_backend = "auto"

    def _linear(self, layer, x):
        from . import engine
        ok = (x.is_cuda and x.dtype == torch.float32 and layer.in_features % 4 == 0 and layer.out_features % 4 == 0
              and not torch.jit.is_tracing())
        if ok and self.projection_backend == "engine":
            return F_amd.linear(x, layer.weight, layer.bias)
        if ok and self.projection_backend == "auto" and engine.linear_x2_preferred(x.numel() // x.shape[-1], layer.in_features, layer.out_features):
            return F_amd.linear(x, layer.weight, layer.bias, backend="x2")
        return layer(x)

    def _project(self, audio_frame, text_frame):
        if hasattr(self, "audio_ln"):
            audio_frame = self._linear(self.audio_ln, audio_frame)
        if hasattr(self, "text_ln"):
            text_frame = self._linear(self.text_ln, text_frame)
        return audio_frame, text_frame

    def forward(self, audio_frame, text_frame):
        """audio_frame [N,T,Fa], text_frame [N,U+1,Ft] -> logits [N,T,U+1,V]."""
        audio_frame, text_frame = self._project(audio_frame, text_frame)
        return F_amd.joint_logits(audio_frame, text_frame, self.joint_ln.weight, self.joint_ln.bias)

    # Arithmetic of the fused training step (RNNTModel.forward): "f16x2" = fp32-CLASS results from the fp16 matrix pipes
    # (include/rnnt_engine.h RNNT_DTYPE_F32_F16X2: operands scaled by powers of two and split into two fp16 pieces = 22
    # significant bits, three MFMA products per fp32 product; the fp32 route's 1e-4 parity bar with its measured error class,
    # ~2.3x its speed); "bf16x3" = the same from six bf16 products of 3-way split operands (24 bits, ~1.5x); "fp32" = exact
    # fp32 products; "bf16" = bf16-rounded operands (BASELINE config 3; not the reference's arithmetic).
    compute_dtype = engine_default_dtype

    def fused_loss(self, audio_frame, text_frame, targets, logit_lengths, target_lengths,
                   blank=-1, reduction="mean", **kw):
        """joint + transducer loss in one engine call (reference model.py:32-41).  Keywords go to joint_rnnt_loss: the latency
        regularisers (fastemit_lambda, delay_penalty) and the alignment restriction (restrict_frames, restrict_left,
        restrict_right) among them."""
        kw.setdefault("dtype", self.compute_dtype)
        audio_frame, text_frame = self._project(audio_frame, text_frame)
        return F_amd.joint_rnnt_loss(audio_frame, text_frame, self.joint_ln.weight,
                                     self.joint_ln.bias, targets, logit_lengths, target_lengths,
                                     blank=blank, reduction=reduction, **kw)

    def align(self, audio_frame, text_frame, targets, logit_lengths, target_lengths, blank=-1, **kw):
        """Forced alignment of the fused path: the inputs of fused_loss (audio_ln / text_ln applied the same way,
        compute_dtype unless `dtype` is given) -> (scores [N] float32, frames [N,U] int32)."""
        kw.setdefault("dtype", self.compute_dtype)
        audio_frame, text_frame = self._project(audio_frame, text_frame)
        return F_amd.joint_rnnt_align(audio_frame, text_frame, self.joint_ln.weight, self.joint_ln.bias, targets,
                                      logit_lengths, target_lengths, blank=blank, **kw)

    def greedy_scan(self, audio_frames, text_frame, t0, nframes):
        """Decode helper (reference rnnt/model.py:108-125): argmax of single_forward for frames
        t0 .. t0+nframes-1 of `audio_frames` [T,H] (ALREADY projected by audio_ln) against one
        predictor frame `text_frame` [Ft], reduced on the device to (first non-blank frame, token).
        Returns the engine's int32 tensor [2+nframes]; the caller syncs once per block."""
        from . import engine
        if hasattr(self, "text_ln"):
            text_frame = self.text_ln(text_frame)
        return engine.greedy_scan(audio_frames, text_frame, self.joint_ln.weight, self.joint_ln.bias,
                                  t0, nframes, self.blank_idx)

    def single_forward(self, audio_frame, text_frame):
        """One (audio, text) frame pair at a time: greedy decode and export (joint.py:44-55)."""
        audio_frame, text_frame = self._project(audio_frame, text_frame)
        return self.joint_ln(self.activation(audio_frame + text_frame))
