"""CTCHead: the CTC auxiliary head of a transducer — one Linear(H, V) on the encoder output, the CTC loss
of hybrid CTC / RNN-T training and a frame-wise greedy decode, each on the HIP engine where it runs.  The reference has no
CTC branch; RNNTModel takes the head as `ctc_head` with `ctc_weight`.
"""
import torch

from . import functional as F_amd


class CTCHead(torch.nn.Module):
    def __init__(self, in_features: int, vocab_size: int):
        super().__init__()
        self.linear = torch.nn.Linear(in_features, vocab_size)

    @property
    def vocab_size(self) -> int:
        return self.linear.out_features

    def forward(self, audio_features: torch.Tensor) -> torch.Tensor:
        """audio_features [N,T,H] (any strides: the permuted encoder view works) -> logits [N,T,V].  float32 HIP tensors: the
        projection and its backward are the engine's GEMMs (rnnt_amd.functional.linear; sizes that are no multiple of 4 are
        zero-padded around the call); anything else — the CPU, float64 — is torch's linear."""
        lin = self.linear
        if not (audio_features.is_cuda and audio_features.dtype == torch.float32 and lin.weight.dtype == torch.float32):
            return lin(audio_features)
        W, b, x = lin.weight, lin.bias, audio_features
        pk, pn = (-lin.in_features) % 4, (-lin.out_features) % 4
        if pk:
            x, W = torch.nn.functional.pad(x, (0, pk)), torch.nn.functional.pad(W, (0, pk))
        if pn:
            W, b = torch.nn.functional.pad(W, (0, 0, 0, pn)), torch.nn.functional.pad(b, (0, pn))
        y = F_amd.linear(x, W, b)
        return y[..., :lin.out_features] if pn else y

    def loss(self, audio_features, targets, logit_lengths, target_lengths, blank=-1, reduction="mean", **kw):
        """rnnt_amd.ctc_loss of the head's logits; keywords (zero_infinity, check_lengths, backend) go to it."""
        return F_amd.ctc_loss(self(audio_features), targets, logit_lengths, target_lengths, blank=blank, reduction=reduction, **kw)

    @torch.no_grad()
    def greedy_decode(self, audio_features, logit_lengths, blank=-1, backend="auto"):
        """rnnt_amd.ctc_greedy_decode of the head's logits: a list of token lists, one host synchronisation."""
        return F_amd.ctc_greedy_decode(self(audio_features), logit_lengths, blank=blank, backend=backend)
