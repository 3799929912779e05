"""Generate tests/golden/decode_lstm_*.npz by importing the REFERENCE's own rnnt.predictor.LSTMPredictor and rnnt.joint.JointNetwork
(reference rnnt/predictor.py:93-186, rnnt/joint.py) and decoding greedily with them on the CPU in float64.

Run on the CPU where the reference is checked out (it never travels to the GPU box):
    PYTHONPATH=<reference checkout> python tests/golden/make_golden_decode_lstm.py

The decode below follows the control flow of the reference's greedy decode for this predictor (rnnt/model.py:45-87: start from the
blank, take the argmax of the joint for the current frame, a blank or ten labels at a frame move to the next frame, a label goes
through the predictor with the carried state, stop at the last frame or at max_length entries) and records the gap between the two
largest logits of every decision.  Stored per case: `dims` (S, O, E, L, Hd, layer_norm, H, V, text_ln), `eps`, both state dicts
(parameters drawn in float32, LayerNorm affines moved away from the identity, the blank's bias raised by one so that the decode
moves through the frames), the frames (1, H, T; float32 values), `max_length`, the token list and the smallest gap.  A seed is
kept only if that gap is above 4e-3, four times the margin the tests ask for.  Fixtures are data (arrays); no reference source is
copied.  Small widths only: each file stays far below the repository's size limit.
"""
import os

import numpy as np
import torch

from rnnt.joint import JointNetwork  # reference, via PYTHONPATH
from rnnt.predictor import LSTMPredictor

OUT = os.path.dirname(os.path.abspath(__file__))
EPS = 1e-3
CASES = {
    # name: (S, O, E, L, Hd, layer_norm, H, V, text_ln, T, max_length)
    "decode_lstm_ln": (16, 32, 16, 2, 32, True, 32, 16, False, 14, 200),
    "decode_lstm_text_noln": (20, 16, 20, 1, 36, False, 24, 20, True, 12, 24),  # text_ln with O != H, x2g bias, a cap that binds
}


@torch.no_grad()
def decode(pred, joint, frames, max_length):
    audio = frames.permute(0, 2, 1)
    blank = joint.blank_idx
    tokens, gaps = [blank], []
    feats, _, state = pred(torch.tensor([[blank]]), torch.tensor([1]))
    t = at_frame = 0
    while t < audio.shape[1] and len(tokens) < max_length:
        logits = joint.single_forward(audio[:, t, :], feats[:, -1, :])[0]
        top = logits.topk(2).values
        tok = int(logits.argmax())
        if at_frame < 10:
            gaps.append(float(top[0] - top[1]))  # (the eleventh look at a frame decides nothing: the frame ends whatever it says)
        if tok == blank or at_frame >= 10:
            t, at_frame = t + 1, 0
            continue
        tokens.append(tok)
        feats, _, state = pred(torch.tensor([[tok]]), torch.tensor([len(tokens)]), state)
        at_frame += 1
    return tokens[1:], min(gaps)


def make(name, S, O, E, L, Hd, ln, H, V, text, T, max_length):
    for seed in range(1, 200):
        torch.manual_seed(seed)
        pred = LSTMPredictor(S, O, E, L, Hd, lstm_layer_norm=ln, lstm_layer_norm_epsilon=EPS, lstm_dropout=0.3).eval()
        joint = JointNetwork(-1, O if text else -1, H, V).eval()
        with torch.no_grad():
            for n_, p in pred.named_parameters():
                if "norm" in n_:
                    p.add_(torch.randn_like(p) * 0.2)
            joint.joint_ln.bias[joint.blank_idx] += 1.0
        frames = torch.randn(1, H, T) * 2.0
        p64 = LSTMPredictor(S, O, E, L, Hd, lstm_layer_norm=ln, lstm_layer_norm_epsilon=EPS, lstm_dropout=0.3).double().eval()
        p64.load_state_dict({k: v.double() for k, v in pred.state_dict().items()})
        j64 = JointNetwork(-1, O if text else -1, H, V).double().eval()
        j64.load_state_dict({k: v.double() for k, v in joint.state_dict().items()})
        tokens, gap = decode(p64, j64, frames.double(), max_length)
        if gap > 4e-3 and len(tokens) >= 6 and len(set(tokens)) >= 3:
            break
    else:
        raise SystemExit(f"{name}: no seed gives a decode clear of near-ties")
    out = {"dims": np.array([S, O, E, L, Hd, int(ln), H, V, int(text)]), "eps": np.array(EPS), "seed": np.array(seed),
           "frames": frames.numpy(), "max_length": np.array(max_length), "tokens": np.array(tokens, dtype=np.int64), "gap": np.array(gap),
           "pred_keys": np.array(list(pred.state_dict().keys())), "joint_keys": np.array(list(joint.state_dict().keys()))}
    for k, v in pred.state_dict().items():
        out["pred__" + k.replace(".", "__")] = v.numpy()
    for k, v in joint.state_dict().items():
        out["joint__" + k.replace(".", "__")] = v.numpy()
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "seed", seed, "gap %.3g" % gap, len(tokens), "labels,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    for k, v in CASES.items():
        make(k, *v)
