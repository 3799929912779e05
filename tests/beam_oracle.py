"""float64 numpy restatement of the beam search of RNNTModel.beam_search / rnnt_engine_beam_decode.

TEST INFRASTRUCTURE ONLY.  Built on oracle.decode_oracle.single_forward (rnnt/joint.py:44-55) and oracle.predictor_oracle.forward
(rnnt/predictor.py:211-229, eval mode).  The search:
    beam = [([], 0)]; for every frame t: all entries active, N = []
      rounds r = 0 .. m-1: per active (y, s): lp = log_softmax(single_forward(frame_t, predictor([blank] + y)[-1]))
          blank candidate (y, s + lp[blank]) joins N (logaddexp with N's entry of the same sequence, if any)
          label candidates (y + [k], s + lp[k]) for k != blank, only while len(y) < max_length - 1
          keep the best `beam` of N + labels: kept finished entries are N, kept labels the next round's actives; none -> frame over
      after round m-1 the kept labels are capped: next beam = N + capped, merged by sequence, sorted by score
Ties: finished first (in N's order), then parent (active order), then token id.  Besides the n-best list the oracle reports how many
candidates were pruned and the smallest score gap at any keep / drop boundary (and between neighbours of the final list): a device
result may be held to identical lists only where that gap is far above fp32 noise.
"""
import math

import numpy as np

from oracle import decode_oracle
from oracle import predictor_oracle as po


def _lae(a, b):
    hi, lo = max(a, b), min(a, b)
    return hi if lo == -math.inf else hi + math.log1p(math.exp(lo - hi))


def _log_softmax(x):
    mx = x.max()
    return x - mx - math.log(np.exp(x - mx).sum())


class Model:
    """frames [T, C] (before audio_ln) and the reference's state dicts -> log-prob rows lp(t, y) (float64, cached)."""

    def __init__(self, frames, pred_sd, joint_sd, eps=1e-5):
        self.pred_sd = {k: np.asarray(v, dtype=np.float64) for k, v in pred_sd.items()}
        jsd = {k: np.asarray(v, dtype=np.float64) for k, v in joint_sd.items()}
        frames = np.asarray(frames, dtype=np.float64)
        if "audio_ln.weight" in jsd:
            frames = frames @ jsd["audio_ln.weight"].T + jsd["audio_ln.bias"]
        self.frames = frames
        self.jsd = {k: v for k, v in jsd.items() if not k.startswith("audio_ln")}
        self.V = jsd["joint_ln.weight"].shape[0]
        self.blank = self.V - 1
        self.eps = eps
        self._feat = {}

    def feat(self, y):
        # the module is causal (k=3 then k=5 behind left zero padding): its last frame is a function of the last 7 tokens
        key = tuple([self.blank, *y][-7:])  # (shorter histories give shorter keys: their left padding differs)
        if key not in self._feat:
            out, _ = po.forward(np.asarray([key], dtype=np.int64), self.pred_sd, eps=self.eps)
            self._feat[key] = out[0, -1]
        return self._feat[key]

    def logits(self, t, y):
        return decode_oracle.single_forward(self.frames[t], self.feat(y), self.jsd)

    def lp(self, t, y):
        return _log_softmax(self.logits(t, y))


def beam_search(model, beam, max_length, max_per_frame=10):
    """-> (nbest [(tokens, score)] best first, pruned candidates, smallest gap at a keep / drop boundary or between neighbours of
    the result)."""
    blank, V = model.blank, model.V
    beam_list = [((), 0.0)]
    pruned, gap = 0, math.inf
    for t in range(model.frames.shape[0]):
        active, fin = beam_list, []
        for r in range(max_per_frame):
            lps = [model.lp(t, list(y)) for y, _ in active]
            for (y, s), lp in zip(active, lps):
                b = s + lp[blank]
                hit = next((e for e in fin if e[0] == y), None)
                if hit is not None:
                    hit[1] = _lae(hit[1], b)
                else:
                    fin.append([y, b])
            cands = [(s, 0, f, 0, y) for f, (y, s) in enumerate(fin)]
            for i, ((y, s), lp) in enumerate(zip(active, lps)):
                if len(y) >= max_length - 1:
                    continue
                cands += [(s + lp[k], 1, i, k, y + (k,)) for k in range(V) if k != blank]
            cands.sort(key=lambda c: (-c[0], c[1], c[2], c[3]))
            if len(cands) > beam:
                pruned += len(cands) - beam
                gap = min(gap, cands[beam - 1][0] - cands[beam][0])
            kept = cands[:beam]
            fin = [[c[4], c[0]] for c in kept if c[1] == 0]
            active = [(c[4], c[0]) for c in kept if c[1] == 1]
            if not active:
                break
        for y, s in active:
            hit = next((e for e in fin if e[0] == y), None)
            if hit is not None:
                hit[1] = _lae(hit[1], s)
            else:
                fin.append([y, s])
        order = sorted(range(len(fin)), key=lambda i: (-fin[i][1], i))
        beam_list = [(fin[i][0], fin[i][1]) for i in order]
    for a, b in zip(beam_list, beam_list[1:]):
        gap = min(gap, a[1] - b[1])
    return [(list(y), float(s)) for y, s in beam_list], pruned, gap


def lattice_logits(model, y):
    """logits [T, U+1, V] of target sequence y: row (t, u) = single_forward(frame_t, predictor([blank] + y[:u])[-1]) — the input of
    oracle.brute_force.nll_bruteforce."""
    T = model.frames.shape[0]
    return np.stack([np.stack([model.logits(t, list(y[:u])) for u in range(len(y) + 1)]) for t in range(T)])
