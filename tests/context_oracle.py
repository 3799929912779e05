"""float64 restatement of the beam search WITH a context graph (DESIGN.md §4h "Context"), on top of tests/beam_oracle.Model.

TEST INFRASTRUCTURE ONLY, and deliberately its own statement of the definition (it shares no code with rnnt_amd/context.py):
    trie: node 0 the root, bonus(n) = score * depth(n); phrases inserted shortest first, insertion stops at a terminal node (a phrase that
          extends another contributes nothing beyond it); fail(n) = the deepest proper suffix of n's path that is a path of the trie
    step(n, k): m = n; while m != root and k no child of m: m = fail(m); m' = child(m, k) or root;
                delta = bonus(m') - bonus(n); next = root if m' terminal else m'
    search: tests/beam_oracle.beam_search with (a) the label candidate (y + [k], .) of an active (y, s) at node n scoring
            s + lp[k] + delta(n, k), over ALL labels k (no per-row shortlist); blank candidates get no delta; (b) the beam keeps these INTERNAL
            scores; the caller's list is FINALISED: internal - bonus(node), re-sorted (stable, descending) — a view that never feeds back.
With `graph=None` the search is beam_oracle.beam_search, float for float.
"""
import math
from collections import namedtuple

import numpy as np

from tests.beam_oracle import _lae

Result = namedtuple("Result", "nbest internal pruned gap events")
EVENTS = ("outside", "cancel", "fail_hop", "banked")


class Trie:
    def __init__(self, phrases, score):
        self.score = float(score)
        self.kids, self.depth, self.term, self.path = [{}], [0], [False], [()]
        for ph in sorted({tuple(int(k) for k in p) for p in phrases}, key=lambda p: (len(p), p)):
            n = 0
            for k in ph:
                if self.term[n]:
                    break
                if k not in self.kids[n]:
                    self.kids[n][k] = len(self.kids)
                    self.kids.append({})
                    self.depth.append(self.depth[n] + 1)
                    self.term.append(False)
                    self.path.append(self.path[n] + (k,))
                n = self.kids[n][k]
            else:
                self.term[n] = True
        # the fail link by its definition (quadratic, no breadth-first bookkeeping): the longest proper suffix that is a path
        index = {p: n for n, p in enumerate(self.path)}
        self.fail = [next(index[p[i:]] for i in range(1, len(p) + 1) if p[i:] in index) if p else 0 for p in self.path]

    def bonus(self, n):
        return self.score * self.depth[n]

    def step(self, n, k):
        """-> (next node, delta, landed through a fail link on a non-root node, banked)"""
        m = n
        while m != 0 and k not in self.kids[m]:
            m = self.fail[m]
        mp = self.kids[m].get(k, 0)
        return (0 if self.term[mp] else mp), self.bonus(mp) - self.bonus(n), (m != n and mp != 0), self.term[mp]

    def walk(self, y):
        n = 0
        for k in y:
            n = self.step(n, k)[0]
        return n


def beam_search(model, beam, max_length, max_per_frame=10, graph=None):
    """-> Result(finalised n-best, internal n-best, pruned candidates, smallest gap — at a keep / drop boundary, between neighbours of the
    internal final list and between neighbours of the finalised list —, event counts over KEPT label candidates: `outside` raw rank within
    its row >= beam, `cancel` delta < 0, `fail_hop` landed on a non-root node through a fail link, `banked`; and `touched`: delta != 0)."""
    blank, V = model.blank, model.V
    beam_list = [((), 0.0, 0)]  # (sequence, internal score, node)
    pruned, gap = 0, math.inf
    events = dict.fromkeys(EVENTS + ("touched",), 0)  # touched: any kept label with delta != 0 (0 everywhere: the graph never acted)
    labels = np.array([k for k in range(V) if k != blank])
    rows = {}  # node -> step(node, k) for every label (a function of the node)
    short = beam + 1  # the best `beam` of all candidates and the first one dropped lie among the best beam + 1 of their rows
    for t in range(model.frames.shape[0]):
        active, fin = beam_list, []
        for r in range(max_per_frame):
            lps = [model.lp(t, list(y)) for y, _, _ in active]
            for (y, s, n), lp in zip(active, lps):
                b = s + lp[blank]
                hit = next((e for e in fin if e[0] == y), None)
                if hit is not None:
                    hit[1] = _lae(hit[1], b)
                else:
                    fin.append([y, b, n])
            cands = [(s, 0, f, 0, y, n, None) for f, (y, s, n) in enumerate(fin)]
            total = len(cands)
            for i, ((y, s, n), lp) in enumerate(zip(active, lps)):
                if len(y) >= max_length - 1:
                    continue
                total += len(labels)
                if graph is None:
                    val = s + lp[labels]
                    top = np.argsort(-val, kind="stable")[:short]  # (stable: the lower id first among equal values)
                    cands += [(val[j], 1, i, int(labels[j]), y + (int(labels[j]),), 0, None) for j in top]
                    continue
                if n not in rows:
                    rows[n] = [graph.step(n, int(k)) for k in labels]
                    rows[n] = (np.array([st[1] for st in rows[n]], dtype=np.float64), rows[n])
                val = s + lp[labels] + rows[n][0]
                for j in np.argsort(-val, kind="stable")[:short]:
                    nn, delta, hop, bank = rows[n][1][j]
                    cands.append((val[j], 1, i, int(labels[j]), y + (int(labels[j]),), nn, (delta, hop, bank)))
            cands.sort(key=lambda c: (-c[0], c[1], c[2], c[3]))
            if total > beam:
                pruned += total - beam
                gap = min(gap, cands[beam - 1][0] - cands[beam][0])
            kept = cands[:beam]
            for c in kept:
                if c[1] == 1 and c[6] is not None:
                    lp = lps[c[2]]
                    raw = lp[labels]
                    rank = int((raw > lp[c[3]]).sum() + ((raw == lp[c[3]]) & (labels < c[3])).sum())
                    delta, hop, bank = c[6]
                    events["outside"] += rank >= beam
                    events["cancel"] += delta < 0
                    events["fail_hop"] += bool(hop)
                    events["banked"] += bool(bank)
                    events["touched"] += delta != 0
            fin = [[c[4], c[0], c[5]] for c in kept if c[1] == 0]
            active = [(c[4], c[0], c[5]) for c in kept if c[1] == 1]
            if not active:
                break
        for y, s, n in active:
            hit = next((e for e in fin if e[0] == y), None)
            if hit is not None:
                hit[1] = _lae(hit[1], s)
            else:
                fin.append([y, s, n])
        order = sorted(range(len(fin)), key=lambda i: (-fin[i][1], i))
        beam_list = [tuple(fin[i]) for i in order]
    for a, b in zip(beam_list, beam_list[1:]):
        gap = min(gap, a[1] - b[1])
    internal = [(list(y), float(s)) for y, s, _ in beam_list]
    if graph is None:
        final = internal
    else:
        final = sorted(((list(y), float(s - graph.bonus(n))) for y, s, n in beam_list), key=lambda e: -e[1])
        for a, b in zip(final, final[1:]):
            gap = min(gap, a[1] - b[1])
    return Result(final, internal, pruned, gap, events)


# ---- the configurations the host loop (CPU) and the device (GPU) are held to: (case, max_length, phrase list, score, beams).  Every one's
# oracle gap is far above fp32 noise (asserted by the tests that use them, never assumed).
PHRASES = {
    "decode_small": [(27, 1, 27), (27, 27, 1), (21, 21, 29), (1, 1, 19), (27, 23, 1, 1), (21, 27, 23, 2), (27, 23, 1)],
    "decode_cap": [(0, 2, 10), (0, 26, 0), (2, 10, 11), (10, 11, 11), (1, 0, 29), (0, 0, 19), (23, 11, 21), (11, 23, 27), (0, 26, 17),
                   (23, 0, 24), (4, 2, 25), (0, 0, 0, 0), (9, 11, 11, 23), (0, 23, 0, 1), (0, 0, 0, 1), (0, 0, 0)],
    "decode_small_proj": [(150, 150, 150), (160, 286, 150), (286, 150, 150), (150, 150, 82), (286, 160, 282)],
    "decode_wide_vocab": [(2808, 2808, 2808), (3140, 2808, 2808), (3601, 1710, 2808), (3909, 3601, 1710), (3795, 3795, 3778),
                          (3909, 1668, 2499), (2874, 2874, 2736), (2874, 3931, 3587), (3795, 3795, 279, 3909), (2874, 3909, 2874, 3931),
                          (3795, 3795, 3795, 280), (3795, 3795, 279)],
    "decode_ref_widths": [(41, 759, 385), (62, 759, 622), (139, 211, 526), (211, 526, 62), (385, 759, 139), (526, 62, 759),
                          (392, 877, 966), (198, 837, 837, 41)],
}


def wide_vocab_long_list(V=4000):
    """decode_wide_vocab's phrases and 600 two-token phrases more: a root with 605 children, 1228 nodes — a long exception list."""
    rng = np.random.default_rng(11)
    first = rng.choice(V - 1, 600, replace=False)
    second = rng.integers(0, V - 1, 600)
    return PHRASES["decode_wide_vocab"] + [(int(a), int(b)) for a, b in zip(first, second)]


PHRASES["decode_wide_vocab+600"] = wide_vocab_long_list()

# (case, max_length, phrases key, score, beams)
CONFIGS = [
    ("decode_small", 60, "decode_small", 1.5, (1, 2, 4, 8, 16)),
    ("decode_cap", 37, "decode_cap", 1.5, (1, 2, 4, 8, 16)),
    ("decode_cap", 37, "decode_cap", 3.0, (2, 4)),
    ("decode_small_proj", 60, "decode_small_proj", 3.0, (1, 2, 4, 8)),
    ("decode_wide_vocab", 60, "decode_wide_vocab", 1.5, (1, 2, 4)),
    ("decode_wide_vocab", 60, "decode_wide_vocab", 3.0, (4,)),
    ("decode_wide_vocab", 60, "decode_wide_vocab+600", 1.5, (4,)),
    ("decode_ref_widths", 200, "decode_ref_widths", 1.5, (2, 4)),
    ("decode_ref_widths", 200, "decode_ref_widths", 3.0, (2, 4)),
]
GAP = 1e-3  # smallest oracle gap for which identical n-best lists are demanded (tests/test_beam_gpu.py's bar)

_models, _results = {}, {}


def result(golden_dir, name, ml, key, score, beam):
    """The oracle's Result of one configuration (computed once per process; the Model's log-prob rows are shared by a case's searches)."""
    from tests import beam_oracle
    from tests.helpers import load_decode_case
    k = (name, ml, key, score, beam)
    if k not in _results:
        if name not in _models:
            c = load_decode_case(golden_dir, name)
            _models[name] = beam_oracle.Model(c["frames"], c["pred_sd"], c["joint_sd"])
        _results[k] = beam_search(_models[name], beam, ml, graph=Trie(PHRASES[key], score) if key else None)
    return _results[k]
