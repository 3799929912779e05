"""Contextual biasing (hotword boosting) of the beam search: the caller's phrase list as an Aho–Corasick trie (DESIGN.md §4h "Context").

    g = ContextGraph([[17, 4, 9], [17, 23]], score=1.5)
    model.beam_search(mel, lens, beam_size=4, context=g)

Node 0 is the root, depth(n) the length of the node's path, bonus(n) = score * depth(n); a node is TERMINAL where a phrase ends.
Phrases are inserted shortest first and insertion stops at a terminal node: a phrase that extends another phrase contributes nothing
beyond it — the shorter phrase wins (its bonus is banked the moment it is complete and the match starts over at the root), the longer
one's tail is unreachable.  fail(n) is the node of the deepest proper suffix of n's path that is also a path of the trie.

step(n, k), for a hypothesis at node n that takes label k:
    m = n; while m is not the root and k is no child of m: m = fail(m)
    m' = child(m, k) if there is one, else the root
    delta = bonus(m') - bonus(n)      (computed as score * (depth(m') - depth(n)), here and on the device)
    the next node is the root if m' is terminal (the phrase's bonus is banked for good), else m'
so a hypothesis's node and its accumulated bonus are functions of its token sequence alone, delta >= -bonus(n) with equality exactly
when the step lands on the root, and a partial match that breaks off gives its bonus back.  The search keeps INTERNAL scores (all deltas
so far); what a caller sees is FINALISED: internal - bonus(node), re-sorted (stable, descending).
"""
import math

import numpy as np

MAX_PHRASE = 64     # tokens per phrase (the device's fail walk is a counted loop of this many hops)
MAX_DEVICE_NODES = 65536  # include/rnnt_engine.h RNNT_BEAM_CONTEXT_MAX_NODES: larger graphs run the host loop


class ContextGraph:
    def __init__(self, phrases, score):
        try:
            score = float(score)
        except (TypeError, ValueError):
            raise ValueError(f"ContextGraph: score {score!r} is not a number") from None
        if not math.isfinite(score) or score < 0:
            raise ValueError(f"ContextGraph: score={score} must be finite and >= 0")
        uniq = set()
        for ph in phrases:
            ph = tuple(ph)
            if not ph:
                raise ValueError("ContextGraph: an empty phrase")
            if len(ph) > MAX_PHRASE:
                raise ValueError(f"ContextGraph: a phrase of {len(ph)} tokens (at most {MAX_PHRASE})")
            for k in ph:
                if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0:
                    raise ValueError(f"ContextGraph: token id {k!r} is not a non-negative integer")
            uniq.add(tuple(int(k) for k in ph))
        self.score = score
        self.phrases = sorted(uniq, key=lambda p: (len(p), p))  # duplicates dropped; shortest first
        self.children = [{}]  # node -> {token: node}
        self.depth = [0]
        self.terminal = [False]
        for ph in self.phrases:
            n = 0
            for k in ph:
                if self.terminal[n]:  # a shorter phrase ends here: the rest is unreachable
                    break
                if k not in self.children[n]:
                    self.children[n][k] = len(self.children)
                    self.children.append({})
                    self.depth.append(self.depth[n] + 1)
                    self.terminal.append(False)
                n = self.children[n][k]
            else:
                self.terminal[n] = True
        self.fail = [0] * len(self.children)
        order = list(self.children[0].values())  # breadth first: a node's fail link is shallower than the node
        for n in order:
            for k, c in self.children[n].items():
                f = self.fail[n]
                while f and k not in self.children[f]:
                    f = self.fail[f]
                self.fail[c] = self.children[f].get(k, 0)
                order.append(c)
        self._rows = {}
        self._device = {}

    n_nodes = property(lambda self: len(self.children))
    max_token = property(lambda self: max((k for p in self.phrases for k in p), default=-1))

    @property
    def active(self):
        """Whether the graph can change a search at all (score 0 or no phrase: the plain search, exactly)."""
        return self.score > 0 and self.n_nodes > 1

    def check(self, vocab, blank):
        """The model-side check: every token inside the vocabulary and none the blank."""
        for p in self.phrases:
            for k in p:
                if k >= vocab or k == blank:
                    raise ValueError(f"ContextGraph: token {k} of phrase {list(p)} is "
                                     f"{'the blank' if k == blank else f'outside the vocabulary of {vocab}'}")

    def bonus(self, n):
        return self.score * self.depth[n]

    def _land(self, n, k):
        m = n
        while m and k not in self.children[m]:
            m = self.fail[m]
        return self.children[m].get(k, 0)

    def step(self, n, k):
        """-> (next node, delta) of a hypothesis at node n that takes label k."""
        mp = self._land(n, k)
        return (0 if self.terminal[mp] else mp), self.score * (self.depth[mp] - self.depth[n])

    def walk(self, tokens, n=0):
        """The node of a hypothesis with these labels."""
        for k in tokens:
            n = self.step(n, k)[0]
        return n

    def exceptions(self, n):
        """The labels whose step from n does not land on the root's constant -bonus(n): the children along n, fail(n), .., root."""
        out, m = set(), n
        while True:
            out.update(self.children[m])
            if not m:
                return out
            m = self.fail[m]

    def delta_row(self, n, vocab):
        """float64 [vocab]: delta(n, k) for every label k (cached per node)."""
        key = (n, vocab)
        if key not in self._rows:
            row = np.full(vocab, -self.bonus(n), dtype=np.float64)
            for k in self.exceptions(n):
                if k < vocab:
                    row[k] = self.step(n, k)[1]
            self._rows[key] = row
        return self._rows[key]

    def finalise(self, nbest):
        """[(tokens, internal score)] -> the caller's view: [(tokens, internal - bonus(node))], re-sorted (stable, descending)."""
        out = [(list(y), s - self.bonus(self.walk(y))) for y, s in nbest]
        return sorted(out, key=lambda e: -e[1])

    def tables(self):
        """The flat arrays of include/rnnt_engine.h rnnt_beam_context (int32 numpy): child_off [n + 1], child_tok / child_node
        [max(children, 1)] sorted by token within a node, fail_link, depth, terminal [n]."""
        off, tok, node = [0], [], []
        for ch in self.children:
            for k in sorted(ch):
                tok.append(k)
                node.append(ch[k])
            off.append(len(tok))
        i32 = lambda a: np.asarray(a, dtype=np.int32)  # noqa: E731
        return dict(child_off=i32(off), child_tok=i32(tok or [0]), child_node=i32(node or [0]), fail_link=i32(self.fail),
                    depth=i32(self.depth), terminal=i32(self.terminal), n_nodes=self.n_nodes, n_children=len(tok), score=self.score)

    def device_tables(self, device):
        """tables() as torch tensors on `device` (uploaded once per device)."""
        import torch
        key = str(device)
        if key not in self._device:
            t = self.tables()
            self._device[key] = {k: (torch.from_numpy(v).to(device) if isinstance(v, np.ndarray) else v) for k, v in t.items()}
        return self._device[key]
