"""Shapes and symbol ids of the ConvPredictor edge tests (rnnt_amd/csrc/predictor.hip, smallgemm.hip) with the premise of every case
stated as an assert, so that a later edit cannot silently leave the path the case is there for.  No GPU, no torch.  Shared by
tests/test_predictor_cases_oracle.py (CPU: the premises, the oracle's pin at short segments) and tests/test_predictor_edges_gpu.py.

The host rules restated below (split counts, slab counts, the embedding gradient's list rounds) are the kernels' own: a change there
fails a premise here, which is the point."""
import collections
import functools

import numpy as np

from oracle import predictor_oracle as po

TAPS = (3, 5)      # conv1, conv2 (rnnt_amd/predictor.py)
EMBED_CAP = 2048   # k_embed_bwd: rows listed per round
E_MAX = 2048       # check_pred_dims

Case = collections.namedtuple("Case", "name S E O B U1 p ids seed constant_row")


def _case(name, S, E, O, B, U1, p, ids, seed, constant_row=None):
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    assert ids.shape == (B, U1) and ids.min() >= 0 and ids.max() < S, name  # (out-of-range ids are clamped by the kernels: not tested)
    assert E % 4 == 0 and O % 4 == 0 and E <= E_MAX, name
    assert 0.0 <= p < 1.0, name
    return Case(name, S, E, O, B, U1, p, ids, seed, constant_row)


# ---- the kernels' host rules --------------------------------------------------------------------------------------------------
def tn_splits_cap(M):
    """sgemm_tn_splits: one contraction range per ~256 rows, at most 16 (sizes the slab buffer)."""
    return min(16, max(1, -(-M // 256)))


def tn_splits_for(M, N, K, taps):
    """sgemm_tn_splits_for: the ranges ONE weight-gradient GEMM runs with (output [taps][N][K], contraction over M rows)."""
    per = -(-N // 128) * -(-K // 128) * taps
    s = max(-(-M // 448), -(-256 // per))
    return min(max(s, 1), tn_splits_cap(M))


def wgrad_splits(c):
    """(linear, conv2, conv1): the split counts of the predictor backward's three weight-gradient GEMMs."""
    M = c.B * c.U1
    return tn_splits_for(M, c.O, c.E, 1), tn_splits_for(M, c.E, c.E, 5), tn_splits_for(M, c.E, c.E, 3)


def colsum_slabs(M):
    return -(-M // 256)


def embed_rounds(ids, s):
    """Rows of symbol `s` listed in each round of k_embed_bwd: 256 rows are scanned per step while another whole step still fits
    into the list (n + 256 <= CAP), then the listed rows are added up and the next round starts where the scan stopped."""
    flat = np.asarray(ids).reshape(-1)
    M, rounds, base = flat.size, [], 0
    while base < M:
        n = 0
        while base < M and n + 256 <= EMBED_CAP:
            n += int((flat[base:base + 256] == s).sum())
            base += 256
        rounds.append(n)
    return rounds


def absent_symbols(c):
    return np.setdiff1d(np.arange(c.S), c.ids.reshape(-1))


# ---- the cases: (S, E, O, B, U1, p) ------------------------------------------------------------------------------------------
def rows_4109(B=7):
    """Training row counts.  B = 7: M = 4109 rows — every weight-gradient GEMM at the cap of 16 splits with uneven ranges and a
    half-empty last step, 17 column-sum slabs, symbol 0 (start symbol + padded tails, as in a real batch) in two list rounds.
    B = 3 (M = 1761, 7 splits): the same ids' first utterances, for the tests that run the case three times."""
    S, E, O, U1, p = 64, 128, 128, 587, 0.3
    rng = np.random.default_rng(4109)
    ids = rng.integers(1, S, (7, U1))
    ids[:, 0] = 0
    for b, n in enumerate(rng.integers(120, 400, 7)):  # utterance b holds n labels; the tail is padding (symbol 0)
        ids[b, 1 + n:] = 0
    c = _case("rows_4109" if B == 7 else "rows_4109_b%d" % B, S, E, O, B, U1, p, ids[:B], seed=41)
    M = B * U1
    assert M % 2 == 1  # the TN kernel walks 2 rows per step: the last step's second row does not exist
    # E = O = 128: one split's grid is ceil(N/128) * ceil(K/128) * taps = taps workgroups for each of the three GEMMs, so
    # by_fill = ceil(256 / taps) = 256 (linear), 52 (conv2), 86 (conv1) >= 52, by_rows = ceil(M/448) <= 10: the count is by_fill
    # cut to the cap min(16, ceil(M/256)) — every GEMM runs at the cap.
    assert -(-256 // max(TAPS)) >= 52
    if B == 7:
        assert M == 4109 and -(-M // 256) == 17 > 16
        assert wgrad_splits(c) == (16, 16, 16)
        assert ((M + 1) // 2) % 16 != 0  # steps_all = 2055: the 16 ranges s_lo .. s_hi are uneven (128 and 129 steps)
        assert colsum_slabs(M) == 17
        n0 = int((c.ids == 0).sum())
        assert EMBED_CAP < n0 < 2 * EMBED_CAP, n0
        r = embed_rounds(c.ids, 0)
        assert len(r) == 2 and EMBED_CAP - 256 < r[0] <= EMBED_CAP and 0 < r[1] < EMBED_CAP - 256, r  # the second partly filled
        assert all(len(embed_rounds(c.ids, s)) == 1 for s in range(1, S))
    else:
        assert wgrad_splits(c) == (tn_splits_cap(M),) * 3 and tn_splits_cap(M) > 2
    return c


def one_symbol():
    """Every id = 3: 2500 occurrences, the first list round ends at exactly CAP rows; the other seven rows of the embedding
    gradient are exactly 0."""
    S, E, O, B, U1 = 8, 64, 32, 5, 500
    c = _case("one_symbol", S, E, O, B, U1, 0.0, np.full((B, U1), 3), seed=42)
    assert embed_rounds(c.ids, 3) == [EMBED_CAP, B * U1 - EMBED_CAP] and B * U1 - EMBED_CAP > 0
    assert list(absent_symbols(c)) == [0, 1, 2, 4, 5, 6, 7]
    return c


def split_edges(B, U1):
    """M = 256, 257, 513: each side of a split / slab boundary; O = 132: a 4-column tail in the NT and TN tiles."""
    S, E, O = 33, 128, 132
    rng = np.random.default_rng(1000 * B + U1)
    c = _case("split_edges_%dx%d" % (B, U1), S, E, O, B, U1, 0.3, rng.integers(0, S, (B, U1)), seed=43 + B + U1)
    M = B * U1
    assert M in (256, 257, 513) and O % 128 == 4
    want = -(-M // 256)  # 1, 2, 3
    assert wgrad_splits(c) == (want,) * 3 and colsum_slabs(M) == want
    assert M % 256 in (0, 1)
    return c


def short_segments(U1):
    """U1 = 1 .. 5: every utterance is no longer than conv2's 5 taps (U1 < 3: than conv1's too), so each tap beyond the first reads
    before an utterance's start somewhere in every utterance; B = 9 utterances share the 32-row tiles, so a causal shift that
    leaks across an utterance boundary reads a real row of the previous utterance.  E % 8 == 4: the kok == false half chunk."""
    S, E, O, B = 11, 36, 20, 9
    rng = np.random.default_rng(500 + U1)
    c = _case("short_segments_u%d" % U1, S, E, O, B, U1, 0.5, rng.integers(0, S, (B, U1)), seed=44 + U1)
    assert 1 <= U1 <= max(TAPS) and B > 1
    assert min(32, B * U1) // U1 >= 6  # utterances inside the first 32-row tile
    assert E % 8 == 4 and O % 8 == 4
    return c


def wide_e(limit=False):
    """E > 1024: the second 1024-column sweep of k_embed_bwd.  E = 1028: that sweep has one live thread, E % 8 == 4, a LayerNorm
    row takes five 256-column passes.  limit: E = 2048, the largest the kernels take."""
    S, E, O, B, U1 = (4, 2048, 4, 1, 3) if limit else (16, 1028, 20, 3, 4)
    rng = np.random.default_rng(E)
    c = _case("wide_e_%d" % E, S, E, O, B, U1, 0.0, rng.integers(0, S, (B, U1)), seed=45 + int(limit))
    assert 1024 < E <= E_MAX
    if limit:
        assert E == E_MAX
    else:
        assert (E - 1024) // 4 == 1 and E % 8 == 4 and -(-E // 256) == 5
    return c


def constant_row():
    """Embedding row 2 = 0.5 everywhere: sum and mean are exact in fp32, the variance is exactly 0 (rstd = 1 / sqrt(eps))."""
    S, E, O, B, U1 = 8, 128, 32, 2, 6
    rng = np.random.default_rng(6)
    ids = rng.integers(0, S, (B, U1))
    ids[0, 1] = ids[1, 4] = 2
    c = _case("constant_row", S, E, O, B, U1, 0.0, ids, seed=47, constant_row=2)
    assert (c.ids == 2).any()
    return c


BUILDERS = collections.OrderedDict(
    [("rows_4109", rows_4109), ("one_symbol", one_symbol)]
    + [("split_edges_%dx%d" % bu, functools.partial(split_edges, *bu)) for bu in ((1, 256), (1, 257), (3, 171))]
    + [("short_segments_u%d" % u, functools.partial(short_segments, u)) for u in (1, 2, 3, 4, 5)]
    + [("wide_e_1028", wide_e), ("wide_e_2048", functools.partial(wide_e, True)), ("constant_row", constant_row)])
BUILDERS["rows_4109_b3"] = functools.partial(rows_4109, 3)  # (the scratch-independence test's; not among the parity cases)
PARITY_CASES = [n for n in BUILDERS if n != "rows_4109_b3"]


@functools.lru_cache(maxsize=None)
def build(name):
    c = BUILDERS[name]()
    assert c.name == name
    return c


# ---- seeded parameters, masks and output gradient of a case (float32 / keep bytes), and the oracle's answer -----------------------
def state_dict(c):
    """The 11 parameters, float32, torch-default-like scales (Linear / Conv1d: U(+-1/sqrt(fan_in)); embedding N(0,1)); the LayerNorm
    affines are NOT the identity (1 + 0.2 N, 0.2 N): a gamma dropped or applied twice must show."""
    rng = np.random.default_rng(c.seed)
    E, O = c.E, c.O

    def uni(shape, fan_in):
        k = 1.0 / np.sqrt(fan_in)
        return rng.uniform(-k, k, shape).astype(np.float32)

    def nrm(shape, scale=1.0, shift=0.0):
        return (shift + scale * rng.standard_normal(shape)).astype(np.float32)

    sd = {"embedding.weight": nrm((c.S, E)),
          "input_layer_norm.weight": nrm(E, 0.2, 1.0), "input_layer_norm.bias": nrm(E, 0.2),
          "conv1.conv.weight": uni((E, E, 3), 3 * E), "conv1.conv.bias": uni(E, 3 * E),
          "conv2.conv.weight": uni((E, E, 5), 5 * E), "conv2.conv.bias": uni(E, 5 * E),
          "linear.weight": uni((O, E), E), "linear.bias": uni(O, E),
          "output_layer_norm.weight": nrm(O, 0.2, 1.0), "output_layer_norm.bias": nrm(O, 0.2)}
    if c.constant_row is not None:
        sd["embedding.weight"][c.constant_row] = 0.5
    assert tuple(sd) == po.PARAMS
    return sd


def masks_and_grad(c):
    """(keep1, keep2) uint8 [B,U1,E] (None, None when p = 0) and the output gradient G float32 [B,U1,O]."""
    rng = np.random.default_rng(c.seed + 1000)
    G = rng.standard_normal((c.B, c.U1, c.O)).astype(np.float32)
    if c.p == 0.0:
        return None, None, G
    k1 = (rng.random((c.B, c.U1, c.E)) >= c.p).astype(np.uint8)
    k2 = (rng.random((c.B, c.U1, c.E)) >= c.p).astype(np.uint8)
    return k1, k2, G


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(out, grads) of the float64 numpy oracle for a case: computed once, shared by the tests, never written to."""
    c = build(name)
    k1, k2, G = masks_and_grad(c)
    f = (lambda k: None if k is None else k.astype(np.float64))
    out, cache = po.forward(c.ids, state_dict(c), f(k1), f(k2), p=c.p)
    grads = po.backward(G, cache)
    out.setflags(write=False)
    for g in grads.values():
        g.setflags(write=False)
    return out, grads
