"""Per-layer cases of the encoder's kernels (rnnt_amd/csrc/encoder.hip: k_enc_conv_few, k_enc_conv_mfma, k_enc_norm) at tile, chunk,
quad, tap-range, slab and state-block edges: the case builder, a float64 oracle written from the definition in include/rnnt_engine.h,
a Python mirror of make_plan's arithmetic (which kernel, tap ranges, slabs, grids, workspace bytes) and the bar.  numpy and torch on
the CPU only.  Shared by tests/test_encoder_layer_cases_oracle.py (CPU) and tests/test_encoder_layers_gpu.py.

Every case states the edges it is there for as asserts on the mirror (check_reach), and the mirror's workspace bytes are held to
rnnt_engine_encoder_workspace_bytes by the CPU test, so an edit of the host rules that moves a case off its edge fails a test."""
import functools
import math
import zlib
from types import SimpleNamespace

import numpy as np
import torch

NORM_NONE, NORM_BATCH, NORM_INSTANCE = 0, 1, 2  # include/rnnt_engine.h RNNT_ENC_NORM_*
PLAIN, FIRST, LAST, RESIDUAL, FINAL = 0, 1, 2, 4, 8  # RNNT_ENC_ROLE_*
AUTO, MANY_ROWS = 0, 1  # RNNT_ENC_REGIME_*
REGIME_NAMES = {AUTO: "auto", MANY_ROWS: "many_rows"}
# encoder.hip's constants
FEW_ROWS, FEW_FRAMES, FEW_WGS, MFMA_WGS, MFMA_SPLITS, NORM_LANES, NORM_THREADS = 64, 224, 256, 512, 8, 64, 1024

EPS = 1e-5
NORM_KINDS = ("none", "batch", "instance", "instance_plain", "instance_offset")
INSTANCE_KINDS = NORM_KINDS[2:]
LAYOUTS = ("ncl", "slice", "tm_pad", "tm_tight", "tm_offset")
FACTOR = 4.0


def pad4(c):
    return (c + 3) & ~3


def _cdiv(a, b):
    return -(-a // b)


def is_1x1(role):
    return bool(role & (RESIDUAL | FINAL))


# ---- the plan mirror ----------------------------------------------------------------------------------------------------------
def _align(floats):
    return ((floats * 4 + 255) & ~255) // 4


def plan(specs, N, L, state_lens, regime):
    """make_plan: per layer (RESIDUAL layers included) the lengths, the kernel, its tap ranges, slabs and grids; and the workspace
    bytes.  specs: objects with cin, cout, taps, stride, dil, norm, role.  Raises ValueError where make_plan refuses."""
    if N < 1 or L < 1:
        raise ValueError("non-positive N or L")
    cur, act, res, slab, rows = L, 0, 0, 0, []
    for i, l in enumerate(specs):
        span = (l.taps - 1) * l.dil
        pad = span - l.stride + 1
        one = is_1x1(l.role)
        slen = 0
        if not one:
            if state_lens is not None:
                slen = state_lens[i]
            else:
                if pad < 0:
                    raise ValueError(f"layer {i}: stride beyond the kernel's span")
                slen = pad
        Lt = slen + cur
        if Lt < span + 1:
            raise ValueError(f"layer {i}: too short for one output frame")
        Lout = (Lt - span - 1) // l.stride + 1
        if l.norm == NORM_INSTANCE and Lout == 1:
            raise ValueError(f"layer {i}: instance norm over a single output frame")
        M, cinp = N * Lout, pad4(l.cin)
        few = regime == AUTO and M <= FEW_ROWS and N * Lt <= FEW_FRAMES
        if few:
            wgs = _cdiv(l.cout, 64) * _cdiv(cinp, 64)
            ts = min(_cdiv(FEW_WGS, wgs), l.taps)
            nsplit = _cdiv(cinp, 64) * ts
            grid = (_cdiv(l.cout, 64), _cdiv(cinp, 64), ts)
        else:
            wgs = _cdiv(l.cout, 128) * _cdiv(M, 32)
            ts = min(_cdiv(MFMA_WGS, wgs), l.taps, MFMA_SPLITS)
            nsplit = ts
            grid = (_cdiv(l.cout, 128), _cdiv(M, 32), ts)
        ranges = [(l.taps * z // ts, l.taps * (z + 1) // ts) for z in range(ts)]
        KC = _cdiv(cinp, 8)
        slen_out = 0 if one else Lt - Lout * l.stride
        streaming = state_lens is not None
        nb_state = _cdiv(N * l.cin * slen_out, NORM_THREADS) if streaming and not one and slen_out > 0 else 0
        rows.append(SimpleNamespace(
            Lin=cur, Lout=Lout, slen=slen, slen_out=slen_out, Lt=Lt, M=M, few=few, tsplit=ts, nsplit=nsplit, grid=grid, ranges=ranges,
            KC=KC, chunks=None if few else [(j1 - j0) * KC for j0, j1 in ranges],  # mfma: (tap, 8 channels) chunks per workgroup
            nb_norm=N * _cdiv(l.cout, 16), nb_state=nb_state, state_values=N * l.cin * slen_out))
        slab = max(slab, nsplit * M * l.cout)
        o = M * pad4(l.cout)
        if l.role == RESIDUAL:
            res = max(res, o)
            continue
        if l.role != FINAL:
            act = max(act, o)
        cur = Lout
    return SimpleNamespace(rows=rows, L_final=cur, ws_bytes=(2 * _align(act) + _align(res) + _align(slab)) * 4)


def slab_members(spec, row, idx):
    """(channels, taps) whose products slab `idx` of a layer holds."""
    if row.few:
        chunk, z = divmod(idx, row.tsplit)
        chans = range(64 * chunk, min(64 * chunk + 64, spec.cin))
    else:
        z, chans = idx, range(spec.cin)
    return chans, range(*row.ranges[z])


# ---- cases --------------------------------------------------------------------------------------------------------------------
def _L(cin, cout, taps=1, stride=1, dil=1, role=PLAIN):
    return (cin, cout, taps, stride, dil, role)


BOTH = (AUTO, MANY_ROWS)
_BLOCK1 = [_L(20, 33, role=RESIDUAL), _L(20, 33, 5, role=FIRST | LAST)]
_BLOCK3 = [_L(12, 33, role=RESIDUAL), _L(12, 33, 3, role=FIRST), _L(33, 33, 3), _L(33, 33, 3, role=LAST)]
_LIST13 = [_L(9, 13, 5, 2), _L(13, 7, 3)]

# name -> (layers, N, L, state lengths per layer or None = whole utterance, regimes)
SHAPES = {
    "few_c201_o70/whole": ([_L(201, 70, 5)], 3, 7, None, BOTH),
    "few_c201_o70/streamed": ([_L(201, 70, 5)], 3, 7, [4], BOTH),
    "few_c68_s2": ([_L(68, 17, 3, 2)], 3, 8, [2], BOTH),
    "few_c68_s2/long_state": ([_L(68, 17, 3, 2)], 3, 8, [6], BOTH),  # (3 - 1) - 2 + 1 = 1 frame of padding, + 5
    "few_at_both_limits": ([_L(12, 20, 5, 3)], 8, 26, None, BOTH),
    "few_at_both_limits/L27": ([_L(12, 20, 5, 3)], 8, 27, None, (AUTO,)),
    "few_rows17_d2": ([_L(20, 33, 7, 1, 2)], 1, 17, None, BOTH),
    "few_epilogue": ([_L(520, 16, 29, 1, 2)], 1, 2, [56], BOTH),
    "few_one": ([_L(1, 1)], 1, 2, None, BOTH),
    "mfma_c201_o130_s2/whole": ([_L(201, 130, 11, 2)], 2, 67, None, BOTH),
    "mfma_c201_o130_s2/streamed": ([_L(201, 130, 11, 2)], 2, 67, [9], BOTH),
    "mfma_k9_d3": ([_L(12, 40, 9, 1, 3)], 2, 70, None, BOTH),
    "list_13ch": (_LIST13, 2, 11, None, BOTH),
    "list_13ch/streamed": (_LIST13, 2, 11, [4, 2], BOTH),
    "block_one_sub": (_BLOCK1, 2, 9, None, BOTH),
    "block_one_sub/final": (_BLOCK1 + [_L(33, 35, role=FINAL)], 2, 9, None, BOTH),
    "block_three_sub": (_BLOCK3, 2, 9, None, BOTH),
    "block_three_sub/final": (_BLOCK3 + [_L(33, 35, role=FINAL)], 2, 9, None, BOTH),
    "plain_final": ([_L(9, 13, 5, 2), _L(13, 7, role=FINAL)], 2, 11, None, BOTH),
}
SLAB_CINS = (512, 520, 1024, 1028)
for _c in SLAB_CINS:
    SHAPES[f"few_1x1_slabs/c{_c}/final"] = ([_L(_c, 8, role=FINAL)], 1, 3, None, BOTH)
    SHAPES[f"few_1x1_slabs/c{_c}/plain"] = ([_L(_c, 8)], 1, 3, None, BOTH)
DEPTH_CINS = (1, 4, 5, 12, 20, 28, 36, 64, 68, 100)
DEPTH_CHUNKS = (1, 1, 1, 2, 3, 4, 5, 8, 9, 13)
for _c in DEPTH_CINS:
    SHAPES[f"mfma_depth/c{_c}"] = ([_L(_c, 33)], 2, 20, None, (MANY_ROWS,))
LANE_LOUTS = (2, 63, 64, 65, 129)
for _t in LANE_LOUTS:
    SHAPES[f"norm_lanes/L{_t}"] = ([_L(12, 20, 3)], 2, _t, None, BOTH)

LIST_CASES = ("list_13ch", "list_13ch/streamed", "block_one_sub", "block_one_sub/final", "block_three_sub", "block_three_sub/final",
              "plain_final")
LAYOUT_CASES = tuple(f"mfma_depth/c{c}" for c in DEPTH_CINS) + ("mfma_c201_o130_s2/whole", "mfma_c201_o130_s2/streamed",
                                                                "few_c201_o70/whole", "few_c201_o70/streamed")


def norm_kinds(name):
    """The norm kinds a case runs with.  A FINAL layer is conv + bias only (the header), so a list that is one FINAL layer has no norm;
    the lists of several layers are about what passes between layers (rows of pad4(cout), the residual branch), not the norm's
    arithmetic: one kind with running statistics and one with the call's own, and no norm where no residual is added."""
    if name.startswith("few_1x1_slabs") and name.endswith("/final"):
        return ("none",)
    if name.startswith("norm_lanes"):
        return INSTANCE_KINDS
    if name.startswith("block_"):
        return ("batch", "instance")
    if name in LIST_CASES:
        return ("none", "batch", "instance")
    return NORM_KINDS


def layouts(name):
    """The layouts of x beside (N, C, L) contiguous that a case runs with."""
    if name not in LAYOUT_CASES:
        return ()
    cin = SHAPES[name][0][0][0]
    return ("slice", "tm_pad", "tm_offset") + (("tm_tight",) if cin % 4 else ())


def _layer(rng, spec, kind):
    cin, cout, taps, stride, dil, role = spec
    g = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    l = SimpleNamespace(cin=cin, cout=cout, taps=taps, stride=stride, dil=dil, role=role, eps=EPS, norm=NORM_NONE,
                        gamma=None, beta=None, mean=None, var=None)
    l.W = (g(cout, cin, taps) / np.float32(math.sqrt(cin * taps))).astype(np.float32)
    l.b = (0.5 * g(cout)).astype(np.float32)
    if role == FINAL or kind == "none":
        return l
    if kind == "instance_offset":  # the conv output sits ~300 standard deviations from 0: what the two-pass variance is for
        l.b = (l.b + np.float32(300.0)).astype(np.float32)
    l.norm = NORM_BATCH if kind == "batch" else NORM_INSTANCE
    if kind != "instance_plain":
        l.gamma, l.beta = (1.0 + 0.4 * g(cout)).astype(np.float32), (0.5 * g(cout)).astype(np.float32)
    if kind == "batch":
        l.mean = (0.5 * g(cout)).astype(np.float32)
        l.var = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    return l


def build(name, norm="none", layout="ncl", seed=0):
    """The case `name` with every layer's norm of kind `norm` and x handed over in `layout`."""
    specs, N, L, state_lens, regimes = SHAPES[name]
    assert norm in NORM_KINDS and layout in LAYOUTS
    rng = np.random.default_rng([zlib.crc32(name.encode()), NORM_KINDS.index(norm), seed])
    layers = [_layer(rng, s, norm) for s in specs]
    x = rng.standard_normal((N, specs[0][0], L)).astype(np.float32)
    states = None
    if state_lens is not None:  # seeded, non-zero frames
        states = [None if is_1x1(l.role) else rng.standard_normal((N, l.cin, state_lens[i])).astype(np.float32)
                  for i, l in enumerate(layers)]
    return make_case(name, layers, N, x, states, regimes, norm=norm, layout=layout)


def make_case(name, layers, N, x, states, regimes=BOTH, norm="none", layout="ncl"):
    """states: per layer an (N, cin, len) array (None at 1x1 layers), or None for a whole utterance."""
    state_lens = None if states is None else [0 if s is None else s.shape[2] for s in states]
    return SimpleNamespace(name=name, norm=norm, layout=layout, layers=layers, N=N, L=x.shape[2], x=x, states=states,
                           state_lens=state_lens, regimes=regimes, cout=layers[-1].cout)


def reads_input(case, i):
    """True where layer i reads the list's own input x (the first layer, or a block's first layer behind its residual 1x1)."""
    return all(l.role == RESIDUAL for l in case.layers[:i])


CHAIN_CHUNKS = (2, 3, 2, 5, 4, 3, 9)
CHAIN_CASES = ("few_c68_s2", "list_13ch")


def chain(name, norm):
    """A streaming chain from zero state: the whole utterance of sum(CHAIN_CHUNKS) frames as a case (its oracle is the chain's), the
    zero states a stream starts from, and push(states, k), the case of push k given the states before it."""
    specs, N, _, _, regimes = SHAPES[name]
    rng = np.random.default_rng([zlib.crc32(name.encode()), NORM_KINDS.index(norm), 77])
    layers = [_layer(rng, s, norm) for s in specs]
    x = rng.standard_normal((N, specs[0][0], sum(CHAIN_CHUNKS))).astype(np.float32)
    whole = make_case(name + "/chain", layers, N, x, None, regimes, norm=norm)
    zeros = [np.zeros((N, l.cin, (l.taps - 1) * l.dil - l.stride + 1), np.float32) for l in layers]
    starts = np.concatenate([[0], np.cumsum(CHAIN_CHUNKS)])

    def push(states, k):
        return make_case(f"{name}/chain/push{k}", layers, N, np.ascontiguousarray(x[:, :, starts[k]:starts[k + 1]]), states, regimes,
                         norm=norm)
    return whole, zeros, push


def case_plan(case, regime):
    return plan(case.layers, case.N, case.L, case.state_lens, regime)


def has_single_frame(name):
    """True where some layer leaves a single output frame (the instance kinds are skipped there)."""
    specs, N, L, state_lens, _ = SHAPES[name]
    ls = [SimpleNamespace(cin=s[0], cout=s[1], taps=s[2], stride=s[3], dil=s[4], role=s[5], norm=NORM_NONE) for s in specs]
    return any(r.Lout < 2 for r in plan(ls, N, L, state_lens, AUTO).rows)


def case_ids(layouts_too=False):
    """[(name, norm kind, layout)] of every conv case."""
    out = []
    for name in SHAPES:
        for kind in norm_kinds(name):
            if kind in INSTANCE_KINDS and has_single_frame(name):
                continue
            out.append((name, kind, "ncl"))
        if layouts_too:
            out.extend((name, "none", lay) for lay in layouts(name))  # the layout is the conv kernels' business: no norm
    return out


def check_reach(case):
    """The edges each case is there for, asserted through the plan mirror."""
    name = case.name
    a, m = case_plan(case, AUTO), case_plan(case, MANY_ROWS)
    ra, rm, l = a.rows[0], m.rows[0], case.layers[0]
    assert not any(r.few for r in m.rows)
    if name.startswith("few_c201_o70"):
        assert ra.few and ra.M == 21 and ra.M % 16 == 5 and ra.Lout == 7 and ra.M > ra.Lout  # 2nd tile: 5 rows, tiles cross entries
        assert ra.grid == (2, 4, 5) and ra.nsplit == 20 and l.cout == 64 + 6
        assert pad4(l.cin) - 3 * 64 == 12 and l.cin % 4 == 1  # last chunk: 3 quads, channels 201 - 203 padding
        assert ra.slen == 4 and ra.slen_out == 4
        if case.states is not None:
            assert ra.state_values == 2412 and ra.nb_state == 3 and ra.state_values % NORM_THREADS != 0
        assert rm.grid[1] == 1 and rm.M < 32  # many_rows: one MFMA row tile with M < 32
    elif name == "few_c68_s2":
        assert ra.few and ra.grid == (1, 2, 3) and ra.nsplit == 6 and pad4(l.cin) - 64 == 4 and l.cout == 17
        assert l.stride == 2 and case.N > 1 and ra.Lout == 4 and ra.slen_out == 2
    elif name == "few_c68_s2/long_state":
        assert ra.few and ra.slen == (l.taps - 1) * l.dil - l.stride + 1 + 5 and ra.Lout == 6 and ra.slen_out == 2
    elif name == "few_at_both_limits":
        assert ra.few and ra.Lt == 28 and ra.Lout == 8 and ra.M == FEW_ROWS and case.N * ra.Lt == FEW_FRAMES
    elif name == "few_at_both_limits/L27":
        assert not ra.few and case.N * ra.Lt == 232 and ra.M == 72
    elif name == "few_rows17_d2":
        assert ra.few and ra.M == 17 and l.dil == 2 and ra.nsplit == 7 and l.cout == 33
    elif name == "few_epilogue":
        assert ra.few and ra.grid == (1, 9, 29) and ra.nsplit == 261 and (ra.nsplit - 1) // 8 == 32 and (ra.nsplit - 1) % 8 == 4
        assert ra.slen == 56 and ra.slen_out == 56 and case.L == 2  # next state: 54 frames of old state, 2 of the chunk
    elif name.startswith("few_1x1_slabs"):
        assert ra.few and ra.nsplit == {512: 8, 520: 9, 1024: 16, 1028: 17}[l.cin] and ra.tsplit == 1
    elif name == "few_one":
        assert ra.few and ra.grid == (1, 1, 1) and ra.M == 2
    elif name.startswith("mfma_c201_o130_s2"):
        assert not ra.few and ra.M == 66 and ra.grid == (2, 3, 8) and l.cout == 128 + 2 and ra.KC == 26 and 8 * 26 - 4 == pad4(l.cin)
        assert [j1 - j0 for j0, j1 in ra.ranges] == [1, 1, 2, 1, 1, 2, 1, 2]
        assert ra.slen == 9 and ra.slen_out == 10
    elif name.startswith("mfma_depth"):
        assert ra.few and rm.chunks == [DEPTH_CHUNKS[DEPTH_CINS.index(l.cin)]] and rm.grid == (1, 2, 1)
    elif name == "mfma_k9_d3":
        assert not ra.few and ra.M == 140 and ra.Lout == 70 > NORM_LANES and sorted(j1 - j0 for j0, j1 in ra.ranges) == [1] * 7 + [2]
    elif name.startswith("norm_lanes"):
        assert ra.Lout == case.L and ra.Lout in LANE_LOUTS
    elif name.startswith("list_13ch"):
        assert pad4(case.layers[1].cin) == 16 and case.layers[1].cin == 13  # 3 vector quads + a scalar tail, columns 13 - 15 unwritten
    elif name.startswith("block_"):
        assert pad4(case.layers[0].cout) == 36 != case.layers[0].cout and case.layers[0].role == RESIDUAL
    elif name == "plain_final":
        assert case.layers[-1].role == FINAL
    else:
        raise AssertionError(f"no reach stated for {name}")


# ---- the float64 oracle -------------------------------------------------------------------------------------------------------
MUTANTS = ("drop_channel", "drop_tap", "shift", "drop_row", "drop_out_channel", "unbiased_var", "res_after_gelu", "state_early",
           "skip_slab_8")
_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu64(v):
    return 0.5 * v * (1.0 + _erf(v / math.sqrt(2.0)))


def oracle(case, mutant=None, plan_regime=AUTO):
    """out (N, L_out, cout) float64, the new state of every layer (None at 1x1 layers), and of the LAST layer the values in front
    of its norm and max |gamma| * rstd (the bar's rounding floor).  `mutant`: one of MUTANTS, a wrong variant (the bar must see it)."""
    assert mutant is None or mutant in MUTANTS
    N = case.N
    cur = case.x.astype(np.float64)
    res, states, pre, scale = None, [], None, 1.0
    rows = case_plan(case, plan_regime).rows if mutant == "skip_slab_8" else None
    for i, l in enumerate(case.layers):
        W, s, d = l.W.astype(np.float64), l.stride, l.dil
        span = (l.taps - 1) * d
        if is_1x1(l.role):
            Xt = cur
        elif case.states is None:
            Xt = np.concatenate([np.zeros((N, l.cin, span - s + 1)), cur], axis=2)
        else:
            Xt = np.concatenate([case.states[i].astype(np.float64), cur], axis=2)
        Lout = (Xt.shape[2] - span - 1) // s + 1
        assert Lout >= 1
        if mutant == "drop_channel":
            W = W.copy(); W[:, l.cin - 1, :] = 0.0
        if mutant == "drop_tap":
            W = W.copy(); W[:, :, l.taps - 1] = 0.0
        t = np.arange(Lout)
        Y = np.zeros((N, l.cout, Lout))
        for j in range(l.taps):
            idx = (t if mutant == "shift" else t * s) + j * d
            Y += np.einsum("oc,nct->not", W[:, :, j], Xt[:, :, idx])
        if mutant == "skip_slab_8" and rows[i].nsplit > 8:
            chans, taps = slab_members(l, rows[i], 8)
            for j in taps:
                Y -= np.einsum("oc,nct->not", W[:, chans, j], Xt[:, chans, :][:, :, t * s + j * d])
        if mutant == "drop_row":
            Y[N - 1, :, Lout - 1] = 0.0
        if mutant == "drop_out_channel":
            Y[:, l.cout - 1, :] = 0.0
        Y += l.b.astype(np.float64)[None, :, None]
        pre, scale = Y, 1.0
        g = 1.0 if l.gamma is None else l.gamma.astype(np.float64)[None, :, None]
        be = 0.0 if l.beta is None else l.beta.astype(np.float64)[None, :, None]
        if l.norm == NORM_BATCH:
            rstd = 1.0 / np.sqrt(l.var.astype(np.float64) + l.eps)[None, :, None]
            V = (Y - l.mean.astype(np.float64)[None, :, None]) * rstd * g + be
            scale = float(np.max(np.abs(g * rstd)))
        elif l.norm == NORM_INSTANCE:
            assert Lout >= 2
            mu = Y.sum(axis=2, keepdims=True) / Lout
            var = ((Y - mu) ** 2).sum(axis=2, keepdims=True) / (Lout - 1 if mutant == "unbiased_var" else Lout)  # biased
            rstd = 1.0 / np.sqrt(var + l.eps)
            V = (Y - mu) * rstd * g + be
            scale = float(np.max(np.abs(g * rstd)))
        else:
            V = Y
        if l.role & LAST:
            V = gelu64(V) + res if mutant == "res_after_gelu" else gelu64(V + res)
        elif not is_1x1(l.role):
            V = gelu64(V)
        states.append(None if is_1x1(l.role) else Xt[:, :, Lout * s - (1 if mutant == "state_early" else 0):][:, :, :Xt.shape[2] - Lout * s])
        if l.role == RESIDUAL:
            res = V
            continue
        cur = V
    return SimpleNamespace(out=np.ascontiguousarray(cur.transpose(0, 2, 1)), states=states, pre=pre, scale=scale)


# ---- the torch composition: conv1d on cat(state, x), instance_norm or the batch formula, gelu ---------------------------------
def torch_forward(case, dtype):
    F = torch.nn.functional
    T = lambda a: None if a is None else torch.from_numpy(a).to(dtype)
    cur, res, states = T(case.x), None, []
    for i, l in enumerate(case.layers):
        if is_1x1(l.role):
            xt = cur
        elif case.states is None:
            xt = F.pad(cur, ((l.taps - 1) * l.dil - l.stride + 1, 0))
        else:
            xt = torch.cat([T(case.states[i]), cur], dim=2)
        y = F.conv1d(xt, T(l.W), T(l.b), stride=l.stride, dilation=l.dil)
        if l.norm == NORM_BATCH:
            y = F.batch_norm(y, T(l.mean), T(l.var), T(l.gamma), T(l.beta), training=False, eps=l.eps)
        elif l.norm == NORM_INSTANCE:
            y = F.instance_norm(y, weight=T(l.gamma), bias=T(l.beta), use_input_stats=True, eps=l.eps)
        if l.role & LAST:
            y = F.gelu(y + res)
        elif not is_1x1(l.role):
            y = F.gelu(y)
        states.append(None if is_1x1(l.role) else xt[:, :, y.shape[2] * l.stride:])
        if l.role == RESIDUAL:
            res = y
            continue
        cur = y
    return cur.permute(0, 2, 1).contiguous(), states


# ---- the bar ------------------------------------------------------------------------------------------------------------------
def bar(case, want=None):
    """(bar, e_ref, e_round): 4 x max(the torch composition's own fp32 error against the float64 oracle, one rounding of the conv sum
    carried through the norm plus one rounding of the result).  Both terms are computed, per case, from the oracle; neither from
    the engine."""
    want = want or oracle(case)
    y32, _ = torch_forward(case, torch.float32)
    e_ref = float(np.abs(y32.numpy().astype(np.float64) - want.out).max())
    e_round = 2.0 ** -23 * (float(np.abs(want.pre).max()) * want.scale + float(np.abs(want.out).max()))
    return FACTOR * max(e_ref, e_round), e_ref, e_round


@functools.lru_cache(maxsize=None)
def prepared(name, norm="none", layout="ncl"):
    """(case, oracle result, (bar, e_ref, e_round)), computed once per process and left unchanged."""
    case = build(name, norm, layout)
    want = oracle(case)
    return case, want, bar(case, want)
