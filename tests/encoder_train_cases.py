"""Shared by tests/test_encoder_train_*.py: the fixtures of tests/golden/make_golden_encoder_train.py, a Python mirror of the training
plan of rnnt_amd/csrc/encoder.hip (make_train_plan: the layout of `saved`, the backward's splits, row ranges and workspace), per-layer
cases at the edges of k_enc_dw / k_enc_bwd_norm / the dX conv, and a float64 numpy oracle of forward and backward written from the
definition in include/rnnt_engine.h.  numpy and torch on the CPU only."""
import functools
import math
import os
import zlib
from types import SimpleNamespace

import numpy as np
import torch

from tests.encoder_cases import GOLDEN, fixture, loaded_small_encoder
from tests.encoder_layer_cases import (AUTO, FINAL, FIRST, LAST, MANY_ROWS, MFMA_SPLITS, MFMA_WGS, NORM_BATCH, NORM_INSTANCE, NORM_NONE, PLAIN,
                                       RESIDUAL, _align, _cdiv, _erf, gelu64, is_1x1, pad4, plan)

DW_WGS, DW_RANGES, DW_STEP = 512, 16, 8  # encoder.hip ENC_DW_*
TRAIN_CASES = ("batch", "instance", "instance_affine", "instance_affine_la2")
FACTOR = 4.0
EPS = 1e-5


# ---- fixtures -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def train_fixture(case, N):
    with np.load(os.path.join(GOLDEN, f"encoder_train_{case}_n{N}.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def lookahead_out():
    with np.load(os.path.join(GOLDEN, "encoder_train_instance_affine_la2_out.npz")) as z:
        return {k: z[k] for k in z.files}


def norm_of(case):
    return "instance_affine" if case == "instance_affine_la2" else case


def small_train_encoder(case):
    """The small encoder of the fixtures with case's state dict, in eval(); instance_affine_la2: look-ahead 2 on the epilogue conv."""
    from rnnt_amd.encoder import CausalConv1d
    enc = loaded_small_encoder(norm_of(case))
    if case == "instance_affine_la2":
        at = len(enc.blocks) - 4
        old = enc.blocks[at]
        new = CausalConv1d(24, 28, 7, 1, 2, additional_context=2)
        new.load_state_dict(old.state_dict())
        enc.blocks[at] = new
        enc.repack()
    return enc.eval()


def grads64(fx):
    return {k[4:]: fx[k].astype(np.float64) + fx["g64_corr/" + k[4:]].astype(np.float64) for k in fx if k.startswith("g32/")}


def zero_bias_bound(fx, key, M):
    """The worst case of an M-term fp32 sum of exactly cancelling terms: M 2^-24 sum|dy| per channel."""
    return M * 2.0 ** -24 * fx["dyabs/" + key]


def check_grads(label, fx, got, M_of, printer=print):
    """got: {parameter name: gradient array}.  Every tensor within FACTOR x the reference's own fp32 error; the bias of a conv that feeds
    an instance norm within the M-term bound (its gradient is exactly zero).  Returns the lines printed."""
    want, worst = grads64(fx), []
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    for k in sorted(want):
        g = np.asarray(got[k], dtype=np.float64)
        assert g.shape == want[k].shape, (k, g.shape)
        if "dyabs/" + k in fx:
            bound = zero_bias_bound(fx, k, M_of(k))
            printer(f"encoder train parity {label} {k}: exactly zero; engine max|g| = {np.abs(g).max():.3e}, bound M 2^-24 sum|dy| >= "
                    f"{bound.min():.3e}")
            if not np.all(np.abs(g) <= bound):
                worst.append((k, float(np.abs(g).max()), float(bound.min())))
            continue
        err, ref = float(np.abs(g - want[k]).max()), float(fx["err/" + k])
        printer(f"encoder train parity {label} {k}: engine max|g - g64| = {err:.3e}, reference fp32 error = {ref:.3e}, bar = {FACTOR * ref:.3e}")
        if not err <= FACTOR * ref:
            worst.append((k, err, ref))
    assert not worst, (label, worst)


def bias_rows(enc, N, L):
    """{conv bias parameter name: M = N * output frames of that conv}."""
    rows, _ = enc._lengths(L, None)
    flat = enc._flat(allow_lookahead=True)
    names = {id(p): k for k, p in enc.named_parameters()}
    out, si, cur = {}, 0, None
    for holder, conv, _, role in flat:
        if holder is not None:
            cur = rows[si][2]
            out[names[id(conv.bias)]] = N * cur
            si += 1
        else:  # a 1x1 on the frames of the layer in front (residual: the block's input = rows[si][0])
            out[names[id(conv.bias)]] = N * (rows[si][0] if role == RESIDUAL else cur)
    return out


# ---- the plan mirror ----------------------------------------------------------------------------------------------------------
def reads_input(specs, i):
    return i == 0 or (i == 1 and specs[0].role == RESIDUAL)


def train_plan(specs, N, L, lead, regime=AUTO):
    """make_train_plan.  specs: objects with cin, cout, taps, stride, dil, norm, role; lead: per layer or None (no look-ahead)."""
    leads = []
    for i, l in enumerate(specs):
        pad = (l.taps - 1) * l.dil - l.stride + 1
        if is_1x1(l.role):
            leads.append(0)
            continue
        if pad < 0:
            raise ValueError(f"layer {i}: stride beyond the kernel's span")
        v = pad if lead is None else lead[i]
        if not 0 <= v <= pad:
            raise ValueError(f"layer {i}: lead outside 0 .. {pad}")
        if not reads_input(specs, i) and l.stride != 1:
            raise ValueError(f"layer {i}: stride behind the list's first layer")
        leads.append(v)
    P = plan(specs, N, L, leads, regime)
    res_at = 0
    for i, l in enumerate(specs):
        if l.role == RESIDUAL:
            res_at = i
        if l.role & LAST and P.rows[i].Lout != P.rows[res_at].Lout:
            raise ValueError(f"layer {i}: lead inside a block")
    off = dy = dres = x1 = x2 = dw = part = 0
    rows = []
    for i, (l, r) in enumerate(zip(specs, P.rows)):
        M, act = r.M, r.M * pad4(l.cout)
        res, gelu = l.role == RESIDUAL, not is_1x1(l.role)
        kept = SimpleNamespace(o=None, z=None, xh=None, rstd=None)
        for name, have, floats in (("o", i != len(specs) - 1 and not res, act), ("z", gelu, act), ("xh", l.norm != NORM_NONE, act),
                                   ("rstd", l.norm == NORM_INSTANCE, N * l.cout)):
            if have:
                setattr(kept, name, off)
                off += _align(floats)
        dy = max(dy, act)
        if l.role & LAST:
            dres = max(dres, act)
        part = max(part, 3 * N * l.cout)
        dx_split = 0
        if not reads_input(specs, i):
            Min = N * r.Lin
            wgs = _cdiv(l.cin, 128) * _cdiv(Min, 32)
            dx_split = min(_cdiv(MFMA_WGS, wgs), l.taps, MFMA_SPLITS)
            s = dx_split * Min * l.cin
            if res:
                x2 = max(x2, s)
            else:
                x1 = max(x1, s)
        tiles = _cdiv(l.cin, 128) * _cdiv(l.cout, 128) * l.taps
        R = min(_cdiv(DW_WGS, tiles), DW_RANGES)
        per = _cdiv(_cdiv(M, R), DW_STEP) * DW_STEP
        ranges = _cdiv(M, per)
        dw = max(dw, ranges * l.taps * l.cout * l.cin)
        rows.append(SimpleNamespace(fwd=r, lead=leads[i], kept=kept, dx_split=dx_split, dw_ranges=ranges, dw_rows=per,
                                    dw_grid=(l.taps * ranges, _cdiv(l.cin, 128), _cdiv(l.cout, 128)), M=M,
                                    last_range_rows=M - (ranges - 1) * per))
    slab = max(r.nsplit * r.M * l.cout for l, r in zip(specs, P.rows))
    resbuf = max([r.M * pad4(l.cout) for l, r in zip(specs, P.rows) if l.role == RESIDUAL], default=0)
    ws_fwd = (_align(resbuf) + _align(slab)) * 4
    ws_bwd = sum(_align(v) for v in (dy, dres, x1, x2, dw, part)) * 4
    return SimpleNamespace(rows=rows, saved_bytes=off * 4, ws_fwd=ws_fwd, ws_bwd=ws_bwd, ws_bytes=max(ws_fwd, ws_bwd), L_final=P.L_final)


# ---- per-layer cases ----------------------------------------------------------------------------------------------------------
def _L(cin, cout, taps=1, stride=1, dil=1, role=PLAIN, ac=0):
    return (cin, cout, taps, stride, dil, role, ac)


_TRIPLE = [_L(9, 12, 3), _L(12, 20, role=RESIDUAL), _L(12, 20, 5, role=FIRST), _L(20, 20, 5, role=LAST)]
# name -> (layers, N, L, drop probability of the layers inside a block)
SHAPES = {
    "c130_o132": ([_L(9, 130, 3), _L(130, 132, 3)], 2, 70, 0.0),
    "c9_s2_odd": ([_L(9, 13, 5, 2)], 2, 11, 0.0),
    "k7_d2": ([_L(9, 12, 3), _L(12, 20, 7, 1, 2)], 2, 20, 0.0),
    "one_by_one": ([_L(9, 12, 3), _L(12, 7, 1), _L(7, 5, role=FINAL)], 2, 9, 0.0),
    "lookahead2": ([_L(9, 12, 3), _L(12, 20, 5, ac=2)], 2, 13, 0.0),
    "rows_127": ([_L(12, 20, 3)], 1, 127, 0.0),
    "rows_129": ([_L(12, 20, 3)], 1, 129, 0.0),
    "triple": (_TRIPLE, 2, 9, 0.0),
    "triple_dropout": (_TRIPLE, 2, 9, 0.25),
}
NORM_KINDS = ("none", "batch", "instance", "instance_plain")


def norm_kinds(name):
    return NORM_KINDS if name == "triple" else ("instance",)


def case_ids():
    return [(n, k) for n in SHAPES for k in norm_kinds(n)]


def build(name, kind):
    specs, N, L, p = SHAPES[name]
    rng = np.random.default_rng([zlib.crc32(name.encode()), NORM_KINDS.index(kind), 5])
    g = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    layers = []
    for cin, cout, taps, stride, dil, role, ac in specs:
        l = SimpleNamespace(cin=cin, cout=cout, taps=taps, stride=stride, dil=dil, role=role, eps=EPS, norm=NORM_NONE, gamma=None,
                            beta=None, mean=None, var=None, lead=0 if is_1x1(role) else (taps - 1) * dil - stride + 1 - ac)
        l.W = (g(cout, cin, taps) / np.float32(math.sqrt(cin * taps))).astype(np.float32)
        l.b = (0.5 * g(cout)).astype(np.float32)
        if role != FINAL and kind != "none":
            l.norm = NORM_BATCH if kind == "batch" else NORM_INSTANCE
            if kind != "instance_plain":
                l.gamma, l.beta = (1.0 + 0.4 * g(cout)).astype(np.float32), (0.5 * g(cout)).astype(np.float32)
            if kind == "batch":
                l.mean, l.var = (0.5 * g(cout)).astype(np.float32), rng.uniform(0.5, 1.5, cout).astype(np.float32)
        layers.append(l)
    x = g(N, specs[0][0], L)
    tp = train_plan(layers, N, L, [l.lead for l in layers])
    keep, ps = [], []
    for l, r in zip(layers, tp.rows):
        inside = bool(l.role & (FIRST | LAST))
        keep.append((rng.random((N, r.fwd.Lout, l.cout)) >= p).astype(np.uint8) if inside and p > 0 else None)
        ps.append(p if inside and p > 0 else 0.0)
    G = g(N, tp.L_final, layers[-1].cout)
    return SimpleNamespace(name=name, kind=kind, layers=layers, N=N, L=L, x=x, keep=keep, p=ps, G=G, lead=[l.lead for l in layers], plan=tp)


def check_reach(case):
    """The edges each case is there for, asserted on the plan mirror."""
    name, rows, ls = case.name, case.plan.rows, case.layers
    if name == "c130_o132":
        r, l = rows[1], ls[1]
        assert r.dw_grid[1:] == (2, 2) and l.cin % 128 == 2 and l.cout % 128 == 4 and l.cin % 4 == 2 and r.M == 140
        assert r.dw_rows == 16 and r.dw_ranges == 9 and 70 % r.dw_rows != 0  # the range of rows 64 .. 79 holds frames of both entries
        assert 70 % DW_STEP != 0 and r.last_range_rows == 12                    # ... inside one 8-row step; the last range is short
        assert r.dx_split >= 1 and _cdiv(l.cin, 128) == 2                       # the dX conv: two column tiles
    elif name == "c9_s2_odd":
        assert ls[0].stride == 2 and case.L % 2 == 1 and ls[0].cin == 9 and rows[0].dx_split == 0 and rows[0].fwd.Lout == 5
    elif name == "k7_d2":
        assert ls[1].taps == 7 and ls[1].dil == 2 and rows[1].lead == 12 and rows[1].dx_split > 1
    elif name == "one_by_one":
        assert ls[1].taps == 1 and ls[1].role == PLAIN and rows[1].lead == 0 and ls[2].role == FINAL and rows[2].dx_split == 1
    elif name == "lookahead2":
        assert rows[1].lead == 4 - 2 and rows[1].fwd.Lout == rows[1].fwd.Lin - 2
    elif name == "rows_127":
        assert rows[0].M == 127 and rows[0].dw_rows == 8 and rows[0].dw_ranges == 16 and rows[0].last_range_rows == 7
    elif name == "rows_129":
        assert rows[0].M == 129 and rows[0].dw_rows == 16 and rows[0].dw_ranges == 9 and rows[0].last_range_rows == 1
    elif name.startswith("triple"):
        assert [l.role for l in ls] == [PLAIN, RESIDUAL, FIRST, LAST] and rows[1].dx_split and rows[2].dx_split and not rows[0].dx_split
        assert (case.keep[2] is not None) == (name == "triple_dropout")
    else:
        raise AssertionError(f"no reach stated for {name}")


# ---- the float64 oracle, from the definition ------------------------------------------------------------------------------------
def _phi(z):
    return np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def _Phi(z):
    return 0.5 * (1.0 + _erf(z / math.sqrt(2.0)))


def oracle(case):
    """out (N, L_out, cout) and per layer {"W", "b", "gamma", "beta"} gradients of sum(out * G), float64.  Also per layer sum|dy| per
    channel (the bound of an exactly zero bias gradient)."""
    N = case.N
    cur, res, tape = case.x.astype(np.float64), None, []
    for i, l in enumerate(case.layers):
        W, s, d = l.W.astype(np.float64), l.stride, l.dil
        Xt = np.concatenate([np.zeros((N, l.cin, case.lead[i])), cur], axis=2)
        Lout = (Xt.shape[2] - (l.taps - 1) * d - 1) // s + 1
        t = np.arange(Lout)
        y = np.zeros((N, l.cout, Lout)) + l.b.astype(np.float64)[None, :, None]
        for j in range(l.taps):
            y += np.einsum("oc,nct->not", W[:, :, j], Xt[:, :, t * s + j * d])
        gam = 1.0 if l.gamma is None else l.gamma.astype(np.float64)[None, :, None]
        bet = 0.0 if l.beta is None else l.beta.astype(np.float64)[None, :, None]
        xh = rstd = None
        if l.norm == NORM_INSTANCE:
            mu = y.mean(axis=2, keepdims=True)
            rstd = 1.0 / np.sqrt(((y - mu) ** 2).mean(axis=2, keepdims=True) + l.eps)
        elif l.norm == NORM_BATCH:
            mu = l.mean.astype(np.float64)[None, :, None]
            rstd = 1.0 / np.sqrt(l.var.astype(np.float64) + l.eps)[None, :, None]
        h = y
        if l.norm != NORM_NONE:
            xh = (y - mu) * rstd
            h = xh * gam + bet
        z = h + res if l.role & LAST else h
        act = not is_1x1(l.role)
        a = gelu64(z) if act else z
        scale = None
        if case.keep[i] is not None:
            scale = case.keep[i].transpose(0, 2, 1).astype(np.float64) / (1.0 - case.p[i])
            a = a * scale
        tape.append(SimpleNamespace(Xt=Xt, Lout=Lout, xh=xh, rstd=rstd, z=z, act=act, scale=scale, gam=gam))
        if l.role == RESIDUAL:
            res = a
        else:
            cur = a
    out = np.ascontiguousarray(cur.transpose(0, 2, 1))
    dcur, dres, dx_first, grads = case.G.astype(np.float64).transpose(0, 2, 1), None, None, [None] * len(case.layers)
    for i in reversed(range(len(case.layers))):
        l, T = case.layers[i], tape[i]
        dO = dres if l.role == RESIDUAL else dcur
        da = dO * T.scale if T.scale is not None else dO
        dz = da * (_Phi(T.z) + T.z * _phi(T.z)) if T.act else da
        if l.role & LAST:
            dres = dz
        g = {"gamma": None, "beta": None}
        if l.norm == NORM_INSTANCE:
            gg = dz * T.gam
            dy = T.rstd * (gg - gg.mean(axis=2, keepdims=True) - T.xh * (gg * T.xh).mean(axis=2, keepdims=True))
        elif l.norm == NORM_BATCH:
            dy = dz * T.gam * T.rstd
        else:
            dy = dz
        if l.norm != NORM_NONE and l.gamma is not None:
            g["gamma"], g["beta"] = (dz * T.xh).sum(axis=(0, 2)), dz.sum(axis=(0, 2))
        g["b"] = dy.sum(axis=(0, 2))
        g["dyabs"] = np.abs(dy).sum(axis=(0, 2))
        W = l.W.astype(np.float64)
        t = np.arange(T.Lout)
        dW, dXt = np.zeros_like(W), np.zeros_like(T.Xt)
        for j in range(l.taps):
            idx = t * l.stride + j * l.dil
            dW[:, :, j] = np.einsum("not,nct->oc", dy, T.Xt[:, :, idx])
            np.add.at(dXt, (slice(None), slice(None), idx), np.einsum("oc,not->nct", W[:, :, j], dy))
        g["W"] = dW
        grads[i] = g
        dx = dXt[:, :, case.lead[i]:]
        if l.role & FIRST:
            dx_first = dx
        elif l.role == RESIDUAL:
            dcur = dx_first + dx
        else:
            dcur = dx
    return SimpleNamespace(out=out, grads=grads)


# ---- the same in torch (autograd), for the bar and as a check of the oracle -----------------------------------------------------
def torch_train(case, dtype):
    F = torch.nn.functional
    T = lambda a: None if a is None else torch.from_numpy(a).to(dtype)
    P = [{k: (None if v is None else T(v).requires_grad_()) for k, v in (("W", l.W), ("b", l.b), ("gamma", l.gamma), ("beta", l.beta))}
         for l in case.layers]
    cur, res = T(case.x), None
    for i, (l, q) in enumerate(zip(case.layers, P)):
        y = F.conv1d(F.pad(cur, (case.lead[i], 0)), q["W"], q["b"], stride=l.stride, dilation=l.dil)
        if l.norm == NORM_BATCH:
            y = F.batch_norm(y, T(l.mean), T(l.var), q["gamma"], q["beta"], training=False, eps=l.eps)
        elif l.norm == NORM_INSTANCE:
            y = F.instance_norm(y, weight=q["gamma"], bias=q["beta"], use_input_stats=True, eps=l.eps)
        if l.role & LAST:
            y = y + res
        if not is_1x1(l.role):
            y = F.gelu(y)
        if case.keep[i] is not None:
            y = y * T(case.keep[i]).permute(0, 2, 1) / (1.0 - case.p[i])
        if l.role == RESIDUAL:
            res = y
        else:
            cur = y
    out = cur.permute(0, 2, 1)
    (out * T(case.G)).sum().backward()
    grads = [{k: (None if v is None else v.grad.numpy().astype(np.float64)) for k, v in q.items()} for q in P]
    return out.detach().numpy().astype(np.float64), grads


GRAD_KEYS = ("W", "b", "gamma", "beta")


def zero_bias(l):
    return l.norm == NORM_INSTANCE


def bars(case, want):
    """Per layer and tensor: FACTOR x max(the torch composition's own fp32 error against the oracle, one rounding of the largest entry);
    for the exactly zero bias gradient of a conv in front of an instance norm the M-term bound M 2^-24 sum|dy| per channel (an array).
    Neither comes from the engine."""
    out32, g32 = torch_train(case, torch.float32)
    e_out = float(np.abs(out32 - want.out).max())
    out_bar = FACTOR * max(e_out, 2.0 ** -23 * float(np.abs(want.out).max()))
    res = []
    for l, r, g, w in zip(case.layers, case.plan.rows, g32, want.grads):
        b = {}
        for k in GRAD_KEYS:
            if w[k] is None:
                continue
            if k == "b" and zero_bias(l):
                b[k] = r.M * 2.0 ** -24 * w["dyabs"]
            else:
                b[k] = FACTOR * max(float(np.abs(g[k] - w[k]).max()), 2.0 ** -23 * float(np.abs(w[k]).max()))
        res.append(b)
    return out_bar, res


@functools.lru_cache(maxsize=None)
def prepared(name, kind):
    case = build(name, kind)
    want = oracle(case)
    return case, want, bars(case, want)
