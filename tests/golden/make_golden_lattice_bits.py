"""Record what rnnt_amd/csrc/lattice.hip, ctc.hip and align.hip leave behind, for tests/test_lattice_bits_gpu.py: the loss tail —
log-softmax gather, the lp_emit pass (delay penalty / alignment restriction), the alpha / beta sweep in its three forms (one wave,
wave chain with mailboxes, barrier sweep), the delay cost, the six coefficient kernels, grad_logits — the CTC head's chain and the
forced alignment share leaf pieces and one argument block, so the files can be rearranged freely as long as every case keeps every
bit.

Run once on a GPU with the library whose output is the reference (RNNT_ENGINE_LIB = the build of the commit BEFORE the change):
    python tests/golden/make_golden_lattice_bits.py
writes tests/golden/lattice_bits.npz.  The standalone and CTC entries run on a workspace of THIS module's: exactly the bytes the
size query asks for, every word the quiet-NaN pattern of make_golden_decode_bits.py, hashed whole after the call.  Costs, scores and
frames are kept raw (int32 views: NaN payloads and the sign of zero survive); every other array raw where it is at most RAW_BYTES
long and as SHA-256 otherwise (the committed file has to stay small: the gradients of the two-wave shape alone would be 1.2 MB).

The shapes are the smallest at which each path can go wrong (SHAPES); the lengths are ragged and hold T_b = 1 and U_b = 0 wherever
the batch has a second utterance to hold them (the barrier shape is one utterance, a little shorter than its buffers).
A case is written only if what is known about it holds on the recording build — plain costs against the float64 oracle, +inf and
dead coefficients for the window without a path, NaN for the NaN logit, flushed AND unflushed cells in the f16x2 coefficients — and
a second run gives the same bytes.  This module is also the test's source of the cases and of the code that runs them."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import ctc_cases  # noqa: E402
from tests.helpers import make_inputs, sha256_of_arrays  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_golden_decode_bits", os.path.join(HERE, "make_golden_decode_bits.py"))
D = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(D)

GOLDEN = os.path.join(HERE, "lattice_bits.npz")
RAW_BYTES = 8192
ALWAYS_RAW = ("costs", "costs_nograd", "scores", "frames", "coef_null")
LEFT, RIGHT = 1, 2
LAMBDA, DELTA = 0.01, 0.02

# name -> (B, T, U1, V, logit_lens, target_lens)
SHAPES = {
    "one_wave": (3, 9, 6, 8, [9, 1, 5], [5, 2, 0]),        # no mailbox
    "two_waves": (2, 40, 70, 8, [40, 1], [69, 0]),
    "three_waves": (2, 20, 129, 8, [20, 1], [128, 0]),     # the column count one past a wave edge
    "barrier": (1, 170, 520, 4, [167], [517]),             # the mailboxes do not fit in LDS
}
# name -> (fastemit lambda, delay penalty, restricted); "plain" goes through rnnt_engine_loss_fwd_bwd, an option through _reg, a
# restriction through _restrict
MODES = {
    "plain": (0.0, 0.0, False),
    "lambda": (LAMBDA, 0.0, False),
    "delta": (0.0, DELTA, False),
    "lambda_delta": (LAMBDA, DELTA, False),
    "restrict": (0.0, 0.0, True),
    "restrict_lambda": (LAMBDA, 0.0, True),
    "restrict_delta": (0.0, DELTA, True),
}
FUSED_DIMS = (2, 40, 69, 128, 128)  # the two-wave shape at H = V = 128; inputs as tests/test_x2_flush_skip_gpu.py makes them
FUSED_SEED, FUSED_GRAD_SCALE = 11, 0.5  # (tests/x2_flush_twin.py CASES["u1_63"])
# the fused restricted calls' window: wide enough that cells the flush rule takes stay reachable (at left 1, right 2 every cell
# that a path still crosses is far above the rule's threshold, and the RS + FLUSH kernel would never flush)
FUSED_LEFT, FUSED_RIGHT = 20, 30
# name -> (dtype, lambda, restricted): the coefficient kernel's FLUSH, RS + FLUSH, plain, RS and FE instantiations
FUSED = {
    "x2_plain": ("f16x2", 0.0, False),
    "x2_restrict": ("f16x2", 0.0, True),
    "f32_plain": ("fp32", 0.0, False),
    "f32_restrict": ("fp32", 0.0, True),
    "x2_lambda": ("f16x2", LAMBDA, False),
}
# name -> (N, T, U, V, logit_lens, target_lens, what)
CTC = {
    "one_wave": (3, 12, 5, 8, [12, 1, 7], [5, 0, 3], None),
    "two_waves": (2, 20, 70, 8, [20, 9], [70, 0], None),            # (T < U: utterance 0 has no path; utterance 1 has no label)
    "two_waves_feasible": (2, 90, 70, 8, [90, 80], [70, 66], None),
    "barrier": (1, 700, 520, 4, [700], [520], None),
    "infeasible": (3, 12, 5, 8, [12, 6, 7], [5, 5, 3], "infeasible"),  # utterance 1: five equal labels in six frames
    "weights_zero": (3, 12, 5, 8, [12, 1, 7], [5, 0, 3], "weights"),
}

CASES = {}
for _s in SHAPES:
    for _m in MODES:
        CASES["loss/%s/%s" % (_s, _m)] = ("loss", _s, _m)
CASES["loss/one_wave/no_path"] = ("loss", "one_wave", "no_path")
CASES["loss/one_wave/nan_logit"] = ("loss", "one_wave", "nan_logit")
for _f in FUSED:
    CASES["fused/" + _f] = ("fused", _f, None)
for _c in CTC:
    CASES["ctc/" + _c] = ("ctc", _c, None)
for _s in ("one_wave", "two_waves"):
    CASES["align/" + _s] = ("align", _s, None)


def chain_mailbox_bytes(columns, steps):
    """launch_lattice's / launch_ctc_loss's formula: 8 B value + 4 B tag per wave boundary and step; the chained sweep runs while
    this fits in 64 KiB of LDS, the barrier form beyond."""
    return ((columns + 63) // 64 - 1) * steps * 12


def _dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def _words(t):
    return t.detach().contiguous().view(torch.uint8).view(torch.int32).cpu().numpy()


def _align_up(x):
    return (x + 255) & ~255


def loss_coef_words(ws_words, B, T, U1):
    """The coef region [B*T*U1, 4] of the standalone entries' workspace (engine.hip carve_loss_ws)."""
    skew, cells = B * (T + U1 - 1) * U1, B * T * U1
    co = 3 * _align_up(skew * 4) + 2 * _align_up(skew * 8)
    assert (co + _align_up(cells * 16) + 256 + 3) // 4 == ws_words.size, (co, ws_words.size)
    return ws_words[co // 4:co // 4 + 4 * cells].reshape(cells, 4)


def coef_null(c):
    """[cells] bool: the coefficients of a cell outside the lattice (c1 = -inf, sb = se = +0, y = -1), from int32 words."""
    return (c[:, 0] == np.float32(-np.inf).view(np.int32)) & (c[:, 1] == 0) & (c[:, 2] == 0) & (c[:, 3] == -1)


def inside(B, T, U1, ll, tl):
    m = np.zeros((B, T, U1), dtype=bool)
    for b in range(B):
        m[b, :ll[b], :tl[b] + 1] = True
    return m.reshape(-1)


def window_frames(B, U, ll, tl):
    """frames[b,u] = the frame label u is emitted at on an evenly spread path: a window of any width around it leaves that path."""
    f = np.zeros((B, max(U, 1)), dtype=np.int32)
    for b in range(B):
        for u in range(tl[b]):
            f[b, u] = min(ll[b] - 1, (u * ll[b]) // (tl[b] + 1))
    return f[:, :U] if U else f[:, :0]


_inputs = {}


def loss_inputs(shape):
    if shape not in _inputs:
        B, T, U1, V, ll, tl = SHAPES[shape]
        rng = np.random.default_rng(1000 + len(shape) + U1)
        x = rng.standard_normal((B, T, U1, V)).astype(np.float32)
        tg = rng.integers(0, V - 1, (B, U1 - 1)).astype(np.int32)
        _inputs[shape] = (x, tg, np.array(ll), np.array(tl), window_frames(B, U1 - 1, ll, tl))
    return _inputs[shape]


# ---- the standalone loss entries -----------------------------------------------------------------------------------------------------
def run_loss(engine, shape, mode):
    B, T, U1, V, _, _ = SHAPES[shape]
    x, tg, ll, tl, frames = loss_inputs(shape)
    blank = V - 1
    if shape == "barrier":
        assert chain_mailbox_bytes(U1, T + U1 - 1) > 64 * 1024
    elif shape != "one_wave":
        assert 0 < chain_mailbox_bytes(U1, T + U1 - 1) <= 64 * 1024
    if mode == "nan_logit":
        x = x.copy()
        x[0, 2, 1, 3] = np.nan  # t = 2 < T_0, u = 1 <= U_0
    if mode == "no_path":
        frames = frames.copy()
        frames[0, 0], frames[0, 1] = 8, 0  # label 0 not before frame 7, label 1 not after frame 2
    lam, delta, restricted = MODES.get(mode, (0.0, 0.0, mode == "no_path"))
    xd, tgd, lld, tld, fd = _dev(x, torch.float32), _dev(tg, torch.int32), _dev(ll, torch.int32), _dev(tl, torch.int32), _dev(frames, torch.int32)

    def call(want_grad):
        with D.own_workspace(engine) as own:
            if restricted:
                costs, grad = engine.loss_fwd_bwd_restrict(xd, tgd, lld, tld, blank, -1.0, lam, delta, fd, LEFT, RIGHT, want_grad=want_grad)
            elif lam or delta:
                costs, grad = engine.loss_fwd_bwd_reg(xd, tgd, lld, tld, blank, -1.0, lam, delta, want_grad=want_grad)
            else:
                costs, grad = engine.loss_fwd_bwd(xd, tgd, lld, tld, blank, want_grad=want_grad)
            (ws,) = own.words()
        return _words(costs), grad, ws

    costs, grad, ws = call(True)
    costs_ng, _, ws_ng = call(False)
    coef = loss_coef_words(ws, B, T, U1)
    c = costs.view(np.float32)
    if mode == "plain" and shape != "barrier":
        from oracle import cpu_oracle
        ref = cpu_oracle.rnnt_loss(x.astype(np.float64), tg, ll, tl, blank=blank, want_grad=False)[0]
        assert np.allclose(c, ref, rtol=1e-4, atol=1e-4), (shape, c, ref)
    if mode == "no_path":
        assert c[0] == np.inf and np.isfinite(c[1:]).all(), c
        assert coef_null(coef)[:T * U1].all() and not coef_null(coef)[T * U1:][inside(B, T, U1, ll, tl)[T * U1:]].all()
        assert (_words(grad)[0] == 0).all() and (_words(grad)[2] != 0).any()
    elif mode == "nan_logit":
        assert np.isnan(c[0]) and np.isfinite(c[1:]).all(), c
    else:
        assert np.isfinite(c).all(), (shape, mode, c)
    return dict(costs=costs, grad_logits=_words(grad), coef=coef.copy(), workspace=ws, costs_nograd=costs_ng, workspace_nograd=ws_ng)


# ---- the fused entries ---------------------------------------------------------------------------------------------------------------
def run_fused(engine, name):
    dtype, lam, restricted = FUSED[name]
    B, T, U, H, V = FUSED_DIMS
    d = make_inputs(B, T, U, H, V, FUSED_SEED, ragged=True)
    g = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    ll, tl = d["logit_lens"], d["target_lens"]
    args = (g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"], V - 1, FUSED_GRAD_SCALE)
    with D.own_workspace(engine) as own:
        if restricted:
            outs = engine.joint_loss_fwd_bwd_restrict(*args, lam, 0.0, _dev(window_frames(B, U, ll, tl), torch.int32), FUSED_LEFT, FUSED_RIGHT,
                                                      dtype=dtype)
        elif lam:
            outs = engine.joint_loss_fwd_bwd_reg(*args, lam, 0.0, dtype=dtype)
        else:
            outs = engine.joint_loss_fwd_bwd(*args, dtype=dtype)
        ws = own.words()[-1]
    L = engine.layout(B, T, U + 1, H, V, dtype)
    cells = B * T * (U + 1)
    coef = ws[L.coef // 4:L.coef // 4 + 4 * cells].reshape(cells, 4).copy()
    null, ins = coef_null(coef), inside(B, T, U + 1, ll, tl)
    assert null[~ins].all() and np.isfinite(_words(outs[0]).view(np.float32)).all()
    if dtype == "f16x2" and not lam:  # the flush rule fired and did not take everything
        assert (null & ins).any() and (~null & ins).any(), name
    elif not restricted:
        assert not (null & ins).any(), name
    res = dict(costs=_words(outs[0]), coef=coef, coef_null=np.packbits(null))
    for k, t in zip(("grad_enc", "grad_pred", "grad_W", "grad_bias"), outs[1:]):
        res[k] = _words(t)
    return res


def flush_fired(golden_get):
    """What the f16x2 cases must show, from the recorded null masks: cells inside the lattice that the flush rule took — null beside
    a live cell of the fp32 route's same call — and cells it left, in the plain and in the restricted call."""
    B, T, U, _, _ = FUSED_DIMS
    d = make_inputs(*FUSED_DIMS, FUSED_SEED, ragged=True)
    ins = inside(B, T, U + 1, d["logit_lens"], d["target_lens"])
    out = {}
    for x2, f32 in (("x2_plain", "f32_plain"), ("x2_restrict", "f32_restrict")):
        a = np.unpackbits(golden_get("fused/%s/coef_null" % x2))[:ins.size].astype(bool)
        b = np.unpackbits(golden_get("fused/%s/coef_null" % f32))[:ins.size].astype(bool)
        out[x2] = (int((a & ~b & ins).sum()), int((~a & ins).sum()))
    return out


# ---- the CTC head ----------------------------------------------------------------------------------------------------------------------
def run_ctc(engine, name):
    N, T, U, V, ll, tl, what = CTC[name]
    rng = np.random.default_rng(2000 + T + U)
    x = rng.standard_normal((N, T, V)).astype(np.float32)
    tg = ctc_cases.make_targets(rng, N, U, V, V - 1, repeat_p=0.1)
    w = None
    if what == "infeasible":
        tg[1] = 3
    if what == "weights":
        w = _dev([0.7, 0.0, 1.9], torch.float32)
    if name == "barrier":
        assert chain_mailbox_bytes(U + 1, T) > 64 * 1024
    elif U + 1 > 64:
        assert 0 < chain_mailbox_bytes(U + 1, T) <= 64 * 1024
    with D.own_workspace(engine) as own:
        costs, grad = engine.ctc_loss_fwd_bwd(_dev(x, torch.float32), _dev(tg, torch.int32), _dev(ll, torch.int32), _dev(tl, torch.int32),
                                              V - 1, cost_weights=w)
        costs_ng, _ = engine.ctc_loss_fwd_bwd(_dev(x, torch.float32), _dev(tg, torch.int32), _dev(ll, torch.int32), _dev(tl, torch.int32),
                                              V - 1, cost_weights=w, want_grad=False)
        ws, ws_ng = own.words()
    c = _words(costs).view(np.float32)
    assert (c == np.inf).tolist() == ctc_cases.infeasible(tg, ll, tl).tolist() and not np.isnan(c).any(), (name, c)
    return dict(costs=_words(costs), grad_logits=_words(grad), workspace=ws, costs_nograd=_words(costs_ng), workspace_nograd=ws_ng)


def run_align(engine, shape):
    x, tg, ll, tl, _ = loss_inputs(shape)
    V = x.shape[-1]
    scores, frames = engine.align(_dev(x, torch.float32), _dev(tg, torch.int32), _dev(ll, torch.int32), _dev(tl, torch.int32), V - 1)
    torch.cuda.synchronize()
    fr = _words(frames).reshape(frames.shape)
    for b in range(len(ll)):  # a path: non-decreasing frames inside the utterance
        f = fr[b, :tl[b]]
        assert (np.diff(f) >= 0).all() and (f >= 0).all() and (f < ll[b]).all(), (shape, b, f)
        fr[b, tl[b]:] = 0  # (entries past U_b are not written)
    return dict(scores=_words(scores), frames=fr)


def run_case(engine, name):
    kind, what, mode = CASES[name]
    if kind == "loss":
        return run_loss(engine, what, mode)
    if kind == "fused":
        return run_fused(engine, what)
    if kind == "ctc":
        return run_ctc(engine, what)
    if kind == "align":
        return run_align(engine, what)
    raise KeyError(kind)


def run_checked(engine, name):
    """One run of a case (its validity asserted on the way) as the fixture keeps it."""
    return {k: (a if k in ALWAYS_RAW or a.nbytes <= RAW_BYTES else np.array(sha256_of_arrays(a))) for k, a in run_case(engine, name).items()}


def same(first, second):
    return sorted(first) == sorted(second) and all(
        first[k].dtype == second[k].dtype and np.array_equal(first[k], second[k]) for k in first)


def main():
    import rnnt_amd
    e = rnnt_amd.engine
    e.lib()
    print("recording from %s" % e.LIB_PATH, flush=True)
    out = {}
    for name in CASES:
        first, second = run_checked(e, name), run_checked(e, name)
        assert same(first, second), (name, [k for k in first if not np.array_equal(first[k], second.get(k))])
        for k, a in first.items():
            out["%s/%s" % (name, k)] = a
        print("%-34s ok %s" % (name, sorted(first)), flush=True)
    fired = flush_fired(lambda k: out[k])
    print("flush rule (flushed, live): %s" % fired, flush=True)
    assert all(f > 0 and l > 0 for f, l in fired.values()), fired
    np.savez_compressed(GOLDEN, **out)
    print("%d cases -> %s (%d bytes)" % (len(CASES), GOLDEN, os.path.getsize(GOLDEN)), flush=True)


if __name__ == "__main__":
    main()
