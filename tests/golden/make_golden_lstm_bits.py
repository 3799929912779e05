"""Record what rnnt_amd/csrc/lstm.hip leaves behind, for tests/test_lstm_bits_gpu.py: the predictor's training and inference forward and
its backward, the lockstep greedy loop, the device streams and the predictor step of the beam search share one LSTM cell body, one
scratch layout and their argument checks, so the file can be rearranged freely as
long as every case keeps every bit: tokens, state words and scores raw, every float buffer — out, state_out, saved, every gradient,
the call's WHOLE workspace and a stream group's whole block — as SHA-256.

Run once on a GPU with the library whose output is the reference (RNNT_ENGINE_LIB = the build of the commit BEFORE the change):
    python tests/golden/make_golden_lstm_bits.py
writes tests/golden/lstm_bits.npz.  Every call goes through the C ABI with buffers of THIS module's: exactly the bytes the size
query asks for, every word the quiet-NaN pattern of make_golden_decode_bits.py (whose workspace replacement runs the decode
entries here too), hashed whole after the call.  The shapes are the existing case lists' (tests/lstm_predictor_cases.EDGES,
tests/lstm_decode_cases.WIDTHS / WIRING_TEXT / batch_mels): the smallest at which these kernels can go wrong.

A case is written only if the assertion the existing test makes about it holds on the recording build — forward and backward within
the bar of tests/test_lstm_predictor_gpu.py's test_edges (4 x the error of the module's fp32 torch path) of the float64 torch
path; greedy and stream token lists equal to the float64 oracle's under its margin premise (checked_oracle; a truncated utterance:
the labels the oracle emitted at its frames); a beam search's beam-1 run equal to the greedy list — and a second run gives the same
bytes.  So a broken build cannot be recorded.  This module is also the test's source of the cases and of the code that runs them."""
import copy
import ctypes
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import lstm_decode_cases as dc  # noqa: E402
from tests import lstm_predictor_cases as lc  # noqa: E402
from tests.helpers import sha256_of_arrays  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_golden_decode_bits", os.path.join(HERE, "make_golden_decode_bits.py"))
D = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(D)

GOLDEN = os.path.join(HERE, "lstm_bits.npz")
PATTERN, ALL = D.PATTERN, D.ALL
RAW_KEYS = ("state", "tokens", "labels", "scores")  # int32 words and float64 scores kept as they are; every other key as a SHA-256
DROPOUT_P = 0.3
# a stream's frames in three pushes: the head of test_lstm_stream_gpu.py's "uneven" plan (3 frames, an empty push) and the rest
UNEVEN = lambda T: [3, 0, T - 3]  # noqa: E731
# three streams of the batch (utterances 0, 2, 3: T = 23, 9, 14), the second sitting the second push out
GROUP_UTT, GROUP_PLANS = (0, 2, 3), ([8, 7, 8], [4, None, 5], [5, 5, 4])

EDGES = {e.name: e for e in lc.EDGES}
# name -> (kind, what, options)
CASES = {}
for _e in lc.EDGES:  # rnnt_engine_lstm_predictor_fwd (saved / saved = NULL) and _bwd
    CASES["pred/" + _e.name] = ("pred", _e.name, dict(dropout=False))
for _n in ("hd260", "l3_noln_state"):  # a seeded keep mask: the second unit pass; the bias-in-xg route and an initial state
    CASES["pred_dropout/" + _n] = ("pred", _n, dict(dropout=True))
for _c in dc.WIDTHS + [dc.WIRING_TEXT]:  # rnnt_engine_greedy_decode_lstm
    CASES["greedy/" + _c.name] = ("greedy", _c.name, dict(n=1))
for _n in (3, 32):  # the ragged batch, state_out requested
    CASES["greedy/batch_n%d" % _n] = ("greedy", "batch", dict(n=_n))
for _n in ("hd260", "wiring_text"):  # rnnt_engine_greedy_stream_lstm_*
    CASES["stream/" + _n] = ("stream", _n, {})
CASES["stream/batch_n3"] = ("stream", "batch", {})
for _n in ("hd260", "l3_noln", "wiring_text"):  # rnnt_engine_beam_decode_lstm: a row tile holds two utterances, three are a tile and a half
    CASES["beam/" + _n] = ("beam", _n, dict(n=3, beam=4))
CASES["beam/hd260_beam1"] = ("beam", "hd260", dict(n=3, beam=1))

_np = D._np


def _buf(nbytes, dev="cuda"):
    """A buffer of exactly `nbytes` (rounded up to words), every word PATTERN."""
    return torch.full(((int(nbytes) + 3) // 4,), PATTERN, dtype=torch.int32, device=dev).view(torch.uint8)


def _floats(*shape):
    return _buf(4 * int(np.prod(shape))).view(torch.float32).view(*shape)


def _words(t):
    return _np(t.contiguous().view(torch.uint8).view(torch.int32))


# ---- the predictor -----------------------------------------------------------------------------------------------------------------------
_pred_cache = {}


def pred_case(name, dropout):
    """The edge's float32 module on the device, its inputs, and the float64 torch path's result with the bar of test_edges (once)."""
    key = (name, dropout)
    if key not in _pred_cache:
        e = EDGES[name]
        s = e.spec
        ids, G, state = lc.edge_inputs(e)
        keep = None
        if dropout:
            keep = (torch.rand((s["L"], s["B"], s["U1"], s["Hd"]), generator=torch.Generator().manual_seed(50 + s["seed"])) >= DROPOUT_P).to(torch.uint8)
            assert 0.5 < keep.float().mean() < 0.9
        m64 = lc.seeded_module(s, dropout=DROPOUT_P)
        mode = (lambda m: m.train()) if dropout else (lambda m: m.eval())
        ref = lc.run(mode(m64), ids, G, state, keep_masks=keep)
        assert m64.last_backend == "torch"
        got32 = lc.run(mode(copy.deepcopy(m64).float()), ids, G, state, keep_masks=keep)
        bar = 4.0 * max(lc.rel_err(got32[k], ref[k]) for k in ref)
        _pred_cache[key] = (e, copy.deepcopy(m64).float().cuda().eval(), ids, G, state, keep, ref, bar)
    return _pred_cache[key]


def run_pred(engine, name, dropout):
    from rnnt_amd.lstm_predictor import _struct
    e, m, ids, G, state, keep, ref, bar = pred_case(name, dropout)
    s = e.spec
    B, U1, L, Hd, ln = s["B"], s["U1"], s["L"], s["Hd"], s["ln"]
    dims = (B, U1, s["S"], s["E"], Hd, s["O"], L, int(ln))
    params = [t.detach() for t in m._params()]
    assert all(t.is_contiguous() for t in params)
    eps = [ctypes.c_float(x) for x in (float(m.input_layer_norm.eps), m.lstm_layer_norm_epsilon, float(m.output_layer_norm.eps))]
    ids_d, d_out = ids.cuda(), G.float().cuda().contiguous()
    state_in = None if state is None else torch.stack([torch.stack([h, c]) for h, c in state]).float().cuda().contiguous()
    keep_d = None if keep is None else keep.cuda().contiguous()
    p = ctypes.c_float(DROPOUT_P if dropout else 0.0)
    lib, n = engine.lib(), ctypes.c_size_t(0)
    sp, _a = _struct(params, L, ln)
    stream = engine._stream(ids_d.device)

    def forward(train):
        saved = None
        if train:
            engine._check(lib.rnnt_engine_lstm_predictor_saved_bytes(*dims, ctypes.byref(n)))
            saved = _buf(n.value)
        engine._check(lib.rnnt_engine_lstm_predictor_workspace_bytes(*dims, 0, ctypes.byref(n)))
        ws, out, state_out = _buf(n.value), _floats(B, U1, s["O"]), _floats(L, 2, B, Hd)
        engine._check(lib.rnnt_engine_lstm_predictor_fwd(
            engine._p(ids_d), *dims, ctypes.byref(sp), engine._p(state_in), engine._p(keep_d), p, *eps, engine._p(out), engine._p(state_out),
            engine._p(saved), ctypes.c_size_t(saved.numel() if train else 0), engine._p(ws), ctypes.c_size_t(ws.numel()), stream))
        return out, state_out, saved, ws

    out_t, st_t, saved, ws_t = forward(True)
    out_i, st_i, _, ws_i = forward(False)
    grads = [_floats(*t.shape) for t in params]
    sg, _b = _struct(grads, L, ln)
    engine._check(lib.rnnt_engine_lstm_predictor_workspace_bytes(*dims, 1, ctypes.byref(n)))
    ws_b = _buf(n.value)
    engine._check(lib.rnnt_engine_lstm_predictor_bwd(
        engine._p(ids_d), *dims, ctypes.byref(sp), engine._p(keep_d), p, *eps, engine._p(d_out), ctypes.byref(sg), engine._p(saved),
        ctypes.c_size_t(saved.numel()), engine._p(ws_b), ctypes.c_size_t(ws_b.numel()), stream))
    torch.cuda.synchronize()
    # the existing test's assertion: every tensor within the bar of the float64 torch path
    names = {t.data_ptr(): k for k, t in m.named_parameters()}
    got = {"out": _np(out_t), "state": _np(st_t)}
    got.update({"grad__" + names[t.data_ptr()].replace(".", "__"): _np(g) for t, g in zip(params, grads)})
    for k in ref:
        assert lc.rel_err(got[k], ref[k]) <= bar, (name, k, lc.rel_err(got[k], ref[k]), bar)
    for k, v in (("out", out_i), ("state", st_i)):  # the call that keeps nothing computes the same function
        assert lc.rel_err(_np(v), ref[k]) <= bar, (name, k, "saved = NULL")
    res = dict(out_train=_words(out_t), state_out_train=_words(st_t), saved=_words(saved), workspace_train=_words(ws_t),
               out_infer=_words(out_i), state_out_infer=_words(st_i), workspace_infer=_words(ws_i), workspace_bwd=_words(ws_b))
    res.update({"grad%02d" % i: _words(g) for i, g in enumerate(grads)})
    return res


# ---- the decode entries --------------------------------------------------------------------------------------------------------------
_model_cache = {}


def _on_device(model64):
    model = copy.deepcopy(model64).float().cuda().eval()
    tl = getattr(model.joint, "text_ln", None)
    args = (model.predictor._decode_bundle(), tl.weight if tl is not None else None, tl.bias if tl is not None else None,
            model.joint.joint_ln.weight, model.joint.joint_ln.bias, model.joint.blank_idx)
    return model, args


def utterances(what, n):
    """(device model, the entries' model arguments, [mel (1, H, T_u) float32 on the device], [the float64 oracle of each], max_length,
    max_per_frame) — a case: the whole utterance, then ever shorter heads of it (the greedy decode is causal: the oracle of a head is the
    labels emitted at its frames); "batch": the first n utterances of the ragged batch."""
    if what not in _model_cache:
        if what == "batch":
            _model_cache[what] = _on_device(lc.wiring_model()) + (None,)
        else:
            case = dc.BY_NAME[what]
            _model_cache[what] = _on_device(dc.build_model(case)) + (dc.checked_oracle(case),)  # the margin premise, in float64 on the CPU
    model, args, o = _model_cache[what]
    if what == "batch":
        mels, oracles = dc.batch_mels()[:n], dc.batch_oracles()[:n]
        return model, args, [m.float().cuda() for m in mels], [(x.tokens, x.per_frame) for x in oracles], 200, 10
    case = dc.BY_NAME[what]
    mel, T = dc.case_frames(case).float().cuda(), case.T
    lens = [max(1, T // (u + 1) + (u > 0)) for u in range(n)]
    return (model, args, [mel[..., :k].contiguous() for k in lens], [(o.tokens[:sum(o.per_frame[:k])], o.per_frame[:k]) for k in lens],
            case.max_length, case.max_per_frame)


def _frames(model, mel):
    return model._decode_frames(mel.permute(0, 2, 1))


def run_greedy(engine, own, what, n):
    model, args, mels, oracles, ml, mpf = utterances(what, n)
    state, tokens, state_out, _ = engine.greedy_decode_lstm([_frames(model, m) for m in mels], *args, ml, max_per_frame=mpf, scan_frames=32,
                                                            chunk=ALL)
    (ws,) = own.words()
    st, tk = _np(state), _np(tokens)
    res = dict(state=st, state_out=_words(state_out), workspace=ws)
    for u, (want, _) in enumerate(oracles):
        res["tokens%d" % u] = tk[u, :1 + st[u, engine.DECODE_NTOK]].copy()
        assert res["tokens%d" % u][1:].tolist() == want, (what, n, u)
    return res


def run_stream(engine, own, what):
    if what == "batch":
        model, args, mels, oracles, ml, mpf = utterances("batch", max(GROUP_UTT) + 1)
        mels, oracles, plans = [mels[i] for i in GROUP_UTT], [oracles[i] for i in GROUP_UTT], GROUP_PLANS
    else:
        model, args, mels, oracles, ml, mpf = utterances(what, 1)
        plans = [UNEVEN(mels[0].shape[-1])]
    assert all(sum(k or 0 for k in p) == m.shape[-1] and len(p) == 3 for p, m in zip(plans, mels))
    n = len(mels)
    S, E, Hd, O, L, ln = model.predictor._decode_sizes()
    H, V, blank = mels[0].shape[1], args[3].shape[0], args[5]
    block = _buf(engine.greedy_stream_lstm_bytes(n, S, E, Hd, O, L, ln, H, V, args[1] is not None))
    engine.greedy_stream_lstm_init(block, n, L, Hd, H, blank)
    res, at, labels = {}, [0] * n, [[] for _ in range(n)]
    for k in range(3):
        chunks = []
        for j, p in enumerate(plans):
            chunks.append(_frames(model, mels[j][..., at[j]:at[j] + p[k]]) if p[k] else None)
            at[j] += p[k] or 0
        count = max(0 if c is None else c.shape[0] for c in chunks)
        out = torch.full((n, max(1, count * mpf)), PATTERN, dtype=torch.int32, device="cuda")
        before = len(own.bufs)
        engine.greedy_stream_lstm_push(chunks, *args, ml, mpf, 32, block, out, chunk=ALL, in_flight=None)
        torch.cuda.synchronize()
        st = _np(engine.greedy_stream_lstm_views(block, n, L, Hd, H)[0]).copy()
        res["state%d" % k], res["block%d" % k] = st, _words(block)
        if count:  # (a push without any frame enqueues nothing and asks for no workspace)
            assert len(own.bufs) == before + 1
            res["workspace%d" % k] = own.words()[before]
            for j in range(n):
                if chunks[j] is not None:
                    res["labels%d_%d" % (k, j)] = _np(out)[j, :st[j, engine.LSTM_STREAM_PUSH_LABELS]].copy()
                    labels[j] += res["labels%d_%d" % (k, j)].tolist()
        for j, (want, per_frame) in enumerate(oracles):  # after every push: the greedy decode of the frames so far
            assert labels[j] == want[:sum(per_frame[:at[j]])], (what, k, j)
    return res


def run_beam(engine, own, what, n, beam):
    model, args, mels, oracles, ml, mpf = utterances(what, n)
    frames = [_frames(model, m) for m in mels]
    search = lambda b: engine.beam_decode_lstm(frames, *args, ml, b, max_per_frame=mpf, chunk=ALL, in_flight=None)  # noqa: E731
    state, tokens, _ = search(1)
    torch.cuda.synchronize()
    st1, tk1 = _np(state).reshape(-1, 32), _np(tokens).reshape(-1, 1, ml)
    for u, (want, _) in enumerate(oracles):  # the beam-1 search is the greedy decode
        assert tk1[u, 0, 1:1 + st1[u, D.BS_LEN]].tolist() == want, (what, u)
    before = len(own.bufs)
    state, tokens, scores = search(beam)
    ws = own.words()[before]
    st, tk, sc = _np(state).reshape(-1, 32), _np(tokens).reshape(-1, beam, ml), _np(scores).reshape(-1, beam)
    assert st[:, D.BS_DONE].all(), (what, st)
    res = dict(state=st, workspace=ws)
    for u in range(n):
        k = int(st[u, D.BS_N])
        res["scores%d" % u] = sc[u, :k].copy()
        for j in range(k):
            res["tokens%d_%d" % (u, j)] = tk[u, j, :1 + st[u, D.BS_LEN + j]].copy()
    return res


def run_case(engine, name):
    kind, what, o = CASES[name]
    if kind == "pred":
        return run_pred(engine, what, o["dropout"])
    with D.own_workspace(engine) as own:
        if kind == "greedy":
            return run_greedy(engine, own, what, o["n"])
        if kind == "stream":
            return run_stream(engine, own, what)
        if kind == "beam":
            return run_beam(engine, own, what, o["n"], o["beam"])
    raise KeyError(kind)


def run_checked(engine, name):
    """One run of a case (its validity asserted on the way) as the fixture keeps it."""
    return {k: (a if k.rstrip("0123456789_") in RAW_KEYS else np.array(sha256_of_arrays(a))) for k, a in run_case(engine, name).items()}


def same(first, second):
    return sorted(first) == sorted(second) and all(np.array_equal(first[k], second[k]) for k in first)


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
        print("%-28s ok %s" % (name, sorted(first)), flush=True)
    np.savez_compressed(GOLDEN, **out)
    print("%d cases -> %s (%d bytes)" % (len(CASES), GOLDEN, os.path.getsize(GOLDEN)), flush=True)


if __name__ == "__main__":
    main()
