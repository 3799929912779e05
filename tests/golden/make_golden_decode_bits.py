"""Record what the decoders leave behind, for tests/test_decode_bits_gpu.py: the host-scan entry, the kernel-per-layer greedy loop, its
lockstep LSTM twin, the persistent loop, both stream paths and both beam searches share one scan tile, one advance rule, one block sum
and one row-LayerNorm (rnnt_amd/csrc/decode_kernels.hpp), so their source can be rearranged freely as long as every case keeps every
bit: tokens, state words and scores raw, every float buffer — the call's WHOLE workspace included — as SHA-256.

Run once on a GPU with the library whose output is the reference (RNNT_ENGINE_LIB = the build of the commit BEFORE the change):
    python tests/golden/make_golden_decode_bits.py
writes tests/golden/decode_bits.npz.  Every call goes through the C ABI with a workspace of THIS module's (engine.workspace is
replaced for the duration of a case): exactly the bytes the size query asks for, every word the quiet-NaN pattern of
make_golden_fused_routes.py, hashed whole after the call.  The layouts are fixed, so that pins candidates, text vectors, rings and
partial products, not only tokens.  The persistent loop's granule buffers are NOT pinned (whether their final content is independent
of timing has not been established): its cases keep state words t .. iterations and the tokens, and the SHA-256 of the model tables.
Loops enqueue their whole bound in one call, so nothing depends on when the host sees the end flag.

A case is written only if (1) the host-computable facts it relies on hold (`REACHES`: H / 8, V % 32, T against scan_frames, ...),
(2) its token lists equal the reference token lists of the fixture it uses — the REFERENCE's own decode (tests/golden/decode_*.npz,
decode_lstm_*.npz): equality for a whole utterance, a prefix for a truncated one (the greedy decode is causal in the frames), for a
beam search its beam-1 run, and the beam-4 n-best lists and scores against the float64 oracle of the search (tests/beam_oracle.py,
at tests/test_beam_gpu.py's gap and score bar); the scan against float64 numpy wherever the top-2 gap is above rounding — and (3) a
second run gives the same bytes.  So a broken build cannot be recorded.  This module is also the test's source of the cases and of the code that runs them.
"""
import ctypes
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import lstm_decode_cases as dc  # noqa: E402
from tests.helpers import DECODE_CASES, load_decode_case, sha256_of_arrays  # noqa: E402

GOLDEN = os.path.join(HERE, "decode_bits.npz")
PATTERN = 0x7FC0BEEF  # a quiet NaN no kernel produces (make_golden_fused_routes.py)
ALL = 10 ** 6         # chunk: the whole bound of a loop in one call

# name -> (kind, fixture, options).  What each one reaches: REACHES, checked by check_reach before anything runs.
CASES = {
    # rnnt_engine_greedy_scan: k_scan_logits + k_argmax_scan on `n` frames from t0 against one seeded text vector
    "scan/small_32": ("scan", "decode_small", dict(t0=0, n=32)),
    "scan/small_5": ("scan", "decode_small", dict(t0=70, n=5)),
    "scan/wide_vocab": ("scan", "decode_wide_vocab", dict(t0=3, n=32)),
    "scan/ref_widths": ("scan", "decode_ref_widths", dict(t0=0, n=33)),
    # rnnt_engine_greedy_decode
    "loop/small_sf32": ("loop", "decode_small", dict(ml=60, sf=32)),
    "loop/small_sf5": ("loop", "decode_small", dict(ml=60, sf=5)),
    "loop/small_proj": ("loop", "decode_small_proj", dict(ml=60, sf=32)),
    "loop/cap_max_length": ("loop", "decode_cap", dict(ml=37, sf=32)),
    "loop/cap_per_frame": ("loop", "decode_cap", dict(ml=200, sf=32)),
    "loop/wide_vocab": ("loop", "decode_wide_vocab", dict(ml=60, sf=32)),
    "loop/ref_widths": ("loop", "decode_ref_widths", dict(ml=200, sf=32)),
    # rnnt_engine_greedy_decode_build_tables / rnnt_engine_greedy_decode_persistent
    "tables/small": ("tables", "decode_small", {}),
    "tables/small_proj": ("tables", "decode_small_proj", {}),
    "persistent/small": ("persistent", "decode_small", dict(ml=60)),
    "persistent/small_proj": ("persistent", "decode_small_proj", dict(ml=60)),
    "persistent/cap_max_length": ("persistent", "decode_cap", dict(ml=37)),
    "persistent/cap_per_frame": ("persistent", "decode_cap", dict(ml=200)),
    "persistent/ref_widths": ("persistent", "decode_ref_widths", dict(ml=200)),
    # rnnt_engine_greedy_stream_decode: three pushes of one utterance
    "stream_loop/cap": ("stream", "decode_cap", dict(ml=200, cuts=(2, 3), persistent=False)),
    "stream_loop/small_proj": ("stream", "decode_small_proj", dict(ml=60, cuts=(2, 10), persistent=False)),
    "stream_persistent/small": ("stream", "decode_small", dict(ml=60, cuts=(30, 60), persistent=True)),
    "stream_persistent/cap": ("stream", "decode_cap", dict(ml=200, cuts=(2, 3), persistent=True)),
    # rnnt_engine_greedy_decode_lstm: n_utt utterances, the whole one and truncated ones
    "lstm/ln_n1": ("lstm", "ln", dict(n=1)),
    "lstm/ln_n3": ("lstm", "ln", dict(n=3)),
    "lstm/text_noln_n1": ("lstm", "text_noln", dict(n=1)),
    "lstm/text_noln_n3": ("lstm", "text_noln", dict(n=3)),
    # rnnt_engine_beam_decode (one utterance) / rnnt_engine_beam_decode_lstm (three), beam 4
    "beam/small": ("beam", "decode_small", dict(ml=60, beam=4)),
    "beam/small_proj": ("beam", "decode_small_proj", dict(ml=60, beam=4)),
    "beam_lstm/ln": ("beam_lstm", "ln", dict(n=3, beam=4)),
    "beam_lstm/text_noln": ("beam_lstm", "text_noln", dict(n=3, beam=4)),
}

# case -> the host-computable facts it is there for, as a predicate over dict(H, V, T, O, text, ...) of its fixture and its options
REACHES = {
    "scan/small_32": lambda f, o: f["H"] // 8 == 8 and f["V"] == 32 and o["n"] == 32,                      # every wave's group mostly clamped; one whole tile
    "scan/small_5": lambda f, o: o["n"] % 32 == 5 and o["t0"] + o["n"] == f["T"],                           # a partial frame block, up to the last frame
    "scan/wide_vocab": lambda f, o: f["H"] // 8 == 24 and f["V"] // 32 == 125 and f["V"] % 32 == 0,
    "scan/ref_widths": lambda f, o: f["H"] // 8 == 128 > 64 and o["n"] == 33,                               # the grouped loop's second trip; two frame blocks
    "loop/small_sf32": lambda f, o: f["H"] // 8 == 8 and not f["text"] and f["T"] % o["sf"] != 0,           # the LN scan; T ends inside a block
    "loop/small_sf5": lambda f, o: o["sf"] == 5 and f["T"] % 5 == 0,                                        # a partial frame block in every scan
    "loop/small_proj": lambda f, o: f["text"] and f["V"] % 32 == 12 and f["V"] // 32 == 9,                  # the non-LN scan; a partial last vocabulary block
    "loop/cap_max_length": lambda f, o: o["ml"] == 37 and f["want_cap"],                                    # 1 + ntok reaches max_length
    "loop/cap_per_frame": lambda f, o: o["ml"] == 200 and f["want_cap"] and f["T"] * 10 < o["ml"],          # every frame runs into max_per_frame; t reaches T
    "loop/wide_vocab": lambda f, o: f["H"] // 8 == 24 and (f["V"] + 31) // 32 == 125,                       # 125 candidates per frame
    "loop/ref_widths": lambda f, o: f["H"] // 8 == 128 and f["E"] == 512 and f["O"] == 1024,                # k_dec_gemv's widest rows
    "tables/small": lambda f, o: not f["text"],
    "tables/small_proj": lambda f, o: f["text"],                                                            # k_dp_fold_text and the folded matrix
    "persistent/small": lambda f, o: not f["text"] and f["E"] <= 256,
    "persistent/small_proj": lambda f, o: f["text"] and f["V"] % 16 == 12,
    "persistent/cap_max_length": lambda f, o: o["ml"] == 37 and f["want_cap"],
    "persistent/cap_per_frame": lambda f, o: o["ml"] == 200 and f["want_cap"],
    "persistent/ref_widths": lambda f, o: 256 < f["E"] <= 512 and f["V"] // 16 == 64,                       # resident rows of two float4 per lane
    "stream_loop/cap": lambda f, o: not f["text"] and o["cuts"][1] - o["cuts"][0] == 1,                     # a one-frame push: scan_frames 1
    "stream_loop/small_proj": lambda f, o: f["text"] and len(o["cuts"]) == 2,
    "stream_persistent/small": lambda f, o: len(o["cuts"]) == 2 and o["cuts"][1] < f["T"],
    "stream_persistent/cap": lambda f, o: f["want_cap"],
    "lstm/ln_n1": lambda f, o: f["ln"] and not f["text"] and f["H"] // 8 == 4,                              # one chunk per wave
    "lstm/ln_n3": lambda f, o: f["ln"] and o["n"] == 3,
    "lstm/text_noln_n1": lambda f, o: f["text"] and not f["ln"] and f["V"] % 32 == 20 and f["H"] // 8 == 3,  # fewer chunks than waves
    "lstm/text_noln_n3": lambda f, o: f["text"] and o["n"] == 3,
    "beam/small": lambda f, o: not f["text"] and o["beam"] == 4,                                            # k_beam_ln16
    "beam/small_proj": lambda f, o: f["text"] and o["beam"] == 4,
    "beam_lstm/ln": lambda f, o: not f["text"] and o["n"] == 3,                                             # ld_rowfin_row<true> is the text vector
    "beam_lstm/text_noln": lambda f, o: f["text"] and o["n"] == 3,
}
BS_N, BS_DONE, BS_LEN = 2, 3, 8  # words of a beam search's state (rnnt_amd/csrc/beam.hip BS_*): entries, done, [BS_LEN + j] entry j's length
ORACLE_GAP, ORACLE_SCORE_TOL = 1e-3, 1e-4  # tests/test_beam_gpu.py's GAP and its bar on scores
RAW_KEYS = ("out", "state", "tokens", "labels", "scores")  # kept as they are; every other key as a SHA-256


def facts(kind, fixture):
    if kind in ("lstm", "beam_lstm"):
        S, O, E, L, Hd, ln, H, V, text = (int(v) for v in dc.load_golden(fixture)["dims"])
        return dict(S=S, O=O, E=E, L=L, Hd=Hd, ln=bool(ln), H=H, V=V, text=bool(text))
    s = DECODE_CASES[fixture]
    return dict(H=s["H"], V=s["V"], E=s["E"], O=s["O"], T=s["T"], text=s["ft"] > 0, want_cap=bool(s.get("want_cap")))


def check_reach(name):
    kind, fixture, opt = CASES[name]
    assert REACHES[name](facts(kind, fixture), opt), name


class own_workspace:
    """engine.workspace replaced: every request gets a buffer of its own, exactly as large as asked, every word PATTERN."""

    def __init__(self, engine):
        self.engine, self.bufs = engine, []

    def __enter__(self):
        self.real, self.engine.workspace = self.engine.workspace, self.take
        return self

    def __exit__(self, *exc):
        self.engine.workspace = self.real

    def take(self, dev, nbytes):
        buf = torch.full(((int(nbytes) + 3) // 4,), PATTERN, dtype=torch.int32, device=dev).view(torch.uint8)
        self.bufs.append(buf)
        return buf

    def words(self):
        torch.cuda.synchronize()
        return [b.view(torch.int32).cpu().numpy() for b in self.bufs]


_conv_cache = {}


def conv_case(fixture):
    """(fixture dict, frames [T,H] on the device with audio_ln applied, the decode entries' model arguments) — the model through the
    project's modules (strict state dicts), audio_ln on the host: float64 products summed by numpy's pairwise sum, rounded once, so
    the frames' bits do not depend on a BLAS."""
    if fixture not in _conv_cache:
        import rnnt_amd
        c = load_decode_case(HERE, fixture)
        spec = c["spec"]
        pred = rnnt_amd.ConvPredictor(spec["V"], spec["O"], spec["E"], 0.3)
        joint = rnnt_amd.JointNetwork(spec["fa"], spec["ft"], spec["H"], spec["V"])
        for mod, sd in ((pred, c["pred_sd"]), (joint, c["joint_sd"])):
            mod.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        frames = c["frames"]
        if spec["fa"] > 0:
            W, b = c["joint_sd"]["audio_ln.weight"].astype(np.float64), c["joint_sd"]["audio_ln.bias"].astype(np.float64)
            frames = ((frames.astype(np.float64)[:, None, :] * W[None]).sum(-1) + b).astype(np.float32)
        model = rnnt_amd.RNNTModel(pred, torch.nn.Identity(), joint).cuda().eval()
        _conv_cache[fixture] = (c, torch.from_numpy(np.ascontiguousarray(frames)).cuda(), model._decode_bundle())
    return _conv_cache[fixture]


_lstm_cache = {}


def lstm_case(fixture, n):
    """(fixture dict, [frames [T_u,H]] of n utterances — the whole one, then ever shorter ones —, the LSTM entries' model arguments)"""
    if fixture not in _lstm_cache:
        fx = dc.load_golden(fixture)
        model64, mel = dc.golden_model(fx)
        model = model64.float().cuda().eval()
        tl = getattr(model.joint, "text_ln", None)
        args = (model.predictor._decode_bundle(), tl.weight if tl is not None else None, tl.bias if tl is not None else None,
                model.joint.joint_ln.weight, model.joint.joint_ln.bias, model.joint.blank_idx)
        _lstm_cache[fixture] = (fx, mel[0].float().t().contiguous().cuda(), args, model)
    fx, frames, args, _ = _lstm_cache[fixture]
    T = frames.shape[0]
    return fx, [frames[:max(1, T // (u + 1) + (u > 0))].contiguous() for u in range(n)], args


_oracle_cache = {}


def beam_oracle_nbest(name):
    """Per utterance of a beam case the float64 oracle's n-best list (tests/beam_oracle.py; the LSTM model through
    tests/beam_lstm_oracle.Model), its keep / drop gap above ORACLE_GAP: computed once on the CPU."""
    if name not in _oracle_cache:
        from tests import beam_lstm_oracle, beam_oracle
        kind, fixture, o = CASES[name]
        if kind == "beam":
            c = load_decode_case(HERE, fixture)
            oms, ml = [beam_oracle.Model(c["frames"], c["pred_sd"], c["joint_sd"])], o["ml"]
        else:
            fx = dc.load_golden(fixture)
            model64, mel = dc.golden_model(fx)
            T, ml = mel.shape[-1], int(fx["max_length"])
            oms = [beam_lstm_oracle.Model(model64, mel[..., :max(1, T // (u + 1) + (u > 0))].contiguous()) for u in range(o["n"])]
        out = []
        for om in oms:
            nbest, _, gap = beam_oracle.beam_search(om, o["beam"], ml)
            assert gap > ORACLE_GAP, (name, gap)
            out.append(nbest)
        _oracle_cache[name] = out
    return _oracle_cache[name]


def _np(t):
    return t.detach().cpu().numpy()


def _decoded(state, tokens):
    """(state words, tokens[0 .. ntok]) of a greedy loop: what lies behind ntok was never written."""
    from rnnt_amd import engine
    st = _np(state)
    return st, _np(tokens)[:1 + int(st[engine.DECODE_NTOK])]


def run_case(engine, name):
    """One run of a case -> (dict of numpy arrays to keep, the token lists to hold against the fixture's)."""
    kind, fixture, o = CASES[name]
    with own_workspace(engine) as own:
        if kind == "scan":
            c, frames, (params, eps, tW, tb, W, bias, blank) = conv_case(fixture)
            text = torch.from_numpy(np.random.default_rng(o["n"] + o["t0"]).standard_normal(frames.shape[1]).astype(np.float32)).cuda()
            out = engine.greedy_scan(frames, text, W, bias, o["t0"], o["n"], blank)
            (ws,) = own.words()
            return dict(out=_np(out), workspace=ws), ("scan", frames, text, W, bias)
        if kind == "tables":
            c, frames, (params, eps, tW, tb, W, bias, blank) = conv_case(fixture)
            m = engine._DecodeModel(None, params, eps, tW, tb, H=frames.shape[1])
            n = ctypes.c_size_t(0)
            engine._check(engine.lib().rnnt_engine_greedy_decode_tables_bytes(m.S, m.E, m.O, m.H, m.has_text, ctypes.byref(n)))
            tables = own.take(m.dev, n.value)
            engine._check(engine.lib().rnnt_engine_greedy_decode_build_tables(
                ctypes.byref(m.struct), m.S, m.E, m.O, ctypes.c_float(m.eps[0]), engine._p(m.text_W), engine._p(m.text_b), m.H,
                engine._p(tables), ctypes.c_size_t(n.value), engine._stream(m.dev)))
            (tb_words,) = own.words()
            return dict(tables=tb_words), None
        if kind == "loop":
            c, frames, bundle = conv_case(fixture)
            state, tokens = engine.greedy_decode_loop(frames, *bundle, o["ml"], max_per_frame=10, scan_frames=o["sf"], chunk=ALL)
            (ws,) = own.words()
            st, tk = _decoded(state, tokens)
            return dict(state=st, tokens=tk, workspace=ws), [(tk[1:].tolist(), c["tokens"][o["ml"]], True)]
        if kind == "persistent":
            c, frames, bundle = conv_case(fixture)
            state, tokens = engine.greedy_decode_persistent(frames, *bundle, o["ml"], max_per_frame=10)
            torch.cuda.synchronize()
            st, tk = _decoded(state, tokens)
            assert st[engine.DECODE_CODE] == 0, (name, st)  # a hand-off that never arrived (the device is shared): not a decode, nothing to record
            return dict(state=st[:engine.DECODE_ITERATIONS + 1], tokens=tk), [(tk[1:].tolist(), c["tokens"][o["ml"]], True)]
        if kind == "stream":
            c, frames, bundle = conv_case(fixture)
            params, eps, tW, tb = bundle[:4]
            tables = engine.greedy_decode_tables(params, eps, tW, tb, frames.shape[1]) if o["persistent"] else None
            W0 = engine.STREAM_STATE_WORDS
            block = torch.full((W0,), PATTERN, dtype=torch.int32, device=frames.device)
            engine.greedy_stream_init(block, bundle[-1])
            res, labels = {}, []
            bounds = (0,) + tuple(o["cuts"]) + (frames.shape[0],)
            for k in range(3):
                push = frames[bounds[k]:bounds[k + 1]]
                cap = min(push.shape[0] * 10, o["ml"] - 1)
                out = torch.full((cap,), PATTERN, dtype=torch.int32, device=frames.device)
                if k == 2 and not o["persistent"]:  # the loop path resumes with a full history: the replay records and k_dec_gemv<2> run
                    assert int(_np(block)[engine.STREAM_LABELS]) >= 7, (name, _np(block))
                before = len(own.bufs)
                engine.greedy_stream_decode(push, *bundle, o["ml"], 10, tables, o["persistent"], block, out)
                torch.cuda.synchronize()
                b = _np(block).copy()
                assert b[engine.STREAM_STATUS] == 0, (name, k, b)
                res["state%d" % k] = b
                res["labels%d" % k] = _np(out)[:int(b[engine.STREAM_PUSH_LABELS])].copy()
                labels += res["labels%d" % k].tolist()
                if not o["persistent"]:
                    res["workspace%d" % k] = own.words()[before]
            return res, [(labels, c["tokens"][o["ml"]], True)]
        if kind == "lstm":
            fx, frames, args = lstm_case(fixture, o["n"])
            state, tokens, state_out, _ = engine.greedy_decode_lstm(frames, *args, int(fx["max_length"]), max_per_frame=10, scan_frames=32, chunk=ALL)
            (ws,) = own.words()
            st, tk = _np(state), _np(tokens)
            lists = [tk[u, :1 + st[u, engine.DECODE_NTOK]] for u in range(o["n"])]
            res = dict(state=st, state_out=_np(state_out), workspace=ws)
            res.update({"tokens%d" % u: t for u, t in enumerate(lists)})
            return res, [(t[1:].tolist(), fx["tokens"].tolist(), u == 0) for u, t in enumerate(lists)]
        if kind in ("beam", "beam_lstm"):
            if kind == "beam":
                c, frames, bundle = conv_case(fixture)
                want, ml = c["tokens"][o["ml"]], o["ml"]
                search = lambda beam: engine.beam_decode(frames, *bundle, ml, beam, max_per_frame=10, chunk=ALL, in_flight=None)  # noqa: E731
            else:
                fx, frames, args = lstm_case(fixture, o["n"])
                want, ml = fx["tokens"].tolist(), int(fx["max_length"])
                search = lambda beam: engine.beam_decode_lstm(frames, *args, ml, beam, max_per_frame=10, chunk=ALL, in_flight=None)  # noqa: E731
            state, tokens, scores = search(1)
            torch.cuda.synchronize()
            st1, tk1 = _np(state).reshape(-1, 32), _np(tokens).reshape(-1, 1, ml)
            greedy = [(tk1[u, 0, 1:1 + st1[u, BS_LEN]].tolist(), want, u == 0) for u in range(st1.shape[0])]
            before = len(own.bufs)
            state, tokens, scores = search(o["beam"])
            ws = own.words()[before]
            st, tk, sc = _np(state).reshape(-1, 32), _np(tokens).reshape(-1, o["beam"], ml), _np(scores).reshape(-1, o["beam"])
            assert st[:, BS_DONE].all(), (name, st)
            res = dict(state=st, workspace=ws)
            for u, oracle in enumerate(beam_oracle_nbest(name)):  # the n-best list against the float64 oracle of the search
                n = int(st[u, BS_N])
                res["scores%d" % u] = sc[u, :n].copy()
                for j in range(n):
                    res["tokens%d_%d" % (u, j)] = tk[u, j, :1 + st[u, BS_LEN + j]].copy()
                assert [res["tokens%d_%d" % (u, j)][1:].tolist() for j in range(n)] == [list(y) for y, _ in oracle], (name, u)
                for j, (_, ws64) in enumerate(oracle):
                    assert abs(sc[u, j] - ws64) <= ORACLE_SCORE_TOL * max(1.0, abs(ws64)), (name, u, j, sc[u, j], ws64)
            return res, greedy
    raise KeyError(kind)


def check_tokens(name, lists):
    """The case decodes what the reference decoded: (got, want, whole) — equality for a whole utterance, a prefix for a truncated one."""
    if lists is None:
        return
    if lists[0] == "scan":
        _, frames, text, W, bias = lists
        kind, fixture, o = CASES[name]
        f = frames[o["t0"]:o["t0"] + o["n"]].double().cpu().numpy()
        logits = np.tanh(f + _np(text.double())) @ _np(W.double()).T + _np(bias.double())
        top = np.sort(logits, axis=1)
        clear = top[:, -1] - top[:, -2] > 1e-3
        assert clear.sum() * 2 >= o["n"], (name, clear)
        return logits.argmax(1), clear
    for got, want, whole in lists:
        assert (got == want) if whole else (got == want[:len(got)]), (name, got, want)


def recorded(result):
    """What the fixture keeps of a run: tokens, state words and scores as they are, a SHA-256 of every other buffer."""
    return {k: (a if k.rstrip("0123456789_") in RAW_KEYS else np.array(sha256_of_arrays(a))) for k, a in result.items()}


def run_checked(engine, name):
    res, lists = run_case(engine, name)
    chk = check_tokens(name, lists)
    if chk is not None:  # the scan: every frame's argmax, where float64 leaves no doubt
        argmax, clear = chk
        assert np.array_equal(res["out"][2:][clear], argmax[clear]), (name, res["out"], argmax)
    return recorded(res)


def main():
    import rnnt_amd
    e = rnnt_amd.engine
    e.lib()
    print("recording from %s" % e.LIB_PATH, flush=True)
    out = {}
    for name in CASES:
        check_reach(name)
        first, second = run_checked(e, name), run_checked(e, name)
        assert sorted(first) == sorted(second) and all(np.array_equal(first[k], second[k]) for k in first), \
            (name, [k for k in first if not np.array_equal(first[k], second.get(k))])
        for k, a in first.items():
            out["%s/%s" % (name, k)] = a
        print("%-28s ok %s" % (name, sorted(first)), flush=True)
    np.savez_compressed(GOLDEN, **out)
    print("%d cases -> %s (%d bytes)" % (len(CASES), GOLDEN, os.path.getsize(GOLDEN)), flush=True)


if __name__ == "__main__":
    main()
