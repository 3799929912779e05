"""CPU tests of the C ABI of the LSTM greedy stream (include/rnnt_engine.h rnnt_engine_greedy_stream_lstm_*): every invalid argument is
refused on the host with its code and a message before anything could be enqueued (there is no GPU here: a launch would be an error
of another code), the size queries grow with n_streams, and the binding's constants are the header's."""
import ctypes
import os
import re

import pytest

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
SIZES = dict(n=2, S=16, E=8, Hd=8, O=16, L=2, ln=1, H=16, V=16, text=0, scan=32)
ORDER = ("n", "S", "E", "Hd", "O", "L", "ln", "H", "V", "text")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from rnnt_amd import engine
    L = engine.lib()
    L.rnnt_engine_last_error.restype = ctypes.c_char_p
    return L


def block_bytes(lib, **kw):
    d, n = dict(SIZES, **kw), ctypes.c_size_t(0)
    return lib.rnnt_engine_greedy_stream_lstm_bytes(*[d[k] for k in ORDER], ctypes.byref(n)), n.value


def ws_bytes(lib, **kw):
    d, n = dict(SIZES, **kw), ctypes.c_size_t(0)
    return lib.rnnt_engine_greedy_stream_lstm_push_workspace_bytes(*[d[k] for k in ORDER], d["scan"], ctypes.byref(n)), n.value


class _Args:
    """Valid arguments of rnnt_engine_greedy_stream_lstm_push over a host buffer that no refused call ever reads."""

    def __init__(self, L=2, ln=1):
        from rnnt_amd.lstm_predictor import _LayerParams, _Params
        self.buf = (ctypes.c_float * 4096)()
        base = (ctypes.cast(self.buf, ctypes.c_void_p).value + 255) & ~255
        self.base = base
        self.p = ctypes.c_void_p(base)
        self.layers = (_LayerParams * L)()
        for l in range(L):
            self.layers[l] = _LayerParams(base, None, base, base, base, base, base) if ln else _LayerParams(base, base, base, None, None, None, None)
        self.params = _Params(*([base] * 7), ctypes.cast(self.layers, ctypes.POINTER(_LayerParams)))

    def push(self, lib, sizes=None, **kw):
        d = dict(SIZES, **(sizes or {}))
        a = dict(frames=self.p, frame_stride=d["H"], rows=8, table=self.p, max_count=8, params=ctypes.byref(self.params),
                 text_W=self.p if d["text"] else None, text_b=self.p if d["text"] else None, W=self.p, bias=self.p, blank=d["V"] - 1,
                 max_length=0, max_per_frame=10, iterations=1, begin=1, host_flag=None, out=self.p, out_stride=80, block=self.p,
                 bytes=1 << 40, ws=self.p, ws_bytes=1 << 40)
        a.update(kw)
        return lib.rnnt_engine_greedy_stream_lstm_push(
            a["frames"], ctypes.c_int64(a["frame_stride"]), a["rows"], a["table"], d["n"], a["max_count"], a["params"], d["S"], d["E"],
            d["Hd"], d["O"], d["L"], d["ln"], ctypes.c_float(1e-5), ctypes.c_float(1e-3), ctypes.c_float(1e-5), a["text_W"], a["text_b"],
            a["W"], a["bias"], d["H"], d["V"], a["blank"], a["max_length"], a["max_per_frame"], d["scan"], a["iterations"], a["begin"],
            a["host_flag"], a["out"], a["out_stride"], a["block"], ctypes.c_size_t(a["bytes"]), a["ws"], ctypes.c_size_t(a["ws_bytes"]), None)

    def init(self, lib, **kw):
        a = dict(n=2, Hd=8, L=2, H=16, blank=15, index=-1, block=self.p, bytes=1 << 40)
        a.update(kw)
        return lib.rnnt_engine_greedy_stream_lstm_init(a["n"], a["Hd"], a["L"], a["H"], a["blank"], a["index"], a["block"],
                                                       ctypes.c_size_t(a["bytes"]), None)


BAD_SIZES = {
    "n = 0": (dict(n=0), INVALID), "n = 33": (dict(n=33), UNSUPPORTED),
    "S = 0": (dict(S=0), INVALID), "E = 0": (dict(E=0), INVALID), "Hd < 0": (dict(Hd=-8), INVALID), "O = 0": (dict(O=0, H=0), INVALID),
    "L = 0": (dict(L=0), INVALID), "H = 0": (dict(H=0), INVALID), "V = 0": (dict(V=0), INVALID),
    "E % 4": (dict(E=10), UNSUPPORTED), "Hd % 4": (dict(Hd=6), UNSUPPORTED), "O % 4": (dict(O=18, text=1), UNSUPPORTED),
    "Hd > 1024": (dict(Hd=1028), UNSUPPORTED), "E > 2048": (dict(E=2052), UNSUPPORTED), "L > 8": (dict(L=9), UNSUPPORTED),
    "H % 8": (dict(H=20, O=20), UNSUPPORTED), "V % 4": (dict(V=18), UNSUPPORTED),
    "O != H without text_ln": (dict(O=8), INVALID),
}


@pytest.mark.parametrize("name", list(BAD_SIZES))
def test_bad_sizes_are_refused_by_every_entry(lib, name):
    kw, code = BAD_SIZES[name]
    assert block_bytes(lib, **kw)[0] == code
    assert lib.rnnt_engine_last_error()
    assert ws_bytes(lib, **kw)[0] == code
    assert _Args(L=max(1, kw.get("L", 2))).push(lib, kw) == code


@pytest.mark.parametrize("scan", [0, 129, -1])
def test_scan_frames_outside_the_range(lib, scan):
    assert ws_bytes(lib, scan=scan)[0] == UNSUPPORTED
    assert _Args().push(lib, dict(scan=scan)) == UNSUPPORTED and b"scan_frames" in lib.rnnt_engine_last_error()


def test_limits_themselves_are_accepted(lib):
    for kw in (dict(n=1), dict(n=32), dict(scan=1), dict(scan=128), dict(Hd=1024, E=2048, L=8), dict(O=8, text=1)):
        assert ws_bytes(lib, **kw)[0] == 0 and block_bytes(lib, **kw)[0] == 0, kw
    assert ws_bytes(lib, n=32, S=1024, E=512, Hd=512, O=1024, L=3, H=1024, V=1024)[0] == 0  # the reference's widths


def test_push_null_pointers_and_scalars(lib):
    a = _Args()
    d = [SIZES[k] for k in ORDER]
    assert lib.rnnt_engine_greedy_stream_lstm_bytes(*d, None) == INVALID
    assert lib.rnnt_engine_greedy_stream_lstm_push_workspace_bytes(*d, 32, None) == INVALID
    for kw in (dict(frames=None), dict(table=None), dict(params=None), dict(W=None), dict(bias=None), dict(out=None), dict(block=None),
               dict(ws=None), dict(max_length=1), dict(max_length=-1), dict(max_per_frame=0), dict(max_count=-1), dict(rows=0),
               dict(rows=4), dict(blank=16), dict(blank=-1), dict(iterations=-1), dict(frame_stride=8), dict(frame_stride=18),
               dict(text_W=a.p), dict(ws=ctypes.c_void_p(a.base + 16)), dict(block=ctypes.c_void_p(a.base + 16)),
               dict(table=ctypes.c_void_p(a.base + 4)), dict(out_stride=79), dict(out_stride=0, max_count=0),
               dict(host_flag=a.p)):  # (an ordinary host word is not mapped pinned memory)
        assert a.push(lib, **kw) == INVALID, kw
        assert lib.rnnt_engine_last_error()
    assert a.push(lib, max_count=1 << 30, rows=1 << 30, out_stride=1 << 30) == INVALID  # (max_count * max_per_frame beyond out_stride)
    a.params.layers = None
    assert a.push(lib) == INVALID
    b = _Args(ln=0)  # the structs were filled for the other kind
    assert b.push(lib) == INVALID and b"g_norm" in lib.rnnt_engine_last_error()


def test_short_workspace_and_short_block(lib):
    a = _Args()
    (rc, need), (rc2, need_block) = ws_bytes(lib), block_bytes(lib)
    assert rc == 0 and rc2 == 0 and need % 256 == 0 and need_block % 256 == 0
    assert a.push(lib, ws_bytes=need - 1) == WORKSPACE and b"workspace" in lib.rnnt_engine_last_error()
    assert a.push(lib, bytes=need_block - 1) == WORKSPACE and b"block" in lib.rnnt_engine_last_error()
    assert a.init(lib, bytes=need_block - 1) == WORKSPACE and b"block" in lib.rnnt_engine_last_error()
    rc, need_text = ws_bytes(lib, text=1, O=8)
    assert a.push(lib, dict(text=1, O=8), ws_bytes=need_text - 1) == WORKSPACE


def test_init_refusals(lib):
    a = _Args()
    for kw in (dict(n=0), dict(Hd=0), dict(L=0), dict(H=0), dict(blank=-1), dict(index=-2), dict(index=2), dict(block=None),
               dict(block=ctypes.c_void_p(a.base + 16))):
        assert a.init(lib, **kw) == INVALID, kw
        assert lib.rnnt_engine_last_error()
    for kw in (dict(n=33), dict(Hd=1028), dict(L=9)):
        assert a.init(lib, **kw) == UNSUPPORTED, kw


def test_size_queries_are_monotone(lib):
    kw = dict(S=1024, E=512, Hd=512, O=1024, L=3, H=1024, V=1024)
    prev = prev_block = 0
    for n in (1, 2, 4, 8, 16, 31, 32):
        (rc, cur), (rc2, blk) = ws_bytes(lib, n=n, **kw), block_bytes(lib, n=n, **kw)
        assert rc == 0 and rc2 == 0 and cur > prev and blk > prev_block, (n, cur, prev, blk, prev_block)
        assert blk >= 4 * n * (16 + 2 * 3 * 512 + 1024)  # the words, h and c of every layer, the text vector
        prev, prev_block = cur, blk
    prev = 0
    for scan in (1, 5, 32, 33, 128):
        rc, cur = ws_bytes(lib, n=4, scan=scan, **kw)
        assert rc == 0 and cur >= prev and cur % 256 == 0, (scan, cur, prev)
        prev = cur
    # the workspace holds none of what the block holds: it is smaller than the offline loop's, which keeps h, c and the text vectors
    off = ctypes.c_size_t(0)
    assert lib.rnnt_engine_greedy_decode_lstm_workspace_bytes(32, 1024, 512, 512, 1024, 3, 1, 1024, 1024, 0, 32, ctypes.byref(off)) == 0
    assert ws_bytes(lib, n=32, **kw)[1] + block_bytes(lib, n=32, **kw)[1] <= off.value + 3 * 256 + 4 * 32 * 16


def test_constants_and_python_queries():
    from rnnt_amd import engine
    text = open(os.path.join(ROOT, "include", "rnnt_engine.h")).read()
    hdr = {k: int(v) for k, v in re.findall(r"#define RNNT_LSTM_STREAM_(\w+) (\d+)", text)}
    assert len(hdr) == 13
    for name, value in hdr.items():
        assert getattr(engine, "LSTM_STREAM_" + name) == value, name
    assert engine.LSTM_STREAM_MAX == 32
    assert [hdr[k] for k in ("T", "EMITTED", "LABELS", "PAUSED", "NEWTOK", "PUSH_ITERATIONS", "AT_REST")] == [
        engine.DECODE_T, engine.DECODE_EMITTED, engine.DECODE_NTOK, engine.DECODE_DONE, engine.DECODE_NEWTOK, engine.DECODE_ITERATIONS,
        engine.DECODE_SETTLED]  # the words the shared kernels read
    ref = (1024, 512, 512, 1024, 3, True, 1024, 1024, False)
    assert engine.greedy_stream_lstm_supported(32, *ref) and not engine.greedy_stream_lstm_supported(33, *ref)
    assert not engine.greedy_stream_lstm_supported(1, *ref, scan_frames=129)
    assert engine.greedy_stream_lstm_bytes(2, *ref) > engine.greedy_stream_lstm_bytes(1, *ref)
    with pytest.raises(RuntimeError):
        engine.greedy_stream_lstm_bytes(33, *ref)


def test_views_cover_the_block():
    import torch
    from rnnt_amd import engine
    n, L, Hd, H = 3, 2, 36, 24
    nbytes = engine.greedy_stream_lstm_bytes(n, 16, 16, Hd, H, L, True, H, 16, False)
    block = torch.zeros(nbytes, dtype=torch.uint8)
    state, hc, text = engine.greedy_stream_lstm_views(block, n, L, Hd, H)
    assert state.shape == (n, 16) and hc.shape == (L, 2, n, Hd) and text.shape == (n, H)
    for v in (state, hc, text):
        assert (v.data_ptr() - block.data_ptr()) % 256 == 0
    assert text.data_ptr() + 4 * n * H <= block.data_ptr() + nbytes < text.data_ptr() + 4 * n * H + 256
    assert state.data_ptr() + 64 * n <= hc.data_ptr() and hc.data_ptr() + 4 * hc.numel() <= text.data_ptr()
