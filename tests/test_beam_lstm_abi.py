"""CPU tests of the C ABI of the LSTM beam search (include/rnnt_engine.h rnnt_engine_beam_decode_lstm*): every invalid argument is
refused on the host with its code and a message before anything could be enqueued (there is no GPU here: a launch would be an error
of another code), and the workspace query grows with n_utt and max_length."""
import ctypes

import pytest

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
SIZES = dict(n_utt=2, S=16, E=8, Hd=8, O=16, L=2, ln=1, H=16, V=16, text=0, ml=8, beam=4)
ORDER = ("n_utt", "S", "E", "Hd", "O", "L", "ln", "H", "V", "text", "ml", "beam")


@pytest.fixture(scope="module")
def lib():
    from rnnt_amd import engine
    L = engine.lib()
    L.rnnt_engine_last_error.restype = ctypes.c_char_p
    return L


def query(lib, **kw):
    d, n = dict(SIZES, **kw), ctypes.c_size_t(0)
    return lib.rnnt_engine_beam_decode_lstm_workspace_bytes(*[d[k] for k in ORDER], ctypes.byref(n)), n.value


class _Args:
    """Valid arguments of rnnt_engine_beam_decode_lstm over a host buffer that no refused call ever reads."""

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

    def call(self, lib, sizes=None, **kw):
        d = dict(SIZES, **(sizes or {}))
        a = dict(frames=self.p, frame_stride=d["H"], rows=8, utt=self.p, max_frames=8, params=ctypes.byref(self.params),
                 text_W=self.p if d["text"] else None, text_b=self.p if d["text"] else None, W=self.p, bias=self.p, blank=d["V"] - 1,
                 max_per_frame=10, iterations=1, init=1, host_flag=None, state=self.p, tokens=self.p, scores=self.p, ws=self.p,
                 ws_bytes=1 << 40)
        a.update(kw)
        return lib.rnnt_engine_beam_decode_lstm(
            a["frames"], ctypes.c_int64(a["frame_stride"]), a["rows"], a["utt"], d["n_utt"], a["max_frames"], a["params"], d["S"], d["E"],
            d["Hd"], d["O"], d["L"], d["ln"], ctypes.c_float(1e-5), ctypes.c_float(1e-3), ctypes.c_float(1e-5), a["text_W"], a["text_b"],
            a["W"], a["bias"], d["H"], d["V"], a["blank"], d["ml"], a["max_per_frame"], d["beam"], a["iterations"], a["init"],
            a["host_flag"], a["state"], a["tokens"], a["scores"], a["ws"], ctypes.c_size_t(a["ws_bytes"]), None)


BAD_SIZES = {
    "n_utt = 0": (dict(n_utt=0), INVALID), "n_utt = 33": (dict(n_utt=33), UNSUPPORTED),
    "beam = 0": (dict(beam=0), INVALID), "beam = 17": (dict(beam=17), UNSUPPORTED),
    "max_length = 1": (dict(ml=1), INVALID), "max_length = 65537": (dict(ml=65537), UNSUPPORTED),
    "S = 0": (dict(S=0), INVALID), "E = 0": (dict(E=0), INVALID), "Hd < 0": (dict(Hd=-8), INVALID), "O = 0": (dict(O=0, H=0), INVALID),
    "L = 0": (dict(L=0), INVALID), "H = 0": (dict(H=0), INVALID), "V = 0": (dict(V=0), INVALID),
    "E % 4": (dict(E=10), UNSUPPORTED), "Hd % 4": (dict(Hd=6), UNSUPPORTED), "O % 4": (dict(O=18, text=1), UNSUPPORTED),
    "Hd > 1024": (dict(Hd=1028), UNSUPPORTED), "E > 2048": (dict(E=2052), UNSUPPORTED), "L > 8": (dict(L=9), UNSUPPORTED),
    "H % 8": (dict(H=20, O=20), UNSUPPORTED), "V % 4": (dict(V=18), UNSUPPORTED),
    "O != H without text_ln": (dict(O=8), INVALID),
}


@pytest.mark.parametrize("name", list(BAD_SIZES))
def test_bad_sizes_are_refused_by_both_entries(lib, name):
    kw, code = BAD_SIZES[name]
    assert query(lib, **kw)[0] == code
    assert lib.rnnt_engine_last_error()
    assert _Args(L=max(1, kw.get("L", 2))).call(lib, kw) == code


def test_limits_themselves_are_accepted(lib):
    for kw in (dict(n_utt=1), dict(n_utt=32), dict(beam=1), dict(beam=16), dict(ml=2), dict(ml=65536), dict(Hd=1024, E=2048, L=8),
               dict(O=8, text=1)):
        assert query(lib, **kw)[0] == 0, kw
    assert query(lib, n_utt=32, S=1024, E=512, Hd=512, O=1024, L=3, H=1024, V=1024, ml=200, beam=16)[0] == 0  # the reference's widths


def test_null_pointers_and_scalars(lib):
    a = _Args()
    d = [SIZES[k] for k in ORDER]
    assert lib.rnnt_engine_beam_decode_lstm_workspace_bytes(*d, None) == INVALID
    for kw in (dict(frames=None), dict(utt=None), dict(params=None), dict(W=None), dict(bias=None), dict(state=None), dict(tokens=None),
               dict(scores=None), dict(ws=None), dict(max_per_frame=0), dict(max_frames=0), dict(rows=4), dict(blank=16), dict(blank=-1),
               dict(iterations=-1), dict(frame_stride=8), dict(text_W=a.p), dict(ws=ctypes.c_void_p(a.base + 16)),
               dict(utt=ctypes.c_void_p(a.base + 4)), dict(scores=ctypes.c_void_p(a.base + 4)),
               dict(host_flag=a.p)):  # (an ordinary host word is not mapped pinned memory)
        assert a.call(lib, **kw) == INVALID, kw
        assert lib.rnnt_engine_last_error()
    a.params.layers = None
    assert a.call(lib) == INVALID
    b = _Args(ln=0)  # the structs were filled for the other kind
    assert b.call(lib) == INVALID and b"g_norm" in lib.rnnt_engine_last_error()


def test_short_workspace(lib):
    a = _Args()
    rc, need = query(lib)
    assert rc == 0 and need % 256 == 0
    assert a.call(lib, ws_bytes=need - 1) == WORKSPACE and b"workspace" in lib.rnnt_engine_last_error()
    rc, need_text = query(lib, text=1, O=8)
    assert a.call(lib, dict(text=1, O=8), ws_bytes=need_text - 1) == WORKSPACE


def test_workspace_query_is_monotone(lib):
    kw = dict(S=1024, E=512, Hd=512, O=1024, L=3, H=1024, V=1024, ml=200, beam=8)
    prev = 0
    for n_utt in (1, 2, 3, 4, 16, 31, 32):
        rc, cur = query(lib, n_utt=n_utt, **kw)
        assert rc == 0 and cur > prev and cur % 256 == 0, (n_utt, cur, prev)
        prev = cur
    assert query(lib, n_utt=4, **dict(kw, ml=400))[1] > query(lib, n_utt=4, **kw)[1]
    # per utterance at the least: the pool of 32 states [L][2][Hd], two buffers of 16 text vectors, 16 rows of logits
    assert query(lib, n_utt=32, **kw)[1] >= 4 * 32 * (32 * 3 * 2 * 512 + 2 * 16 * 1024 + 16 * 1024)
    assert query(lib, **dict(kw, beam=1))[1] == query(lib, **dict(kw, beam=16))[1]  # (the slots are the 16 rows whatever the beam)


def test_python_support_query():
    from rnnt_amd import engine
    ref = (1024, 512, 512, 1024, 3, True, 1024, 1024, False)
    assert engine.beam_decode_lstm_supported(32, *ref, 200, 16)
    assert not engine.beam_decode_lstm_supported(33, *ref, 200, 16)
    assert not engine.beam_decode_lstm_supported(1, *ref, 200, 17)
    assert not engine.beam_decode_lstm_supported(1, *ref, 1, 4)
    assert not engine.beam_decode_lstm_supported(1, 16, 16, 32, 32, 2, True, 24, 16, False, 200, 4)  # O != H without text_ln
    assert engine.beam_decode_lstm_supported(1, 16, 16, 32, 32, 2, True, 24, 16, True, 200, 4)
    assert engine.BEAM_LSTM_MAX == 32
    assert engine.SIGNATURES["rnnt_engine_beam_decode_lstm"] == engine.SIGNATURES["rnnt_engine_greedy_decode_lstm"]  # beam for scan_frames, scores for state_out
