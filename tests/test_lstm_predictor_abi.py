"""CPU tests of the LSTMPredictor's C ABI (include/rnnt_engine.h rnnt_engine_lstm_predictor_*): every invalid argument is refused on
the host with its code and a message, before anything could be enqueued (there is no GPU here: a launch would be an error of another
code), and the size queries grow with B and U1."""
import ctypes

import pytest

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
DIMS = dict(B=2, U1=3, S=16, E=8, Hd=8, O=8, L=2, ln=1)


@pytest.fixture(scope="module")
def lib():
    from rnnt_amd import engine
    L = engine.lib()
    L.rnnt_engine_last_error.restype = ctypes.c_char_p
    return L


class _Args:
    """Valid arguments of rnnt_engine_lstm_predictor_fwd / _bwd over a host buffer that no refused call ever reads."""

    def __init__(self, L=2, ln=1):
        from rnnt_amd.lstm_predictor import _LayerParams, _Params
        self.buf = (ctypes.c_float * 4096)()
        base = ctypes.cast(self.buf, ctypes.c_void_p).value
        base = (base + 15) & ~15
        self.p = ctypes.c_void_p(base)
        self.layers = (_LayerParams * L)()
        for l in range(L):
            self.layers[l] = _LayerParams(base, None, base, base, base, base, base) if ln else _LayerParams(base, base, base, None, None, None, None)
        self.params = _Params(*([base] * 7), ctypes.cast(self.layers, ctypes.POINTER(_LayerParams)))

    def dims(self, **kw):
        d = dict(DIMS, **kw)
        return [d[k] for k in ("B", "U1", "S", "E", "Hd", "O", "L", "ln")]

    def fwd(self, lib, dims=None, **kw):
        a = dict(ids=self.p, params=ctypes.byref(self.params), state_in=None, keep=None, p=0.0, out=self.p, state_out=self.p,
                 saved=self.p, saved_bytes=1 << 40, ws=self.p, ws_bytes=1 << 40)
        a.update(kw)
        return lib.rnnt_engine_lstm_predictor_fwd(a["ids"], *self.dims(**(dims or {})), a["params"], a["state_in"], a["keep"],
                                                  ctypes.c_float(a["p"]), ctypes.c_float(1e-5), ctypes.c_float(1e-3), ctypes.c_float(1e-5),
                                                  a["out"], a["state_out"], a["saved"], ctypes.c_size_t(a["saved_bytes"]), a["ws"],
                                                  ctypes.c_size_t(a["ws_bytes"]), None)

    def bwd(self, lib, dims=None, **kw):
        a = dict(ids=self.p, params=ctypes.byref(self.params), keep=None, p=0.0, d_out=self.p, grads=ctypes.byref(self.params),
                 saved=self.p, saved_bytes=1 << 40, ws=self.p, ws_bytes=1 << 40)
        a.update(kw)
        return lib.rnnt_engine_lstm_predictor_bwd(a["ids"], *self.dims(**(dims or {})), a["params"], a["keep"], ctypes.c_float(a["p"]),
                                                  ctypes.c_float(1e-5), ctypes.c_float(1e-3), ctypes.c_float(1e-5), a["d_out"], a["grads"],
                                                  a["saved"], ctypes.c_size_t(a["saved_bytes"]), a["ws"], ctypes.c_size_t(a["ws_bytes"]), None)

    def sizes(self, lib, **kw):
        n = ctypes.c_size_t(0)
        return [lib.rnnt_engine_lstm_predictor_saved_bytes(*self.dims(**kw), ctypes.byref(n)),
                lib.rnnt_engine_lstm_predictor_workspace_bytes(*self.dims(**kw), 0, ctypes.byref(n)),
                lib.rnnt_engine_lstm_predictor_workspace_bytes(*self.dims(**kw), 1, ctypes.byref(n))]


BAD_DIMS = {
    "B = 0": (dict(B=0), INVALID), "U1 = 0": (dict(U1=0), INVALID), "S = 0": (dict(S=0), INVALID), "E < 0": (dict(E=-4), INVALID),
    "Hd = 0": (dict(Hd=0), INVALID), "O = 0": (dict(O=0), INVALID), "L = 0": (dict(L=0), INVALID),
    "E % 4": (dict(E=10), UNSUPPORTED), "Hd % 4": (dict(Hd=6), UNSUPPORTED), "O % 4": (dict(O=9), UNSUPPORTED),
    "Hd > 1024": (dict(Hd=1028), UNSUPPORTED), "E > 2048": (dict(E=2052), UNSUPPORTED), "L > 8": (dict(L=9), UNSUPPORTED),
}


@pytest.mark.parametrize("name", list(BAD_DIMS))
def test_bad_dims_are_refused_by_every_entry(lib, name):
    kw, code = BAD_DIMS[name]
    a = _Args(L=max(1, kw.get("L", 2)))
    assert a.sizes(lib, **kw) + [a.fwd(lib, kw), a.bwd(lib, kw)] == [code] * 5
    assert lib.rnnt_engine_last_error()


def test_limits_themselves_are_accepted(lib):
    a = _Args(L=8)
    assert a.sizes(lib, Hd=1024, E=2048, L=8) == [0, 0, 0]


def test_null_pointers_and_dropout_range(lib):
    a, n = _Args(), ctypes.c_size_t(0)
    assert lib.rnnt_engine_lstm_predictor_saved_bytes(*a.dims(), None) == INVALID
    assert lib.rnnt_engine_lstm_predictor_workspace_bytes(*a.dims(), 0, None) == INVALID
    for kw in (dict(ids=None), dict(params=None), dict(out=None), dict(state_out=None), dict(ws=None), dict(p=1.0), dict(p=-0.1),
               dict(p=float("nan"))):
        assert a.fwd(lib, **kw) == INVALID, kw
        assert lib.rnnt_engine_last_error()
    for kw in (dict(ids=None), dict(params=None), dict(grads=None), dict(d_out=None), dict(saved=None), dict(ws=None), dict(p=1.0)):
        assert a.bwd(lib, **kw) == INVALID, kw
        assert lib.rnnt_engine_last_error()
    a.params.layers = None
    assert a.fwd(lib) == INVALID and a.bwd(lib) == INVALID


@pytest.mark.parametrize("ln", [0, 1])
def test_layer_pointers_follow_layer_norm(lib, ln):
    """With layer norm the four norm affines must be there (x2g has no bias); without it the x2g bias must."""
    a = _Args(ln=ln)
    dims = dict(ln=1 - ln)  # the structs were filled for the other kind
    assert a.fwd(lib, dims) == INVALID and a.bwd(lib, dims) == INVALID
    assert (b"g_norm" if ln == 0 else b"bias") in lib.rnnt_engine_last_error()
    a = _Args(ln=ln)
    a.layers[1].p2g_w = None
    assert a.fwd(lib, dict(ln=ln)) == INVALID and b"layer 1" in lib.rnnt_engine_last_error()


def test_short_buffers(lib):
    a, n = _Args(), ctypes.c_size_t(0)
    assert lib.rnnt_engine_lstm_predictor_saved_bytes(*a.dims(), ctypes.byref(n)) == 0
    saved = n.value
    assert lib.rnnt_engine_lstm_predictor_workspace_bytes(*a.dims(), 0, ctypes.byref(n)) == 0
    ws_f = n.value
    assert lib.rnnt_engine_lstm_predictor_workspace_bytes(*a.dims(), 1, ctypes.byref(n)) == 0
    ws_b = n.value
    assert a.fwd(lib, saved_bytes=saved - 1) == WORKSPACE and b"saved" in lib.rnnt_engine_last_error()
    assert a.fwd(lib, ws_bytes=ws_f - 1) == WORKSPACE and b"workspace" in lib.rnnt_engine_last_error()
    assert a.fwd(lib, saved=None, saved_bytes=0, ws_bytes=ws_f - 1) == WORKSPACE  # inference: no saved buffer, the workspace still checked
    assert a.bwd(lib, saved_bytes=saved - 1) == WORKSPACE and b"saved" in lib.rnnt_engine_last_error()
    assert a.bwd(lib, ws_bytes=ws_b - 1) == WORKSPACE and b"workspace" in lib.rnnt_engine_last_error()


def test_size_queries_are_monotone_in_rows(lib):
    a = _Args()

    def q(**kw):
        n, out = ctypes.c_size_t(0), []
        assert lib.rnnt_engine_lstm_predictor_saved_bytes(*a.dims(**kw), ctypes.byref(n)) == 0
        out.append(n.value)
        for backward in (0, 1):
            assert lib.rnnt_engine_lstm_predictor_workspace_bytes(*a.dims(**kw), backward, ctypes.byref(n)) == 0
            out.append(n.value)
        return out

    kw = dict(E=512, Hd=512, O=1024, S=1024, L=3)
    for big in (dict(B=33), dict(U1=202)):
        lo, hi = q(B=32, U1=201, **kw), q(**dict(dict(B=32, U1=201, **kw), **big))
        assert all(h > l for h, l in zip(hi, lo)), (big, lo, hi)
    prev = q(B=1, U1=1, **kw)
    for B, U1 in ((1, 2), (2, 2), (4, 101), (32, 201)):
        cur = q(B=B, U1=U1, **kw)
        assert all(c >= p for c, p in zip(cur, prev)) and all(v % 256 == 0 for v in cur)
        prev = cur
    # per row the forward keeps E + O + 4 floats and 8 Hd + 2 per layer, rounded up to 256-byte blocks
    M = 32 * 201
    assert q(B=32, U1=201, **kw)[0] >= 4 * M * (512 + 1024 + 4 + 3 * (8 * 512 + 2))
