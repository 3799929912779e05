"""CPU tests of the CTC head's C ABI (include/rnnt_engine.h rnnt_engine_ctc_*): symbols, the workspace query and the host-side
argument checks; nothing is launched."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    import os
    from rnnt_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build()
    L = engine.lib()
    L.rnnt_engine_last_error.restype = ctypes.c_char_p
    return L


NAMES = ("rnnt_engine_ctc_workspace_bytes", "rnnt_engine_ctc_loss_fwd_bwd", "rnnt_engine_ctc_greedy_decode")
P = ctypes.c_void_p(4096)  # a non-null, 256-byte aligned dummy: every call below is refused before anything reads it


def _ws(lib, N, T, U, V):
    n = ctypes.c_size_t(0)
    assert lib.rnnt_engine_ctc_workspace_bytes(N, T, U, V, ctypes.byref(n)) == 0, lib.rnnt_engine_last_error()
    return n.value


def test_symbols_exist(lib):
    from rnnt_amd import engine
    for name in NAMES:
        assert hasattr(lib, name)
        assert name in engine.EXPORTS and name in engine.SIGNATURES
    assert lib.rnnt_engine_version() == 4  # callers detect the CTC entries by symbol


def test_workspace_query_is_monotone_and_aligned(lib):
    base = _ws(lib, 2, 50, 10, 32)
    assert base % 256 == 0
    # at least the fp64 alpha and beta planes of two states per label and the final blank
    assert base >= 2 * 2 * 50 * (2 * 10 + 1) * 8
    prev = base
    for N in (3, 4, 9):
        cur = _ws(lib, N, 50, 10, 32)
        assert cur > prev and cur % 256 == 0
        prev = cur
    prev = base
    for T in (51, 100, 1000):
        cur = _ws(lib, 2, T, 10, 32)
        assert cur > prev and cur % 256 == 0
        prev = cur
    prev = _ws(lib, 2, 50, 0, 32)
    for U in (1, 10, 11, 64, 1023):
        cur = _ws(lib, 2, 50, U, 32)
        assert cur > prev and cur % 256 == 0
        prev = cur
    assert _ws(lib, 1, 1, 0, 4) % 256 == 0


def _loss(lib, N=2, T=50, U=10, V=32, blank=31, logits=P, targets=P, ll=P, tl=P, weights=None, costs=P, grad=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = 1 << 40
    return lib.rnnt_engine_ctc_loss_fwd_bwd(logits, targets, ll, tl, N, T, U, V, blank, weights, costs, grad, ws,
                                            ctypes.c_size_t(ws_bytes), None)


def test_loss_entry_refuses_with_a_message(lib):
    n = ctypes.c_size_t(0)
    assert lib.rnnt_engine_ctc_workspace_bytes(2, 50, 1024, 32, ctypes.byref(n)) == -2 and b"1023" in lib.rnnt_engine_last_error()
    assert _loss(lib, U=1024) == -2 and b"U=1024" in lib.rnnt_engine_last_error()
    assert lib.rnnt_engine_ctc_workspace_bytes(2, 50, 10, 6, ctypes.byref(n)) == -2 and b"multiple of 4" in lib.rnnt_engine_last_error()
    assert _loss(lib, V=6, blank=5) == -2 and b"V=6" in lib.rnnt_engine_last_error()
    assert _loss(lib, blank=32) == -1 and b"blank=32" in lib.rnnt_engine_last_error()
    assert _loss(lib, blank=-1) == -1 and b"blank" in lib.rnnt_engine_last_error()
    for kw in ({"logits": None}, {"targets": None}, {"ll": None}, {"tl": None}, {"costs": None}, {"ws": None}):
        assert _loss(lib, **kw) == -1 and b"null" in lib.rnnt_engine_last_error(), kw
    need = _ws(lib, 2, 50, 10, 32)
    assert _loss(lib, ws_bytes=need - 1) == -3
    msg = lib.rnnt_engine_last_error()
    assert b"workspace" in msg and str(need).encode() in msg
    assert _loss(lib, N=0) == -1 and _loss(lib, T=0) == -1 and _loss(lib, U=-1) == -1
    assert _loss(lib, logits=ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.rnnt_engine_last_error()
    assert _loss(lib, ws=ctypes.c_void_p(4096 + 16)) == -1 and b"aligned" in lib.rnnt_engine_last_error()
    assert lib.rnnt_engine_ctc_workspace_bytes(2, 50, 10, 32, None) == -1 and b"null" in lib.rnnt_engine_last_error()


def test_greedy_entry_refuses_with_a_message(lib):
    def call(N=2, T=50, V=32, blank=31, logits=P, ll=P, tokens=P, counts=P):
        return lib.rnnt_engine_ctc_greedy_decode(logits, ll, N, T, V, blank, tokens, counts, None)
    assert call(V=6, blank=5) == -2 and b"multiple of 4" in lib.rnnt_engine_last_error()
    assert call(blank=32) == -1 and b"blank=32" in lib.rnnt_engine_last_error()
    for kw in ({"logits": None}, {"ll": None}, {"tokens": None}, {"counts": None}):
        assert call(**kw) == -1 and b"null" in lib.rnnt_engine_last_error(), kw
    assert call(N=0) == -1 and call(T=0) == -1
