"""CPU: the streaming greedy-decode ABI (include/rnnt_engine.h rnnt_engine_greedy_stream_*) — exported symbols, the state-block
constants shared with rnnt_amd/engine.py, workspace queries, and argument refusals as codes and messages before anything is enqueued
(no device is needed: nothing is launched)."""
import ctypes
import os
import re

import pytest

from tests.helpers import DECODE_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rnnt_engine_greedy_stream_init", "rnnt_engine_greedy_stream_decode_workspace_bytes", "rnnt_engine_greedy_stream_decode")


@pytest.fixture(scope="module")
def lib():
    from rnnt_amd import engine
    L = engine.lib()
    L.rnnt_engine_last_error.restype = ctypes.c_char_p
    return L


def test_symbols_are_exported_and_bound(lib):
    from rnnt_amd import engine
    for name in NAMES:
        assert hasattr(lib, name) and name in engine.EXPORTS and name in engine.SIGNATURES


def test_header_constants_match_the_binding():
    from rnnt_amd import engine
    text = open(os.path.join(ROOT, "include", "rnnt_engine.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define RNNT_STREAM_(\w+) (\d+)", text)}
    assert consts["STATE_WORDS"] == engine.STREAM_STATE_WORDS == 16
    for k, v in consts.items():
        if k != "STATE_WORDS":
            assert getattr(engine, "STREAM_" + k) == v, k
    assert consts["TOKENS"] + 7 <= consts["PUSH_LABELS"] < consts["STATE_WORDS"]


def _ws(lib, n, S, E, O, H, V, has_text, ml, m, persistent):
    q = ctypes.c_size_t(0)
    rc = lib.rnnt_engine_greedy_stream_decode_workspace_bytes(n, S, E, O, H, V, has_text, ml, m, persistent, ctypes.byref(q))
    return rc, q.value


def test_workspace_queries_cover_the_decode_cases(lib):
    for name, c in DECODE_CASES.items():
        has_text = 1 if c["ft"] > 0 else 0
        for n in (0, 1, 16, 17, c["T"], 1000):
            for ml in (0, *c["max_lengths"]):
                for persistent in (0, 1):
                    rc, size = _ws(lib, n, c["V"], c["E"], c["O"], c["H"], c["V"], has_text, ml, 10, persistent)
                    assert rc == 0 and size > 0, (name, n, ml, persistent, lib.rnnt_engine_last_error())
        # the persistent query covers the loop too; the label buffer grows with the push
        sizes = [_ws(lib, c["T"], c["V"], c["E"], c["O"], c["H"], c["V"], has_text, 0, 10, p)[1] for p in (0, 1)]
        assert sizes[1] >= sizes[0]
    small = _ws(lib, 10, 32, 48, 64, 64, 32, 0, 0, 10, 0)[1]
    large = _ws(lib, 1000, 32, 48, 64, 64, 32, 0, 0, 10, 0)[1]
    assert large >= small + 4 * 9900


def test_workspace_refusals_are_codes_and_messages(lib):
    ok = dict(n=16, S=32, E=48, O=64, H=64, V=32, has_text=0, ml=0, m=10, persistent=1)

    def q(**kw):
        a = dict(ok, **kw)
        return _ws(lib, a["n"], a["S"], a["E"], a["O"], a["H"], a["V"], a["has_text"], a["ml"], a["m"], a["persistent"])[0]

    assert q() == 0
    for bad in (dict(n=-1), dict(S=0), dict(ml=1), dict(ml=-3), dict(m=0), dict(persistent=2), dict(O=56)):
        assert q(**bad) == -1, bad
        assert b"stream decode" in lib.rnnt_engine_last_error() or b"output dim" in lib.rnnt_engine_last_error(), bad
    assert q(H=60, O=60) == -2  # H % 8
    assert q(E=1028) == -2
    assert q(V=30) == -2  # V % 4
    assert q(n=1 << 27, m=10) == -2  # n * max_per_frame beyond 2^30
    assert b"2^30" in lib.rnnt_engine_last_error()
    assert q(n=1 << 19, m=1, persistent=1) == -2 and b"2^20" in lib.rnnt_engine_last_error()
    assert q(n=1 << 19, m=1, persistent=0) == 0  # the loop has no such limit
    assert q(n=1 << 19, m=1, ml=60, persistent=1) == 0  # max_length bounds the labels per push
    assert q(H=72, O=72, persistent=1) == -2 and q(H=72, O=72, persistent=0) == 0  # the persistent launch needs H % 64 == 0
    assert lib.rnnt_engine_greedy_stream_decode_workspace_bytes(16, 32, 48, 64, 64, 32, 0, 0, 10, 1, None) == -1


def _call(lib, frames=16, n=10, params=True, W=16, bias=16, state=16, out=16, ws=256, ws_bytes=1 << 30, ml=0, m=10, persistent=0,
          tables=None):
    from rnnt_amd.engine import _PredParams
    p = _PredParams(*([16] * 11)) if params else None
    return lib.rnnt_engine_greedy_stream_decode(frames, ctypes.c_int64(64), n, ctypes.byref(p) if p is not None else None, 32, 48, 64,
                                                ctypes.c_float(1e-5), ctypes.c_float(1e-5), None, None, W, bias, 64, 32, 31, ml, m,
                                                tables, persistent, state, out, ws, ctypes.c_size_t(ws_bytes), None)


def test_decode_refusals_before_any_launch(lib):
    for kw in (dict(frames=None), dict(params=False), dict(W=None), dict(bias=None), dict(state=None), dict(out=None), dict(ws=None)):
        assert _call(lib, **kw) == -1, kw
        assert b"null" in lib.rnnt_engine_last_error(), kw
    assert _call(lib, n=-1) == -1
    assert _call(lib, ml=1) == -1
    assert _call(lib, m=0) == -1
    assert _call(lib, persistent=5) == -1
    assert _call(lib, state=18) == -1  # not 4-byte aligned
    assert _call(lib, ws=128) == -1  # not 256-byte aligned
    assert _call(lib, tables=64) == -1  # not 256-byte aligned
    assert _call(lib, ws_bytes=64) == -3
    assert b"workspace" in lib.rnnt_engine_last_error()
    assert lib.rnnt_engine_greedy_stream_init(None, 31, None) == -1
    assert lib.rnnt_engine_greedy_stream_init(16, -1, None) == -1
