"""CPU: the C ABI of the streaming beam search (rnnt_engine_beam_stream_bytes / _init / _push) — exports, the state words'
names, the size query, and every refusal as a code and a message before anything is enqueued (no device is needed: nothing is launched)."""
import ctypes
import os
import re

import pytest

from tests.helpers import DECODE_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rnnt_engine_beam_stream_bytes", "rnnt_engine_beam_stream_init", "rnnt_engine_beam_stream_push")


@pytest.fixture(scope="module")
def lib():
    from rnnt_amd import engine
    L = engine.lib()
    L.rnnt_engine_last_error.restype = ctypes.c_char_p
    return L


def test_symbols_are_exported_and_listed(lib):
    from rnnt_amd import engine
    header = open(os.path.join(ROOT, "include", "rnnt_engine.h")).read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in engine.EXPORTS and n in engine.SIGNATURES, n
        assert re.search(r"\bint " + n + r"\(", header), n
    # the push takes the batched search's arguments, in its order
    assert engine.SIGNATURES["rnnt_engine_beam_stream_push"] == engine.SIGNATURES["rnnt_engine_beam_decode_batch"]


def test_state_words_of_the_header_are_mirrored(lib):
    from rnnt_amd import engine
    header = open(os.path.join(ROOT, "include", "rnnt_engine.h")).read()
    macros = {m: int(v) for m, v in re.findall(r"#define RNNT_BEAM_STREAM_(\w+) (\d+)", header)}
    assert set(macros) == {"FRAMES", "AT_REST", "BASE"}
    for m, v in macros.items():
        assert getattr(engine, "BEAM_STREAM_" + m) == v, m
    # the new words take free slots: not the search's words 0 .. 6, not the result's lengths 8 .. 23
    assert macros["FRAMES"] == 0
    assert len({macros["AT_REST"], macros["BASE"]}) == 2 and all(macros[m] == 7 or 24 <= macros[m] < 32 for m in ("AT_REST", "BASE"))


def _bytes(lib, S, E, O, H, V, has_text, ml, beam, n):
    out = ctypes.c_size_t(0)
    rc = lib.rnnt_engine_beam_stream_bytes(S, E, O, H, V, has_text, ml, beam, n, ctypes.byref(out))
    return rc, out.value


def _ws1(lib, S, E, O, H, V, has_text, ml, beam):
    n = ctypes.c_size_t(0)
    rc = lib.rnnt_engine_beam_decode_workspace_bytes(S, E, O, H, V, has_text, ml, beam, ctypes.byref(n))
    return rc, n.value


def _tables_bytes(lib, S, E, O, H, has_text):
    n = ctypes.c_size_t(0)
    assert lib.rnnt_engine_greedy_decode_tables_bytes(S, E, O, H, has_text, ctypes.byref(n)) == 0
    return n.value


def test_block_grows_with_the_streams(lib):
    from rnnt_amd import engine
    for name, c in DECODE_CASES.items():
        has_text = 1 if c["ft"] > 0 else 0
        for ml in c["max_lengths"]:
            sizes = (c["V"], c["E"], c["O"], c["H"], c["V"], has_text, ml, 4)
            rc1, one = _ws1(lib, *sizes)
            assert rc1 == 0
            # the single search's per-utterance state: its workspace without the tables it may build there
            state1 = one - _tables_bytes(lib, c["V"], c["E"], c["O"], c["H"], has_text)
            assert state1 >= 16 * c["V"] * 4 + 2 * 16 * ml * 4
            got = [_bytes(lib, *sizes, n) for n in (1, 2, 7, 64)]
            assert all(rc == 0 for rc, _ in got), name
            b = [n for _, n in got]
            assert b[0] < b[1] < b[2] < b[3], (name, ml)
            for n, have in zip((1, 2, 7, 64), b):
                assert have >= n * (state1 - 512), (name, ml, n)  # (512: the roundings of the two size queries)
                assert engine.beam_stream_bytes(*sizes, n) == have and engine.beam_stream_supported(*sizes, n)
            assert b[2] - b[1] == 5 * ((b[3] - b[1]) // 62)


def test_the_query_refuses_what_the_single_query_refuses(lib):
    from rnnt_amd import engine
    ok = (32, 48, 64, 64, 32, 0, 60, 4)
    assert _bytes(lib, *ok, 8)[0] == 0
    for n in (0, 65, -1):
        assert _bytes(lib, *ok, n)[0] == -2, n
        assert b"n_streams" in lib.rnnt_engine_last_error()
        assert not engine.beam_stream_supported(*ok, n)
    assert _bytes(lib, 32, 48, 64, 64, 32, 0, 60, 17, 1)[0] == -2
    assert b"beam" in lib.rnnt_engine_last_error()
    bad = [(32, 48, 64, 64, 32, 0, 60, 0), (32, 48, 64, 64, 32, 0, 60, 17), (32, 48, 64, 60, 32, 0, 60, 4), (32, 48, 64, 64, 30, 0, 60, 4),
           (32, 1028, 64, 64, 32, 0, 60, 4), (32, 48, 66, 64, 32, 1, 60, 4), (32, 48, 64, 64, 32, 0, 1, 4), (32, 48, 56, 64, 32, 0, 60, 4),
           (0, 48, 64, 64, 32, 0, 60, 4), (32, 48, 64, 64, 32, 0, 70000, 4)]
    for sizes in bad:
        rc1 = _ws1(lib, *sizes)[0]
        assert rc1 != 0
        assert _bytes(lib, *sizes, 8)[0] == rc1, sizes
    assert _bytes(lib, 32, 48, 64, 60, 32, 0, 60, 4, 8)[0] == -2  # a size the beam kernels refuse
    assert lib.rnnt_engine_beam_stream_bytes(*ok, 8, None) == -1


def _push(lib, frames=16, table=16, params=True, W=16, bias=16, state=16, tokens=16, scores=16, block=256, tables=16, beam=4, rows=40,
          n_streams=4, max_count=10, nbytes=1 << 30, iterations=0, H=64):
    from rnnt_amd.engine import _PredParams
    p = _PredParams(*([16] * 11)) if params else None
    return lib.rnnt_engine_beam_stream_push(frames, ctypes.c_int64(64), rows, table, n_streams, max_count,
                                            ctypes.byref(p) if p is not None else None, 32, 48, 64, ctypes.c_float(1e-5), ctypes.c_float(1e-5),
                                            None, None, W, bias, H, 32, 31, 60, 10, beam, tables, iterations, 1, None, state, tokens, scores,
                                            block, ctypes.c_size_t(nbytes), None)


def test_push_refuses_bad_arguments_before_any_launch(lib):
    for kw in (dict(frames=None), dict(table=None), dict(params=False), dict(W=None), dict(bias=None), dict(state=None), dict(tokens=None),
               dict(scores=None), dict(block=None), dict(tables=None)):
        assert _push(lib, **kw) == -1, kw
        assert b"null" in lib.rnnt_engine_last_error(), kw
    assert _push(lib, n_streams=0) == -2
    assert b"n_streams" in lib.rnnt_engine_last_error()
    assert _push(lib, n_streams=65) == -2
    assert _push(lib, beam=17) == -2
    assert b"beam" in lib.rnnt_engine_last_error()
    assert _push(lib, H=60) == -2          # a size the beam kernels refuse
    assert _push(lib, beam=0) == -1
    assert _push(lib, max_count=-1) == -1  # a negative count
    assert b"max_count" in lib.rnnt_engine_last_error()
    assert _push(lib, rows=-3) == -1
    assert _push(lib, rows=5, max_count=10) == -1  # fewer rows than the longest chunk
    assert _push(lib, table=12) == -1              # the table is not 8-byte aligned
    assert _push(lib, iterations=-1) == -1
    assert _push(lib, block=128) == -1             # not 256-byte aligned
    assert _push(lib, nbytes=64) == -3             # a short block
    assert b"workspace" in lib.rnnt_engine_last_error()
    rc, four = _bytes(lib, 32, 48, 64, 64, 32, 0, 60, 4, 4)
    rc1, one = _bytes(lib, 32, 48, 64, 64, 32, 0, 60, 4, 1)
    assert rc == 0 and rc1 == 0
    assert _push(lib, nbytes=one) == -3   # a block for one stream does not hold four
    assert _push(lib, nbytes=four - 1) == -3


def _init(lib, state=16, scores=16, block=256, beam=4, n_streams=4, index=-1, nbytes=1 << 30, blank=31, H=64):
    return lib.rnnt_engine_beam_stream_init(32, 48, 64, H, 32, 0, 60, beam, blank, n_streams, index, state, scores, block,
                                            ctypes.c_size_t(nbytes), None)


def test_init_refuses_bad_arguments_before_any_launch(lib):
    for kw in (dict(state=None), dict(scores=None), dict(block=None)):
        assert _init(lib, **kw) == -1, kw
        assert b"null" in lib.rnnt_engine_last_error(), kw
    assert _init(lib, n_streams=0) == -2
    assert _init(lib, n_streams=65) == -2
    assert _init(lib, beam=17) == -2
    assert _init(lib, H=60) == -2
    assert _init(lib, index=4) == -1   # one of streams 0 .. 3, or -1 for all
    assert _init(lib, index=-2) == -1
    assert _init(lib, blank=32) == -1
    assert _init(lib, block=128) == -1
    assert _init(lib, nbytes=64) == -3
    assert b"workspace" in lib.rnnt_engine_last_error()
