"""CPU: argument checks of rnnt_engine_beam_decode_batch(_workspace_bytes) — every refusal is a code and a message, before anything is
enqueued (no device is needed: nothing is launched)."""
import ctypes

import pytest

from tests.helpers import DECODE_CASES


@pytest.fixture(scope="module")
def lib():
    from rnnt_amd import engine
    L = engine.lib()
    assert hasattr(L, "rnnt_engine_beam_decode_batch") and hasattr(L, "rnnt_engine_beam_decode_batch_workspace_bytes")
    return L


def _ws(lib, S, E, O, H, V, has_text, ml, beam, n_utt):
    n = ctypes.c_size_t(0)
    rc = lib.rnnt_engine_beam_decode_batch_workspace_bytes(S, E, O, H, V, has_text, ml, beam, n_utt, ctypes.byref(n))
    return rc, n.value


def _ws1(lib, S, E, O, H, V, has_text, ml, beam):
    n = ctypes.c_size_t(0)
    rc = lib.rnnt_engine_beam_decode_workspace_bytes(S, E, O, H, V, has_text, ml, beam, ctypes.byref(n))
    return rc, n.value


def test_workspace_grows_with_the_utterances(lib):
    for name, c in DECODE_CASES.items():
        has_text = 1 if c["ft"] > 0 else 0
        for ml in c["max_lengths"]:
            sizes = (c["V"], c["E"], c["O"], c["H"], c["V"], has_text, ml, 4)
            rc1, one = _ws1(lib, *sizes)
            got = [_ws(lib, *sizes, n) for n in (1, 2, 7, 64)]
            assert rc1 == 0 and all(rc == 0 for rc, _ in got), name
            b = [n for _, n in got]
            assert one <= b[0] < b[1] < b[2] < b[3], (name, ml)
            # per utterance: at least the logits [16][V] and both token buffers, and no more than the single search's whole workspace
            step = (b[3] - b[1]) // 62
            assert 16 * c["V"] * 4 + 2 * 16 * ml * 4 <= step <= one, (name, ml, step, one)
            assert b[2] - b[1] == 5 * step


def test_the_query_refuses_what_the_single_query_refuses(lib):
    lib.rnnt_engine_last_error.restype = ctypes.c_char_p
    ok = (32, 48, 64, 64, 32, 0, 60, 4)
    assert _ws(lib, *ok, 8)[0] == 0
    for n_utt in (0, 65, -1):
        assert _ws(lib, *ok, n_utt)[0] == -2, n_utt
        assert b"n_utt" in lib.rnnt_engine_last_error()
    bad = [(32, 48, 64, 64, 32, 0, 60, 0), (32, 48, 64, 64, 32, 0, 60, 17), (32, 48, 64, 60, 32, 0, 60, 4), (32, 48, 64, 64, 30, 0, 60, 4),
           (32, 1028, 64, 64, 32, 0, 60, 4), (32, 48, 66, 64, 32, 1, 60, 4), (32, 48, 64, 64, 32, 0, 1, 4), (32, 48, 56, 64, 32, 0, 60, 4),
           (0, 48, 64, 64, 32, 0, 60, 4), (32, 48, 64, 64, 32, 0, 70000, 4)]
    for sizes in bad:
        rc1 = _ws1(lib, *sizes)[0]
        assert rc1 != 0
        assert _ws(lib, *sizes, 8)[0] == rc1, sizes
    assert lib.rnnt_engine_beam_decode_batch_workspace_bytes(*ok, 8, None) == -1


def _call(lib, frames=16, utt=16, params=True, W=16, bias=16, state=16, tokens=16, scores=16, ws=256, beam=4, rows=40, n_utt=4, max_frames=10,
          ws_bytes=1 << 30, iterations=0):
    from rnnt_amd.engine import _PredParams
    p = _PredParams(*([16] * 11)) if params else None
    return lib.rnnt_engine_beam_decode_batch(frames, ctypes.c_int64(64), rows, utt, n_utt, max_frames, ctypes.byref(p) if p is not None else None,
                                             32, 48, 64, ctypes.c_float(1e-5), ctypes.c_float(1e-5), None, None, W, bias, 64, 32, 31, 60, 10, beam,
                                             None, iterations, 1, None, state, tokens, scores, ws, ctypes.c_size_t(ws_bytes), None)


def test_bad_pointers_and_sizes_are_refused_before_any_launch(lib):
    lib.rnnt_engine_last_error.restype = ctypes.c_char_p
    for kw in (dict(frames=None), dict(utt=None), dict(params=False), dict(W=None), dict(bias=None), dict(state=None), dict(tokens=None),
               dict(scores=None), dict(ws=None)):
        assert _call(lib, **kw) == -1, kw
        assert b"null" in lib.rnnt_engine_last_error(), kw
    assert _call(lib, n_utt=0) == -2
    assert b"n_utt" in lib.rnnt_engine_last_error()
    assert _call(lib, n_utt=65) == -2
    assert b"n_utt" in lib.rnnt_engine_last_error()
    assert _call(lib, beam=0) == -1
    assert _call(lib, beam=17) == -2
    assert b"beam" in lib.rnnt_engine_last_error()
    assert _call(lib, max_frames=0) == -1
    assert _call(lib, rows=5, max_frames=10) == -1  # fewer rows than the longest utterance
    assert _call(lib, utt=12) == -1                 # the table is not 8-byte aligned
    assert _call(lib, iterations=-1) == -1
    assert _call(lib, ws=128) == -1  # not 256-byte aligned
    assert _call(lib, ws_bytes=64) == -3
    assert b"workspace" in lib.rnnt_engine_last_error()
    # a workspace that holds one utterance's search does not hold four
    n = ctypes.c_size_t(0)
    assert lib.rnnt_engine_beam_decode_workspace_bytes(32, 48, 64, 64, 32, 0, 60, 4, ctypes.byref(n)) == 0
    assert _call(lib, ws_bytes=n.value) == -3
