"""CPU: argument checks of rnnt_engine_beam_decode(_workspace_bytes) — every refusal is a code and a message, before anything is
enqueued (no device is needed: nothing is launched)."""
import ctypes

import pytest

from tests.helpers import DECODE_CASES


@pytest.fixture(scope="module")
def lib():
    from rnnt_amd import engine
    L = engine.lib()
    assert hasattr(L, "rnnt_engine_beam_decode") and hasattr(L, "rnnt_engine_beam_decode_workspace_bytes")
    return L


def _ws(lib, S, E, O, H, V, has_text, ml, beam):
    n = ctypes.c_size_t(0)
    rc = lib.rnnt_engine_beam_decode_workspace_bytes(S, E, O, H, V, has_text, ml, beam, ctypes.byref(n))
    return rc, n.value


def test_workspace_queries_cover_the_decode_cases(lib):
    for name, c in DECODE_CASES.items():
        has_text = 1 if c["ft"] > 0 else 0
        for beam in (1, 4, 16):
            for ml in c["max_lengths"]:
                rc, n = _ws(lib, c["V"], c["E"], c["O"], c["H"], c["V"], has_text, ml, beam)
                assert rc == 0 and n > 16 * c["V"] * 4, (name, beam, ml)
    rc1, small = _ws(lib, 32, 48, 64, 64, 32, 0, 60, 4)
    rc2, large = _ws(lib, 32, 48, 64, 64, 32, 0, 600, 4)
    assert rc1 == rc2 == 0 and large > small  # token buffers grow with max_length


def test_refusals_are_codes_and_messages(lib):
    lib.rnnt_engine_last_error.restype = ctypes.c_char_p
    assert _ws(lib, 32, 48, 64, 64, 32, 0, 60, 0)[0] == -1
    assert b"beam" in lib.rnnt_engine_last_error()
    assert _ws(lib, 32, 48, 64, 64, 32, 0, 60, 17)[0] == -2
    assert b"beam" in lib.rnnt_engine_last_error()
    assert _ws(lib, 32, 48, 64, 60, 32, 0, 60, 4)[0] == -2   # H % 8
    assert _ws(lib, 32, 48, 64, 64, 30, 0, 60, 4)[0] == -2   # V % 4
    assert _ws(lib, 32, 1028, 64, 64, 32, 0, 60, 4)[0] == -2  # E > 1024
    assert _ws(lib, 32, 48, 66, 64, 32, 1, 60, 4)[0] == -2   # O % 4
    assert _ws(lib, 32, 48, 64, 64, 32, 0, 1, 4)[0] == -1    # max_length < 2
    assert _ws(lib, 32, 48, 56, 64, 32, 0, 60, 4)[0] == -1   # no text_ln: O must equal H
    assert _ws(lib, 0, 48, 64, 64, 32, 0, 60, 4)[0] == -1    # S
    n = ctypes.c_size_t(0)
    assert lib.rnnt_engine_beam_decode_workspace_bytes(32, 48, 64, 64, 32, 0, 60, 4, None) == -1


def _call(lib, frames=16, params=True, W=16, bias=16, state=16, tokens=16, scores=16, ws=256, beam=4, T=10, ws_bytes=1 << 30, iterations=0):
    from rnnt_amd.engine import _PredParams
    p = _PredParams(*([16] * 11)) if params else None
    return lib.rnnt_engine_beam_decode(frames, ctypes.c_int64(64), T, ctypes.byref(p) if p is not None else None, 32, 48, 64,
                                       ctypes.c_float(1e-5), ctypes.c_float(1e-5), None, None, W, bias, 64, 32, 31, 60, 10, beam, None,
                                       iterations, 1, None, state, tokens, scores, ws, ctypes.c_size_t(ws_bytes), None)


def test_bad_pointers_and_sizes_are_refused_before_any_launch(lib):
    lib.rnnt_engine_last_error.restype = ctypes.c_char_p
    for kw in (dict(frames=None), dict(params=False), dict(W=None), dict(bias=None), dict(state=None), dict(tokens=None),
               dict(scores=None), dict(ws=None)):
        assert _call(lib, **kw) == -1, kw
        assert b"null" in lib.rnnt_engine_last_error(), kw
    assert _call(lib, beam=0) == -1
    assert _call(lib, beam=17) == -2
    assert _call(lib, T=0) == -1
    assert _call(lib, iterations=-1) == -1
    assert _call(lib, ws=128) == -1  # not 256-byte aligned
    assert _call(lib, ws_bytes=64) == -3
    assert b"workspace" in lib.rnnt_engine_last_error()
