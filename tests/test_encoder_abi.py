"""CPU tests of the encoder's C ABI (include/rnnt_engine.h rnnt_engine_encoder_*): symbols, size queries and host-side argument
checks; nothing is launched."""
import ctypes

import pytest

from rnnt_amd.encoder import (NORM_BATCH, NORM_INSTANCE, NORM_NONE, REGIME_AUTO, REGIME_MANY_ROWS, ROLE_FINAL, ROLE_FIRST, ROLE_LAST,
                              ROLE_PLAIN, ROLE_RESIDUAL, _Layer)


@pytest.fixture(scope="module")
def lib():
    import os
    from rnnt_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build()
    L = engine.lib()
    L.rnnt_engine_last_error.restype = ctypes.c_char_p
    return L


def layers(spec):
    """spec: [(cin, cout, taps, stride, dilation, norm, role)]; pointers are dummies (the size queries read none)."""
    arr = (_Layer * max(1, len(spec)))()
    for L, (cin, cout, taps, stride, dil, norm, role) in zip(arr, spec):
        L.cin, L.cout, L.taps, L.stride, L.dilation, L.norm, L.role, L.eps = cin, cout, taps, stride, dil, norm, role, 1e-5
    return arr


SMALL = [(9, 12, 5, 2, 1, NORM_BATCH, ROLE_PLAIN),
         (12, 20, 1, 1, 1, NORM_BATCH, ROLE_RESIDUAL), (12, 20, 5, 1, 1, NORM_BATCH, ROLE_FIRST), (20, 20, 5, 1, 1, NORM_BATCH, ROLE_LAST),
         (20, 24, 1, 1, 1, NORM_INSTANCE, ROLE_RESIDUAL), (20, 24, 7, 1, 1, NORM_INSTANCE, ROLE_FIRST),
         (24, 24, 7, 1, 1, NORM_INSTANCE, ROLE_PLAIN), (24, 24, 7, 1, 1, NORM_INSTANCE, ROLE_LAST),
         (24, 28, 7, 1, 2, NORM_BATCH, ROLE_PLAIN), (28, 36, 1, 1, 1, NORM_NONE, ROLE_FINAL)]


def test_symbols_exist(lib):
    for name in ("rnnt_engine_encoder_packed_bytes", "rnnt_engine_encoder_pack", "rnnt_engine_encoder_workspace_bytes",
                 "rnnt_engine_encoder_fwd", "rnnt_engine_encoder_stream_push"):
        assert hasattr(lib, name)
    from rnnt_amd import engine
    assert all(n in engine.EXPORTS and n in engine.SIGNATURES for n in ("rnnt_engine_encoder_fwd", "rnnt_engine_encoder_stream_push"))


def test_size_queries_answer(lib):
    arr, n = layers(SMALL), ctypes.c_size_t(0)
    assert lib.rnnt_engine_encoder_packed_bytes(arr, len(SMALL), ctypes.byref(n)) == 0
    floats = sum(t * co * ((ci + 3) // 4 * 4) for ci, co, t, *_ in SMALL)
    assert floats * 4 <= n.value <= floats * 4 + 256 * len(SMALL) and n.value % 256 == 0  # rows padded to 16 bytes (F = 9 -> 12)
    w = ctypes.c_size_t(0)
    assert lib.rnnt_engine_encoder_workspace_bytes(arr, len(SMALL), 3, 101, REGIME_AUTO, None, ctypes.byref(w)) == 0
    assert w.value >= 3 * 50 * 36 * 4
    lens = (ctypes.c_int32 * len(SMALL))(3, 0, 4, 4, 0, 6, 6, 6, 12, 0)
    s = ctypes.c_size_t(0)
    assert lib.rnnt_engine_encoder_workspace_bytes(arr, len(SMALL), 1, 7, REGIME_AUTO, lens, ctypes.byref(s)) == 0
    m = ctypes.c_size_t(0)
    assert lib.rnnt_engine_encoder_workspace_bytes(arr, len(SMALL), 1, 7, REGIME_MANY_ROWS, lens, ctypes.byref(m)) == 0
    assert 0 < m.value < w.value and 0 < s.value < w.value
    # one sub-block per block: first and last at once
    one = [(8, 8, 3, 1, 1, NORM_BATCH, ROLE_PLAIN), (8, 16, 1, 1, 1, NORM_BATCH, ROLE_RESIDUAL),
           (8, 16, 3, 1, 1, NORM_BATCH, ROLE_FIRST | ROLE_LAST), (16, 4, 1, 1, 1, NORM_NONE, ROLE_FINAL)]
    assert lib.rnnt_engine_encoder_packed_bytes(layers(one), len(one), ctypes.byref(n)) == 0


def _refused(lib, spec, word, n_layers=None):
    n = ctypes.c_size_t(0)
    k = len(spec) if n_layers is None else n_layers
    for call in (lambda: lib.rnnt_engine_encoder_packed_bytes(layers(spec), k, ctypes.byref(n)),
                 lambda: lib.rnnt_engine_encoder_workspace_bytes(layers(spec), k, 1, 50, REGIME_AUTO, None, ctypes.byref(n))):
        assert call() == -1
        assert word in lib.rnnt_engine_last_error(), lib.rnnt_engine_last_error()


def test_bad_descriptors_are_refused_with_a_message(lib):
    def edit(i, **kw):
        spec = [list(r) for r in SMALL]
        for k, v in kw.items():
            spec[i][("cin", "cout", "taps", "stride", "dilation", "norm", "role").index(k)] = v
        return [tuple(r) for r in spec]
    _refused(lib, edit(2, taps=0), b"taps")
    _refused(lib, edit(0, stride=0), b"stride")
    _refused(lib, edit(8, dilation=0), b"dilation")
    _refused(lib, SMALL, b"empty", n_layers=0)
    _refused(lib, edit(3, cin=24), b"inconsistent")            # cin != the previous cout
    _refused(lib, edit(2, cin=16), b"inconsistent")            # the block's first layer reads the residual's input
    _refused(lib, edit(3, cout=24), b"inconsistent")           # last-of-block cout != the residual branch's (and the next cin)
    _refused(lib, edit(2, role=ROLE_PLAIN), b"inconsistent")   # residual 1x1 not followed by first-of-block
    _refused(lib, SMALL[:-3], b"inconsistent")                 # ends inside a block
    _refused(lib, edit(5, norm=7), b"norm")
    _refused(lib, edit(1, taps=3), b"1x1")
    n = ctypes.c_size_t(0)
    assert lib.rnnt_engine_encoder_packed_bytes(None, 3, ctypes.byref(n)) == -1 and b"null" in lib.rnnt_engine_last_error()
    assert lib.rnnt_engine_encoder_packed_bytes(layers(SMALL), len(SMALL), None) == -1
    assert lib.rnnt_engine_encoder_workspace_bytes(layers(SMALL), len(SMALL), 0, 50, REGIME_AUTO, None, ctypes.byref(n)) == -1
    assert lib.rnnt_engine_encoder_workspace_bytes(layers(SMALL), len(SMALL), 1, 1, REGIME_AUTO, None, ctypes.byref(n)) == -1
    assert b"too short" in lib.rnnt_engine_last_error()
    assert lib.rnnt_engine_encoder_workspace_bytes(layers(SMALL), len(SMALL), 1, 50, 9, None, ctypes.byref(n)) == -1


def test_run_entries_check_arguments_before_launching(lib):
    arr = layers(SMALL)
    strides = (ctypes.c_int64 * 3)(9 * 50, 50, 1)
    rc = lib.rnnt_engine_encoder_fwd(arr, len(SMALL), None, None, strides, 1, 50, REGIME_AUTO, None, None, ctypes.c_size_t(0), None)
    assert rc == -1 and b"null" in lib.rnnt_engine_last_error()
    rc = lib.rnnt_engine_encoder_stream_push(arr, len(SMALL), None, None, strides, 1, 50, None, None, None, None, REGIME_AUTO, None, None,
                                             ctypes.c_size_t(0), None)
    assert rc == -1 and b"null" in lib.rnnt_engine_last_error()
    assert lib.rnnt_engine_encoder_pack(arr, len(SMALL), None, ctypes.c_size_t(0), None) == -1


def test_instance_norm_over_one_output_frame_is_refused_by_the_size_query(lib):
    """No variance over one frame: the reference and the Python path raise; the C ABI refuses from the size query on (no GPU needed)
    and so, by the same make_plan, from the run entries before anything is enqueued."""
    n = ctypes.c_size_t(0)

    def ask(spec, L, lens=None, regime=REGIME_AUTO):
        st = None if lens is None else (ctypes.c_int32 * len(spec))(*lens)
        return lib.rnnt_engine_encoder_workspace_bytes(layers(spec), len(spec), 2, L, regime, st, ctypes.byref(n))

    one = lambda norm: [(8, 12, 3, 1, 1, norm, ROLE_PLAIN)]
    for regime in (REGIME_AUTO, REGIME_MANY_ROWS):
        assert ask(one(NORM_INSTANCE), 1, regime=regime) == -1  # whole utterance: 2 zeros + 1 frame -> 1 output frame
        msg = lib.rnnt_engine_last_error()
        assert b"instance norm" in msg and b"layer 0" in msg, msg
        assert ask(one(NORM_INSTANCE), 1, [2], regime) == -1 and b"instance norm" in lib.rnnt_engine_last_error()
        assert ask(one(NORM_BATCH), 1, regime=regime) == 0 and n.value > 0   # the same layer with batch norm
        assert ask(one(NORM_NONE), 1, regime=regime) == 0
        assert ask(one(NORM_INSTANCE), 2, regime=regime) == 0 and n.value > 0  # ... or with two frames
        assert ask(one(NORM_INSTANCE), 1, [3], regime) == 0                    # (3 of state + 1: two frames)
    # the layer is named: here the block's residual 1x1 (layer 1) is the first with instance norm and one frame
    block = [(8, 8, 3, 2, 1, NORM_BATCH, ROLE_PLAIN), (8, 16, 1, 1, 1, NORM_INSTANCE, ROLE_RESIDUAL),
             (8, 16, 3, 1, 1, NORM_BATCH, ROLE_FIRST | ROLE_LAST), (16, 4, 1, 1, 1, NORM_NONE, ROLE_FINAL)]
    assert ask(block, 2) == -1
    msg = lib.rnnt_engine_last_error()
    assert b"instance norm" in msg and b"layer 1" in msg, msg
    assert ask(block, 4) == 0


def test_lists_without_a_final_layer_are_accepted_by_the_size_queries(lib):
    """`out` takes the last layer of the list whatever its role (the header); the workspace is what it was."""
    n, w = ctypes.c_size_t(0), ctypes.c_size_t(0)
    lists = ([(8, 12, 3, 1, 1, NORM_BATCH, ROLE_PLAIN)],
             [(8, 12, 3, 2, 1, NORM_NONE, ROLE_PLAIN), (12, 7, 5, 1, 2, NORM_INSTANCE, ROLE_PLAIN)],
             [(8, 16, 1, 1, 1, NORM_BATCH, ROLE_RESIDUAL), (8, 16, 3, 1, 1, NORM_BATCH, ROLE_FIRST | ROLE_LAST)],
             SMALL[:-1])
    for spec in lists:
        assert lib.rnnt_engine_encoder_packed_bytes(layers(spec), len(spec), ctypes.byref(n)) == 0 and n.value > 0
        for regime in (REGIME_AUTO, REGIME_MANY_ROWS):
            assert lib.rnnt_engine_encoder_workspace_bytes(layers(spec), len(spec), 3, 40, regime, None, ctypes.byref(w)) == 0
            assert w.value > 0 and w.value % 256 == 0
    # a trailing FINAL adds no activation buffer: the plan of the layers in front of it is the plan of the list without it
    with_final, without = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.rnnt_engine_encoder_workspace_bytes(layers(SMALL), len(SMALL), 3, 40, REGIME_AUTO, None, ctypes.byref(with_final)) == 0
    assert lib.rnnt_engine_encoder_workspace_bytes(layers(SMALL), len(SMALL) - 1, 3, 40, REGIME_AUTO, None, ctypes.byref(without)) == 0
    assert without.value <= with_final.value
