"""CPU tests of the encoder's training C ABI (include/rnnt_engine.h rnnt_engine_encoder_train_*): symbols, size queries, host-side
argument checks (nothing is launched: every run call here is refused before its first kernel) and the Python mirror of the training
plan (tests/encoder_train_cases.py train_plan) held to the C size queries."""
import ctypes

import pytest

from rnnt_amd.encoder import NORM_BATCH, NORM_INSTANCE, REGIME_AUTO, REGIME_MANY_ROWS, ROLE_FIRST, ROLE_LAST, ROLE_PLAIN, ROLE_RESIDUAL, _Grads
from tests import encoder_train_cases as C
from tests.test_encoder_abi import SMALL, layers

NAMES = ("rnnt_engine_encoder_train_packed_bytes", "rnnt_engine_encoder_train_pack", "rnnt_engine_encoder_train_saved_bytes",
         "rnnt_engine_encoder_train_workspace_bytes", "rnnt_engine_encoder_train_fwd", "rnnt_engine_encoder_train_bwd")


@pytest.fixture(scope="module")
def lib():
    import os
    from rnnt_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build()
    L = engine.lib()
    L.rnnt_engine_last_error.restype = ctypes.c_char_p
    return L


def test_symbols_exist(lib):
    from rnnt_amd import engine
    for name in NAMES:
        assert hasattr(lib, name)
        assert name in engine.EXPORTS and name in engine.SIGNATURES


def test_size_queries_answer(lib):
    arr, n, f = layers(SMALL), ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.rnnt_engine_encoder_packed_bytes(arr, len(SMALL), ctypes.byref(f)) == 0
    assert lib.rnnt_engine_encoder_train_packed_bytes(arr, len(SMALL), ctypes.byref(n)) == 0
    second = sum(t * ci * ((co + 3) // 4 * 4) for ci, co, t, *_ in SMALL) * 4  # [tap][in][out padded to 4]
    assert f.value + second <= n.value <= f.value + second + 256 * len(SMALL) and n.value % 256 == 0
    s, w, m = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.rnnt_engine_encoder_train_saved_bytes(arr, len(SMALL), 3, 101, None, ctypes.byref(s)) == 0
    assert s.value >= 3 * 50 * 12 * 4 * 3 and s.value % 256 == 0  # at least the prologue's o, z and xhat
    assert lib.rnnt_engine_encoder_train_workspace_bytes(arr, len(SMALL), 3, 101, REGIME_AUTO, None, ctypes.byref(w)) == 0
    assert lib.rnnt_engine_encoder_train_workspace_bytes(arr, len(SMALL), 3, 101, REGIME_MANY_ROWS, None, ctypes.byref(m)) == 0
    assert w.value > 0 and m.value > 0 and w.value % 256 == 0
    lead = (ctypes.c_int32 * len(SMALL))(3, 0, 4, 4, 0, 6, 6, 6, 10, 0)  # the epilogue looks 2 frames ahead
    s2 = ctypes.c_size_t(0)
    assert lib.rnnt_engine_encoder_train_saved_bytes(arr, len(SMALL), 3, 101, lead, ctypes.byref(s2)) == 0
    assert 0 < s2.value < s.value  # two frames fewer behind the epilogue


def test_bad_descriptors_lead_and_null_pointers_are_refused_with_a_message(lib):
    n = ctypes.c_size_t(0)
    err = lib.rnnt_engine_last_error

    def both(spec, lead, word, N=1, L=50):
        arr = layers(spec)
        ld = None if lead is None else (ctypes.c_int32 * len(spec))(*lead)
        for call in (lambda: lib.rnnt_engine_encoder_train_saved_bytes(arr, len(spec), N, L, ld, ctypes.byref(n)),
                     lambda: lib.rnnt_engine_encoder_train_workspace_bytes(arr, len(spec), N, L, REGIME_AUTO, ld, ctypes.byref(n))):
            assert call() != 0
            assert word in err(), err()

    bad = [list(r) for r in SMALL]
    bad[2][2] = 0
    both([tuple(r) for r in bad], None, b"taps")
    both(SMALL[:-3], None, b"inconsistent")
    good = [3, 0, 4, 4, 0, 6, 6, 6, 12, 0]
    for at, v in ((0, 4), (0, -1), (8, 13)):  # beyond (taps-1)*dilation - stride + 1, negative
        lead = list(good)
        lead[at] = v
        both(SMALL, lead, b"lead")
    inside = list(good)
    inside[5] = 4  # look-ahead inside the second block: its last layer and its residual branch differ in length
    both(SMALL, inside, b"inside a block")
    strided = [(9, 12, 5, 2, 1, NORM_BATCH, ROLE_PLAIN), (12, 12, 5, 2, 1, NORM_BATCH, ROLE_PLAIN)]
    both(strided, None, b"stride")  # dX exists for stride 1 only
    both(SMALL, None, b"too short", L=1)
    both([(8, 12, 3, 1, 1, NORM_INSTANCE, ROLE_PLAIN)], None, b"instance norm", L=1)
    arr = layers(SMALL)
    assert lib.rnnt_engine_encoder_train_saved_bytes(arr, len(SMALL), 1, 50, None, None) == -1 and b"null" in err()
    assert lib.rnnt_engine_encoder_train_workspace_bytes(arr, len(SMALL), 1, 50, REGIME_AUTO, None, None) == -1
    assert lib.rnnt_engine_encoder_train_workspace_bytes(arr, len(SMALL), 1, 50, 9, None, ctypes.byref(n)) == -1 and b"regime" in err()
    assert lib.rnnt_engine_encoder_train_packed_bytes(None, 3, ctypes.byref(n)) == -1 and b"null" in err()
    assert lib.rnnt_engine_encoder_train_pack(arr, len(SMALL), None, ctypes.c_size_t(0), None) == -1
    assert lib.rnnt_engine_encoder_train_pack(arr, len(SMALL), ctypes.c_void_p(4096), ctypes.c_size_t(16), None) == -3 and b"packed buffer" in err()


def test_run_entries_check_everything_before_launching(lib):
    """Null pointers, misaligned buffers, a short `saved`, a short workspace, a dropout p of 1, a mask on a 1x1 layer, a norm gradient
    asked of a layer without one: each is refused with its message.  The non-null pointers are never read: every call ends in a
    refusal."""
    k = len(SMALL)
    arr = layers(SMALL)
    for L in arr:  # bias and statistics pointers are checked for NULL, not read
        L.bias = L.mean = L.var = 4096
    err = lib.rnnt_engine_last_error
    strides = (ctypes.c_int64 * 3)(9 * 50, 50, 1)
    big, P = ctypes.c_size_t(1 << 40), ctypes.c_void_p(4096)
    grads = (_Grads * k)()

    def fwd(packed=P, x=P, out=P, saved=P, saved_bytes=big, ws=P, ws_bytes=big, lead=None, keep=None, p=None):
        return lib.rnnt_engine_encoder_train_fwd(arr, k, packed, x, strides, 1, 50, lead, keep, p, REGIME_AUTO, out, saved, saved_bytes, ws,
                                                 ws_bytes, None)

    def bwd(packed=P, x=P, dout=P, saved=P, saved_bytes=big, ws=P, ws_bytes=big, g=grads, keep=None, p=None):
        return lib.rnnt_engine_encoder_train_bwd(arr, k, packed, x, strides, 1, 50, None, keep, p, dout, saved, saved_bytes, g, ws, ws_bytes,
                                                 None)

    for call in (fwd, bwd):
        for name in ("packed", "x", "saved", "ws"):
            assert call(**{name: None}) == -1 and b"null" in err()
        assert call(saved=ctypes.c_void_p(4100)) == -1 and b"aligned" in err()
        assert call(saved_bytes=ctypes.c_size_t(1024)) == -3 and b"saved" in err()
        assert call(ws_bytes=ctypes.c_size_t(1024)) == -3 and b"workspace" in err()
        assert call(p=(ctypes.c_float * k)(*([0.0] * 3 + [1.0] + [0.0] * 6))) == -1 and b"dropout" in err()
        keep = (ctypes.c_void_p * k)()
        keep[1] = 4096  # the first block's residual 1x1
        assert call(keep=keep) == -1 and b"keep mask" in err()
    assert fwd(out=None) == -1 and b"null" in err()
    assert bwd(dout=None) == -1 and b"null" in err()
    assert bwd(g=None) == -1 and b"null" in err()
    lead = (ctypes.c_int32 * k)(3, 0, 5, 4, 0, 6, 6, 6, 12, 0)
    assert fwd(lead=lead) == -1 and b"lead" in err()
    grads[9].gamma = 4096  # the output 1x1 has no norm
    assert bwd() == -1 and b"without a norm" in err()


def _c_sizes(lib, specs, N, L, lead, regime):
    spec = [(l.cin, l.cout, l.taps, l.stride, l.dil, l.norm, l.role) for l in specs]
    arr = layers(spec)
    ld = None if lead is None else (ctypes.c_int32 * len(spec))(*lead)
    s, w = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.rnnt_engine_encoder_train_saved_bytes(arr, len(spec), N, L, ld, ctypes.byref(s)) == 0, lib.rnnt_engine_last_error()
    assert lib.rnnt_engine_encoder_train_workspace_bytes(arr, len(spec), N, L, regime, ld, ctypes.byref(w)) == 0
    return s.value, w.value


@pytest.mark.parametrize("name,kind", C.case_ids())
def test_the_plan_mirror_gives_the_c_size_queries(lib, name, kind):
    case = C.build(name, kind)
    C.check_reach(case)
    for regime in (REGIME_AUTO, REGIME_MANY_ROWS):
        tp = C.train_plan(case.layers, case.N, case.L, case.lead, regime)
        assert (tp.saved_bytes, tp.ws_bytes) == _c_sizes(lib, case.layers, case.N, case.L, case.lead, regime), (name, regime)
    if all(l.lead == (l.taps - 1) * l.dil - l.stride + 1 or l.taps == 1 for l in case.layers):  # lead NULL = no look-ahead
        assert (case.plan.saved_bytes, case.plan.ws_bytes) == _c_sizes(lib, case.layers, case.N, case.L, None, REGIME_AUTO)


def test_the_plan_mirror_at_the_module_shapes(lib):
    """The small config of the fixtures (N = 3, 101 frames, with and without the epilogue's look-ahead) and the reference's widths at
    (4, 1000): saved bytes, workspace bytes; and the saved set is what the header documents."""
    from types import SimpleNamespace as S
    small = [S(cin=a, cout=b, taps=t, stride=s, dil=d, norm=n, role=r) for a, b, t, s, d, n, r in SMALL]
    for lead in (None, [3, 0, 4, 4, 0, 6, 6, 6, 10, 0]):
        for regime in (REGIME_AUTO, REGIME_MANY_ROWS):
            tp = C.train_plan(small, 3, 101, lead, regime)
            assert (tp.saved_bytes, tp.ws_bytes) == _c_sizes(lib, small, 3, 101, lead, regime)
    tp = C.train_plan(small, 3, 101, None)
    k = tp.rows[0].kept
    assert 3 * 50 * 12 == 1800 and (k.o, k.z, k.xh, k.rstd) == (0, 1856, 3712, None)  # batch norm: no rstd; pieces of 29 x 256 bytes
    assert tp.rows[1].kept.o is None and tp.rows[1].kept.z is None and tp.rows[1].kept.xh is not None  # a residual 1x1 keeps xhat only
    assert tp.rows[-1].kept.__dict__ == dict(o=None, z=None, xh=None, rstd=None)                        # the output 1x1 keeps nothing
    assert tp.rows[5].kept.rstd is not None
    I = NORM_INSTANCE
    wide = [S(cin=201, cout=256, taps=11, stride=2, dil=1, norm=I, role=ROLE_PLAIN)]
    for k_, ci, co in ((11, 256, 256), (13, 256, 384), (25, 384, 512)):
        wide.append(S(cin=ci, cout=co, taps=1, stride=1, dil=1, norm=I, role=ROLE_RESIDUAL))
        for j in range(4):
            role = (ROLE_FIRST if j == 0 else 0) | (ROLE_LAST if j == 3 else 0)
            wide.append(S(cin=ci if j == 0 else co, cout=co, taps=k_, stride=1, dil=1, norm=I, role=role))
    wide.append(S(cin=512, cout=512, taps=29, stride=1, dil=2, norm=I, role=ROLE_PLAIN))
    wide.append(S(cin=512, cout=1024, taps=1, stride=1, dil=1, norm=0, role=8))
    tp = C.train_plan(wide, 4, 1000, None)
    assert (tp.saved_bytes, tp.ws_bytes) == _c_sizes(lib, wide, 4, 1000, None, REGIME_AUTO)
    assert tp.rows[-2].dw_ranges == 2 and tp.rows[0].dw_ranges == 12  # 4 x 4 x 29 tiles need two row ranges, the prologue's 44 twelve
