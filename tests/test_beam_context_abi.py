"""CPU: the C ABI of contextual biasing — rnnt_engine_beam_decode_ctx, rnnt_engine_beam_decode_batch_ctx and their workspace queries
(include/rnnt_engine.h): exported and bound, every refusal a code and a message before anything is enqueued (no device is needed: nothing
is launched), each query refusing what the plain query refuses, the version unchanged."""
import ctypes

import pytest

NAMES = ("rnnt_engine_beam_decode_ctx_workspace_bytes", "rnnt_engine_beam_decode_ctx",
         "rnnt_engine_beam_decode_batch_ctx_workspace_bytes", "rnnt_engine_beam_decode_batch_ctx")


@pytest.fixture(scope="module")
def lib():
    from rnnt_amd import engine
    L = engine.lib()
    L.rnnt_engine_last_error.restype = ctypes.c_char_p
    return L


def test_symbols_are_exported_bound_and_the_version_stays(lib):
    from rnnt_amd import engine
    for n in NAMES:
        assert hasattr(lib, n) and n in engine.EXPORTS and n in engine.SIGNATURES, n
        assert len(getattr(lib, n).argtypes) == len(engine.SIGNATURES[n])
    # the plain entry point's arguments, then the graph, then the stream
    assert engine.SIGNATURES["rnnt_engine_beam_decode_ctx"] == engine.SIGNATURES["rnnt_engine_beam_decode"][:-1] + "pp"
    assert engine.SIGNATURES["rnnt_engine_beam_decode_batch_ctx"] == engine.SIGNATURES["rnnt_engine_beam_decode_batch"][:-1] + "pp"
    assert engine.SIGNATURES["rnnt_engine_beam_decode_ctx_workspace_bytes"] == engine.SIGNATURES["rnnt_engine_beam_decode_workspace_bytes"]
    assert lib.rnnt_engine_version() == 4  # callers detect the feature by symbol


def _q(fn, *sizes):
    n = ctypes.c_size_t(0)
    return fn(*sizes, ctypes.byref(n)), n.value


OK = (32, 48, 64, 64, 32, 0, 60, 4)
BAD = [(32, 48, 64, 64, 32, 0, 60, 0), (32, 48, 64, 64, 32, 0, 60, 17), (32, 48, 64, 60, 32, 0, 60, 4), (32, 48, 64, 64, 30, 0, 60, 4),
       (32, 1028, 64, 64, 32, 0, 60, 4), (32, 48, 66, 64, 32, 1, 60, 4), (32, 48, 64, 64, 32, 0, 1, 4), (32, 48, 56, 64, 32, 0, 60, 4),
       (0, 48, 64, 64, 32, 0, 60, 4), (32, 48, 64, 64, 32, 0, 70000, 4)]


def test_queries_refuse_what_the_plain_queries_refuse(lib):
    rc, plain = _q(lib.rnnt_engine_beam_decode_workspace_bytes, *OK)
    rc2, ctx = _q(lib.rnnt_engine_beam_decode_ctx_workspace_bytes, *OK)
    assert rc == rc2 == 0 and plain <= ctx <= plain + 512  # a node per slot more, nothing else
    for n_utt in (1, 7, 64):
        rb, pb = _q(lib.rnnt_engine_beam_decode_batch_workspace_bytes, *OK, n_utt)
        rc3, cb = _q(lib.rnnt_engine_beam_decode_batch_ctx_workspace_bytes, *OK, n_utt)
        assert rb == rc3 == 0 and pb <= cb <= pb + 512 * n_utt
    for sizes in BAD:
        want = _q(lib.rnnt_engine_beam_decode_workspace_bytes, *sizes)[0]
        assert want != 0
        assert _q(lib.rnnt_engine_beam_decode_ctx_workspace_bytes, *sizes)[0] == want, sizes
        assert _q(lib.rnnt_engine_beam_decode_batch_ctx_workspace_bytes, *sizes, 8)[0] == want, sizes
    for n_utt in (0, 65, -1):
        assert _q(lib.rnnt_engine_beam_decode_batch_ctx_workspace_bytes, *OK, n_utt)[0] == -2
        assert b"n_utt" in lib.rnnt_engine_last_error()
    assert lib.rnnt_engine_beam_decode_ctx_workspace_bytes(*OK, None) == -1
    assert lib.rnnt_engine_beam_decode_batch_ctx_workspace_bytes(*OK, 8, None) == -1


def _graph(n_nodes=3, n_children=2, score=1.5, **arrays):
    from rnnt_amd.engine import _BeamContext
    ptr = dict(child_off=16, child_tok=16, child_node=16, fail_link=16, depth=16, terminal=16)
    ptr.update(arrays)
    return _BeamContext(n_nodes, n_children, score, *[ptr[k] for k in ("child_off", "child_tok", "child_node", "fail_link", "depth", "terminal")])


def _single(lib, graph="ok", frames=16, params=True, W=16, bias=16, state=16, tokens=16, scores=16, ws=256, beam=4, T=10, ws_bytes=1 << 30,
            iterations=0):
    from rnnt_amd.engine import _PredParams
    p = _PredParams(*([16] * 11)) if params else None
    g = _graph() if graph == "ok" else graph
    return lib.rnnt_engine_beam_decode_ctx(frames, ctypes.c_int64(64), T, ctypes.byref(p) if p is not None else None, 32, 48, 64,
                                           ctypes.c_float(1e-5), ctypes.c_float(1e-5), None, None, W, bias, 64, 32, 31, 60, 10, beam, None,
                                           iterations, 1, None, state, tokens, scores, ws, ctypes.c_size_t(ws_bytes),
                                           ctypes.byref(g) if g is not None else None, None)


def _batch(lib, graph="ok", frames=16, utt=16, params=True, W=16, bias=16, state=16, tokens=16, scores=16, ws=256, beam=4, rows=40, n_utt=4,
           max_frames=10, ws_bytes=1 << 30, iterations=0):
    from rnnt_amd.engine import _PredParams
    p = _PredParams(*([16] * 11)) if params else None
    g = _graph() if graph == "ok" else graph
    return lib.rnnt_engine_beam_decode_batch_ctx(frames, ctypes.c_int64(64), rows, utt, n_utt, max_frames,
                                                 ctypes.byref(p) if p is not None else None, 32, 48, 64, ctypes.c_float(1e-5),
                                                 ctypes.c_float(1e-5), None, None, W, bias, 64, 32, 31, 60, 10, beam, None, iterations, 1, None,
                                                 state, tokens, scores, ws, ctypes.c_size_t(ws_bytes),
                                                 ctypes.byref(g) if g is not None else None, None)


@pytest.mark.parametrize("call", [_single, _batch], ids=["single", "batch"])
def test_bad_graphs_are_refused_before_any_launch(lib, call):
    """Every other argument is valid-looking (never dereferenced by the host): the refusal is the graph's."""
    assert call(lib, graph=None) == -1 and b"null" in lib.rnnt_engine_last_error() and b"ctx" in lib.rnnt_engine_last_error()
    for name in ("child_off", "child_tok", "child_node", "fail_link", "depth", "terminal"):
        assert call(lib, graph=_graph(**{name: None})) == -1, name
        assert b"null" in lib.rnnt_engine_last_error(), name
    for kw in (dict(n_nodes=0), dict(n_nodes=-3), dict(n_children=-1), dict(n_nodes=3, n_children=3)):
        assert call(lib, graph=_graph(**kw)) == -1, kw
        assert b"n_nodes" in lib.rnnt_engine_last_error()
    for score in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert call(lib, graph=_graph(score=score)) == -1, score
        assert b"score" in lib.rnnt_engine_last_error()
    assert call(lib, graph=_graph(n_nodes=65537, n_children=65536)) == -2  # beyond the device's envelope: the caller's host loop
    assert b"n_nodes" in lib.rnnt_engine_last_error()
    assert call(lib, graph=_graph(depth=18)) == -1 and b"aligned" in lib.rnnt_engine_last_error()


@pytest.mark.parametrize("call", [_single, _batch], ids=["single", "batch"])
def test_every_refusal_of_the_plain_entry_point_stands(lib, call):
    for kw in (dict(frames=None), dict(params=False), dict(W=None), dict(bias=None), dict(state=None), dict(tokens=None), dict(scores=None),
               dict(ws=None)):
        assert call(lib, **kw) == -1, kw
        assert b"null" in lib.rnnt_engine_last_error(), kw
    assert call(lib, beam=0) == -1
    assert call(lib, beam=17) == -2 and b"beam" in lib.rnnt_engine_last_error()
    assert call(lib, iterations=-1) == -1
    assert call(lib, ws=128) == -1  # not 256-byte aligned
    assert call(lib, ws_bytes=64) == -3 and b"workspace" in lib.rnnt_engine_last_error()
    if call is _batch:
        assert call(lib, utt=None) == -1
        assert call(lib, utt=12) == -1
        assert call(lib, n_utt=0) == -2 and call(lib, n_utt=65) == -2
        assert call(lib, max_frames=0) == -1 and call(lib, rows=5, max_frames=10) == -1
        n = ctypes.c_size_t(0)
        assert lib.rnnt_engine_beam_decode_ctx_workspace_bytes(*OK, ctypes.byref(n)) == 0
        assert call(lib, ws_bytes=n.value) == -3  # one search's workspace does not hold four
    else:
        n, m = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert lib.rnnt_engine_beam_decode_workspace_bytes(*OK, ctypes.byref(n)) == 0
        assert lib.rnnt_engine_beam_decode_ctx_workspace_bytes(*OK, ctypes.byref(m)) == 0
        if m.value > n.value:
            assert call(lib, ws_bytes=n.value) == -3  # the plain search's workspace has no room for the nodes
