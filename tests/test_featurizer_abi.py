"""CPU tests of the featurizer's C ABI (include/rnnt_engine.h rnnt_engine_featurizer_*): every invalid argument is refused on the host,
before anything could be enqueued (there is no GPU here: a launch would be an error of another code), and the size queries agree with
a Python mirror of the frame, state and layout arithmetic."""
import ctypes

import pytest

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    from rnnt_amd import engine
    L = engine.lib()
    L.rnnt_engine_last_error.restype = ctypes.c_char_p
    return L


def _desc(n_fft=400, win=400, hop=160, center=0, log_kind=1, gain=1.0, n_filters=0):
    from rnnt_amd.featurizer import _Desc
    return _Desc(n_fft, win, hop, center, log_kind, gain, n_filters)


class _Args:
    """Valid arguments of rnnt_engine_featurizer_fwd / _stream_push over host buffers that no refused call ever reads."""

    def __init__(self, N=2, T=1000, L=4):
        self.buf = (ctypes.c_float * 4096)()
        p = ctypes.cast(self.buf, ctypes.c_void_p)
        self.p = p
        self.other = ctypes.c_void_p(p.value + 4096)
        self.strides = (ctypes.c_int64 * 3)(201 * L, L, 1)
        self.N, self.T, self.L = N, T, L

    def fwd(self, lib, d, **kw):
        a = dict(basis=self.p, fbank=None, wave=self.p, stride=self.T, N=self.N, T=self.T, lens=None, pcm=0, mean=self.p, invstd=self.p,
                 out=self.p, strides=self.strides, L=self.L, ws=None, ws_bytes=0)
        a.update(kw)
        return lib.rnnt_engine_featurizer_fwd(None if d is None else ctypes.byref(d), a["basis"], a["fbank"], a["wave"], a["stride"], a["N"],
                                              a["T"], a["lens"], a["pcm"], a["mean"], a["invstd"], a["out"], a["strides"], a["L"], a["ws"],
                                              ctypes.c_size_t(a["ws_bytes"]), None)

    def push(self, lib, d, **kw):
        a = dict(basis=self.p, fbank=None, state_in=self.p, slen=240, chunk=self.p, stride=self.T, N=self.N, T=self.T, pcm=1, mean=self.p,
                 invstd=self.p, out=self.p, strides=self.strides, L=6, state_out=self.other, slen_out=280, ws=None, ws_bytes=0)
        a.update(kw)
        return lib.rnnt_engine_featurizer_stream_push(None if d is None else ctypes.byref(d), a["basis"], a["fbank"], a["state_in"], a["slen"],
                                                      a["chunk"], a["stride"], a["N"], a["T"], a["pcm"], a["mean"], a["invstd"], a["out"],
                                                      a["strides"], a["L"], a["state_out"], a["slen_out"], a["ws"],
                                                      ctypes.c_size_t(a["ws_bytes"]), None)


BAD_DESCS = {
    "hop < 1": (dict(hop=0), b"hop_length"),
    "win_length > n_fft": (dict(win=401), b"win_length"),
    "win_length < 1": (dict(win=0), b"win_length"),
    "odd n_fft - win_length": (dict(win=399), b"odd"),
    "center": (dict(center=2), b"center"),
    "log kind": (dict(log_kind=3), b"log kind"),
    "gain": (dict(log_kind=2, gain=0.0), b"gain"),
    "n_filters": (dict(n_filters=-1), b"n_filters"),
}


@pytest.mark.parametrize("name", list(BAD_DESCS))
def test_bad_descriptions_are_refused_by_every_entry(lib, name):
    kw, msg = BAD_DESCS[name]
    d, a, n = _desc(**kw), _Args(), ctypes.c_size_t(0)
    calls = [lib.rnnt_engine_featurizer_basis_bytes(ctypes.byref(d), ctypes.byref(n)),
             lib.rnnt_engine_featurizer_pack(ctypes.byref(d), a.p, a.p, ctypes.c_size_t(1 << 30), None),
             lib.rnnt_engine_featurizer_workspace_bytes(ctypes.byref(d), 2, 4, ctypes.byref(n)),
             a.fwd(lib, d), a.push(lib, d)]
    assert calls == [INVALID] * 5
    assert msg in lib.rnnt_engine_last_error()


def test_null_pointers(lib):
    d, a, n = _desc(), _Args(), ctypes.c_size_t(0)
    assert lib.rnnt_engine_featurizer_basis_bytes(None, ctypes.byref(n)) == INVALID
    assert lib.rnnt_engine_featurizer_basis_bytes(ctypes.byref(d), None) == INVALID
    assert lib.rnnt_engine_featurizer_workspace_bytes(ctypes.byref(d), 2, 4, None) == INVALID
    assert lib.rnnt_engine_featurizer_pack(ctypes.byref(d), None, a.p, ctypes.c_size_t(1 << 30), None) == INVALID
    assert lib.rnnt_engine_featurizer_pack(ctypes.byref(d), a.p, None, ctypes.c_size_t(1 << 30), None) == INVALID
    assert lib.rnnt_engine_featurizer_pack(ctypes.byref(d), a.p, a.p, ctypes.c_size_t(16), None) == WORKSPACE
    assert a.fwd(lib, None) == INVALID
    for k in ("basis", "wave", "mean", "invstd", "out", "strides"):
        assert a.fwd(lib, d, **{k: None}) == INVALID and b"null" in lib.rnnt_engine_last_error(), k
    assert a.fwd(lib, _desc(n_filters=10)) == INVALID and b"null" in lib.rnnt_engine_last_error()  # a filterbank without its matrix
    assert a.fwd(lib, _desc(n_filters=10), fbank=a.p) == WORKSPACE  # ... and without its workspace
    for k in ("basis", "chunk", "mean", "invstd", "out", "strides", "state_in", "state_out"):
        assert a.push(lib, d, **{k: None}) == INVALID and b"null" in lib.rnnt_engine_last_error(), k


def test_lengths_are_checked(lib):
    d, a = _desc(), _Args()
    assert a.fwd(lib, d, N=0) == INVALID and a.fwd(lib, d, T=-1) == INVALID and a.fwd(lib, d, pcm=2) == INVALID
    assert a.fwd(lib, d, L=3) == INVALID and b"frames" in lib.rnnt_engine_last_error()  # 1000 samples give 4
    assert a.fwd(lib, d, lens=(ctypes.c_int32 * 2)(1000, 1001)) == INVALID
    assert a.fwd(lib, d, lens=(ctypes.c_int32 * 2)(-1, 10)) == INVALID
    c = _desc(n_fft=64, win=48, hop=16, center=1)
    assert a.fwd(lib, c, T=32, L=3) == INVALID and b"reflect" in lib.rnnt_engine_last_error()
    assert a.fwd(lib, c, T=200, L=13, lens=(ctypes.c_int32 * 2)(200, 32)) == INVALID and b"reflect" in lib.rnnt_engine_last_error()
    assert a.fwd(lib, _desc(n_fft=40000, win=40000, hop=160)) == UNSUPPORTED
    # streaming: 240 + 1000 samples complete 6 frames and leave 280
    assert a.push(lib, d, L=5) == INVALID and b"completes 6" in lib.rnnt_engine_last_error()
    assert a.push(lib, d, slen_out=279) == INVALID and b"leaves 280" in lib.rnnt_engine_last_error()
    assert a.push(lib, d, slen=-1) == INVALID
    assert a.push(lib, d, state_out=a.p) == INVALID and b"in place" in lib.rnnt_engine_last_error()
    assert a.push(lib, _desc(center=1)) == INVALID and b"centred" in lib.rnnt_engine_last_error()
    assert a.push(lib, _desc(n_fft=64, win=64, hop=100)) == UNSUPPORTED


def test_stage_limit_follows_the_python_mirror(lib):
    """backend "auto" leaves to the torch path exactly the sizes the C side refuses as unsupported (the 64 KB LDS stage)."""
    import rnnt_amd
    n = ctypes.c_size_t(0)
    for n_fft, hop in ((400, 160), (14922, 16), (14924, 16), (10860, 2), (10862, 2), (16352, 1), (16354, 1), (2000, 463), (2000, 464)):
        rc = lib.rnnt_engine_featurizer_basis_bytes(ctypes.byref(_desc(n_fft=n_fft, win=n_fft, hop=hop)), ctypes.byref(n))
        words = rnnt_amd.TFJSSpectrogram(n_fft, hop, n_fft)._stage_words()
        assert rc == (UNSUPPORTED if words > 16384 else 0), (n_fft, hop, words)


def test_size_queries_follow_the_python_mirror(lib):
    from rnnt_amd.featurizer import frame_count, stream_lengths
    n = ctypes.c_size_t(0)
    for n_fft, win, hop in ((400, 400, 160), (64, 48, 16), (126, 126, 40), (16, 16, 8), (30, 10, 7)):
        d = _desc(n_fft=n_fft, win=win, hop=hop)
        assert lib.rnnt_engine_featurizer_basis_bytes(ctypes.byref(d), ctypes.byref(n)) == 0
        bins = n_fft // 2 + 1
        # [bin tile of 32][chunk of 4 samples][64 lanes] x 16 bytes; at 400: 7 x 100 x 64 x 16 = 716 800
        assert n.value == -(-bins // 32) * -(-n_fft // 4) * 64 * 16
        assert lib.rnnt_engine_featurizer_workspace_bytes(ctypes.byref(d), 3, 50, ctypes.byref(n)) == 0 and n.value == 0
        f = _desc(n_fft=n_fft, win=win, hop=hop, n_filters=10)
        assert lib.rnnt_engine_featurizer_workspace_bytes(ctypes.byref(f), 3, 50, ctypes.byref(n)) == 0
        assert 3 * bins * 50 * 4 <= n.value < 3 * bins * 50 * 4 + 256 and n.value % 256 == 0
        # the stream entry accepts exactly the mirror's (frames, state) and nothing next to it; no frame and no samples is a valid push
        a = _Args()
        for slen, T in ((0, 0), (0, n_fft - 1), (n_fft - 1, 1), (3, 5 * hop + n_fft), (n_fft - hop, hop)):
            frames, left = stream_lengths(slen, T, n_fft, hop)
            assert frames == frame_count(slen + T, n_fft, hop) and left == slen + T - frames * hop
            for dL, dS in ((1, 0), (0, 1), (0, -1)):
                assert a.push(lib, d, slen=slen, T=T, L=frames + dL, slen_out=left + dS) == INVALID, (slen, T, dL, dS)
