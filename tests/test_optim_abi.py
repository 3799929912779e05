"""CPU tests of the optimizer's C ABI (include/rnnt_engine.h rnnt_engine_grad_norm*, rnnt_engine_adamw_step*): every invalid
argument is refused on the host with its code and a message, before anything could be enqueued (there is no GPU here: a launch
would be an error of another code), wherever in the list it stands; the workspace query ties tests/optim_cases.py's CHUNK to the
library.  Only refused calls are made: no pointer handed over is ever read."""
import ctypes

import pytest

from tests import optim_cases as oc

OK, INVALID, WORKSPACE = 0, -1, -3


@pytest.fixture(scope="module")
def lib():
    from rnnt_amd import engine
    return engine.lib()


class _Args:
    """A valid argument set over one host buffer (16-byte aligned slices of 64 floats)."""

    def __init__(self, n=3, numel=16):
        self.n = n
        self.buf = (ctypes.c_float * (64 * (n + 4) * 4 + 8))()
        base = (ctypes.addressof(self.buf) + 15) & ~15
        self.lists = {k: [base + 256 * (i * 4 + j) for i in range(n)] for j, k in enumerate("pgmv")}
        self.numels = [numel] * n
        self.scalar = base + 256 * 4 * n  # total_norm / lr / step / hyper / workspace stand-ins
        self.hp = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)

    def arr(self, k):
        return (ctypes.c_void_p * max(self.n, 1))(*self.lists[k])

    def numel_arr(self):
        return (ctypes.c_int64 * max(self.n, 1))(*self.numels)

    def step(self, lib, n_tensors=None, step=1, null=(), total_norm=None, **hp):
        h = dict(self.hp, **hp)
        a = {k: (None if k in null else self.arr(k)) for k in "pgmv"}
        return lib.rnnt_engine_adamw_step(self.n if n_tensors is None else n_tensors, a["p"], a["g"], a["m"], a["v"],
                                          None if "numels" in null else self.numel_arr(), h["lr"], h["beta1"], h["beta2"], h["eps"],
                                          h["weight_decay"], step, total_norm, ctypes.c_float(-1.0), 1, None)

    def step_dev(self, lib, n_tensors=None, null=(), **hp):
        h = dict(self.hp, **hp)
        a = {k: (None if k in null else self.arr(k)) for k in "pgmv"}
        s = {k: (None if k in null else self.scalar) for k in ("lr", "step", "hyper")}
        return lib.rnnt_engine_adamw_step_dev(self.n if n_tensors is None else n_tensors, a["p"], a["g"], a["m"], a["v"],
                                              None if "numels" in null else self.numel_arr(), s["lr"], h["beta1"], h["beta2"], h["eps"],
                                              h["weight_decay"], s["step"], s["hyper"], None, ctypes.c_float(-1.0), 1, None)

    def norm(self, lib, n_tensors=None, null=(), ws_bytes=1 << 30):
        return lib.rnnt_engine_grad_norm(self.n if n_tensors is None else n_tensors, None if "g" in null else self.arr("g"),
                                         None if "numels" in null else self.numel_arr(), None if "out" in null else self.scalar,
                                         None if "ws" in null else self.scalar, ctypes.c_size_t(ws_bytes), None)


def refused(lib, rc, code=INVALID, word=None):
    msg = lib.rnnt_engine_last_error()
    assert rc == code, (rc, msg)
    assert msg and (word is None or word in msg), msg
    return True


def ws_bytes(lib, numels):
    n = ctypes.c_size_t(0)
    assert lib.rnnt_engine_grad_norm_workspace_bytes(len(numels), (ctypes.c_int64 * max(len(numels), 1))(*numels), ctypes.byref(n)) == OK
    return n.value


def test_counts_and_null_arrays(lib):
    a = _Args()
    for call in (a.step, a.step_dev, a.norm):
        refused(lib, call(lib, n_tensors=-1))
    for call in (a.step, a.step_dev):
        for k in ("p", "g", "m", "v", "numels"):
            refused(lib, call(lib, null=(k,)), word=b"null")
    for k in ("g", "numels", "out", "ws"):
        refused(lib, a.norm(lib, null=(k,)))
    n = ctypes.c_size_t(0)
    refused(lib, lib.rnnt_engine_grad_norm_workspace_bytes(1, a.numel_arr(), None))
    refused(lib, lib.rnnt_engine_grad_norm_workspace_bytes(1, None, ctypes.byref(n)))
    refused(lib, lib.rnnt_engine_grad_norm_workspace_bytes(-1, a.numel_arr(), ctypes.byref(n)))


def test_step_count_and_device_scalars(lib):
    a = _Args()
    for step in (0, -1, -2 ** 40):
        refused(lib, a.step(lib, step=step), word=b"step")
    for k in ("lr", "step", "hyper"):
        refused(lib, a.step_dev(lib, null=(k,)), word=b"device scalar")


BAD_HYPER = [("lr", -1e-3), ("lr", float("nan")), ("eps", -1e-8), ("eps", float("nan")), ("beta1", -0.1), ("beta1", 1.0),
             ("beta1", float("nan")), ("beta2", -0.1), ("beta2", 1.0), ("beta2", float("nan")), ("weight_decay", -0.01),
             ("weight_decay", float("nan")), ("lr", float("-inf"))]


@pytest.mark.parametrize("name,value", BAD_HYPER)
def test_invalid_hyper_parameters(lib, name, value):
    a = _Args()
    refused(lib, a.step(lib, **{name: value}), word=b"hyper-parameter")
    if name != "lr":  # the capturable form reads lr on the device
        refused(lib, a.step_dev(lib, **{name: value}), word=b"hyper-parameter")


def test_negative_element_count(lib):
    for at in (0, 2, 45):
        a = _Args(n=max(3, at + 1))
        a.numels[at] = -1
        n = ctypes.c_size_t(0)
        refused(lib, lib.rnnt_engine_grad_norm_workspace_bytes(a.n, a.numel_arr(), ctypes.byref(n)), word=b"negative")
        for call in (a.step, a.step_dev, a.norm):
            refused(lib, call(lib), word=b"negative")


@pytest.mark.parametrize("at", [0, 1, 39, 40, 45, 80])
@pytest.mark.parametrize("bad", ["null", "2-byte offset"])
def test_bad_tensor_pointer_anywhere_in_the_list(lib, at, bad):
    """Among the first 40 tensors and in every later launch: the whole list is checked before the first launch."""
    for k in "pgmv":
        a = _Args(n=81)
        a.lists[k][at] = 0 if bad == "null" else a.lists[k][at] + 2
        for call in (a.step, a.step_dev) + ((a.norm,) if k == "g" else ()):
            refused(lib, call(lib), word=b"pointer")
            assert b"tensor %d" % at in lib.rnnt_engine_last_error()


def test_workspace_one_byte_short(lib):
    a = _Args()
    need = ws_bytes(lib, a.numels)
    refused(lib, a.norm(lib, ws_bytes=need - 1), code=WORKSPACE, word=b"workspace")
    refused(lib, a.norm(lib, ws_bytes=0), code=WORKSPACE)


def test_workspace_query_counts_chunks_of_CHUNK_elements(lib):
    C = oc.CHUNK
    assert ws_bytes(lib, [1]) == ws_bytes(lib, [C]) == ws_bytes(lib, [0]) + 4
    assert ws_bytes(lib, [C + 1]) == ws_bytes(lib, [C]) + 4
    assert ws_bytes(lib, [2 * C]) == ws_bytes(lib, [C + 1]) and ws_bytes(lib, [2 * C + 1]) == ws_bytes(lib, [C]) + 8
    base = ws_bytes(lib, [])
    assert ws_bytes(lib, [0, 0, 0]) == base
    for sizes in ([1, C, C + 1], oc.SIZE_LIST, oc.LISTS["n81"]):  # additive over tensors: one float per chunk
        assert ws_bytes(lib, sizes) - base == sum(ws_bytes(lib, [n]) - base for n in sizes) == 4 * sum(oc.chunks_of(n) for n in sizes)
