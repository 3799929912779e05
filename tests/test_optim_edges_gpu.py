"""-m gpu: the clip and AdamW kernels of rnnt_amd/csrc/optim.hip (k_mt_sumsq, k_mt_norm_final, k_adam_prepare, k_mt_adamw)
against float64 at chunk, quad and list edges — tests/optim_cases.py holds the sizes, the lists, the oracle and the bar rule.

Most calls go through the C ABI on arenas: every p of a case is a slice of one device buffer (so g, m, v), slices sit at chosen
offsets from the 16-byte grid of the vector path and are fenced by guard floats whose bits must survive.  lr = 0.05: an element
that is skipped or updated twice is off by about lr, five orders of magnitude above the bar.  With RNNT_OPTIM_PARITY_OUT=<file>
every measured ratio is appended to that file (profiles/optim_parity.txt is such a run)."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import optim_cases as oc

pytestmark = pytest.mark.gpu
OK, INVALID = 0, -1
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def lib():
    from rnnt_amd import engine
    return engine.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _arr(ptrs):
    return (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)


def _i64(values):
    return (ctypes.c_int64 * max(len(values), 1))(*values)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def scalar(x, dtype=F32):
    return torch.tensor([x], dtype=dtype, device="cuda")


def pointers(ar, idx, null_empties=True):
    """Pointer lists of slices `idx` of the four arenas; an empty tensor hands over NULL, as an empty torch tensor does."""
    sizes = [ar["p"].sizes[i] for i in idx]
    return {k: [0 if (null_empties and n == 0) else ar[k].ptr(i) for i, n in zip(idx, sizes)] for k in oc.ARENAS}, sizes


class DevState:
    """lr, step counter and scratch of the capturable form."""

    def __init__(self, lr, done):
        self.lr, self.step, self.hyper = scalar(lr), scalar(done, torch.int64), torch.zeros(4, dtype=F32, device="cuda")


def abi_step(lib, ptrs, sizes, hp, step, norm=None, max_norm=-1.0, write=1, dev=None):
    """rnnt_engine_adamw_step, or with `dev` (a DevState whose counter stands at step - 1) rnnt_engine_adamw_step_dev."""
    lists = [_arr(ptrs[k]) for k in oc.ARENAS]
    (b1, b2) = hp["betas"]
    tail = (_ptr(norm), ctypes.c_float(max_norm), int(write), _stream())
    if dev is None:
        return lib.rnnt_engine_adamw_step(len(sizes), *lists, _i64(sizes), hp["lr"], b1, b2, hp["eps"], hp["weight_decay"], int(step), *tail)
    return lib.rnnt_engine_adamw_step_dev(len(sizes), *lists, _i64(sizes), _ptr(dev.lr), b1, b2, hp["eps"], hp["weight_decay"],
                                          _ptr(dev.step), _ptr(dev.hyper), *tail)


def step_all(lib, ar, hp, step, form, alone=False, **kw):
    """One update of every slice of the arenas: as one list, or (`alone`) one call per tensor."""
    n = len(ar["p"].sizes)
    for idx in ([[i] for i in range(n)] if alone else [list(range(n))]):
        dev = DevState(hp["lr"], step - 1) if form == "dev" else None
        ptrs, sizes = pointers(ar, idx)
        assert abi_step(lib, ptrs, sizes, hp, step, dev=dev, **kw) == OK, lib.rnnt_engine_last_error()
        if dev is not None:
            assert int(dev.step) == step


def abi_norm(lib, gptrs, sizes, fill=0xFF):
    """rnnt_engine_grad_norm over a workspace filled with `fill`; returns the device scalar."""
    n = ctypes.c_size_t(0)
    assert lib.rnnt_engine_grad_norm_workspace_bytes(len(sizes), _i64(sizes), ctypes.byref(n)) == OK
    ws = torch.full((n.value,), fill, dtype=torch.uint8, device="cuda")
    out = torch.full((1,), float("nan"), device="cuda")
    rc = lib.rnnt_engine_grad_norm(len(sizes), _arr(gptrs), _i64(sizes), _ptr(out), _ptr(ws), ctypes.c_size_t(n.value), _stream())
    assert rc == OK, lib.rnnt_engine_last_error()
    return out


def arena_norm(lib, ar):
    ptrs, sizes = pointers(ar, list(range(len(ar["g"].sizes))))
    return abi_norm(lib, ptrs["g"], sizes)


def results(ar):
    return {k: ar[k].all() for k in oc.ARENAS}


def all_bits(ar):
    return {k: ar[k].bits() for k in oc.ARENAS}


def same_bits(a, b, keys=oc.ARENAS):
    return [k for k in keys if not torch.equal(a[k], b[k])] == []


def clipped_grads_close(got, ref64):
    return all(np.allclose(a, b, rtol=2e-6, atol=0) for a, b in zip(got, ref64))


# ------------------------------------------------------------------------------------------------ 1. every size, every alignment
@functools.lru_cache(maxsize=None)
def size_case(zero):
    x = oc.make_inputs(oc.SIZE_LIST, 21, zero_state=zero)
    step = 1 if zero else 4
    ref = oc.torch_step(x, oc.HP, step, F64)
    return x, step, ref, oc.bars(ref, oc.torch_step(x, oc.HP, step, F32))


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("zero", [False, True], ids=["warm", "zero"])
@pytest.mark.parametrize("mode", oc.MODES)
def test_update_at_every_size_and_alignment(lib, mode, zero, form):
    """Each size stepped alone (one launch each): p, m, v within the bar of float64, every guard intact, g untouched."""
    x, step, ref, bar = size_case(zero)
    ar = oc.make_arenas(x, mode, "cuda")
    g_before = ar["g"].bits()
    step_all(lib, ar, oc.HP, step, form, alone=True)
    oc.assert_guards(ar)
    assert torch.equal(ar["g"].bits(), g_before)
    oc.check(f"sizes {mode} {'zero' if zero else 'warm'} {form}", results(ar), ref, bar)


# ------------------------------------------------------------------------------------------------ 2. lists
@functools.lru_cache(maxsize=None)
def list_case(name):
    x = oc.make_inputs(oc.LISTS[name], 22, gscale=2.0)
    ref = oc.torch_step(x, oc.HP, 3, F64, max_norm=2.0)
    assert ref["norm"] > 2.0
    return x, ref, oc.bars(ref, oc.torch_step(x, oc.HP, 3, F32, max_norm=2.0))


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("name", list(oc.LISTS))
def test_lists_across_launch_boundaries(lib, name, form):
    """The whole list in one call under the clip (norm from the engine): within the bar of float64, and every tensor's bits are
    those it gets when stepped alone with the same device norm."""
    x, ref, bar = list_case(name)
    ar = oc.make_arenas(x, "mix", "cuda")
    norm = arena_norm(lib, ar)
    assert abs(float(norm) - ref["norm"]) <= 1e-6 * ref["norm"]
    step_all(lib, ar, oc.HP, 3, form, norm=norm, max_norm=2.0, write=1)
    oc.assert_guards(ar)
    got = results(ar)
    oc.check(f"list {name} {form}", got, ref, bar)
    assert clipped_grads_close(got["g"], ref["g"])
    alone = oc.make_arenas(x, "mix", "cuda")
    step_all(lib, alone, oc.HP, 3, form, alone=True, norm=norm, max_norm=2.0, write=1)
    assert same_bits(all_bits(ar), all_bits(alone))


@pytest.mark.parametrize("form", ["host", "dev"])
def test_nothing_to_do_changes_nothing(lib, form):
    ar = oc.make_arenas(oc.make_inputs(oc.ONLY_EMPTIES, 1), "aligned", "cuda")
    full = oc.make_arenas(oc.make_inputs([5, 4097], 1), "aligned", "cuda")
    before, before_full = all_bits(ar), all_bits(full)
    for null_empties in (True, False):
        ptrs, sizes = pointers(ar, [0, 1, 2], null_empties)
        assert abi_step(lib, ptrs, sizes, oc.HP, 1, dev=DevState(oc.LR, 0) if form == "dev" else None) == OK
    ptrs, _ = pointers(full, [0, 1])
    assert abi_step(lib, ptrs, [], oc.HP, 1, dev=DevState(oc.LR, 0) if form == "dev" else None) == OK  # n_tensors = 0
    torch.cuda.synchronize()
    assert same_bits(all_bits(ar), before) and same_bits(all_bits(full), before_full)


# ------------------------------------------------------------------------------------------------ 3. norm
@pytest.mark.parametrize("mode", ["aligned", "g"])
def test_norm_at_every_size(lib, mode):
    x = oc.make_inputs(oc.SIZE_LIST, 31)
    ar = oc.make_arenas(x, mode, "cuda")
    before = ar["g"].bits()
    for i, n in enumerate(oc.SIZE_LIST):
        ref = oc.norm64([x["g"][i]])
        got = float(abi_norm(lib, [ar["g"].ptr(i)], [n]))
        print(f"norm size {n:6d} {mode:8s} rel err {abs(got - ref) / ref if ref else abs(got):.3e}")
        assert abs(got - ref) <= 1e-6 * ref, (n, got, ref)
    ref = oc.norm64(x["g"])
    assert abs(float(arena_norm(lib, ar)) - ref) <= 1e-6 * ref
    assert torch.equal(ar["g"].bits(), before)


@pytest.mark.parametrize("name", list(oc.LISTS))
def test_norm_of_every_list(lib, name):
    x, ref, _ = list_case(name)
    ar = oc.make_arenas(x, "mix", "cuda")
    ptrs, sizes = pointers(ar, list(range(len(oc.LISTS[name]))))
    runs = [abi_norm(lib, ptrs["g"], sizes, fill) for fill in (0xFF, 0xFF, 0x00)]
    assert abs(float(runs[0]) - ref["norm"]) <= 1e-6 * ref["norm"]
    assert all(torch.equal(r.view(torch.int32), runs[0].view(torch.int32)) for r in runs)  # reads nothing it did not write


def test_norm_of_zeros_and_of_nothing(lib):
    sizes = [5, 4097, 0, 1028]
    x = oc.make_inputs(sizes, 32, gscale=0.0)
    ar = oc.make_arenas(x, "mix", "cuda")
    out = arena_norm(lib, ar)
    assert float(out) == 0.0 and int(out.view(torch.int32)) == 0
    assert float(abi_norm(lib, [0, 0, 0], oc.ONLY_EMPTIES)) == 0.0
    assert float(abi_norm(lib, [], [])) == 0.0


# ------------------------------------------------------------------------------------------------ 4. clip
CLIP_SIZES = [7, 1028, 3076, 4097]


def clip_run(lib, x, mode="g", **kw):
    ar = oc.make_arenas(x, mode, "cuda")
    step_all(lib, ar, oc.HP, 4, "host", **kw)
    oc.assert_guards(ar)
    return ar


def test_clip_below_at_and_above_max_norm(lib):
    x = oc.make_inputs(CLIP_SIZES, 41, gscale=2.0)
    probe = oc.make_arenas(x, "g", "cuda")
    norm = arena_norm(lib, probe)
    total = float(norm)
    for tag, max_norm in (("below", 2.0 * total), ("at", total), ("above", 2.0)):
        ref = oc.torch_step(x, oc.HP, 4, F64, max_norm=max_norm)
        bar = oc.bars(ref, oc.torch_step(x, oc.HP, 4, F32, max_norm=max_norm))
        ar = clip_run(lib, x, norm=norm, max_norm=max_norm, write=1)
        got = results(ar)
        oc.check(f"clip {tag} max_norm", got, ref, bar)
        assert clipped_grads_close(got["g"], ref["g"])
        if tag == "below":
            assert torch.equal(ar["g"].bits(), probe["g"].bits())
        if tag == "above":
            assert not torch.equal(ar["g"].bits(), probe["g"].bits())
            # write_clipped_grads = 0: the gradients keep their bits and the moments see the clipped values
            quiet = clip_run(lib, x, norm=norm, max_norm=max_norm, write=0)
            assert torch.equal(quiet["g"].bits(), probe["g"].bits())
            assert same_bits(all_bits(quiet), all_bits(ar), "pmv")


def test_no_clip_without_a_norm_or_a_positive_max_norm(lib):
    x = oc.make_inputs(CLIP_SIZES, 42, gscale=2.0)
    plain = clip_run(lib, x)
    norm = arena_norm(lib, plain)
    assert float(norm) > 2.0
    for kw in (dict(norm=norm, max_norm=0.0), dict(norm=norm, max_norm=-1.0), dict(norm=None, max_norm=2.0)):
        for write in (0, 1):
            assert same_bits(all_bits(clip_run(lib, x, write=write, **kw)), all_bits(plain)), (kw, write)
    ref = oc.torch_step(x, oc.HP, 4, F64)
    oc.check("no clip", results(plain), ref, oc.bars(ref, oc.torch_step(x, oc.HP, 4, F32)))


def test_zero_norm_only_decays(lib):
    x = oc.make_inputs(CLIP_SIZES, 43, gscale=0.0, zero_state=True)
    ar = oc.make_arenas(x, "mix", "cuda")
    norm = arena_norm(lib, ar)
    assert float(norm) == 0.0
    step_all(lib, ar, oc.HP, 1, "host", norm=norm, max_norm=1.0, write=1)
    got = results(ar)
    decay = np.float32(1.0 - oc.HP["lr"] * oc.HP["weight_decay"])
    for i in range(len(CLIP_SIZES)):
        assert np.array_equal(got["p"][i], x["p"][i] * decay)
        assert not got["g"][i].any() and not got["m"][i].any() and not got["v"][i].any()


def test_one_inf_in_the_second_launch(lib):
    """The norm is inf, the coefficient 0: the Inf becomes a NaN and every other gradient 0.  Which p stay finite is what torch's
    fp32 path says."""
    x = oc.make_inputs(oc.LISTS["n41"], 44)
    x["g"][40][0] = np.inf
    assert oc.launches_of(oc.LISTS["n41"])[1] == [40]
    with np.errstate(invalid="ignore"):
        ref = oc.torch_step(x, oc.HP, 4, F32, max_norm=2.0)
    ar = oc.make_arenas(x, "mix", "cuda")
    norm = arena_norm(lib, ar)
    assert float(norm) == float("inf") == ref["norm"]
    step_all(lib, ar, oc.HP, 4, "host", norm=norm, max_norm=2.0, write=1)
    got = results(ar)
    for k in "pgmv":
        assert all(np.array_equal(np.isfinite(a), np.isfinite(b)) for a, b in zip(got[k], ref[k])), k
    assert not np.isfinite(got["p"][40][0]) and sum(int((~np.isfinite(a)).sum()) for a in got["p"]) == 1
    oc.assert_guards(ar)


# ------------------------------------------------------------------------------------------------ 5. / 6. hyper-parameters
def optimizer_run(p0, grads, groups, max_norm, capturable, resume_after=None):
    """rnnt_amd.optim.AdamW over the steps of `grads`.  `resume_after` = k: the state dict after k steps moves into a fresh
    non-capturable optimizer, which makes the remaining steps."""
    import rnnt_amd
    make = lambda ps, cap: rnnt_amd.optim.AdamW([dict(params=[ps[i] for i in idx], **hp) for idx, hp in groups],
                                                max_grad_norm=max_norm, capturable=cap)
    ps = [torch.tensor(a, device="cuda").requires_grad_(True) for a in p0]
    opt = make(ps, capturable)
    for k, gs in enumerate(grads):
        if resume_after == k:
            saved = copy.deepcopy(opt.state_dict())
            ps = [p.detach().clone().requires_grad_(True) for p in ps]
            opt = make(ps, False)
            opt.load_state_dict(saved)
        for p, g in zip(ps, gs):
            p.grad = torch.tensor(g, device="cuda")
        opt.step()
        if capturable and resume_after is None:
            assert all(int(opt.state[p]["step"]) == k + 1 for p in ps)
    out = dict(p=[p.detach().cpu().numpy() for p in ps], g=[p.grad.cpu().numpy() for p in ps],
               m=[opt.state[p]["exp_avg"].cpu().numpy() for p in ps], v=[opt.state[p]["exp_avg_sq"].cpu().numpy() for p in ps],
               norm=float(opt.last_grad_norm) if max_norm is not None else None)
    assert all(int(opt.state[p]["step"]) == len(grads) for p in ps)
    return out


@functools.lru_cache(maxsize=None)
def hyper_case(name, max_norm):
    p0, grads = oc.hyper_run_inputs()
    groups = [(list(range(len(p0))), oc.HYPERS[name])]
    ref = oc.torch_run(p0, grads, groups, F64, max_norm)
    return p0, grads, groups, ref, oc.bars(ref, oc.torch_run(p0, grads, groups, F32, max_norm))


@pytest.mark.parametrize("capturable", [False, True], ids=["host", "capturable"])
@pytest.mark.parametrize("max_norm", [None, 2.0], ids=["noclip", "clip2"])
@pytest.mark.parametrize("name", list(oc.HYPERS))
def test_hyper_parameter_sets_over_three_steps(name, max_norm, capturable):
    p0, grads, groups, ref, bar = hyper_case(name, max_norm)
    got = optimizer_run(p0, grads, groups, max_norm, capturable)
    oc.check(f"hyper {name} clip {max_norm} {'capturable' if capturable else 'host'}", got, ref, bar)
    if max_norm is not None:
        assert abs(got["norm"] - ref["norm"]) <= 1e-6 * ref["norm"]
        assert clipped_grads_close(got["g"], ref["g"])
    hp = oc.HYPERS[name]
    if hp["lr"] == 0.0 and hp["weight_decay"] == 0.0:
        assert all(np.array_equal(a, b) for a, b in zip(got["p"], p0))


@pytest.mark.parametrize("form", ["host", "dev"])
def test_reference_betas_at_step_one_million(lib, form):
    x = oc.make_inputs(oc.HYPER_SIZES, 23)
    ref = oc.torch_step(x, oc.HP, oc.LATE_STEP, F64)
    bar = oc.bars(ref, oc.torch_step(x, oc.HP, oc.LATE_STEP, F32))
    ar = oc.make_arenas(x, "mix", "cuda")
    step_all(lib, ar, oc.HP, oc.LATE_STEP, form)
    oc.assert_guards(ar)
    oc.check(f"step 1e6 {form}", results(ar), ref, bar)


def test_device_counter_counts_calls(lib):
    x = oc.make_inputs([5, 1028], 61)
    ar = oc.make_arenas(x, "aligned", "cuda")
    dev = DevState(oc.LR, 7)
    ptrs, sizes = pointers(ar, [0, 1])
    ref = {k: [a.astype(np.float64) for a in x[k]] for k in "pgmv"}
    for k in range(1, 4):
        assert abi_step(lib, ptrs, sizes, oc.HP, None, dev=dev) == OK
        assert int(dev.step) == 7 + k
        for i in range(2):
            ref["p"][i], _, ref["m"][i], ref["v"][i] = oc.adamw_restated(ref["p"][i], ref["g"][i], ref["m"][i], ref["v"][i], oc.HP, 7 + k)
    x32 = x
    for step in (8, 9, 10):  # the bar: torch's fp32 path over the same three steps
        x32 = dict(oc.torch_step(x32, oc.HP, step, F32), g=x["g"])
    oc.check("device counter 8..10", results(ar), ref, oc.bars(ref, x32))


@pytest.mark.parametrize("max_norm", [None, 2.0], ids=["noclip", "clip2"])
def test_capturable_state_dict_resumes_in_a_host_optimizer(max_norm):
    p0, grads, groups, ref, bar = hyper_case("reference betas", max_norm)
    got = optimizer_run(p0, grads, groups, max_norm, True, resume_after=2)
    oc.check(f"capturable -> host resume clip {max_norm}", got, ref, bar)


# ------------------------------------------------------------------------------------------------ 7. two parameter groups
@pytest.mark.parametrize("capturable", [False, True], ids=["host", "capturable"])
def test_two_groups_share_one_clip_coefficient(capturable):
    p0, grads = oc.hyper_run_inputs(seed=71)
    groups = [([0, 2, 4], dict(lr=oc.LR, betas=(0.95, 0.9999), eps=1e-8, weight_decay=0.01)),
              ([1, 3], dict(lr=0.01, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1))]
    ref = oc.torch_run(p0, grads, groups, F64, 2.0)
    bar = oc.bars(ref, oc.torch_run(p0, grads, groups, F32, 2.0))
    alone = oc.norm64([grads[-1][i] for i in groups[0][0]])
    assert ref["norm"] > 2.0 and ref["norm"] > 1.05 * alone  # the second group's gradients weigh in
    got = optimizer_run(p0, grads, groups, 2.0, capturable)
    assert abs(got["norm"] - ref["norm"]) <= 1e-6 * ref["norm"]
    assert clipped_grads_close(got["g"], ref["g"])  # both groups by the one coefficient
    oc.check(f"two groups {'capturable' if capturable else 'host'}", got, ref, bar)


# ------------------------------------------------------------------------------------------------ 8. refusal before the first launch
@pytest.mark.parametrize("entry", ["adamw_step", "adamw_step_dev", "grad_norm"])
@pytest.mark.parametrize("bad", ["2-byte offset", "null"])
def test_bad_entry_45_is_refused_before_anything_runs(lib, entry, bad):
    """An 81-tensor list (three launches) whose entry 45 cannot be used: INVALID_ARG, and the 40 tensors of the first launch keep
    their bits — under the fused clip their gradients would otherwise already be rescaled.  No pointer is dereferenced."""
    sizes = oc.LISTS["n81"]
    assert oc.launches_of(sizes)[1][5] == 45
    ar = oc.make_arenas(oc.make_inputs(sizes, 81, gscale=2.0), "mix", "cuda")
    norm, before = scalar(100.0), all_bits(ar)
    for k in (oc.ARENAS if entry != "grad_norm" else "g"):
        ptrs, _ = pointers(ar, list(range(len(sizes))))
        ptrs[k][45] = 0 if bad == "null" else ptrs[k][45] + 2
        if entry == "grad_norm":
            n = ctypes.c_size_t(0)
            assert lib.rnnt_engine_grad_norm_workspace_bytes(len(sizes), _i64(sizes), ctypes.byref(n)) == OK
            ws, out = torch.zeros(n.value, dtype=torch.uint8, device="cuda"), scalar(-3.0)
            rc = lib.rnnt_engine_grad_norm(len(sizes), _arr(ptrs["g"]), _i64(sizes), _ptr(out), _ptr(ws), ctypes.c_size_t(n.value), _stream())
            torch.cuda.synchronize()
            assert rc == INVALID and float(out) == -3.0 and not ws.any()  # not one partial sum was written
        else:
            dev = DevState(oc.LR, 7) if entry == "adamw_step_dev" else None
            rc = abi_step(lib, ptrs, sizes, oc.HP, 8, norm=norm, max_norm=2.0, write=1, dev=dev)
            torch.cuda.synchronize()
            assert rc == INVALID, (k, rc)
            if dev is not None:
                assert int(dev.step) == 7 and not dev.hyper.any()
        assert same_bits(all_bits(ar), before), k
        assert b"pointer" in lib.rnnt_engine_last_error() and b"tensor 45" in lib.rnnt_engine_last_error()
