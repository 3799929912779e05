"""CPU tests of tests/optim_cases.py: the restated update is torch's float64 AdamW, the size and list tables state what they claim,
the arenas lay out what they promise, and the bar (4 x max(fp32 CPU path's error, 2^-24)) leaves an fp32 implementation of the
kernel's formula at half of it or less.  The ratios are printed (pytest -s)."""
import numpy as np
import pytest
import torch

from tests import optim_cases as oc


def test_size_list_and_offset_premises():
    oc.check_size_premises()
    oc.check_list_premises()
    oc.check_offset_premises()


@pytest.mark.parametrize("max_norm", [None, 2.0, 1e9])
def test_restated_update_is_torch_float64(max_norm):
    sizes = [0, 1, 5, 257, 1028]
    steps = [3, 3, 2, 3, 1]  # tensors that skipped a step or joined later carry their own count
    x = oc.make_inputs(sizes, 3, gscale=2.0)
    ref = oc.torch_step(x, oc.HP, None, torch.float64, max_norm, steps=steps)
    total = oc.norm64(x["g"])
    if max_norm is not None:
        assert abs(ref["norm"] - total) <= 1e-14 * total
    for i, step in enumerate(steps):
        for write in (0, 1):
            p, g, m, v = oc.adamw_restated(x["p"][i], x["g"][i], x["m"][i], x["v"][i], oc.HP, step,
                                           total if max_norm is not None else None, max_norm if max_norm is not None else -1.0, write)
            for name, got in (("p", p), ("m", m), ("v", v)):
                assert oc.rel_err(got, ref[name][i]) <= 1e-14, (name, i)
            if write:
                assert oc.rel_err(g, ref["g"][i]) <= 1e-14
            else:
                assert np.array_equal(g, x["g"][i].astype(np.float64))
    if max_norm == 2.0:
        assert total > 2.0 and not np.array_equal(ref["g"][4], x["g"][4].astype(np.float64))  # the clip did something


def test_restated_update_without_clip_arguments():
    x = oc.make_inputs([33], 4)
    one = lambda **kw: oc.adamw_restated(x["p"][0], x["g"][0], x["m"][0], x["v"][0], oc.HP, 7, **kw)
    plain = one()
    for kw in (dict(total_norm=100.0, max_norm=0.0), dict(total_norm=100.0, max_norm=-1.0), dict(total_norm=None, max_norm=1.0)):
        assert all(np.array_equal(a, b) for a, b in zip(one(**kw), plain)), kw
    zero = oc.adamw_restated(x["p"][0], 0 * x["g"][0], 0 * x["m"][0], 0 * x["v"][0], oc.HP, 1, total_norm=0.0, max_norm=1.0)
    assert np.array_equal(zero[0], x["p"][0].astype(np.float64) * (1 - oc.LR * 0.01)) and not zero[2].any() and not zero[3].any()


def test_arena_layout_and_guards():
    sizes = [0, 1, 5, 4097, 3, 64, 7]
    for mode in oc.MODES + ("mix",):
        x = oc.make_inputs(sizes, 5)
        ar = oc.make_arenas(x, mode, "cpu")
        for k in oc.ARENAS:
            a, offs = ar[k], oc.offsets(mode, k, len(sizes))
            assert [(a.ptr(i) % 16) // 4 for i in range(len(sizes))] == offs
            assert all(np.array_equal(a.get(i), x[k][i]) for i in range(len(sizes)))
            ends = [0] + [s + n for s, n in zip(a.starts, a.sizes)]
            assert all(s - e >= oc.GUARD for s, e in zip(a.starts, ends)) and a.buf.numel() - ends[-1] == oc.GUARD
        oc.assert_guards(ar)
    on_grid = lambda a: all(a.ptr(i) % 16 == 0 for i in range(len(sizes)))
    ar = oc.make_arenas(oc.make_inputs(sizes, 5), "g", "cpu")
    assert on_grid(ar["p"]) and on_grid(ar["m"]) and on_grid(ar["v"]) and not any(ar["g"].ptr(i) % 16 == 0 for i in range(len(sizes)))
    # one float written before, after or between slices is noticed; a write inside a slice is not a guard's business
    for pos in (0, ar["g"].starts[2] - 1, ar["g"].starts[2] + 5, ar["g"].buf.numel() - 1):
        ar = oc.make_arenas(oc.make_inputs(sizes, 5), "g", "cpu")
        ar["g"].view(2).fill_(1.0)
        assert ar["g"].guards_intact()
        ar["g"].buf[pos] = 0.0
        assert not ar["g"].guards_intact(), pos
        with pytest.raises(AssertionError, match="g arena"):
            oc.assert_guards(ar)


def _single_step_cases():
    for zero in (False, True):
        yield f"sizes {'zero' if zero else 'warm'} state", oc.make_inputs(oc.SIZE_LIST, 21, zero_state=zero), 1 if zero else 4, None
    for name, sizes in oc.LISTS.items():
        yield "list " + name, oc.make_inputs(sizes, 22, gscale=2.0), 3, 2.0
    yield "step 1e6", oc.make_inputs(oc.HYPER_SIZES, 23), oc.LATE_STEP, None


def test_fp32_cpu_path_is_inside_its_own_bar():
    """By construction; what the run shows is how far above the 2^-24 floor each case's bar lies."""
    for tag, x, step, max_norm in _single_step_cases():
        ref, got = oc.torch_step(x, oc.HP, step, torch.float64, max_norm), oc.torch_step(x, oc.HP, step, torch.float32, max_norm)
        bar = oc.bars(ref, got)
        assert all(4 * oc.FLOOR <= b < 1e-5 for b in bar.values()), (tag, bar)
        assert oc.check("torch fp32: " + tag, got, ref, bar) <= 1.0 / oc.MARGIN
        # the kernel's formula in fp32 on the same case
        coef = oc.clip_coef_f32(oc.norm64(x["g"]), max_norm) if max_norm is not None else 1.0
        emu = dict(zip("pgmv", zip(*[oc.kernel_emulation_f32(x["p"][i], x["g"][i], x["m"][i], x["v"][i], oc.HP, step, coef)
                                     for i in range(len(x["p"]))])))
        assert oc.check("fp32 emulation: " + tag, emu, ref, bar) <= 0.5


@pytest.mark.parametrize("name", list(oc.HYPERS))
@pytest.mark.parametrize("max_norm", [None, 2.0])
def test_fp32_emulation_of_the_kernel_sits_at_half_the_bar(name, max_norm):
    hp = oc.HYPERS[name]
    p0, grads = oc.hyper_run_inputs()
    groups = [(list(range(len(p0))), hp)]
    ref, got = oc.torch_run(p0, grads, groups, torch.float64, max_norm), oc.torch_run(p0, grads, groups, torch.float32, max_norm)
    if max_norm is not None:
        assert ref["norm"] > max_norm  # the last step clips
    bar = oc.bars(ref, got)
    assert oc.check(f"torch fp32: {name} clip {max_norm}", got, ref, bar) <= 1.0 / oc.MARGIN
    emu = oc.emulation_run(p0, grads, hp, max_norm)
    assert oc.check(f"fp32 emulation: {name} clip {max_norm}", emu, ref, bar) <= 0.5
    if hp["lr"] == 0.0 and hp["weight_decay"] == 0.0:
        assert all(np.array_equal(a, b) for a, b in zip(emu["p"], p0))


def test_lerp_switch_is_what_keeps_beta1_0_beta2_0_inside_the_bar():
    """m += (1 - b1)(g - m) at b1 = 0 keeps an ulp of the old m; at b2 = 0 the update m / (|g| + eps) magnifies it for small |g|.
    Without the switch the fp32 formula misses this bar by orders of magnitude, with it it does not."""
    hp = oc.HYPERS["beta1 0 beta2 0"]
    p0, grads = oc.hyper_run_inputs()
    groups = [(list(range(len(p0))), hp)]
    ref, got = oc.torch_run(p0, grads, groups, torch.float64), oc.torch_run(p0, grads, groups, torch.float32)
    bar = oc.bars(ref, got)
    without = oc.emulation_run(p0, grads, hp, lerp_switch=False)
    ratio = oc.worst(without, ref, "p") / bar["p"]
    print(f"beta1 0 beta2 0 without the lerp switch: p at {ratio:.1f} x the bar")
    assert ratio > 10.0
    assert oc.worst(oc.emulation_run(p0, grads, hp), ref, "p") <= 0.5 * bar["p"]
