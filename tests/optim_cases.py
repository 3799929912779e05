"""Shared by tests/test_optim_oracle.py (CPU), tests/test_optim_abi.py (CPU) and tests/test_optim_edges_gpu.py: the sizes of
rnnt_amd/csrc/optim.hip restated, the float64 oracle of clip + AdamW, the error measure and the bar rule, the size and list tables
with their premises, and the arena builder.  No test functions.

Error measure (the LSTM tests'): max |got - ref| relative to the float64 tensor's largest entry; an identically zero reference
demands exact zeros.  Bar, per case and for each of p, m, v: 4 x max(e32, 2^-24), where e32 is the largest error, over the case's
tensors, of torch's own fp32 CPU path against float64 — 4 is the margin the LSTM, encoder and featurizer tests give a kernel with
another rounding order, 2^-24 the rounding of the stored fp32 result (without that floor e32 is exactly 0 wherever fp32 is exact,
m at beta1 = 0 for one, and the bar would demand bit equality)."""
import math
import os

import numpy as np
import torch

# rnnt_amd/csrc/optim.hip: MT_CHUNK, MT_MAX, MT_THREADS and the quads a thread loads per trip of k_mt_adamw's first loop
CHUNK = 4096
LIST_MAX = 40
THREADS = 256
QUADS_PER_TRIP = 4

FLOOR = 2.0 ** -24
MARGIN = 4.0
LR = 0.05  # an element skipped or applied twice is off by about lr: five orders of magnitude above the bar
HP = dict(lr=LR, betas=(0.95, 0.9999), eps=1e-8, weight_decay=0.01)  # the reference's betas / eps / decay at the tests' lr

# ---------------------------------------------------------------------------------------------------------------- sizes
# (n, n4, tail, premise): n4 = (n % CHUNK) // 4 quads and tail = n % 4 scalars in the last, partial chunk (n % CHUNK == 0: none)
SIZES = [
    (0, 0, 0, "empty: no chunk, never part of a launch"),
    (1, 0, 1, "scalar tail only"),
    (2, 0, 2, "scalar tail only"),
    (3, 0, 3, "scalar tail only"),
    (4, 1, 0, "one quad, no tail"),
    (5, 1, 1, "one quad and a tail"),
    (7, 1, 3, "one quad and the longest tail"),
    (1023, 255, 3, "thread 255 has no quad"),
    (1024, 256, 0, "exactly one quad per thread"),
    (1028, 257, 0, "thread 0 takes a second trip of the one-quad loop"),
    (3072, 768, 0, "no thread takes the four-quad trip"),
    (3076, 769, 0, "thread 0 alone takes the four-quad trip"),
    (4092, 1023, 0, "thread 255 alone misses the four-quad trip"),
    (4095, 1023, 3, "thread 255 alone misses the four-quad trip; tail of 3"),
    (4096, 0, 0, "exactly one full chunk"),
    (4097, 0, 1, "a second chunk of exactly one element"),
    (4099, 0, 3, "a second chunk that is a tail only"),
    (8191, 1023, 3, "a full chunk, then one short of full"),
    (8192, 0, 0, "two full chunks"),
    (8193, 0, 1, "two full chunks and one element"),
    (3 * 4096 + 3076, 769, 0, "fourth chunk: thread 0 alone takes the four-quad trip"),
]
SIZE_LIST = [s[0] for s in SIZES]


def chunks_of(n):
    return (n + CHUNK - 1) // CHUNK


def four_quad_threads(n4):
    """Threads whose first trip of k_mt_adamw's loop is the four-quad one: i + 3 * THREADS < n4."""
    return [i for i in range(THREADS) if i + (QUADS_PER_TRIP - 1) * THREADS < n4]


def one_quad_trips(n4, thread):
    """Trips thread `thread` makes through the one-quad loop that follows the four-quad one."""
    i = thread
    while i + (QUADS_PER_TRIP - 1) * THREADS < n4:
        i += QUADS_PER_TRIP * THREADS
    return len(range(i, n4, THREADS))


def check_size_premises():
    for n, n4, tail, _ in SIZES:
        assert (n % CHUNK) // 4 == n4 and n % 4 == tail, n
    by = {s[0]: s for s in SIZES}
    assert four_quad_threads(by[3072][1]) == [] and by[3072][1] == 768
    assert four_quad_threads(by[3076][1]) == [0] and four_quad_threads(by[3 * 4096 + 3076][1]) == [0]
    assert four_quad_threads(by[4092][1]) == list(range(255)) == four_quad_threads(by[4095][1])
    assert four_quad_threads(CHUNK // 4) == list(range(THREADS))  # a full chunk: everyone, exactly once
    assert one_quad_trips(CHUNK // 4, 0) == 0 and one_quad_trips(CHUNK // 4, 255) == 0
    assert one_quad_trips(257, 0) == 2 and one_quad_trips(257, 1) == 1 and one_quad_trips(256, 0) == 1
    assert one_quad_trips(255, 255) == 0 and one_quad_trips(255, 254) == 1
    assert 4097 % CHUNK == 1 and chunks_of(4097) == 2 and chunks_of(4096) == 1 and chunks_of(0) == 0
    assert chunks_of(8192) == 2 and chunks_of(8193) == 3 and chunks_of(3 * 4096 + 3076) == 4
    assert len(set(SIZE_LIST)) == len(SIZE_LIST) == 21


# ---------------------------------------------------------------------------------------------------------------- lists
_SMALL = (5, 33, 3, 64, 1, 130, 7, 260)
THREE_CHUNKS = 2 * CHUNK + 5


def _sizes(k):
    """k non-empty tensors; the second one has two chunks, so every later tensor's first chunk sits at a prefix sum that is not
    its index."""
    s = [_SMALL[i % len(_SMALL)] for i in range(k)]
    if k >= 3:
        s[1] = CHUNK + 1
    return s


LISTS = {
    "n1": _sizes(1), "n39": _sizes(39), "n40": _sizes(40), "n41": _sizes(41), "n80": _sizes(80), "n81": _sizes(81),
    "empty_at_0": [0] + _sizes(41),
    "empty_at_39": _sizes(39) + [0] + _sizes(2),
    "empty_at_40": _sizes(40) + [0] + _sizes(1),
    "empty_last": _sizes(41) + [0],
    "empty_after_full_launch": _sizes(40) + [0],
    "three_chunks_last_of_launch": _sizes(39) + [THREE_CHUNKS] + _sizes(1),
    "three_chunks_first_of_next": _sizes(40) + [THREE_CHUNKS],
}
ONLY_EMPTIES = [0, 0, 0]


def launches_of(sizes):
    """The launches the host cuts a list into: lists of list indices, LIST_MAX non-empty tensors each."""
    out, cur = [], []
    for i, n in enumerate(sizes):
        if n > 0:
            cur.append(i)
            if len(cur) == LIST_MAX:
                out.append(cur)
                cur = []
    if cur:
        out.append(cur)
    return out


def check_list_premises():
    count = lambda name: sum(1 for n in LISTS[name] if n > 0)
    assert [count("n%d" % k) for k in (1, 39, 40, 41, 80, 81)] == [1, 39, 40, 41, 80, 81]
    assert [len(launches_of(LISTS["n%d" % k])) for k in (1, 39, 40, 41, 80, 81)] == [1, 1, 1, 2, 2, 3]
    assert [len(l) for l in launches_of(LISTS["n81"])] == [40, 40, 1]
    for name, at in (("empty_at_0", 0), ("empty_at_39", 39), ("empty_at_40", 40)):
        assert LISTS[name][at] == 0 and count(name) == 41 and len(launches_of(LISTS[name])) == 2
    assert launches_of(LISTS["empty_at_39"])[0][-1] == 40  # the empty tensor moves the cut one entry on
    assert launches_of(LISTS["empty_at_40"])[1] == [41]
    assert LISTS["empty_last"][-1] == 0 and len(launches_of(LISTS["empty_last"])) == 2
    assert len(launches_of(LISTS["empty_after_full_launch"])) == 1  # the second pass over the list finds nothing to launch
    assert launches_of(ONLY_EMPTIES) == []
    a, b = LISTS["three_chunks_last_of_launch"], LISTS["three_chunks_first_of_next"]
    assert chunks_of(THREE_CHUNKS) == 3
    assert a[39] == THREE_CHUNKS and launches_of(a)[0][-1] == 39
    assert b[40] == THREE_CHUNKS and launches_of(b)[1][0] == 40
    assert all(any(chunks_of(n) == 2 for n in s[:3]) for s in LISTS.values() if len(s) >= 3)
    assert all(sum(s) < 16384 for s in LISTS.values())


# ---------------------------------------------------------------------------------------------------------------- arenas
GUARD = 8
GUARD_BITS = 0x7FC5A5A5  # a quiet NaN: a guard that is read into an update poisons it
MODES = ("aligned", "p", "g", "m", "v", "all")
ARENAS = "pgmv"


def offsets(mode, arena, count):
    """Start of slice i of arena `arena` ('p', 'g', 'm', 'v') in floats modulo 4 (4 floats = the 16-byte grid of the vector path).
    "aligned": every slice on the grid; "p" / "g" / "m" / "v": that arena alone off it, at 4, 8 and 12 bytes in turn;
    "all": all four arenas, each at another offset; "mix": every third tensor on the grid, the rest off it per arena."""
    k = ARENAS.index(arena)
    if mode == "aligned":
        return [0] * count
    if mode in ARENAS:
        return [1 + i % 3 if mode == arena else 0 for i in range(count)]
    if mode == "all":
        return [(i + 1 + k) % 4 for i in range(count)]
    assert mode == "mix", mode
    return [0 if i % 3 == 0 else (i + k * (1 + i // 4)) % 4 for i in range(count)]


def check_offset_premises():
    n = 12
    for mode in ARENAS:  # that arena alone leaves the grid, and visits 4, 8 and 12 bytes
        for a in ARENAS:
            assert set(offsets(mode, a, n)) == ({1, 2, 3} if a == mode else {0})
    assert all(len({offsets("all", a, n)[i] for a in ARENAS}) == 4 for i in range(n))
    mix = [[offsets("mix", a, 41)[i] for a in ARENAS] for i in range(41)]
    assert any(not any(o) for o in mix[:40]) and any(any(o) for o in mix[:40]) and any(any(o) for o in mix[40:])
    for a in ARENAS:
        assert set(offsets("mix", a, 41)) == {0, 1, 2, 3}


class Arena:
    """All tensors of one kind (p, g, m or v) of a case as slices of ONE buffer: slice i starts `offs[i]` floats past the 16-byte
    grid, at least GUARD floats holding GUARD_BITS lie before, between and after the slices."""

    def __init__(self, sizes, offs, device):
        self.sizes, self.starts, pos = list(sizes), [], 0
        for n, o in zip(sizes, offs):
            pos += GUARD
            pos += (o - pos) % 4
            self.starts.append(pos)
            pos += n
        pos += GUARD
        self.buf = torch.empty(pos, dtype=torch.float32, device=device)
        self.buf.view(torch.int32).fill_(GUARD_BITS)
        assert self.buf.data_ptr() % 16 == 0
        mask = torch.zeros(pos, dtype=torch.bool)
        for s, n in zip(self.starts, sizes):
            mask[s:s + n] = True
        self._guard = (~mask).to(device)

    def view(self, i):
        return self.buf[self.starts[i]:self.starts[i] + self.sizes[i]]

    def ptr(self, i):
        return self.buf.data_ptr() + 4 * self.starts[i]

    def fill(self, arrays):
        for i, a in enumerate(arrays):
            self.view(i).copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
        return self

    def get(self, i):
        return self.view(i).cpu().numpy().copy()

    def all(self):
        return [self.get(i) for i in range(len(self.sizes))]

    def bits(self):
        return self.buf.view(torch.int32).clone()

    def guards_intact(self):
        g = self.buf.view(torch.int32)[self._guard]
        return g.numel() >= GUARD * (len(self.sizes) + 1) and bool((g == GUARD_BITS).all())


def make_arenas(inputs, mode, device):
    """inputs: dict p/g/m/v -> list of fp32 arrays.  Returns dict p/g/m/v -> filled Arena."""
    sizes = [a.size for a in inputs["p"]]
    return {k: Arena(sizes, offsets(mode, k, len(sizes)), device).fill(inputs[k]) for k in ARENAS}


def assert_guards(arenas):
    for k, a in arenas.items():
        assert a.guards_intact(), f"a guard of the {k} arena was overwritten"


# ---------------------------------------------------------------------------------------------------------------- oracle
def make_inputs(sizes, seed, gscale=1.0, zero_state=False):
    """fp32 p, g, m, v (v >= 0) for every size, from one seeded generator."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda n: torch.randn(n, generator=gen).numpy()
    out = dict(p=[], g=[], m=[], v=[])
    for n in sizes:
        out["p"].append(rn(n))
        out["g"].append(rn(n) * np.float32(gscale))
        m, v = rn(n) * np.float32(0.1), (rn(n) * np.float32(0.3)) ** 2
        out["m"].append(np.zeros_like(m) if zero_state else m)
        out["v"].append(np.zeros_like(v) if zero_state else v)
    return out


def norm64(gs):
    return math.sqrt(sum(float((np.asarray(g, dtype=np.float64) ** 2).sum()) for g in gs))


def adamw_restated(p, g, m, v, hp, step, total_norm=None, max_norm=-1.0, write_clipped_grads=1):
    """The single-tensor update in float64 numpy, as the C ABI states it (explicit step count, norm and write flag).
    Returns (p, g as the call leaves it, m, v)."""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    clip = total_norm is not None and max_norm > 0
    gc = g * min(1.0, max_norm / (total_norm + 1e-6)) if clip else g
    (b1, b2), lr = hp["betas"], hp["lr"]
    p = p * (1.0 - lr * hp["weight_decay"])
    m = m + (1.0 - b1) * (gc - m)
    v = b2 * v + (1.0 - b2) * gc * gc
    denom = np.sqrt(v) / math.sqrt(1.0 - b2 ** step) + hp["eps"]
    p = p - lr / (1.0 - b1 ** step) * (m / denom)
    return p, (gc if clip and write_clipped_grads else g), m, v


def kernel_emulation_f32(p, g, m, v, hp, step, coef=1.0, lerp_switch=True):
    """adamw_one of optim.hip in fp32 numpy (without the device's fused multiply-adds): scalars in double on the host, rounded
    once; with `lerp_switch` the first moment leaves from g once 1 - beta1 reaches 0.5, as Tensor.lerp_ does."""
    f = np.float32
    p, g, m, v = (np.asarray(x, dtype=f) for x in (p, g, m, v))
    (b1, b2), lr = hp["betas"], hp["lr"]
    omb1, omb2, beta2, eps = f(1.0 - b1), f(1.0 - b2), f(b2), f(hp["eps"])
    decay, step_size, bc2 = f(1.0 - lr * hp["weight_decay"]), f(lr / (1.0 - b1 ** step)), f(math.sqrt(1.0 - b2 ** step))
    g = g * f(coef)
    p = p * decay
    m = g - (g - m) * (f(1.0) - omb1) if lerp_switch and omb1 >= f(0.5) else m + omb1 * (g - m)
    v = beta2 * v + omb2 * (g * g)
    p = p - step_size * (m / (np.sqrt(v) / bc2 + eps))
    return p, g, m, v


def clip_coef_f32(total_norm, max_norm):
    f = np.float32
    return min(f(1.0), f(max_norm) / (f(total_norm) + f(1e-6)))


def torch_step(inputs, hp, step, dtype, max_norm=None, steps=None):
    """torch's own path on CPU copies of the fp32 inputs in `dtype`: clip_grad_norm_ (max_norm not None), then one step of
    torch.optim.AdamW(foreach=False, fused=False) from the state (step - 1, m, v).  `steps`: a count per tensor instead.
    Returns dict p/g/m/v -> list of arrays, and "norm"."""
    ps = [torch.tensor(np.asarray(a), dtype=dtype).requires_grad_(True) for a in inputs["p"]]
    opt = torch.optim.AdamW(ps, foreach=False, fused=False, **hp)
    for i, p in enumerate(ps):
        p.grad = torch.tensor(np.asarray(inputs["g"][i]), dtype=dtype)
        opt.state[p] = dict(step=torch.tensor(float((steps[i] if steps else step) - 1)),
                            exp_avg=torch.tensor(np.asarray(inputs["m"][i]), dtype=dtype),
                            exp_avg_sq=torch.tensor(np.asarray(inputs["v"][i]), dtype=dtype))
    norm = float(torch.nn.utils.clip_grad_norm_(ps, max_norm)) if max_norm is not None else None
    opt.step()
    return dict(p=[p.detach().numpy() for p in ps], g=[p.grad.numpy() for p in ps],
                m=[opt.state[p]["exp_avg"].numpy() for p in ps], v=[opt.state[p]["exp_avg_sq"].numpy() for p in ps], norm=norm)


GRAD_SCALES = (3.0, 0.2, 3.0)  # three steps, gradient scale alternating
HYPER_SIZES = (1, 7, 1028, 3076, CHUNK + 1)
HYPERS = {
    "reference betas": dict(lr=LR, betas=(0.95, 0.9999), eps=1e-8, weight_decay=0.01),
    "torch defaults lr 3e-4 wd 0.1": dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1),
    "beta1 0.3": dict(lr=LR, betas=(0.3, 0.999), eps=1e-8, weight_decay=0.01),
    "beta1 0": dict(lr=LR, betas=(0.0, 0.999), eps=1e-8, weight_decay=0.01),
    "beta2 0": dict(lr=LR, betas=(0.9, 0.0), eps=1e-8, weight_decay=0.01),
    "beta1 0.3 beta2 0": dict(lr=LR, betas=(0.3, 0.0), eps=1e-8, weight_decay=0.01),
    "beta1 0 beta2 0": dict(lr=LR, betas=(0.0, 0.0), eps=1e-8, weight_decay=0.01),
    "wd 0": dict(lr=LR, betas=(0.95, 0.9999), eps=1e-8, weight_decay=0.0),
    "eps 1": dict(lr=LR, betas=(0.95, 0.9999), eps=1.0, weight_decay=0.01),
    "lr 0 wd 0": dict(lr=0.0, betas=(0.95, 0.9999), eps=1e-8, weight_decay=0.0),
}
LATE_STEP = 10 ** 6  # the reference betas again, through the ABI with an explicit count


def hyper_run_inputs(seed=11):
    """Start parameters and the three gradient sets of a hyper-parameter run."""
    p0 = make_inputs(HYPER_SIZES, seed)["p"]
    grads = [make_inputs(HYPER_SIZES, seed + 1 + k, gscale=s)["g"] for k, s in enumerate(GRAD_SCALES)]
    return p0, grads


def torch_run(p0, grads, groups, dtype, max_norm=None):
    """Len(grads) steps of clip_grad_norm_ (over all groups) + AdamW on the CPU in `dtype`.  groups: list of (indices, hp).
    Returns dict p/m/v -> list of arrays in tensor order, "g": the gradients as the last step leaves them, "norm": the last norm."""
    ps = [torch.tensor(np.asarray(a), dtype=dtype).requires_grad_(True) for a in p0]
    opt = torch.optim.AdamW([dict(params=[ps[i] for i in idx], **hp) for idx, hp in groups], foreach=False, fused=False)
    norm = None
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.tensor(np.asarray(g), dtype=dtype)
        if max_norm is not None:
            norm = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
        opt.step()
    return dict(p=[p.detach().numpy() for p in ps], g=[p.grad.numpy() for p in ps],
                m=[opt.state[p]["exp_avg"].numpy() for p in ps], v=[opt.state[p]["exp_avg_sq"].numpy() for p in ps], norm=norm)


def emulation_run(p0, grads, hp, max_norm=None, lerp_switch=True):
    """The kernel's formula in fp32 numpy over the same steps (the norm in float64, rounded once, as k_mt_norm_final leaves it)."""
    p = [np.asarray(a, dtype=np.float32) for a in p0]
    m, v = [np.zeros_like(a) for a in p], [np.zeros_like(a) for a in p]
    for k, gs in enumerate(grads):
        coef = clip_coef_f32(norm64(gs), max_norm) if max_norm is not None else 1.0
        for i, g in enumerate(gs):
            p[i], _, m[i], v[i] = kernel_emulation_f32(p[i], g, m[i], v[i], hp, k + 1, coef, lerp_switch)
    return dict(p=p, m=m, v=v)


# ---------------------------------------------------------------------------------------------------------------- measure
def rel_err(got, ref):
    """max |got - ref| relative to ref's largest entry (ref float64); an identically zero (or empty) ref demands exact zeros."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), "non-finite values"
    m = np.abs(ref).max() if ref.size else 0.0
    if m == 0.0:
        return 0.0 if not np.any(got) else float("inf")
    return float(np.abs(got - ref).max() / m)


def worst(got, ref, key):
    return max([rel_err(a, b) for a, b in zip(got[key], ref[key])], default=0.0)


def bars(ref64, got32):
    """The case's bar for each of p, m, v from torch's fp32 CPU path `got32` against float64 `ref64`."""
    return {k: MARGIN * max(worst(got32, ref64, k), FLOOR) for k in "pmv"}


def check(tag, got, ref64, bar, keys="pmv"):
    """Every tensor of got[k] within bar[k] of ref64[k]; the worst ratio of each k goes to stdout and, with
    RNNT_OPTIM_PARITY_OUT=<file> set, to that file (profiles/optim_parity.txt is such a run)."""
    lines, fails, top = [], [], 0.0
    for k in keys:
        errs = [rel_err(a, b) for a, b in zip(got[k], ref64[k])]
        e = max(errs, default=0.0)
        top = max(top, e / bar[k])
        lines.append(f"{tag:64s} {k}  err {e:.3e}  bar {bar[k]:.3e}  ratio {e / bar[k]:.3f}")
        if not e <= bar[k]:
            fails.append(f"{k}: tensor {int(np.argmax(errs))} of {len(errs)} err {e:.3e} > bar {bar[k]:.3e}")
    print("\n".join(lines))
    path = os.environ.get("RNNT_OPTIM_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")
    assert not fails, f"{tag}: " + "; ".join(fails)
    return top
