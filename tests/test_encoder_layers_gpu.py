"""GPU tests of the encoder's kernels layer by layer (rnnt_amd/csrc/encoder.hip through the C ABI rnnt_engine_encoder_*) against the
float64 oracle of tests/encoder_layer_cases.py, at the tile, chunk, quad, tap-range, slab and state-block edges that module states
and asserts.  The bar of every comparison is ec.bar: 4 x max(the torch composition's own fp32 error against float64, one rounding of
the conv sum carried through the norm plus one of the result); a new state is a copy and is held bit for bit.  Every comparison
prints `case, engine error, e_ref, bar` (profiles/encoder_layer_parity.txt holds a run's).

The helper owns every buffer: the workspace has exactly the bytes rnnt_engine_encoder_workspace_bytes reports, `out`, every new state
and the workspace are pre-filled (signalling NaNs unless a test says otherwise) and followed by 64 guard words that must survive; so is
the packed buffer.  Beside the results abi_run hands back the workspace and the packed tables as the call left them and the sizes
the queries gave (tests/golden/make_golden_encoder_bits.py pins their bytes)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import encoder_layer_cases as ec

pytestmark = pytest.mark.gpu
GUARD, GUARD_WORDS = 0x5AA5C33C, 64
SNAN, QNAN = 0x7FA00000, 0xFFFFFFFF


def _buffer(nwords, fill, dev):
    """nwords 32-bit words of `fill` with GUARD_WORDS guard words behind them."""
    t = torch.full((nwords + GUARD_WORDS,), fill - (1 << 32) if fill >= (1 << 31) else fill, dtype=torch.int32, device=dev)
    t[nwords:] = GUARD
    return t


def _place(x, layout, dev):
    """x (N, C, L) on the device in `layout`; what lies between the frames is NaN (nothing may read it)."""
    N, C, L = x.shape
    t = torch.from_numpy(x)
    if layout == "ncl":
        return t.to(dev).contiguous()
    if layout == "slice":  # a time slice of a longer tensor: batch stride != C * L
        big = torch.full((N, C, L + 5), float("nan"))
        big[:, :, 2:2 + L] = t
        return big.to(dev)[:, :, 2:2 + L]
    ld = C if layout == "tm_tight" else ec.pad4(C)   # time-major rows of ld floats ...
    off = 1 if layout == "tm_offset" else 0           # ... from a base 16-byte aligned, or one float behind it
    flat = torch.full((off + N * L * ld,), float("nan"))
    flat[off:].view(N, L, ld)[:, :, :C] = t.permute(0, 2, 1)
    v = flat.to(dev)[off:].view(N, L, ld)[:, :, :C].permute(0, 2, 1)
    vec = v.stride(1) == 1 and v.stride(0) % 4 == 0 and v.stride(2) % 4 == 0 and v.data_ptr() % 16 == 0  # run()'s test
    assert vec == (layout == "tm_pad") and v.stride() == (L * ld, 1, ld)
    return v


def abi_run(case, regime, fill=SNAN):
    """packed_bytes -> pack -> workspace_bytes -> fwd (whole utterance) or stream_push (case.states) on buffers of its own.
    Returns out (N, L_out, cout) and the new states (None where the list carries none), on the device."""
    from rnnt_amd import engine
    from rnnt_amd.encoder import _Layer
    lib = engine.lib()
    dev = torch.device("cuda", 0)
    nl, N, L = len(case.layers), case.N, case.L
    P = ec.case_plan(case, regime)
    keep, arr = [], (_Layer * nl)()

    def ptr(a):
        if a is None:
            return None
        keep.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        return keep[-1].data_ptr()

    for d, l in zip(arr, case.layers):
        d.cin, d.cout, d.taps, d.stride, d.dilation, d.norm, d.role, d.eps = l.cin, l.cout, l.taps, l.stride, l.dil, l.norm, l.role, l.eps
        d.weight, d.bias, d.gamma, d.beta, d.mean, d.var = ptr(l.W), ptr(l.b), ptr(l.gamma), ptr(l.beta), ptr(l.mean), ptr(l.var)
    x = _place(case.x, case.layout, dev)
    strides = (ctypes.c_int64 * 3)(*x.stride())
    n_out = N * P.L_final * case.cout
    with torch.cuda.device(dev):
        n = ctypes.c_size_t(0)
        engine._check(lib.rnnt_engine_encoder_packed_bytes(arr, nl, ctypes.byref(n)))
        n_packed = n.value
        packed = _buffer(n_packed // 4, fill, dev)
        engine._check(lib.rnnt_engine_encoder_pack(arr, nl, engine._p(packed), ctypes.c_size_t(n_packed), engine._stream(dev)))
        lens_in = None if case.states is None else (ctypes.c_int32 * nl)(*case.state_lens)
        engine._check(lib.rnnt_engine_encoder_workspace_bytes(arr, nl, N, L, regime, lens_in, ctypes.byref(n)))
        assert n.value == P.ws_bytes and n.value % 4 == 0
        ws, out = _buffer(n.value // 4, fill, dev), _buffer(n_out, fill, dev)
        new = []
        if case.states is None:
            engine._check(lib.rnnt_engine_encoder_fwd(arr, nl, engine._p(packed), engine._p(x), strides, N, L, regime, engine._p(out),
                                                      engine._p(ws), ctypes.c_size_t(n.value), engine._stream(dev)))
        else:
            lens_out = (ctypes.c_int32 * nl)(*[r.slen_out for r in P.rows])
            ptr_in, ptr_out = (ctypes.c_void_p * nl)(), (ctypes.c_void_p * nl)()
            for i, (l, r) in enumerate(zip(case.layers, P.rows)):
                new.append(_buffer(r.state_values, fill, dev) if r.state_values else None)
                ptr_in[i] = ptr(case.states[i]) if r.slen else None
                ptr_out[i] = new[i].data_ptr() if r.state_values else None
            engine._check(lib.rnnt_engine_encoder_stream_push(arr, nl, engine._p(packed), engine._p(x), strides, N, L, ptr_in, lens_in,
                                                              ptr_out, lens_out, regime, engine._p(out), engine._p(ws),
                                                              ctypes.c_size_t(n.value), engine._stream(dev)))
    torch.cuda.synchronize()
    for what, t, words in [("out", out, n_out), ("workspace", ws, n.value // 4), ("packed", packed, n_packed // 4)] + [
            (f"state_out {i}", t, P.rows[i].state_values) for i, t in enumerate(new) if t is not None]:
        assert bool((t[words:] == GUARD).all()), f"{case.name}: the guard words behind {what} were written"
    states = [None if t is None else t[:r.state_values].view(torch.float32).view(N, l.cin, r.slen_out)
              for t, l, r in zip(new, case.layers, P.rows)]
    return SimpleNamespace(out=out[:n_out].view(torch.float32).view(N, P.L_final, case.cout), states=states or None, plan=P,
                           workspace=ws[:n.value // 4], packed=packed[:n_packed // 4],
                           sizes=dict(packed_bytes=n_packed, workspace_bytes=n.value))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(case, want, bars, got, regime, label=None):
    """out within the bar (printed first), every new state of the list's input bit-equal to the oracle's X~ tail."""
    b, e_ref, e_round = bars
    y = got.out.cpu().numpy().astype(np.float64)
    assert y.shape == want.out.shape
    err = float(np.abs(y - want.out).max()) if np.isfinite(y).all() else float("inf")
    kernels = "+".join("few" if r.few else "mfma" for r in got.plan.rows)
    print(f"encoder layer parity {label or case.name} [{case.norm}, {case.layout}, {ec.REGIME_NAMES[regime]}: {kernels}]: "
          f"engine max|y - fp64| = {err:.3e}, e_ref = {e_ref:.3e}, e_round = {e_round:.3e}, bar = {b:.3e}, err/bar = {err / b:.2f}")
    assert err <= b, (case.name, case.norm, case.layout, regime, err, b)
    if got.states is not None:
        for i, (s, w) in enumerate(zip(got.states, want.states)):
            assert (s is None) == (w is None or w.shape[2] == 0)
            if s is None:
                continue
            assert tuple(s.shape) == w.shape
            if ec.reads_input(case, i):  # a copy of fp32 frames the caller handed over: bit for bit
                assert torch.equal(_bits(s.cpu()), _bits(torch.from_numpy(w.astype(np.float32)))), (case.name, i)
            else:  # a copy of an activation the engine computed: test_streaming_chain holds its bits to the first layer run alone
                assert torch.isfinite(s).all()


PARITY = [(cid, r) for cid in ec.case_ids(layouts_too=True) for r in ec.SHAPES[cid[0]][4]]


@pytest.mark.parametrize("cid,regime", PARITY, ids=["-".join(c) + "-" + ec.REGIME_NAMES[r] for c, r in PARITY])
def test_layer_meets_the_float64_oracle(cid, regime):
    case, want, bars = ec.prepared(*cid)
    _check(case, want, bars, abi_run(case, regime), regime)


@pytest.mark.parametrize("regime", (ec.AUTO, ec.MANY_ROWS), ids=lambda r: ec.REGIME_NAMES[r])
@pytest.mark.parametrize("name,kind", [("few_c201_o70/streamed", "instance_offset"), ("mfma_c201_o130_s2/streamed", "instance"),
                                       ("list_13ch/streamed", "batch"), ("block_three_sub/final", "instance")])
def test_workspace_out_and_states_are_scratch_and_nothing_is_written_beyond_them(name, kind, regime):
    """Zeros, signalling NaNs or quiet NaNs beforehand in the workspace, `out` and every state_out change no bit of `out` or of a
    state; the results are finite and meet the oracle; the guard words behind every buffer survive (abi_run asserts that)."""
    case, want, bars = ec.prepared(name, kind)
    runs = [abi_run(case, regime, fill) for fill in (0, SNAN, QNAN)]
    for r in runs[1:]:
        assert torch.equal(_bits(r.out), _bits(runs[0].out))
        for a, b in zip(r.states or [], runs[0].states or []):
            assert (a is None) == (b is None) and (a is None or torch.equal(_bits(a), _bits(b)))
    assert torch.isfinite(runs[0].out).all() and all(s is None or torch.isfinite(s).all() for s in runs[0].states or [])
    _check(case, want, bars, runs[0], regime)


@pytest.mark.parametrize("name,kind,regime", [("few_epilogue", "instance_offset", ec.AUTO), ("few_epilogue", "batch", ec.AUTO),
                                              ("mfma_c201_o130_s2/streamed", "instance", ec.MANY_ROWS)])
def test_identical_calls_give_identical_bits(name, kind, regime):
    case, _, _ = ec.prepared(name, kind)
    a, b = abi_run(case, regime), abi_run(case, regime)
    assert torch.equal(_bits(a.out), _bits(b.out)) and all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a.states, b.states))
    assert a.plan.rows[0].nsplit == (261 if name == "few_epilogue" else 8)


@pytest.mark.parametrize("regime", (ec.AUTO, ec.MANY_ROWS), ids=lambda r: ec.REGIME_NAMES[r])
def test_a_list_without_final_writes_out(regime):
    """[PLAIN] alone leaves its result in `out` (rows of cout floats, the NaNs it was filled with gone); [PLAIN, FINAL] computes what it
    did: the oracle within the bar, and bit for bit the FINAL layer alone on what [PLAIN] alone left in `out`."""
    both, want, bars = ec.prepared("plain_final", "batch")
    first = ec.make_case("plain_final/first", both.layers[:1], both.N, both.x, None, norm="batch")
    got1 = abi_run(first, regime, fill=SNAN)
    assert torch.isfinite(got1.out).all() and got1.out.shape == (both.N, got1.plan.L_final, 13)
    _check(first, ec.oracle(first), ec.bar(first), got1, regime)
    got = abi_run(both, regime)
    _check(both, want, bars, got, regime)
    mid = np.ascontiguousarray(got1.out.cpu().numpy().transpose(0, 2, 1))
    for layout in ("ncl", "tm_tight"):  # (rows of 13 floats: the scalar gather, where the list's own activation has rows of 16)
        second = ec.make_case("plain_final/second", both.layers[1:], both.N, mid, None, layout=layout)
        assert torch.equal(_bits(abi_run(second, regime).out), _bits(got.out)), layout


@pytest.mark.parametrize("regime", (ec.AUTO, ec.MANY_ROWS), ids=lambda r: ec.REGIME_NAMES[r])
@pytest.mark.parametrize("norm", ("none", "batch"))
@pytest.mark.parametrize("name", ec.CHAIN_CASES)
def test_streaming_chain(name, norm, regime):
    """Pushes of CHAIN_CHUNKS from zero state: the concatenated outputs meet the whole utterance's float64 oracle within its bar;
    after every push each state has the length the arithmetic gives and is, bit for bit, the tail of X~ — the state before the push
    followed by the layer's input, which for a second layer is what the first layer alone leaves in `out` for the same push."""
    whole, states, push = ec.chain(name, norm)
    want = ec.oracle(whole)
    bars = ec.bar(whole, want)
    outs = []
    for k in range(len(ec.CHAIN_CHUNKS)):
        case = push(states, k)
        got = abi_run(case, regime)
        inputs = [torch.from_numpy(case.x)]
        if len(case.layers) == 2:
            alone = abi_run(ec.make_case(case.name + "/first", case.layers[:1], case.N, case.x, states[:1], norm=norm), regime)
            assert torch.equal(_bits(alone.states[0]), _bits(got.states[0]))
            inputs.append(alone.out.cpu().permute(0, 2, 1))
        new = []
        for i, (l, r) in enumerate(zip(case.layers, got.plan.rows)):
            xt = torch.cat([torch.from_numpy(states[i]), inputs[i]], dim=2)
            assert r.slen_out == xt.shape[2] - r.Lout * l.stride and tuple(got.states[i].shape) == (case.N, l.cin, r.slen_out)
            assert torch.equal(_bits(got.states[i].cpu()), _bits(xt[:, :, r.Lout * l.stride:])), (k, i)
            new.append(got.states[i].cpu().numpy())
        states = new
        outs.append(got.out)
    got.out = torch.cat(outs, dim=1)
    got.states = None
    _check(whole, want, bars, got, regime, label=f"{name} streamed {list(ec.CHAIN_CHUNKS)}")


def test_run_entries_refuse_instance_norm_over_one_frame():
    """Refused by both run entries before anything is enqueued: `out` and the new state keep what they held."""
    from rnnt_amd import engine
    from rnnt_amd.encoder import _Layer
    lib, dev = engine.lib(), torch.device("cuda", 0)
    case = ec.build("few_c68_s2", "instance")  # 3 taps, stride 2: 3 frames of state + input leave one output frame
    l, N = case.layers[0], case.N
    W, b, g, be, x, st = (torch.from_numpy(a).to(dev) for a in (l.W, l.b, l.gamma, l.beta, case.x, case.states[0]))
    arr = (_Layer * 1)()
    d = arr[0]
    d.cin, d.cout, d.taps, d.stride, d.dilation, d.norm, d.role, d.eps = l.cin, l.cout, l.taps, l.stride, l.dil, l.norm, l.role, l.eps
    d.weight, d.bias, d.gamma, d.beta = W.data_ptr(), b.data_ptr(), g.data_ptr(), be.data_ptr()
    n = ctypes.c_size_t(0)
    with torch.cuda.device(dev):
        engine._check(lib.rnnt_engine_encoder_packed_bytes(arr, 1, ctypes.byref(n)))
        packed = torch.empty(n.value, dtype=torch.uint8, device=dev)
        engine._check(lib.rnnt_engine_encoder_pack(arr, 1, engine._p(packed), ctypes.c_size_t(n.value), engine._stream(dev)))
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
        out, new = _buffer(N * l.cout, SNAN, dev), _buffer(N * l.cin, SNAN, dev)
        strides = (ctypes.c_int64 * 3)(*x.stride())
        args = (engine._p(out), engine._p(ws), ctypes.c_size_t(ws.numel()), engine._stream(dev))
        assert lib.rnnt_engine_encoder_fwd(arr, 1, engine._p(packed), engine._p(x), strides, N, 2, ec.AUTO, *args) == -1  # 1 zero + 2
        assert "instance norm" in lib.rnnt_engine_last_error().decode()
        lens_in, lens_out = (ctypes.c_int32 * 1)(2), (ctypes.c_int32 * 1)(1)
        ptr_in, ptr_out = (ctypes.c_void_p * 1)(st.data_ptr()), (ctypes.c_void_p * 1)(new.data_ptr())
        for regime in (ec.AUTO, ec.MANY_ROWS):
            assert lib.rnnt_engine_encoder_stream_push(arr, 1, engine._p(packed), engine._p(x), strides, N, 1, ptr_in, lens_in, ptr_out,
                                                       lens_out, regime, *args) == -1  # 2 of state + 1
            assert "instance norm" in lib.rnnt_engine_last_error().decode()
        lens_in[0], lens_out[0] = 2, 2  # one frame more: two output frames, accepted
        engine._check(lib.rnnt_engine_encoder_workspace_bytes(arr, 1, N, 3, ec.AUTO, lens_in, ctypes.byref(n)))
    torch.cuda.synchronize()
    assert bool((out[:N * l.cout] == SNAN).all()) and bool((new[:N * l.cin] == SNAN).all())
