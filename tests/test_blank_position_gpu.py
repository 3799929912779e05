"""-m gpu: every loss, alignment and regulariser kernel at a blank other than V - 1.

`blank` is an argument of every loss entry of the C ABI and of rnnt_loss / joint_rnnt_loss / rnnt_align / joint_rnnt_align, and
each route has its own position-dependent code for it: the G producers subtract the blank's coefficient in ONE element of one
4- / 8- / 16- / 32-wide group of one 128-wide chunk (x2.hip, x3.hip, bf16.hip, joint_bwd.hip gen() / k_dhidden_gen / k_make_g),
the forward epilogues gather logit[blank] (joint_fwd.hip, x2.hip, x3.hip, bf16.hip), lattice.hip gathers and corrects it on
materialised logits.  With the blank last, as every other GPU test has it, that fix-up only ever runs in the last group at the
last element, never shares a vector with a label above it, and no label is the last real column beside the host's padding.

Here the problems of tests/helpers.make_inputs are relabelled (tests/helpers.relabel_blank: the blank's row of W / bias moves to
`blank`, the targets move with it; utterance 0's first two labels are forced to blank - 1 and blank + 1) and every entry is held
to its EXISTING bar against the float64 oracle evaluated at that blank (tests/test_blank_position_oracle.py pins the oracles'
side on the CPU).  A sweep reports all failing positions at once."""
import functools

import numpy as np
import pytest
import torch

from oracle import cpu_oracle
from tests import align_oracle as ao
from tests import latency_reg_oracle as lro
from tests.helpers import (BF16_GRAD_RTOL, BF16_LOSS_RTOL, BF16_LOSS_RTOL_EXACT, GRAD_RTOL, LOSS_RTOL, assert_close_grad,
                           assert_close_loss, has_live_label, make_inputs, oracle_fused, oracle_fused_bf16, relabel_blank)

pytestmark = pytest.mark.gpu

ROUTES = ("fp32", "bf16x3", "f16x2", "bf16")
FP32_BAR_ROUTES = ("fp32", "bf16x3", "f16x2")
GRADS = ("grad_enc", "grad_pred", "grad_W", "grad_bias")
SWEEP_SHAPE = (2, 9, 4, 128, 128)  # the smallest shape the split routes take without padding


@pytest.fixture(scope="module")
def amd():
    import rnnt_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    rnnt_amd.engine.lib()  # fail loudly if the HIP extension is missing
    return rnnt_amd


def _dev(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _base(shape):
    return make_inputs(*shape, seed=sum(shape))


@functools.lru_cache(maxsize=None)
def _problem(shape, blank):
    """make_inputs(*shape) with the blank at `blank` and labels on both sides of it (shared, read-only)."""
    return relabel_blank(_base(shape), blank, neighbours=True)[0]


@functools.lru_cache(maxsize=None)
def _reference(shape, blank, bf16=False):
    """The float64 oracle (bf16: the rounding-point oracle) of _problem(shape, blank), computed once for all routes and tests."""
    return (oracle_fused_bf16 if bf16 else oracle_fused)(_problem(shape, blank), blank=blank)


def _positions(V, wanted=(0, 3, 4, 7, 8, 15, 16, 31, 32, 127, 128)):
    return sorted({b for b in wanted if b < V} | {V - 2})


def _signed(b, V):
    """Odd positions are passed as negative indices (blank = b - V), even ones as they are."""
    return b - V if b % 2 else b


def _run_fused(amd, d, route, blank, **kw):
    g = _dev(d)
    leaves = [g[k].requires_grad_(True) for k in ("enc", "pred", "W", "bias")]
    loss, costs = amd.joint_rnnt_loss(*leaves, g["targets"], g["logit_lens"], g["target_lens"], blank=blank, reduction="mean",
                                      return_costs=True, dtype=route, **kw)
    loss.backward()
    torch.cuda.synchronize()
    out = dict(loss=loss.item(), costs=costs.cpu().numpy())
    for k, t in zip(GRADS, leaves):
        out[k] = t.grad.cpu().numpy()
    return out


def _compare(r, ref, bf16=False):
    lt, gt = (BF16_LOSS_RTOL, BF16_GRAD_RTOL) if bf16 else (LOSS_RTOL, GRAD_RTOL)
    if "loss" in r:
        assert_close_loss("loss", r["loss"], ref["loss"], rtol=lt)
    assert_close_loss("costs", r["costs"], ref["costs"], rtol=lt)
    for k in GRADS:
        assert_close_grad(k, r[k], ref[k], rtol=gt)


def _mismatch(r, ref, bf16=False):
    """None, or what _compare has to say: the sweeps go on to the next position and report every failing one."""
    try:
        _compare(r, ref, bf16)
    except AssertionError as e:
        return str(e)
    return None


def _assert_none_failed(failed, what, n):
    assert not failed, "%s: %d of %d blank positions fail: %s" % (
        what, len(failed), n, "; ".join("blank=%s: %s" % kv for kv in sorted(failed.items())))


def _engine_run(amd, d, blank, dtype, variant=0):
    g = _dev(d)
    outs = amd.engine.joint_loss_fwd_bwd(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"],
                                         blank, 1.0 / d["enc"].shape[0], dtype=dtype, variant=variant)
    torch.cuda.synchronize()
    return [o.clone() for o in outs]


def _as_result(outs):
    return dict(zip(("costs",) + GRADS, (o.cpu().numpy() for o in outs)))


# ---- a. every position of a 128-wide vocabulary, per route -------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_every_blank_position(amd, route):
    """(B,T,U,H,V) = (2,9,4,128,128), ragged, blank = 0 .. 127 through joint_rnnt_loss: loss, costs and the four gradients against
    the oracle at that blank.  128 positions visit every element of every 4-, 8-, 16-, 32- and 128-wide grouping a kernel may
    use, whatever it is; the forced labels blank - 1 / blank + 1 put a label fix-up on either side of the blank's in the same
    vector, and at blank = 126 the label 127 is the last column."""
    V = SWEEP_SHAPE[-1]
    bf16 = route == "bf16"
    failed, last_label = {}, False
    for b in range(V):
        d = _problem(SWEEP_SHAPE, b)
        assert not has_live_label(d, b)
        assert (b == 0 or d["targets"][0, 0] == b - 1) and (b == V - 1 or d["targets"][0, 1] == b + 1)
        last_label |= b < V - 1 and has_live_label(d, V - 1)
        msg = _mismatch(_run_fused(amd, d, route, _signed(b, V)), _reference(SWEEP_SHAPE, b, bf16), bf16)
        if msg:
            failed[b] = msg
    assert last_label  # the label V - 1 occurred with the blank below it
    _assert_none_failed(failed, route, V)


# ---- b. the shapes at which the kernels take another path --------------------------------------------------------------------
PATH_SHAPES = [
    (3, 23, 19, 36, 132),   # the host pads H and V to 128 / 256: blank at 127, 128 and 130, the label 131 beside the padding
    (2, 13, 6, 640, 256),   # H > 512: k_make_g + k_dhidden, the generator's blank chunk
    (3, 21, 18, 1024, 64),  # whole 512-groups reading G's planes
    (2, 9, 4, 516, 96),     # the H % 512 rest, V padded
]
# the bf16 route takes H % 128 == 0 and V % 128 == 0 only: the one such shape above and test_bf16_fused_vs_rounding_point_oracle's
# H = 1024 shape (one more k_dhidden_bf16 launch per further 512 columns)
BF16_PATH_SHAPES = [(2, 13, 6, 640, 256), (2, 13, 20, 1024, 256)]


@pytest.mark.parametrize("shape", PATH_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("route", FP32_BAR_ROUTES)
def test_kernel_path_shapes(amd, route, shape):
    V = shape[-1]
    pos = _positions(V)
    failed, last_label = {}, False
    for b in pos:
        d = _problem(shape, b)
        last_label |= b < V - 1 and has_live_label(d, V - 1)
        msg = _mismatch(_run_fused(amd, d, route, _signed(b, V)), _reference(shape, b))
        if msg:
            failed[b] = msg
    assert last_label
    _assert_none_failed(failed, "%s %s" % (route, shape), len(pos))


@pytest.mark.parametrize("shape", BF16_PATH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_path_shapes_bf16(amd, shape):
    V = shape[-1]
    pos = _positions(V)
    failed, last_label = {}, False
    for b in pos:
        d = _problem(shape, b)
        last_label |= b < V - 1 and has_live_label(d, V - 1)
        msg = _mismatch(_run_fused(amd, d, "bf16", _signed(b, V)), _reference(shape, b, True), True)
        if msg:
            failed[b] = msg
    assert last_label
    _assert_none_failed(failed, "bf16 %s" % (shape,), len(pos))


# ---- c. per-call kernel variants (rnnt_engine_run_stages) --------------------------------------------------------------------
VARIANT_SHAPES = [(2, 13, 20, 1024, 256), (2, 9, 4, 128, 128)]


def _variant_blanks(V):
    return (0, 5, 12, V - 2)


OUTPUTS = ("costs",) + GRADS


def _variant_differences(amd, shape, names, outputs):
    """{(blank, variant): which of `outputs` are not bit-identical to the default fp32 kernels' and by how much}; the default
    kernels' own results are held to the oracle on the way."""
    failed = {}
    for b in _variant_blanks(shape[-1]):
        d = _problem(shape, b)
        ref = _engine_run(amd, d, b, "fp32")
        msg = _mismatch(_as_result(ref), _reference(shape, b))
        if msg:
            failed[(b, "default")] = msg
        for name in names:
            got = _engine_run(amd, d, b, "fp32", variant=getattr(amd.engine, name))
            bad = ["%s (max |diff| %.3e)" % (k, float((x - y).abs().max()))
                   for k, x, y in zip(OUTPUTS, got, ref) if k in outputs and not torch.equal(x, y)]
            if bad:
                failed[(b, name)] = "differs from the default kernels in " + ", ".join(bad)
            msg = _mismatch(_as_result(got), _reference(shape, b))
            if msg:
                failed[(b, name + " vs oracle")] = msg
    return failed


@pytest.mark.parametrize("shape", VARIANT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp32_stage_variants_agree_bitwise(amd, shape):
    """include/rnnt_engine.h: every RNNT_VARIANT_* of the exact-fp32 route multiplies the same numbers in the same order as the
    default kernels — at every blank, all five outputs bit for bit.  VARIANT_SEPARATE_G replaces the producer that makes G inside
    dHidden (gen(), k_dhidden_gen's main loop) by k_make_g, each with its own blank test; the tile kernel then reads that G and
    sums in the default order.  (Until this test the variant ran the persistent k_dhidden behind k_make_g, whose other summation
    order left grad_enc / grad_pred 1.2e-8 .. 2.2e-8 away from the default kernels' at every blank, V - 1 included.)"""
    failed = _variant_differences(amd, shape, ("VARIANT_SEPARATE_G", "VARIANT_SEPARATE_HIDDEN", "VARIANT_FWD_LDS_RING",
                                               "VARIANT_FWD_ONE_WG_PER_TILE"), OUTPUTS)
    _assert_none_failed(failed, "fp32 %s" % (shape,), 4)


@pytest.mark.parametrize("shape", VARIANT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("variant", ["dw_only", "dw_dhidden"])
@pytest.mark.parametrize("route", ["bf16x3", "f16x2"])
def test_split_route_kernels_in_isolation(amd, route, variant, shape):
    """RNNT_VARIANT_X3_FP32_FWD (| _DH) on the bf16x3 and f16x2 routes, as test_x3_kernels_in_isolation /
    test_x2_kernels_in_isolation run them: the forward (and dHidden + G) on the exact-fp32 kernels, the plain splitting kernels in
    between, the route's own dHidden / dW behind them — against the oracle."""
    E = amd.engine
    var = {"dw_only": E.VARIANT_X3_FP32_FWD | E.VARIANT_X3_FP32_DH, "dw_dhidden": E.VARIANT_X3_FP32_FWD}[variant]
    V = shape[-1]
    failed = {}
    for b in _variant_blanks(V):
        msg = _mismatch(_as_result(_engine_run(amd, _problem(shape, b), b, route, variant=var)), _reference(shape, b))
        if msg:
            failed[b] = msg
    _assert_none_failed(failed, "%s %s %s" % (route, variant, shape), 4)


@pytest.mark.parametrize("shape", VARIANT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_f16x2_flush_skip_is_exact_at_every_blank(amd, shape):
    """f16x2 with and without RNNT_VARIANT_X2_NO_FLUSH_SKIP: costs, grad_enc and grad_pred bit for bit (grad_W / grad_bias differ
    in summation order only, tests/test_x2_flush_skip_gpu.py)."""
    E = amd.engine
    V = shape[-1]
    failed = {}
    for b in _variant_blanks(V):
        d = _problem(shape, b)
        new, ref = _engine_run(amd, d, b, "f16x2"), _engine_run(amd, d, b, "f16x2", variant=E.VARIANT_X2_NO_FLUSH_SKIP)
        bad = [k for k, x, y in zip(("costs", "grad_enc", "grad_pred"), new, ref) if not torch.equal(x, y)]
        if bad:
            failed[b] = "differs in " + ", ".join(bad)
    _assert_none_failed(failed, "f16x2 %s" % (shape,), 4)


# ---- d. the forward-only entry -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_forward_only_costs(amd, route):
    """joint_rnnt_loss under torch.no_grad() (rnnt_engine_joint_loss_fwd: the forward epilogue's gather of logit[blank] and the
    lattice sweep alone): the oracle's costs, and the training-mode call's bit for bit."""
    V = SWEEP_SHAPE[-1]
    bf16 = route == "bf16"
    failed = {}
    for b in (0, 5, 64, 126):
        d = _problem(SWEEP_SHAPE, b)
        g = _dev(d)
        with torch.no_grad():
            loss, costs = amd.joint_rnnt_loss(g["enc"].requires_grad_(True), g["pred"], g["W"], g["bias"], g["targets"],
                                              g["logit_lens"], g["target_lens"], blank=_signed(b, V), return_costs=True,
                                              dtype=route)
        assert not loss.requires_grad
        ref = _reference(SWEEP_SHAPE, b, bf16)
        try:
            assert_close_loss("costs", costs.cpu().numpy(), ref["costs"], rtol=BF16_LOSS_RTOL if bf16 else LOSS_RTOL)
            assert_close_loss("loss", loss.item(), ref["loss"], rtol=BF16_LOSS_RTOL if bf16 else LOSS_RTOL)
            train = _run_fused(amd, d, route, b)
            assert np.array_equal(costs.cpu().numpy(), train["costs"]), "forward-only costs differ from the training call's"
        except AssertionError as e:
            failed[b] = str(e)
    _assert_none_failed(failed, route, 4)


# ---- e. the unfused loss on materialised logits --------------------------------------------------------------------------------
def _logits_problem(shape, blank, scale=2.0):
    B, T, U, V = shape
    rng = np.random.default_rng(sum(shape))
    logits = (rng.standard_normal((B, T, U + 1, V)) * scale).astype(np.float32)
    d = relabel_blank(make_inputs(B, T, U, 4, V, seed=sum(shape)), blank, neighbours=True)[0]
    return logits, d


@pytest.mark.parametrize("clamp", [-1, 0.05])
@pytest.mark.parametrize("shape", [(2, 6, 3, 40), (2, 8, 4, 7)])
def test_unfused_loss_every_blank_position(amd, shape, clamp):
    """rnnt_loss on logits (lattice.hip k_logsoftmax_gather and the gradient kernel), V = 40 and V = 7 (V % 4 != 0: the host pads the
    logits), every blank: costs and grad_logits against cpu_oracle.rnnt_loss at that blank, plain and clamped."""
    B, T, U, V = shape
    w = np.arange(1, B + 1, dtype=np.float64)
    failed, clamped, last_label = {}, False, False
    for b in range(V):
        logits, d = _logits_problem(shape, b)
        last_label |= b < V - 1 and has_live_label(d, V - 1)
        g = _dev(d)
        lt = torch.from_numpy(logits).cuda().requires_grad_(True)
        costs = amd.rnnt_loss(lt, g["targets"], g["logit_lens"], g["target_lens"], blank=_signed(b, V), clamp=clamp,
                              reduction="none")
        (costs * torch.from_numpy(w).float().cuda()).sum().backward()
        ref_c, ref_g = cpu_oracle.rnnt_loss(logits, d["targets"], d["logit_lens"], d["target_lens"], blank=b, clamp=clamp)
        if clamp > 0:
            clamped |= bool((np.abs(ref_g) >= clamp).any())
        try:
            assert_close_loss("costs", costs.detach().cpu().numpy(), ref_c)
            assert_close_grad("grad_logits", lt.grad.cpu().numpy(), ref_g * w.reshape(B, 1, 1, 1))
        except AssertionError as e:
            failed[b] = str(e)
    assert last_label and (clamp < 0 or clamped)
    _assert_none_failed(failed, "rnnt_loss %s clamp %s" % (shape, clamp), V)


def test_unfused_loss_long_lattice_blank_first(amd):
    """(B,T,U,V) = (2,70,200,8): the lattice sweep on four chained waves (test_loss_only_vs_oracle's shape), blank = 0."""
    shape = (2, 70, 200, 8)
    logits, d = _logits_problem(shape, 0)
    g = _dev(d)
    lt = torch.from_numpy(logits).cuda().requires_grad_(True)
    costs = amd.rnnt_loss(lt, g["targets"], g["logit_lens"], g["target_lens"], blank=0, reduction="none")
    costs.sum().backward()
    ref_c, ref_g = cpu_oracle.rnnt_loss(logits, d["targets"], d["logit_lens"], d["target_lens"], blank=0)
    assert_close_loss("costs", costs.detach().cpu().numpy(), ref_c)
    assert_close_grad("grad_logits", lt.grad.cpu().numpy(), ref_g)


# ---- f. forced alignment ---------------------------------------------------------------------------------------------------------
ALIGN_SHAPE = (3, 23, 9, 128, 128)
ALIGN_BLANKS = (0, 5, 16, 126)


@functools.lru_cache(maxsize=None)
def _align_case(blank):
    from tests.test_align_gpu import _oracle_logits, _ragged
    d = relabel_blank(_ragged(*ALIGN_SHAPE, seed=sum(ALIGN_SHAPE)), blank, neighbours=True)[0]
    logits = _oracle_logits(d)
    ref = ao.viterbi_logits(logits, d["targets"], d["logit_lens"], d["target_lens"], blank)
    return d, logits, ref


def test_align_on_logits(amd):
    from tests.test_align_gpu import MARGIN, _check_against_oracle
    for b in ALIGN_BLANKS:
        d, logits, _ = _align_case(b)
        g = _dev(d)
        lg32 = logits.astype(np.float32)
        ref32 = ao.viterbi_logits(lg32, d["targets"], d["logit_lens"], d["target_lens"], b)
        s, f = amd.rnnt_align(torch.from_numpy(lg32).cuda(), g["targets"], g["logit_lens"], g["target_lens"], blank=_signed(b, 128))
        counted = _check_against_oracle(s, f, *ref32, d["target_lens"], what=("logits", b))
        assert counted >= 1 and ref32[2][0] > MARGIN, (b, ref32[2])  # the full utterance's frames WERE compared


@pytest.mark.parametrize("route", ROUTES)
def test_joint_align(amd, route):
    from tests.test_align_gpu import MARGIN, _check_against_oracle
    B, V = ALIGN_SHAPE[0], ALIGN_SHAPE[-1]
    for b in ALIGN_BLANKS:
        d, logits, ref = _align_case(b)
        g = _dev(d)
        s, f = amd.joint_rnnt_align(g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"],
                                    blank=_signed(b, V), dtype=route)
        if route != "bf16":
            _check_against_oracle(s, f, *ref, d["target_lens"], what=(route, b))
            assert ref[2][0] > MARGIN, (b, ref[2])  # the full utterance's frames WERE compared
            continue
        # bf16 operands (tests/test_align_gpu.py test_every_route): the bar of its loss tests against the unrounded oracle; the path
        # it returns, rescored in float64, is within that bar of the best one
        _check_against_oracle(s, f, ref[0], ref[1], np.zeros(B), d["target_lens"], rtol=BF16_LOSS_RTOL_EXACT, what=(route, b))
        for i in range(B):
            lpb, lpe = ao.lattice_logprobs(logits[i], d["targets"][i], b)
            r = ao.rescore(lpb, lpe, f[i].cpu().numpy(), int(d["logit_lens"][i]), int(d["target_lens"][i]))
            assert abs(r - ref[0][i]) <= BF16_LOSS_RTOL_EXACT * abs(ref[0][i]), (b, i, r, ref[0][i])


# ---- g. FastEmit and the delay penalty -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_latency_regularisers(amd, route):
    """Option "both" (lambda = 0.5, delta = 0.05) of tests/test_latency_reg_gpu.py on its ragged case, relabelled."""
    from tests.test_latency_reg_gpu import OPTIONS, _case
    from tests.test_latency_reg_gpu import _compare as compare_reg
    lam, dp = OPTIONS["both"]
    base = _case("ragged", seed=13)
    bf16 = route == "bf16"
    failed = {}
    for b in (0, 7, 8, 126):
        d = relabel_blank(base, b, neighbours=True)[0]
        ref = (lro.fused_bf16 if bf16 else lro.fused)(d, lam, dp, blank=b)
        r = _run_fused(amd, d, route, _signed(b, 128), fastemit_lambda=lam, delay_penalty=dp)
        try:
            compare_reg(r, ref, bf16=bf16)
        except AssertionError as e:
            failed[b] = str(e)
    _assert_none_failed(failed, route, 4)


@pytest.mark.parametrize("blank", [0, 17])
def test_standalone_regularised_loss(amd, blank):
    shape = (3, 13, 6, 40)
    lam, dp = 0.5, 0.05
    logits, d = _logits_problem(shape, blank)
    g = _dev(d)
    x = torch.from_numpy(logits).cuda().requires_grad_(True)
    out = amd.rnnt_loss(x, g["targets"], g["logit_lens"], g["target_lens"], blank=blank, reduction="none", fastemit_lambda=lam,
                        delay_penalty=dp)
    out.sum().backward()
    costs, G = lro.loss_and_grad(logits, d["targets"], d["logit_lens"], d["target_lens"], blank, lam, dp)
    assert_close_loss("costs", out.detach().cpu().numpy(), costs)
    assert_close_grad("grad_logits", x.grad.cpu().numpy(), G)
