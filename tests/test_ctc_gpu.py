"""GPU tests of the CTC head: rnnt_amd.ctc_loss / ctc_greedy_decode on the engine, CTCHead and RNNTModel's
hybrid loss against the float64 oracle of tests/ctc_cases.py (torch.nn.functional.ctc_loss on the CPU) at the project's bars
(tests/helpers.py: costs 1e-4 relative, gradients 1e-4 of the largest reference entry + 1e-7).  Shapes are (N, T, U, V), the
smallest at which each mechanism can go wrong; every check prints its measured worst errors (profiles/ctc_parity.txt)."""
import numpy as np
import pytest
import torch

import rnnt_amd
from tests import ctc_cases
from tests.helpers import GRAD_ATOL, GRAD_RTOL, assert_close_grad, assert_close_loss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def engine_run(x, tg, ll, tl, blank, weights=None, backend="engine"):
    """-> (costs [N], d sum_n weights[n] costs[n] / d logits [N,T,V]) as numpy, through rnnt_amd.ctc_loss(reduction="none")."""
    xt = _dev(x, torch.float32).requires_grad_(True)
    costs = rnnt_amd.ctc_loss(xt, _dev(tg, torch.int32), _dev(ll, torch.int32), _dev(tl, torch.int32),
                              blank=blank, reduction="none", backend=backend)
    w = torch.ones_like(costs) if weights is None else _dev(weights, torch.float32)
    costs.backward(w)
    return costs.detach().cpu().numpy(), xt.grad.cpu().numpy()


def check(name, x, tg, ll, tl, blank, weights=None):
    """Engine against oracle: +inf exactly where no path exists (with exactly zero gradient there), the bars elsewhere."""
    costs, grad = engine_run(x, tg, ll, tl, blank, weights)
    tg2 = np.asarray(tg)
    ref_c, ref_g = ctc_cases.oracle(x, tg2, ll, tl, blank, weights)
    inf = ctc_cases.infeasible(tg2, ll, tl)
    assert (costs[inf] == np.inf).all(), (name, costs, inf)
    assert (grad[inf] == 0.0).all(), name
    if (~inf).any():
        rel = np.abs(costs[~inf] - ref_c[~inf]) / np.maximum(np.abs(ref_c[~inf]), 1e-12)
        err = np.abs(grad.astype(np.float64) - ref_g).max()
        bound = GRAD_RTOL * np.abs(ref_g).max() + GRAD_ATOL
        print(f"ctc_parity {name}: cost rel err {rel.max():.3e} (bar 1.0e-04), grad abs err {err:.3e} (bar {bound:.3e})")
        assert_close_loss(name + " costs", costs[~inf], ref_c[~inf])
    for n in range(len(ll)):  # frames past T_n: exact zeros
        assert (grad[n, int(ll[n]):] == 0.0).all(), (name, n)
    assert_close_grad(name + " grad", grad, ref_g)
    return costs, grad


def rand_case(seed, N, T, U, V, blank=None, scale=1.0, repeat_p=0.3):
    rng = np.random.default_rng(seed)
    blank = V - 1 if blank is None else blank
    x = (scale * rng.standard_normal((N, T, V))).astype(np.float32)
    return x, ctc_cases.make_targets(rng, N, U, V, blank, repeat_p), np.full(N, T), np.full(N, U), blank


# ---- edges of the lattice
def test_one_frame_no_label_and_one_label():
    x, tg, ll, tl, blank = rand_case(1, 1, 1, 0, 4)
    check("(1,1,0,4)", x, tg, ll, tl, blank)
    x, tg, ll, tl, blank = rand_case(2, 1, 1, 1, 4)
    check("(1,1,1,4)", x, tg, ll, tl, blank)


def test_repeated_pair_with_exactly_one_path():
    x, _, ll, tl, blank = rand_case(3, 1, 3, 2, 4)
    costs, _ = check("(1,3,2,4) [a,a]", x, [[1, 1]], ll, tl, blank)
    lp = torch.log_softmax(torch.tensor(x[0], dtype=torch.float64), -1)
    assert abs(costs[0] + (lp[0, 1] + lp[1, 3] + lp[2, 1]).item()) <= 1e-4 * abs(costs[0])  # a _ a


def test_infeasible_pair_is_inf_with_zero_gradient_and_no_error_word():
    x, _, ll, tl, blank = rand_case(4, 1, 2, 2, 4)
    costs, grad = check("(1,2,2,4) [a,a]", x, [[1, 1]], ll, tl, blank)
    assert costs[0] == np.inf and not np.isnan(costs).any() and (grad == 0.0).all()
    z = rnnt_amd.ctc_loss(_dev(x, torch.float32), _dev([[1, 1]], torch.int32), _dev(ll, torch.int32), _dev(tl, torch.int32),
                          reduction="sum", zero_infinity=True, backend="engine")
    assert z.item() == 0.0


def test_as_many_frames_as_distinct_labels():
    x, _, ll, tl, blank = rand_case(5, 1, 4, 4, 8)
    check("(1,4,4,8) T=U", x, [[0, 1, 2, 3]], ll, tl, blank)


# ---- wave boundaries of the chain, the mailbox and the barrier form, the largest lattice
@pytest.mark.parametrize("U", [63, 64, 65, 130])
def test_chain_wave_boundaries(U):
    x, tg, ll, tl, blank = rand_case(10 + U, 2, U + 20, U, 8, repeat_p=0.1)
    ll[1], tl[1] = U + 3, U - 2  # a second utterance whose last lane sits elsewhere (feasible or not by its repeats)
    assert not ctc_cases.infeasible(tg, ll, tl)[0]
    check(f"(2,{U + 20},{U},8)", x, tg, ll, tl, blank)


def test_largest_lattice_and_the_u_limit():
    x, tg, ll, tl, blank = rand_case(20, 1, 1100, 1023, 8, repeat_p=0.05)
    assert not ctc_cases.infeasible(tg, ll, tl)[0]
    check("(1,1100,1023,8)", x, tg, ll, tl, blank)
    x, tg, ll, tl, blank = rand_case(21, 1, 1100, 1024, 8, repeat_p=0.05)
    args = (_dev(x, torch.float32), _dev(tg, torch.int32), _dev(ll, torch.int32), _dev(tl, torch.int32))
    with pytest.raises(RuntimeError):
        rnnt_amd.ctc_loss(*args, backend="engine")
    assert torch.isfinite(rnnt_amd.ctc_loss(*args, backend="auto"))


def test_mailbox_chain_over_several_waves_and_many_frames():
    """U = 130 at T = 1500: the mailboxes (2 boundaries x 1500 steps) still fit; one more wave (U = 200, 3 x 1500 x 12 B
    < 64 KiB too) and the barrier form beyond (U = 300 at T = 1500) at the same shapes' cost."""
    for U in (130, 200, 300):
        x, tg, ll, tl, blank = rand_case(30 + U, 1, 1500, U, 8)
        check(f"(1,1500,{U},8)", x, tg, ll, tl, blank)


# ---- deterministic scatter
@pytest.mark.parametrize("kind", ["all_equal", "alternating"])
def test_repeated_labels_scatter_is_deterministic(kind):
    x, _, ll, tl, blank = rand_case(40, 2, 90, 40, 8)
    tg = np.full((2, 40), 2) if kind == "all_equal" else np.tile([1, 5], (2, 20))
    ll[1], tl[1] = 70, 31
    a = check(f"(2,90,40,8) {kind}", x, tg, ll, tl, blank)
    b = engine_run(x, tg, ll, tl, blank)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    xt = _dev(x, torch.float32)
    runs = [rnnt_amd.engine.ctc_loss_fwd_bwd(xt, _dev(tg, torch.int32), _dev(ll, torch.int32), _dev(tl, torch.int32), blank)
            for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ---- ragged batch with garbage past the lengths
def _ragged():
    rng = np.random.default_rng(50)
    N, T, U, V = 5, 37, 9, 12
    x = rng.standard_normal((N, T, V)).astype(np.float32)
    tg = ctc_cases.make_targets(rng, N, U, V, V - 1)
    ll = np.array([1, 20, 37, 9, 30])
    tl = np.array([1, 0, 9, 9, 5])
    tg[3] = [4, 4, 4, 4, 4, 4, 4, 4, 4]  # 9 labels, 8 repeats, 9 frames: infeasible
    for n in range(N):
        x[n, ll[n]:] = np.nan
        tg[n, tl[n]:] = -1
    return x, tg, ll, tl, V - 1


def test_ragged_batch_ignores_garbage_past_the_lengths():
    x, tg, ll, tl, blank = _ragged()
    assert ctc_cases.infeasible(tg, ll, tl).tolist() == [False, False, False, True, False]
    costs, grad = check("ragged (5,37,9,12)", x, tg, ll, tl, blank)
    assert np.isfinite(grad).all()


def test_nan_inside_one_utterance_stays_there():
    x, tg, ll, tl, blank = _ragged()
    clean, _ = engine_run(x, tg, ll, tl, blank)
    x[4, 11, 3] = np.nan
    costs, _ = engine_run(x, tg, ll, tl, blank)
    assert np.isnan(costs[4])
    assert np.array_equal(costs[:4], clean[:4])


# ---- blank position, vocabulary loops, peaked logits
@pytest.mark.parametrize("blank", [0, 6, 11])
def test_blank_position(blank):
    x, tg, ll, tl, _ = rand_case(60 + blank, 3, 20, 6, 12, blank=blank)
    ll[1], tl[1] = 13, 4
    check(f"(3,20,6,12) blank {blank}", x, tg, ll, tl, blank)


@pytest.mark.parametrize("V", [4, 1024, 1028, 5, 29])
def test_vocabulary_loops_and_padding(V):
    x, tg, ll, tl, blank = rand_case(70 + V, 2, 12, 4, V)
    check(f"(2,12,4,{V})", x, tg, ll, tl, blank)
    if V in (5, 29):  # the padded columns get no gradient and the blank may sit in the middle of the odd vocabulary
        x, tg, ll, tl, blank = rand_case(71 + V, 2, 12, 4, V, blank=V // 2)
        check(f"(2,12,4,{V}) blank {V // 2}", x, tg, ll, tl, blank)


def test_peaked_logits():
    x, tg, ll, tl, blank = rand_case(80, 2, 30, 8, 16, scale=30.0)
    check("(2,30,8,16) x30", x, tg, ll, tl, blank)


# ---- upstream weights and reductions
def test_upstream_weights_and_reductions():
    x, tg, ll, tl, blank = rand_case(90, 4, 25, 7, 12)
    ll[2], tl[2] = 17, 5
    w = np.array([0.7, 0.0, 1.9, 0.25], dtype=np.float32)
    _, grad = check("(4,25,7,12) weighted", x, tg, ll, tl, blank, weights=w)
    assert (grad[1] == 0.0).all()
    # the ABI's own per-utterance weights: the same gradient without the multiply pass
    _, g2 = rnnt_amd.engine.ctc_loss_fwd_bwd(_dev(x, torch.float32), _dev(tg, torch.int32), _dev(ll, torch.int32), _dev(tl, torch.int32),
                                             blank, cost_weights=_dev(w, torch.float32))
    g2 = g2.cpu().numpy()
    assert (g2[1] == 0.0).all()
    assert_close_grad("cost_weights grad", g2, ctc_cases.oracle(x, tg, ll, tl, blank, w)[1])
    ref_c, ref_g = ctc_cases.oracle(x, tg, ll, tl, blank)
    for reduction, scale in (("sum", 1.0), ("mean", 0.25)):
        xt = _dev(x, torch.float32).requires_grad_(True)
        loss = rnnt_amd.ctc_loss(xt, _dev(tg, torch.int32), _dev(ll, torch.int32), _dev(tl, torch.int32), reduction=reduction,
                                 backend="engine")
        loss.backward()
        assert_close_loss(reduction, loss.item(), ref_c.sum() * scale)
        assert_close_grad(reduction + " grad", xt.grad.cpu().numpy(), ref_g * scale)


# ---- the head and the model
def test_head_loss_and_gradients_against_a_float64_linear():
    torch.manual_seed(0)
    head = rnnt_amd.CTCHead(64, 128).to(DEV)
    rng = np.random.default_rng(100)
    enc = rng.standard_normal((2, 24, 64)).astype(np.float32)
    tg = ctc_cases.make_targets(rng, 2, 9, 128, 127)
    ll, tl = np.array([24, 17]), np.array([9, 6])
    e = _dev(enc, torch.float32).requires_grad_(True)
    loss = head.loss(e, _dev(tg, torch.int32), _dev(ll, torch.int32), _dev(tl, torch.int32), backend="engine")
    loss.backward()
    ref = torch.nn.Linear(64, 128).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in head.linear.state_dict().items()})
    e64 = torch.tensor(enc, dtype=torch.float64, requires_grad=True)
    want = rnnt_amd.ctc_loss(ref(e64), torch.tensor(tg), torch.tensor(ll, dtype=torch.int32), torch.tensor(tl, dtype=torch.int32),
                             backend="torch")
    want.backward()
    assert_close_loss("head loss", loss.item(), want.item())
    assert_close_grad("head d enc", e.grad.cpu().numpy(), e64.grad.numpy())
    assert_close_grad("head d weight", head.linear.weight.grad.cpu().numpy(), ref.weight.grad.numpy())
    assert_close_grad("head d bias", head.linear.bias.grad.cpu().numpy(), ref.bias.grad.numpy())


class _Encoder(torch.nn.Module):
    def __init__(self, n_mels, feats):
        super().__init__()
        self.c1 = torch.nn.Conv1d(n_mels, feats, 3, stride=2, padding=1)

    def forward(self, x):
        return torch.tanh(self.c1(x))

    def calc_output_lens(self, lens):
        return (lens + 1) // 2


def _model(head):
    torch.manual_seed(7)
    vocab, feats = 32, 64
    model = rnnt_amd.RNNTModel(rnnt_amd.ConvPredictor(vocab, feats, 32, dropout=0.0), _Encoder(16, feats),
                               rnnt_amd.JointNetwork(-1, -1, feats, vocab))
    if head:
        model.ctc_head = rnnt_amd.CTCHead(feats, vocab)
    return model.to(DEV)


def _batch():
    g = torch.Generator().manual_seed(8)
    mel = torch.randn(3, 16, 48, generator=g)
    ids = torch.randint(0, 31, (3, 7), generator=g)
    return mel.to(DEV), torch.tensor([48, 30, 41], device=DEV), ids.to(DEV), torch.tensor([7, 4, 6], device=DEV)


def test_model_hybrid_loss():
    plain, hybrid = _model(False), _model(True)
    hybrid.load_state_dict(plain.state_dict(), strict=False)
    batch = _batch()
    la, lb = plain(*batch, 31), hybrid(*batch, 31)  # ctc_weight = 0: the headless model bit for bit
    assert torch.equal(la, lb)
    la.backward()
    lb.backward()
    for (ka, pa), (kb, pb) in zip(plain.named_parameters(), ((k, p) for k, p in hybrid.named_parameters() if not k.startswith("ctc_head"))):
        assert ka == kb and torch.equal(pa.grad, pb.grad), ka
    assert all(p.grad is None for p in hybrid.ctc_head.parameters())
    hybrid.ctc_weight = 0.3
    got = hybrid(*batch, 31)
    mel, mel_lens, ids, id_lens = batch
    enc_lens = hybrid.encoder.calc_output_lens(mel_lens)
    logits = torch.nn.functional.linear(hybrid.encoder(mel).permute(0, 2, 1).double(), hybrid.ctc_head.linear.weight.double(),
                                        hybrid.ctc_head.linear.bias.double())
    ctc = rnnt_amd.ctc_loss(logits.cpu(), ids.int().cpu(), enc_lens.int().cpu(), id_lens.int().cpu(), blank=31, backend="torch")
    assert_close_loss("hybrid loss", got.item(), 0.7 * la.item() + 0.3 * ctc.item())
    got.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in hybrid.ctc_head.parameters())
    # the model's CTC decode is the head's decode of encoder(mel)
    want = hybrid.ctc_head.greedy_decode(hybrid.encoder(mel).permute(0, 2, 1), enc_lens.int(), blank=31)
    assert hybrid.ctc_greedy_decode(mel, mel_lens) == want and len(want) == 3


# ---- greedy decode
@pytest.mark.parametrize("V,blank", [(12, 11), (12, 0), (12, 7), (1028, 1027), (29, 14)])
def test_greedy_decode_against_the_numpy_collapse(V, blank):
    rng = np.random.default_rng(110 + V + blank)
    x = rng.standard_normal((5, 37, V)).astype(np.float32)
    ll = np.array([37, 1, 20, 5, 36])
    x[0] = 0.0
    x[0, np.arange(37), rng.integers(0, 3, 37)] = 5.0   # few distinct winners: runs to merge, blank 0 among them
    x[3, :5, blank] = 9.0                               # all-blank frames
    for n in range(5):
        x[n, ll[n]:] = np.nan                           # never read
    got = rnnt_amd.ctc_greedy_decode(_dev(x, torch.float32), _dev(ll, torch.int32), blank=blank, backend="engine")
    best = np.stack([np.concatenate([x[n, :ll[n]].argmax(-1), np.zeros(37 - ll[n], dtype=np.int64)]) for n in range(5)])
    assert got == ctc_cases.collapse(best, ll, blank)
    assert got[3] == [] and len(got[1]) <= 1


def test_greedy_decode_repeats_ties_and_long_utterances():
    y = np.full((1, 4, 4), -1.0, dtype=np.float32)
    for t, v in enumerate((1, 1, 3, 1)):
        y[0, t, v] = 2.0
    assert rnnt_amd.ctc_greedy_decode(_dev(y, torch.float32), _dev([4], torch.int32), blank=3, backend="engine") == [[1, 1]]
    y[0, 0, 0] = 2.0  # two columns exactly equal in frame 0: the lower index wins
    assert rnnt_amd.ctc_greedy_decode(_dev(y, torch.float32), _dev([4], torch.int32), blank=3, backend="engine") == [[0, 1, 1]]
    # more frames than one pass of the collapse's block scan (1024), a run that crosses the pass boundary
    rng = np.random.default_rng(120)
    x = rng.standard_normal((2, 2500, 8)).astype(np.float32)
    x[0, 1020:1030, 2] = 50.0
    ll = np.array([2500, 1025])
    got = rnnt_amd.ctc_greedy_decode(_dev(x, torch.float32), _dev(ll, torch.int32), blank=7, backend="engine")
    assert got == ctc_cases.collapse(x.argmax(-1), ll, 7)
    assert got == rnnt_amd.ctc_greedy_decode(_dev(x, torch.float32), _dev(ll, torch.int32), blank=7, backend="torch")
