"""CPU tests of the CTC head's definition: rnnt_amd.ctc_loss(backend="torch") — the carrier of the GPU tests'
oracle — against a brute-force enumeration of every frame labelling; the torch-path greedy decode against a numpy collapse;
RNNTModel's hybrid loss on the CPU with plain torch modules."""
import itertools

import numpy as np
import pytest
import torch

import rnnt_amd
from tests import ctc_cases
from tests.stream_models import PassThroughEncoder, TorchConvPredictor

V = 3


def _i32(x):
    return torch.tensor(np.asarray(x), dtype=torch.int32)


def brute_force_cost(logits, target, blank):
    """-log of the summed probability of every labelling of the T frames that collapses to `target`; logits [T,V] float64
    tensor (differentiable).  +inf when there is none."""
    T, nv = logits.shape
    lp = torch.log_softmax(logits, dim=-1)
    terms = []
    for path in itertools.product(range(nv), repeat=T):
        if ctc_cases.collapse([np.array(path)], [T], blank)[0] == list(target):
            terms.append(sum(lp[t, v] for t, v in enumerate(path)))
    if not terms:
        return torch.tensor(float("inf"), dtype=torch.float64)
    return -torch.logsumexp(torch.stack(terms), dim=0)


# (T, target, blank): every U <= 2 with T <= 5, the repeated-label target at its shortest feasible T and beyond, each blank
CASES = [(1, [], 2), (3, [], 0), (1, [0], 2), (2, [1], 2), (4, [0], 1), (2, [0, 1], 2), (3, [1, 0], 2), (5, [0, 1], 2),
         (3, [0, 0], 2), (4, [1, 1], 2), (5, [0, 0], 2), (5, [2, 2], 0), (4, [0, 2], 1), (5, [2, 1], 0)]


@pytest.mark.parametrize("T,target,blank", CASES)
def test_torch_backend_equals_brute_force(T, target, blank):
    g = torch.Generator().manual_seed(17 * T + len(target) + blank)
    x = torch.randn(1, T, V, generator=g, dtype=torch.float64)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    got = rnnt_amd.ctc_loss(xa, _i32([target]).reshape(1, len(target)), _i32([T]), _i32([len(target)]), blank=blank,
                            reduction="none", backend="torch")
    ref = brute_force_cost(xb[0], target, blank)
    assert got.shape == (1,)
    assert abs(got.item() - ref.item()) <= 1e-12 * max(1.0, abs(ref.item()))
    got.sum().backward()
    ref.backward()
    assert np.abs(xa.grad.numpy() - xb.grad.numpy()).max() <= 1e-12


def _batch():
    """Three utterances in one padded batch: [a,a] feasible (T = 3: one path), [a,a] infeasible (T = 2), [b] with T = 5."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 5, V, generator=g, dtype=torch.float64)
    return x, _i32([[0, 0], [0, 0], [1, 0]]), _i32([3, 2, 5]), _i32([2, 2, 1])


def test_reductions_and_the_infeasible_rule():
    x, tg, ll, tl = _batch()
    ref = [brute_force_cost(x[n, :int(ll[n])], tg[n, :int(tl[n])].tolist(), 2).item() for n in range(3)]
    assert ref[1] == float("inf") and np.isfinite(ref[0]) and np.isfinite(ref[2])
    xa = x.clone().requires_grad_(True)
    none = rnnt_amd.ctc_loss(xa, tg, ll, tl, reduction="none", backend="torch")
    assert none[1].item() == float("inf")
    assert np.allclose(none.detach().numpy()[[0, 2]], [ref[0], ref[2]], rtol=1e-12, atol=0)
    # the infeasible utterance sends an exactly zero gradient, frames past T_n too; the others their own
    (none[0] + 2.0 * none[2] + none[1]).backward()
    assert torch.equal(xa.grad[1], torch.zeros_like(xa.grad[1]))
    assert torch.equal(xa.grad[0, 3:], torch.zeros_like(xa.grad[0, 3:]))
    xb = x.clone().requires_grad_(True)
    (brute_force_cost(xb[0, :3], [0, 0], 2) + 2.0 * brute_force_cost(xb[2], [1], 2)).backward()
    assert np.abs(xa.grad.numpy() - xb.grad.numpy()).max() <= 1e-12
    # zero_infinity: that cost counts 0; "mean" is the mean of the per-utterance costs (NOT torch's length-normalised mean)
    z = rnnt_amd.ctc_loss(x, tg, ll, tl, reduction="none", zero_infinity=True, backend="torch")
    assert z[1].item() == 0.0 and torch.equal(z[[0, 2]], none.detach()[[0, 2]])
    s = rnnt_amd.ctc_loss(x, tg, ll, tl, reduction="sum", zero_infinity=True, backend="torch")
    m = rnnt_amd.ctc_loss(x, tg, ll, tl, reduction="mean", zero_infinity=True, backend="torch")
    assert abs(s.item() - (ref[0] + ref[2])) <= 1e-12 * abs(s.item())
    assert abs(m.item() - (ref[0] + ref[2]) / 3.0) <= 1e-12 * abs(m.item())
    assert rnnt_amd.ctc_loss(x, tg, ll, tl, reduction="mean", backend="torch").item() == float("inf")


def test_oracle_helper_agrees_with_the_torch_backend():
    """tests/ctc_cases.oracle (what the GPU tests compare against) and the package's torch path are the same function of the inputs."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, 9, 6)).astype(np.float32)
    tg = ctc_cases.make_targets(rng, 4, 3, 6, blank=5)
    ll, tl = np.array([9, 4, 1, 7]), np.array([3, 2, 0, 3])
    w = np.array([1.0, 0.5, 2.0, 0.0])
    costs, grad = ctc_cases.oracle(x, tg, ll, tl, 5, w)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    got = rnnt_amd.ctc_loss(xt, _i32(tg), _i32(ll), _i32(tl), reduction="none", zero_infinity=True, backend="torch")
    (got * torch.tensor(w)).sum().backward()
    assert np.abs(got.detach().numpy() - costs).max() <= 1e-12
    assert np.abs(xt.grad.numpy() - grad).max() <= 1e-12


def test_argument_checks():
    x, tg, ll, tl = _batch()
    with pytest.raises(ValueError):
        rnnt_amd.ctc_loss(x, tg, ll, tl, reduction="avg", backend="torch")
    with pytest.raises(ValueError):
        rnnt_amd.ctc_loss(x, tg, ll, tl, backend="hip")
    with pytest.raises(RuntimeError):
        rnnt_amd.ctc_loss(x, tg, ll, tl, blank=3, backend="torch")
    with pytest.raises(RuntimeError):
        rnnt_amd.ctc_loss(x, tg, _i32([3, 2, 6]), tl, backend="torch")  # T_n > T
    with pytest.raises(RuntimeError):
        rnnt_amd.ctc_loss(x, tg.long(), ll, tl, backend="torch")
    with pytest.raises(RuntimeError):  # the engine has no CPU path, and says so
        rnnt_amd.ctc_loss(x.float(), tg, ll, tl, backend="engine")
    with pytest.raises(RuntimeError):
        rnnt_amd.ctc_greedy_decode(x.float(), ll, backend="engine")


def test_torch_greedy_decode_equals_numpy_collapse():
    rng = np.random.default_rng(11)
    x = rng.standard_normal((5, 37, 12)).astype(np.float32)
    ll = np.array([37, 1, 20, 5, 36])
    x[0, :, :] = 0.0
    x[0, np.arange(37), rng.integers(0, 3, 37)] = 5.0  # few distinct winners: many repeats to merge
    x[3, :5, 7] = 9.0                                  # all-blank frames (blank = 7 below)
    for blank in (11, 0, 7):
        got = rnnt_amd.ctc_greedy_decode(torch.tensor(x), _i32(ll), blank=blank, backend="torch")
        assert got == ctc_cases.collapse(x.argmax(-1), ll, blank)
    assert rnnt_amd.ctc_greedy_decode(torch.tensor(x), _i32(ll), blank=7, backend="torch")[3] == []
    # a a _ a -> [a, a]; ties go to the lowest index
    y = np.full((1, 4, 4), -1.0, dtype=np.float32)
    for t, v in enumerate((1, 1, 3, 1)):
        y[0, t, v] = 2.0
    assert rnnt_amd.ctc_greedy_decode(torch.tensor(y), _i32([4]), blank=3, backend="torch") == [[1, 1]]
    y[0, 0, 0] = 2.0  # frame 0: entries 0 and 1 tie
    assert rnnt_amd.ctc_greedy_decode(torch.tensor(y), _i32([4]), blank=3, backend="torch") == [[0, 1, 1]]


# ---- RNNTModel on the CPU: plain torch modules, the transducer loss as a small differentiable lattice
class _TorchJoint(torch.nn.Module):
    def __init__(self, H, num_classes):
        super().__init__()
        self.joint_ln = torch.nn.Linear(H, num_classes)
        self.blank_idx = num_classes - 1

    def fused_loss(self, audio, text, targets, logit_lengths, target_lengths, blank=-1, reduction="mean", **kw):
        lp = torch.log_softmax(self.joint_ln(torch.tanh(audio[:, :, None, :] + text[:, None, :, :])), dim=-1)
        costs = []
        for n in range(lp.shape[0]):
            Tn, Un = int(logit_lengths[n]), int(target_lengths[n])
            alpha = {(0, 0): lp.new_zeros(())}
            for t in range(Tn):
                for u in range(Un + 1):
                    if (t, u) == (0, 0):
                        continue
                    terms = []
                    if t > 0:
                        terms.append(alpha[(t - 1, u)] + lp[n, t - 1, u, self.blank_idx])
                    if u > 0:
                        terms.append(alpha[(t, u - 1)] + lp[n, t, u - 1, int(targets[n, u - 1])])
                    alpha[(t, u)] = torch.logsumexp(torch.stack(terms), dim=0)
            costs.append(-(alpha[(Tn - 1, Un)] + lp[n, Tn - 1, Un, self.blank_idx]))
        return torch.stack(costs).mean()


def _cpu_model(head):
    torch.manual_seed(4)
    H, NV = 8, 6
    model = rnnt_amd.RNNTModel(TorchConvPredictor(NV, H, 8), PassThroughEncoder(), _TorchJoint(H, NV))
    if head:
        model.ctc_head = rnnt_amd.CTCHead(H, NV)
    return model.double()


def _cpu_batch():
    g = torch.Generator().manual_seed(9)
    mel = torch.randn(2, 8, 6, generator=g, dtype=torch.float64)  # (N, C, L): the pass-through encoder's output
    return mel, torch.tensor([6, 4]), torch.tensor([[0, 0, 3], [2, 1, 0]]), torch.tensor([3, 2])


def test_model_with_zero_ctc_weight_is_the_headless_model_bit_for_bit():
    plain, hybrid = _cpu_model(False), _cpu_model(True)
    hybrid.load_state_dict(plain.state_dict(), strict=False)
    assert sorted(k for k in hybrid.state_dict() if k.startswith("ctc_head")) == ["ctc_head.linear.bias", "ctc_head.linear.weight"]
    batch = _cpu_batch()
    la, lb = plain(*batch, 5), hybrid(*batch, 5)
    assert torch.equal(la, lb)
    la.backward()
    lb.backward()
    for (ka, pa), (kb, pb) in zip(plain.named_parameters(), ((k, p) for k, p in hybrid.named_parameters() if not k.startswith("ctc_head"))):
        assert ka == kb and torch.equal(pa.grad, pb.grad), ka
    assert all(p.grad is None for p in hybrid.ctc_head.parameters())


def test_model_hybrid_loss_is_the_weighted_sum():
    plain, hybrid = _cpu_model(False), _cpu_model(True)
    hybrid.load_state_dict(plain.state_dict(), strict=False)
    hybrid.ctc_weight = 0.3
    mel, mel_lens, ids, id_lens = _cpu_batch()
    got = hybrid(mel, mel_lens, ids, id_lens, 5)
    rnnt = plain(mel, mel_lens, ids, id_lens, 5)
    logits = hybrid.ctc_head.linear(mel.permute(0, 2, 1))
    ctc = rnnt_amd.ctc_loss(logits, ids.int(), mel_lens.int(), id_lens.int(), blank=5, reduction="mean", backend="torch")
    assert torch.isfinite(ctc) and ctc.item() > 0
    assert abs(got.item() - (0.7 * rnnt.item() + 0.3 * ctc.item())) <= 1e-12 * abs(got.item())
    got.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in hybrid.ctc_head.parameters())
    # the head's decode of the encoder output is the model's
    assert hybrid.ctc_greedy_decode(mel, mel_lens) == hybrid.ctc_head.greedy_decode(mel.permute(0, 2, 1), mel_lens.int(), blank=5)
    with pytest.raises(RuntimeError):
        plain.ctc_greedy_decode(mel, mel_lens)
