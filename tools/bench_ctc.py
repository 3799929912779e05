"""The CTC head on the engine against the same operators through torch on the same device and inputs.
HIP-event medians per call on resident inputs (ms):
  loss     rnnt_amd.ctc_loss(reduction="mean") forward + backward, backend="engine" (rnnt_engine_ctc_loss_fwd_bwd) against
           backend="torch" (log_softmax + torch.nn.functional.ctc_loss), at BASELINE config 2's and config 4's (N, T, U, V) and
           at one ragged batch;
  greedy   rnnt_amd.ctc_greedy_decode, backend="engine" (two launches, one synchronisation) against backend="torch" (argmax
           on the device, the collapse on the host), at the same shapes;
  step     forward + backward of an RNNTModel (stand-in encoder, rnnt_amd.ConvPredictor, JointNetwork, CTCHead) with
           ctc_weight 0 and 0.3.
Writes profiles/ctc_bench.txt (or --out).  Needs an MI355X; there is no fallback."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rnnt_amd  # noqa: E402
from tests import ctc_cases  # noqa: E402

# (N, T, U, V, ragged): BASELINE.md config 2 and config 4, and a batch with lengths between half and all of the padding
SHAPES = {"cfg2": (32, 1000, 200, 1024, False), "cfg4": (8, 4000, 600, 1024, False), "ragged": (16, 800, 150, 1024, True)}


def _time(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def _inputs(N, T, U, V, ragged, seed=1):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((N, T, V)).astype(np.float32)).cuda()
    tg = torch.from_numpy(ctc_cases.make_targets(rng, N, U, V, V - 1, repeat_p=0.1)).cuda()
    ll, tl = np.full(N, T), np.full(N, U)
    if ragged:
        ll, tl = rng.integers(T // 2, T + 1, N), rng.integers(U // 2, U + 1, N)
        ll[0], tl[0] = T, U
    return x, tg, torch.from_numpy(ll.astype(np.int32)).cuda(), torch.from_numpy(tl.astype(np.int32)).cuda()


def _loss_step(x, tg, ll, tl, backend):
    x.grad = None
    rnnt_amd.ctc_loss(x, tg, ll, tl, reduction="mean", check_lengths=False, backend=backend).backward()


class _Encoder(torch.nn.Module):
    def __init__(self, n_mels, feats):
        super().__init__()
        self.c1 = torch.nn.Conv1d(n_mels, feats, 3, stride=2, padding=1)
        self.c2 = torch.nn.Conv1d(feats, feats, 3, stride=2, padding=1)

    def forward(self, x):
        return self.c2(torch.relu(self.c1(x)))

    def calc_output_lens(self, lens):
        return ((lens + 1) // 2 + 1) // 2


def _model_step(model, batch, blank):
    model.zero_grad(set_to_none=True)
    model(*batch, blank).backward()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append", help="default: every shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_ctc.py needs a HIP device"
    lines = [f"# tools/bench_ctc.py on {torch.cuda.get_device_name(0)}: HIP-event median (min .. max) of {args.reps} calls, ms",
             f"{'what':>7} {'shape':>7} {'N':>3} {'T':>5} {'U':>4} {'V':>5} {'engine':>26} {'torch':>26} {'torch/engine':>12}"]
    for name in args.shape or list(SHAPES):
        N, T, U, V, ragged = SHAPES[name]
        x, tg, ll, tl = _inputs(N, T, U, V, ragged)
        # the two backends compute the same loss on these inputs (the bars of tests/test_ctc_gpu.py are checked there)
        a = rnnt_amd.ctc_loss(x, tg, ll, tl, backend="engine").item()
        b = rnnt_amd.ctc_loss(x, tg, ll, tl, backend="torch").item()
        assert abs(a - b) <= 1e-3 * abs(b), (name, a, b)
        x.requires_grad_(True)
        te = _time(lambda: _loss_step(x, tg, ll, tl, "engine"), args.warmup, args.reps)
        tt = _time(lambda: _loss_step(x, tg, ll, tl, "torch"), args.warmup, args.reps)
        fmt = lambda t: f"{t[0]:9.3f} ({t[1]:.3f} .. {t[2]:.3f})"  # noqa: E731
        lines.append(f"{'loss':>7} {name:>7} {N:>3} {T:>5} {U:>4} {V:>5} {fmt(te):>26} {fmt(tt):>26} {tt[0] / te[0]:>12.2f}")
        x.requires_grad_(False)
        ge = rnnt_amd.ctc_greedy_decode(x, ll, backend="engine")
        assert ge == rnnt_amd.ctc_greedy_decode(x, ll, backend="torch")
        te = _time(lambda: rnnt_amd.ctc_greedy_decode(x, ll, backend="engine"), args.warmup, args.reps)
        tt = _time(lambda: rnnt_amd.ctc_greedy_decode(x, ll, backend="torch"), args.warmup, args.reps)
        lines.append(f"{'greedy':>7} {name:>7} {N:>3} {T:>5} {U:>4} {V:>5} {fmt(te):>26} {fmt(tt):>26} {tt[0] / te[0]:>12.2f}")
        print("\n".join(lines[-2:]), flush=True)
        del x, tg
        rnnt_amd.engine.release_workspaces()
    # a training step with and without the CTC branch: N = 8, 1000 mel frames -> 250 encoder frames, U = 50, H = 512, V = 1024
    torch.manual_seed(0)
    vocab, feats, n_mels = 1024, 512, 80
    model = rnnt_amd.RNNTModel(rnnt_amd.ConvPredictor(vocab, feats, 512, dropout=0.0), _Encoder(n_mels, feats),
                               rnnt_amd.JointNetwork(-1, -1, feats, vocab)).cuda()
    model.ctc_head = rnnt_amd.CTCHead(feats, vocab).cuda()
    g = torch.Generator().manual_seed(1)
    batch = (torch.randn(8, n_mels, 1000, generator=g).cuda(), torch.full((8,), 1000).cuda(),
             torch.randint(0, vocab - 1, (8, 50), generator=g).cuda(), torch.full((8,), 50).cuda())
    lines.append(f"# RNNTModel forward + backward, N=8, 250 encoder frames, U=50, H={feats}, V={vocab} (f16x2 route), ms")
    for w in (0.0, 0.3):
        model.ctc_weight = w
        t = _time(lambda: _model_step(model, batch, vocab - 1), args.warmup, args.reps)
        lines.append(f"{'step':>7} ctc_weight {w:.1f}: {t[0]:9.3f} ({t[1]:.3f} .. {t[2]:.3f})")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
