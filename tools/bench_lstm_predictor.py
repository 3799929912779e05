#!/usr/bin/env python
"""LSTMPredictor on the engine against the same module's torch path (rnnt_amd/lstm_predictor.py) at the reference's sizes
(config/basic_sp.yaml: S = 1024, E = Hd = 512, O = 1024, L = 3, layer norm, eps 1e-3, dropout 0.3), seeded, both paths in one process
on one GPU, medians of host-clock times around a device synchronise (the number of calls behind each median is printed with it), the
two paths alternating:
  training forward + backward (train mode, p = 0.3, masks drawn per call on either path) at B = 4, U1 = 101 and B = 32, U1 = 201;
  inference forward (eval mode, no_grad) at the same two shapes;
  the decode step: U1 = 1 with a state at B = 1.
Also printed: the engine's launches per call (from the launch sequence of rnnt_amd/csrc/lstm.hip), the torch path's kernel count of
one call (torch.profiler; n/a where the profiler is not available) and the largest difference between the two paths' outputs.

    python tools/bench_lstm_predictor.py [--reps 30] [--out profiles/lstm_predictor_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rnnt_amd  # noqa: E402

S, E, HD, O, L, EPS, P = 1024, 512, 512, 1024, 3, 1e-3, 0.3


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def engine_launches(U1, train, with_state, backward):
    """Kernel launches of one call (lstm.hip): forward = embedding + LayerNorm, per layer the x2g GEMM, (training) the initial-state
    rows, per step the recurrent GEMM (none at step 0 from zero state) and the row kernel, then linear and LayerNorm; backward =
    5 for the output LayerNorm and linear + 1 dx GEMM, per layer per step the row kernel and (t > 0) the recurrent GEMM, 2 + 2
    weight-gradient launches, 2 + 2 affine column sums, the dx GEMM; then 4 for the input LayerNorm and the embedding."""
    fwd = 1 + L * (1 + (1 if train else 0) + 2 * U1 - (0 if with_state else 1)) + 2
    bwd = 0
    if backward:
        bwd = 3 + 3 + 1 + L * (2 * U1 - 1 + 2 + 2 + 4 + 1) + 2 + 1 + 1
    return fwd, bwd


def torch_kernels(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages() if getattr(e, "device_type", None) is not None
                   and "cuda" in str(e.device_type).lower())
    except Exception as exc:  # the count is an extra: the timings stand without it
        return f"n/a ({type(exc).__name__})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-profiler", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lstm_predictor needs a HIP device"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/bench_lstm_predictor.py on {torch.cuda.get_device_name(0)}; medians (min) of n calls, ms; "
        f"S = {S}, E = Hd = {HD}, O = {O}, L = {L}, layer norm, eps {EPS}, p = {P}")
    torch.manual_seed(1)
    m = rnnt_amd.LSTMPredictor(S, O, E, L, HD, lstm_layer_norm=True, lstm_layer_norm_epsilon=EPS, lstm_dropout=P).cuda()
    g = torch.Generator().manual_seed(2)

    def case(label, B, U1, train, with_state, reps):
        ids = torch.randint(0, S, (B, U1), generator=g).cuda()
        lens = torch.full((B,), U1).cuda()
        G = torch.randn(B, U1, O, generator=g).cuda()
        state = None
        if with_state:
            state = [[torch.randn(B, HD, generator=g).cuda() * 0.5, torch.randn(B, HD, generator=g).cuda()] for _ in range(L)]
        m.train(train)

        def run():
            if train:
                m.zero_grad(set_to_none=True)
                out = m(ids, lens, state)[0]
                (out * G).sum().backward()
                return out
            with torch.no_grad():
                return m(ids, lens, state)[0]
        res = {}
        for backend in ("torch", "engine", "torch", "engine"):
            m.backend = backend
            m.eval()
            with torch.no_grad():
                y = m(ids, lens, state)[0].clone()  # eval-mode output of the path: the two are compared below
            m.train(train)
            res.setdefault(backend, []).append(median_ms(run, reps) + (y,))
            assert m.last_backend == backend
        t_t, t_e = min(r[0] for r in res["torch"]), min(r[0] for r in res["engine"])
        diff = (res["torch"][0][2] - res["engine"][0][2]).abs().max().item()
        fwd, bwd = engine_launches(U1, train, with_state, train)
        m.backend = "torch"
        nk = "not counted (see the smaller shape)" if a.no_profiler or B * U1 > 404 else torch_kernels(run)
        say(f"{label} B = {B}, U1 = {U1}, n = {reps}: torch {t_t:.3f} ms  (runs {', '.join('%.3f (%.3f)' % r[:2] for r in res['torch'])}); "
            f"engine {t_e:.3f} ms  (runs {', '.join('%.3f (%.3f)' % r[:2] for r in res['engine'])}); torch / engine = {t_t / t_e:.2f}; "
            f"max|engine - torch| = {diff:.2e}")
        say(f"    launches per call: engine {fwd} forward" + (f" + {bwd} backward" if train else "")
            + f" (2 per step and layer); torch path kernels: {nk}")

    case("training forward + backward,", 4, 101, True, False, a.reps)
    case("training forward + backward,", 32, 201, True, False, max(5, a.reps // 3))
    case("inference forward,", 4, 101, False, False, a.reps)
    case("inference forward,", 32, 201, False, False, max(5, a.reps // 3))
    case("decode step (state in),", 1, 1, False, True, a.reps * 10)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
