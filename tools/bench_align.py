"""Forced alignment (rnnt_amd.joint_rnnt_align) against the forward-only loss (rnnt_engine_joint_loss_fwd) on the
same inputs, on the default f16x2 route, at config 2 (B=32, T=1000, U=200, H=512, V=1024) and at the reference's widths (B=8,
T=500, U=100, H=V=1024).  HIP-event medians per call on resident inputs:
  align        joint_rnnt_align (operand producers + joint-forward GEMM + Viterbi sweep + backtrace)
  loss_fwd     rnnt_engine_joint_loss_fwd (the same producers + GEMM + the alpha || beta sweep)
  gemm         the producers + GEMM alone (rnnt_engine_run_stages, stages 0-1)
  align-gemm   what the Viterbi sweep and the backtrace add;  loss-gemm  what the alpha || beta sweep adds
With --kernel-stats CSV (rocprofv3 --kernel-trace --stats over this script), the per-kernel averages of k_viterbi, k_backtrace
and k_lattice_chain are added.  Writes profiles/align_bench.txt (or --out)."""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import rnnt_amd  # noqa: E402
from rnnt_amd import engine  # noqa: E402
from tests.helpers import make_inputs  # noqa: E402

SHAPES = {"cfg2": (32, 1000, 200, 512, 1024), "ref_widths": (8, 500, 100, 1024, 1024)}


def _time(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default=engine.DEFAULT_DTYPE)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append", help="default: every shape")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.txt"))
    args = ap.parse_args()
    lines = [f"# tools/bench_align.py on {torch.cuda.get_device_name(0)}, route {args.dtype}, "
             f"HIP-event medians of {args.reps} calls (ms)",
             f"{'shape':>10} {'B':>3} {'T':>5} {'U':>4} {'H':>5} {'V':>5} {'align':>8} {'loss_fwd':>8} {'gemm':>8} "
             f"{'align-gemm':>10} {'loss-gemm':>9} {'align/loss':>10}"]
    for name in args.shape or list(SHAPES):
        B, T, U, H, V = SHAPES[name]
        d = make_inputs(B, T, U, H, V, seed=1)
        g = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
        a = (g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"])
        outs = engine.alloc_fused_outputs(g["enc"], g["pred"], g["W"])
        t_align = _time(lambda: rnnt_amd.joint_rnnt_align(*a, dtype=args.dtype, check_lengths=False), args.warmup, args.reps)
        t_loss = _time(lambda: engine.joint_loss_fwd(*a, V - 1, dtype=args.dtype), args.warmup, args.reps)
        t_gemm = _time(lambda: engine.joint_loss_fwd_bwd(*a, V - 1, 1.0 / B, outs=outs, dtype=args.dtype, stage_mask=3),
                       args.warmup, args.reps)
        lines.append(f"{name:>10} {B:>3} {T:>5} {U:>4} {H:>5} {V:>5} {t_align:8.3f} {t_loss:8.3f} {t_gemm:8.3f} "
                     f"{t_align - t_gemm:10.3f} {t_loss - t_gemm:9.3f} {t_align / t_loss:10.3f}")
        del g, a, outs
        engine.release_workspaces()
    if args.kernel_stats:
        lines.append("# per-kernel averages (rocprofv3 --kernel-trace --stats over `tools/bench_align.py --shape cfg2 --out ''`)")
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                if any(k in row["Name"] for k in ("k_viterbi", "k_backtrace", "k_lattice_chain", "k_lattice(")):
                    lines.append(f"#   {row['Name']}: {int(row['Calls'])} calls, average {float(row['AverageNs']) / 1e3:.1f} us, "
                                 f"min {float(row['MinNs']) / 1e3:.1f} us, max {float(row['MaxNs']) / 1e3:.1f} us")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
