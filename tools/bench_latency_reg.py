"""FastEmit and the delay penalty against the plain fused step, on the default f16x2 route, at config 2
(B=32, T=1000, U=200, H=512, V=1024) and at the reference-width shape of profiles/r06_small_shapes.txt (B=4, T=400, U=100,
H=V=1024).  Per shape the four forms run alternated in one process on the same resident inputs (plain = the existing entry
rnnt_engine_joint_loss_fwd_bwd; fastemit = lambda 0.01; delay = delta 0.001; both), HIP-event time per fused
forward + backward call, median over --reps warm calls of each.  Target: the regularised step at config 2 <= 1.02x plain.
Writes profiles/latency_reg_bench.txt (or --out)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rnnt_amd import engine  # noqa: E402
from tests.helpers import make_inputs  # noqa: E402

SHAPES = {"cfg2": (32, 1000, 200, 512, 1024), "ref_small": (4, 400, 100, 1024, 1024)}
FORMS = (("plain", 0.0, 0.0), ("fastemit", 0.01, 0.0), ("delay", 0.0, 0.001), ("both", 0.01, 0.001))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default=engine.DEFAULT_DTYPE)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append", help="default: every shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latency_reg_bench.txt"))
    args = ap.parse_args()
    lines = [f"# tools/bench_latency_reg.py on {torch.cuda.get_device_name(0)}, route {args.dtype}: fused forward + backward, "
             f"full lengths, HIP-event medians of {args.reps} warm calls per form, forms alternated call by call (ms)",
             f"{'shape':>10} {'B':>3} {'T':>5} {'U':>4} {'H':>5} {'V':>5} " + " ".join(f"{f:>9}" for f, _, _ in FORMS) +
             " " + " ".join(f"{f + '/plain':>15}" for f, _, _ in FORMS[1:])]
    for name in args.shape or list(SHAPES):
        B, T, U, H, V = SHAPES[name]
        d = make_inputs(B, T, U, H, V, seed=1, ragged=False)  # full lengths, as bench.py times config 2
        g = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
        a = (g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"], V - 1, 1.0 / B)
        outs = engine.alloc_fused_outputs(g["enc"], g["pred"], g["W"])

        def call(lam, dp):
            if lam or dp:
                engine.joint_loss_fwd_bwd_reg(*a, lam, dp, outs=outs, dtype=args.dtype)
            else:
                engine.joint_loss_fwd_bwd(*a, outs=outs, dtype=args.dtype)

        for _ in range(args.warmup):
            for _, lam, dp in FORMS:
                call(lam, dp)
        ts = {f: [] for f, _, _ in FORMS}
        for _ in range(args.reps):
            for f, lam, dp in FORMS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(lam, dp)
                e1.record()
                e1.synchronize()
                ts[f].append(e0.elapsed_time(e1))
        med = {f: sorted(v)[len(v) // 2] for f, v in ts.items()}
        lines.append(f"{name:>10} {B:>3} {T:>5} {U:>4} {H:>5} {V:>5} " + " ".join(f"{med[f]:9.3f}" for f, _, _ in FORMS) +
                     " " + " ".join(f"{med[f] / med['plain']:15.4f}" for f, _, _ in FORMS[1:]))
        del g, a, outs
        engine.release_workspaces()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
