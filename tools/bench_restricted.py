"""The alignment-restricted loss against the plain fused step at config 2 (B=32, T=1000, U=200, H=512, V=1024),
on the f16x2 and fp32 routes.  Frames: joint_rnnt_align on the same inputs.  Per route the plain step (the existing entry
rnnt_engine_joint_loss_fwd_bwd) and the restricted step at windows (0,0), (5,5), (25,25) and (T,T) run alternated call by call
in one process on the same resident inputs; HIP-event time per fused forward + backward call; median, minimum and maximum over
--reps warm calls of each.  (T,T) restricts nothing: its margin over plain is what the masking pass and the -inf-safe
instantiations cost.  Per window also the share of lattice cells a surviving path can cross (non-zero occupancy; from the
frames, on the host) and, on f16x2, what the backward walked: live dHidden tiles, dW k-steps and 4-cell groups
(engine.x2_live_counts / x2_live_group_counts).  Writes profiles/restricted_bench.txt (or --out); --append FILE copies FILE's
text behind the table (the bench.py runs of parent and this commit, taken in the same session)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rnnt_amd  # noqa: E402
from rnnt_amd import engine  # noqa: E402
from tests.helpers import make_inputs  # noqa: E402

SHAPE = (32, 1000, 200, 512, 1024)


def reachable_share(frames, logit_lens, target_lens, left, right):
    """Cells (t,u) with alpha > -inf and beta > -inf, over all lattice cells.  Blank arcs are free, so column u is reachable
    from the start for t >= lo_u and reaches the end for t <= hi_u: lo_{u+1} = max(lo_u, f_u - left) (needs <= f_u + right),
    hi_u = min(hi_{u+1}, f_u + right) (needs >= f_u - left)."""
    live = total = 0
    for f, Tb, Ub in zip(frames, logit_lens, target_lens):
        Tb, Ub = int(Tb), int(Ub)
        total += Tb * (Ub + 1)
        lo, hi = np.zeros(Ub + 1, dtype=np.int64), np.full(Ub + 1, Tb - 1, dtype=np.int64)
        ok = True
        for u in range(Ub):
            lo[u + 1] = max(lo[u], int(f[u]) - left)
            ok = ok and lo[u + 1] <= min(Tb - 1, int(f[u]) + right)
        for u in range(Ub - 1, -1, -1):
            hi[u] = min(hi[u + 1], int(f[u]) + right)
            ok = ok and hi[u] >= max(0, int(f[u]) - left)
        if ok:
            live += int(np.maximum(hi - lo + 1, 0).sum())
    return live / total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--route", action="append", choices=["f16x2", "fp32"], help="default: both")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restricted_bench.txt"))
    ap.add_argument("--append", help="a text file copied behind the table")
    args = ap.parse_args()
    B, T, U, H, V = SHAPE
    forms = (("plain", None), ("w0", (0, 0)), ("w5", (5, 5)), ("w25", (25, 25)), ("wT", (T, T)))
    d = make_inputs(B, T, U, H, V, seed=1, ragged=False)  # full lengths, as bench.py times config 2
    g = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    a = (g["enc"], g["pred"], g["W"], g["bias"], g["targets"], g["logit_lens"], g["target_lens"], V - 1, 1.0 / B)
    dev = g["enc"].device
    lines = [f"# tools/bench_restricted.py on {torch.cuda.get_device_name(0)}: fused forward + backward at B={B} T={T} U={U} H={H} V={V}, "
             f"full lengths; HIP-event ms over {args.reps} warm calls per form, forms alternated call by call; window (l,r) in frames "
             "around joint_rnnt_align's frames of the same route",
             f"{'route':>6} {'form':>6} {'window':>11} {'median':>9} {'min':>9} {'max':>9} {'/plain':>8} {'reachable':>10} "
             f"{'live_tiles':>16} {'live_ksteps':>16} {'live_groups':>16}"]
    for route in args.route or ["f16x2", "fp32"]:
        _, frames = rnnt_amd.joint_rnnt_align(*a[:7], dtype=route)
        frames_h = frames.cpu().numpy()
        outs = engine.alloc_fused_outputs(g["enc"], g["pred"], g["W"])

        def call(win):
            if win is None:
                engine.joint_loss_fwd_bwd(*a, outs=outs, dtype=route)
            else:
                engine.joint_loss_fwd_bwd_restrict(*a, 0.0, 0.0, frames, win[0], win[1], outs=outs, dtype=route)

        counts, costs = {}, {}
        for _ in range(args.warmup):
            for name, win in forms:
                call(win)
                if name not in counts:  # (the counters belong to the last call: read once per form, outside the timing)
                    costs[name] = outs[0].double().mean().item()
                    counts[name] = dict(engine.x2_live_counts(dev, B, T, U + 1, H, V),
                                        **engine.x2_live_group_counts(dev, B, T, U + 1, H, V)) if route == "f16x2" else None
        ts = {name: [] for name, _ in forms}
        for _ in range(args.reps):
            for name, win in forms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(win)
                e1.record()
                e1.synchronize()
                ts[name].append(e0.elapsed_time(e1))
        med = {n: sorted(v)[len(v) // 2] for n, v in ts.items()}
        for name, win in forms:
            share = 1.0 if win is None else reachable_share(frames_h, d["logit_lens"], d["target_lens"], *win)
            c = counts[name]
            cnt = ["-"] * 3 if c is None else [f"{c['live_tiles']}/{c['tiles']}", f"{c['live_ksteps']}/{c['ksteps']}",
                                               f"{c['live_groups']}/{c['groups']}"]
            lines.append(f"{route:>6} {name:>6} {str(win or '-'):>11} {med[name]:9.3f} {min(ts[name]):9.3f} {max(ts[name]):9.3f} "
                         f"{med[name] / med['plain']:8.4f} {share:10.4f} " + " ".join(f"{x:>16}" for x in cnt) +
                         f"   mean cost {costs[name]:.3f}")
        del outs
        engine.release_workspaces()
    text = "\n".join(lines) + "\n"
    if args.append and os.path.exists(args.append):
        text += "\n" + open(args.append).read()
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
