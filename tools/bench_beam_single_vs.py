"""Gate 2 of the batched beam search: the single search (RNNTModel.beam_search, tools/bench_beam.py) of THIS tree against another
checkout's (--other DIR: the parent commit, built), as fresh child processes alternated on the same device — other, this, other, this,
... (--pairs of them).  Writes every run's medians, the difference of the means per beam and both trees' run-to-run ranges to --out
(default profiles/beam_batch_gate2.txt); the gate's bound is --spread-ms, the sequential loop's min - max spread that
tools/bench_beam_batch.py measured (N = 8, beam 4, profiles/beam_batch_bench.txt).  A child that fails or outlasts --timeout ends the comparison."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(tree, a, tmp):
    out = os.path.join(tmp, "rows.txt")
    subprocess.run([sys.executable, os.path.join(tree, "tools", "bench_beam.py"), "--host-beams", "", "--beams", a.beams, "--blank-bias",
                    str(a.blank_bias), "--reps", str(a.reps), "--out", out], cwd=tree, check=True, timeout=a.timeout, stdout=subprocess.DEVNULL)
    rows = {}
    for line in open(out):
        m = re.match(r"beam\s+(\d+): device\s+([\d.]+) ms", line)
        if m:
            rows[int(m.group(1))] = float(m.group(2))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True, help="a built checkout of the commit to compare with")
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--beams", default="1,4,8,16")
    ap.add_argument("--blank-bias", type=float, default=1.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=float, default=120.0)
    ap.add_argument("--spread-ms", type=float, default=0.33, help="the gate's bound: the sequential loop's measured min - max spread")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_batch_gate2.txt"))
    a = ap.parse_args()
    other, this = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(a.pairs):
            other.append(run(os.path.abspath(a.other), a, tmp))
            this.append(run(ROOT, a, tmp))
    lines = [f"single beam search (tools/bench_beam.py: T=1000, E=512, O=H=V=1024, max_length=200, blank bias +{a.blank_bias}; median ms of "
             f"{a.reps} runs per process), the parent commit's against this one's: {a.pairs} pairs of fresh processes, alternated "
             "(parent, this, parent, this, ...)"]
    ok = True
    for beam in sorted(this[0]):
        o, t = [r[beam] for r in other], [r[beam] for r in this]
        diff = sum(t) / len(t) - sum(o) / len(o)
        ok = ok and diff <= a.spread_ms
        lines.append(f"beam {beam:2d}: parent {' / '.join(f'{x:7.2f}' for x in o)} ms   this commit {' / '.join(f'{x:7.2f}' for x in t)} ms   "
                     f"difference of the means {diff:+6.2f} ms ({diff / (sum(o) / len(o)) * 100:+5.2f} %)   run-to-run range: parent "
                     f"{max(o) - min(o):4.2f}, this {max(t) - min(t):4.2f} ms")
    lines.append(f"gate 2 (this commit not slower than the parent by more than the sequential loop's spread, {a.spread_ms} ms, at every beam): "
                 f"{'PASS' if ok else 'FAIL'}")
    print("\n".join(lines), flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
