"""Beam search with and without a context graph (RNNTModel.beam_search / beam_search_many with context=ContextGraph(...): C ABI
rnnt_engine_beam_decode_ctx / _batch_ctx; DESIGN.md §4h "Context"), in one process: tools/bench_beam.py's set-up — random utterances of
T = 1000 frames at the fullcausal config's widths (ConvPredictor E = 512, O = H = V = 1024), max_length 200, 10 symbols per frame, its
three blank biases — beam 4, 100 random phrases of 2 - 5 tokens.

Per blank bias and N (1: beam_search; 8, 32: beam_search_many as one batch), ms per utterance, median of --reps repetitions that
alternate the three searches:
    plain     no graph: today's kernels
    same      the graph at a boost of 1e-6 per token: the context kernels on (within fp64 noise) the SAME search, so the difference to
              `plain` is what the re-ranking tail of k_beam_reduce and the step of k_beam_select cost per round
    boosted   the graph at --score: the search a caller gets — it keeps other hypotheses, so it runs other rounds
Writes the table to --out (default profiles/beam_context_bench.txt)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rnnt_amd  # noqa: E402


class Enc(torch.nn.Module):
    def forward(self, x):
        return x  # (1, H, T) already

    def calc_output_lens(self, lens):
        return lens


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--beam", type=int, default=4)
    ap.add_argument("--ns", default="1,8,32")
    ap.add_argument("--blank-biases", default="1.5,0.0,3.0")
    ap.add_argument("--phrases", type=int, default=100)
    ap.add_argument("--score", type=float, default=1.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "beam_context_bench.txt"))
    a = ap.parse_args()
    torch.manual_seed(0)
    T, E, H, V = a.T, 512, 1024, 1024
    ns = [int(n) for n in a.ns.split(",")]
    model = rnnt_amd.RNNTModel(rnnt_amd.ConvPredictor(V, H, E, 0.3), Enc(), rnnt_amd.JointNetwork(-1, -1, H, V)).cuda().eval()
    mels = [torch.randn(1, H, T, device="cuda") for _ in range(max(ns))]
    lens = torch.tensor([T], device="cuda")
    rng = np.random.default_rng(0)
    phrases = [tuple(int(k) for k in rng.integers(0, V - 1, rng.integers(2, 6))) for _ in range(a.phrases)]
    graphs = {"plain": None, "same": rnnt_amd.ContextGraph(phrases, 1e-6), "boosted": rnnt_amd.ContextGraph(phrases, a.score)}
    bias0 = model.joint.joint_ln.bias.detach().clone()
    lines = []

    def say(line=""):
        print(line, flush=True)
        lines.append(line)

    g = graphs["boosted"]
    say(f"beam search with a context graph: {a.phrases} random phrases of 2 - 5 tokens ({g.n_nodes} nodes, {len(g.children[0])} children of "
        f"the root), boost {a.score} per token; beam {a.beam}, T={T}, ConvPredictor E={E} O={H}, joint H={H} V={V}, max_length=200, 10 "
        f"symbols per frame; ms per utterance, median of {a.reps} repetitions after a warm-up ({torch.cuda.get_device_name()})")
    for bb in (float(b) for b in a.blank_biases.split(",")):
        with torch.no_grad():
            model.joint.joint_ln.bias.copy_(bias0)
            model.joint.joint_ln.bias[V - 1] += bb  # blank wins most frames, as in a trained model
        say(f"blank bias +{bb}")
        for n in ns:
            kw = dict(beam_size=a.beam, max_length=200, return_nbest=True)
            if n == 1:
                run = lambda g: [model.beam_search(mels[0], lens, context=g, **kw)]  # noqa: E731
            else:
                run = lambda g: model.beam_search_many(mels[:n], batch=n, context=g, **kw)  # noqa: E731
            ts, outs = {k: [] for k in graphs}, {}
            for r in range(a.reps + 1):  # repetition 0 warms every shape up
                for k, g in graphs.items():
                    t, outs[k] = clock(lambda: run(g))
                    if r:
                        ts[k].append(t / n)
            med = {k: statistics.median(v) for k, v in ts.items()}
            same = sum([y for y, _ in a_] == [y for y, _ in b_] for a_, b_ in zip(outs["plain"], outs["same"]))
            moved = sum(a_[0][0] != b_[0][0] for a_, b_ in zip(outs["plain"], outs["boosted"]))
            say(f"  N {n:2d}: plain {med['plain'] * 1e3:8.2f} ms (min {min(ts['plain']) * 1e3:8.2f}, max {max(ts['plain']) * 1e3:8.2f})   "
                f"same {med['same'] * 1e3:8.2f} ms ({med['same'] / med['plain']:5.3f}x plain; {same}/{n} n-best lists equal plain's)   "
                f"boosted {med['boosted'] * 1e3:8.2f} ms ({med['boosted'] / med['plain']:5.3f}x plain; best hypothesis changed in {moved}/{n})")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
