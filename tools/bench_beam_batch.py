"""Batched beam search (RNNTModel.beam_search_many -> rnnt_engine_beam_decode_batch) against the sequential loop of
RNNTModel.beam_search over the same utterances, in one process: N different random utterances of T = 1000 frames at the fullcausal
config's widths (ConvPredictor E = 512, O = H = V = 1024), max_length 200, 10 symbols per frame — tools/bench_beam.py's set-up.

Every repetition times beam_search of each utterance on its own (each call ends in its own synchronisation, so the sequential loop
over the first N utterances costs the sum of their times) and then beam_search_many of the first N utterances as ONE batch, for every
N of --ns: both sides of a row come from the same repetitions, alternating.  Reported per row: the median time per utterance of both,
the min - max spread of the sequential loop over the repetitions, and their ratio; then gate 1 (batched below sequential by more than
that spread at N = 8, beam 4) and the smallest N within 10 % of the best batched time per utterance.  Writes the table to --out
(default profiles/beam_batch_bench.txt)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
    ap.add_argument("--beams", default="4,8")
    ap.add_argument("--ns", default="1,2,4,8,16,32")
    ap.add_argument("--blank-biases", default="1.5,3.0")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one-batch", type=int, default=0, metavar="N",
                    help="no timing: beam_search_many of N utterances as one batch, twice, at the first of --beams and --blank-biases — the "
                         "program of a `rocprofv3 --kernel-trace --stats` run (profiles/beam_batch_kernels.txt)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "beam_batch_bench.txt"))
    a = ap.parse_args()
    torch.manual_seed(0)
    T, E, H, V = a.T, 512, 1024, 1024
    ns = [int(n) for n in a.ns.split(",")]
    model = rnnt_amd.RNNTModel(rnnt_amd.ConvPredictor(V, H, E, 0.3), Enc(), rnnt_amd.JointNetwork(-1, -1, H, V)).cuda().eval()
    mels = [torch.randn(1, H, T, device="cuda") for _ in range(max(ns + [a.one_batch]))]
    lens = torch.tensor([T], device="cuda")
    bias0 = model.joint.joint_ln.bias.detach().clone()
    if a.one_batch:
        with torch.no_grad():
            model.joint.joint_ln.bias[V - 1] += float(a.blank_biases.split(",")[0])
        for _ in range(2):
            out = model.beam_search_many(mels[:a.one_batch], beam_size=int(a.beams.split(",")[0]), max_length=200, batch=a.one_batch)
        torch.cuda.synchronize()
        print(f"one batch of {a.one_batch} utterances, T={T}: {[len(o) for o in out]} tokens")
        return
    lines = []

    def say(line=""):
        print(line, flush=True)
        lines.append(line)

    for bb in (float(b) for b in a.blank_biases.split(",")):
        with torch.no_grad():
            model.joint.joint_ln.bias.copy_(bias0)
            model.joint.joint_ln.bias[V - 1] += bb  # blank wins most frames, as in a trained model
        say(f"batched beam search: N random utterances of T={T}, ConvPredictor E={E} O={H}, joint H={H} V={V}, max_length=200, 10 symbols "
            f"per frame, blank bias +{bb}; ms per utterance, median of {a.reps} repetitions after a warm-up ({torch.cuda.get_device_name()})")
        for beam in (int(b) for b in a.beams.split(",")):
            kw = dict(beam_size=beam, max_length=200, return_nbest=True)
            seq = [[] for _ in mels]          # seq[i][r]: beam_search of utterance i alone, repetition r
            bat = {n: [] for n in ns}         # bat[n][r]: beam_search_many of the first n utterances as one batch
            same = True
            for r in range(a.reps + 1):       # repetition 0 warms every shape up and compares the results
                alone = []
                for i, mel in enumerate(mels):
                    t, out = clock(lambda: model.beam_search(mel, lens, **kw))
                    alone.append(out)
                    if r:
                        seq[i].append(t)
                for n in ns:
                    t, out = clock(lambda: model.beam_search_many(mels[:n], batch=n, **kw))
                    if r:
                        bat[n].append(t)
                    else:
                        same = same and out == alone[:n]
            say(f"beam {beam}: batched results equal the sequential ones exactly: {same}")
            per_utt = {}
            for n in ns:
                loop = [sum(seq[i][r] for i in range(n)) / n for r in range(a.reps)]
                s_med, b_med = statistics.median(loop), statistics.median(bat[n]) / n
                per_utt[n] = b_med
                say(f"beam {beam:2d} N {n:2d}: sequential {s_med * 1e3:8.2f} ms (min {min(loop) * 1e3:8.2f}, max {max(loop) * 1e3:8.2f}, spread "
                    f"{(max(loop) - min(loop)) * 1e3:6.2f})   batched {b_med * 1e3:8.2f} ms (min {min(bat[n]) / n * 1e3:8.2f}, max "
                    f"{max(bat[n]) / n * 1e3:8.2f})   sequential / batched {s_med / b_med:5.2f}x")
                if n == 8 and beam == 4:
                    gap, spread = s_med - b_med, max(loop) - min(loop)
                    say(f"    gate 1 (N = 8, beam 4): batched is {gap * 1e3:.2f} ms per utterance below the sequential loop, the loop's spread "
                        f"is {spread * 1e3:.2f} ms: {'PASS' if gap > spread else 'FAIL'}")
            best = min(per_utt.values())
            say(f"    best batched time per utterance {best * 1e3:.2f} ms; smallest N within 10 % of it: "
                f"{min(n for n in ns if per_utt[n] <= 1.1 * best)}")
        say()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
