#!/usr/bin/env python
"""Greedy decoding of an LSTMPredictor model at the reference's widths (config/basic_sp.yaml: S = V = 1024, E = Hd = 512, O = H = 1024,
L = 3, layer norm, eps 1e-3; no text_ln), seeded, every path in one process on one GPU, medians of host-clock times around the call
(each decode ends in its own synchronisation), the paths alternating:
  host     greedy_decode(device_loop=False): the host loop with the engine's predictor step and scan — the path before the device loop;
  loop     greedy_decode(device_loop=True): rnnt_engine_greedy_decode_lstm with one utterance;
  many N   greedy_decode_many(batch=N) of N utterances of the same length, N = 4, 8, 16, 32, against N single `loop` decodes.
Two lengths: T = 1000 frames with about 200 labels (the blank's bias is raised until the seeded model emits about one label per five
frames; the label counts are printed) and T = 100 of the same model.  Also printed: the iterations that did work (state word 5),
the launches per iteration (5 + 2 L without text_ln) and the time per iteration.  The frames are encoder outputs (PassThroughEncoder
of the tests): the encoder is not part of the measurement.

    python tools/bench_lstm_decode.py [--reps 10] [--out profiles/lstm_decode_bench.txt]
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
from tests.stream_models import PassThroughEncoder  # noqa: E402

S, E, HD, O, L, EPS = 1024, 512, 512, 1024, 3, 1e-3
BATCHES = (4, 8, 16, 32)


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lstm_decode needs a HIP device"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/bench_lstm_decode.py on {torch.cuda.get_device_name(0)}; medians of n calls, ms; S = V = {S}, E = Hd = {HD}, O = H = {O}, "
        f"L = {L}, layer norm, eps {EPS}, no text_ln; launches per iteration: {5 + 2 * L}")
    torch.manual_seed(1)
    pred = rnnt_amd.LSTMPredictor(S, O, E, L, HD, lstm_layer_norm=True, lstm_layer_norm_epsilon=EPS, lstm_dropout=0.3)
    joint = rnnt_amd.JointNetwork(-1, -1, O, S)
    model = rnnt_amd.RNNTModel(pred, PassThroughEncoder(), joint).cuda().eval()
    g = torch.Generator().manual_seed(2)
    mels = {T: [(torch.randn(1, O, T, generator=g) * 2.0).cuda() for _ in range(max(BATCHES))] for T in (1000, 100)}
    lens = {T: torch.tensor([T]).cuda() for T in mels}
    ml = 1001  # no cap: the label count is the model's

    # the blank's bias at which the first utterance of T = 1000 emits closest to 200 labels
    base = joint.joint_ln.bias.data[joint.blank_idx].item()
    best = None
    for step in range(0, 41):
        joint.joint_ln.bias.data[joint.blank_idx] = base + 0.25 * step
        n = len(model.greedy_decode(mels[1000][0], lens[1000], max_length=ml, device_loop=True))
        if best is None or abs(n - 200) < abs(best[1] - 200):
            best = (step, n)
        if n < 100:
            break
    joint.joint_ln.bias.data[joint.blank_idx] = base + 0.25 * best[0]
    say(f"blank bias raised by {0.25 * best[0]:.2f}: {best[1]} labels in the first utterance of T = 1000")

    for T in (1000, 100):
        ms, ln = mels[T], lens[T]
        paths = {"host": dict(device_loop=False), "loop": dict(device_loop=True)}
        want = [model.greedy_decode(m, ln, max_length=ml, device_loop=False) for m in ms[:4]]
        assert [model.greedy_decode(m, ln, max_length=ml, device_loop=True) for m in ms[:4]] == want, "the two paths' token lists differ"
        labels = [len(w) for w in want]
        res = {k: [] for k in paths}
        for _ in range(2):  # alternated
            for k, kw in paths.items():
                res[k].append(statistics.mean(timed(lambda m=m: model.greedy_decode(m, ln, max_length=ml, **kw), a.reps if k == "loop" else max(3, a.reps // 3))
                                              for m in ms[:4]))
                assert model.last_decode_path == ("lstm_loop" if k == "loop" else "host")
        t_host, t_loop = min(res["host"]), min(res["loop"])
        state = rnnt_amd.engine.greedy_decode_lstm([model._decode_frames(model.encoder(ms[0]).permute(0, 2, 1))], pred._decode_bundle(), None, None,
                                                   joint.joint_ln.weight, joint.joint_ln.bias, joint.blank_idx, ml)[0]
        its = int(state[0, 5]) + 1  # + the iteration in which the last label is taken in / the utterance settles
        say(f"T = {T}, labels {labels} (first four utterances), n = {a.reps}: host {t_host:.2f} ms (runs {', '.join('%.2f' % v for v in res['host'])}); "
            f"loop, n_utt = 1: {t_loop:.2f} ms (runs {', '.join('%.2f' % v for v in res['loop'])}); host / loop = {t_host / t_loop:.2f}")
        say(f"    loop, first utterance: {its} iterations, {5 + 2 * L} launches each, {1e3 * t_loop / its:.1f} us per iteration "
            f"(host clock of the whole call over the iterations)")
        single = {}
        for N in BATCHES:
            t_many, t_singles = [], []
            for _ in range(2):  # alternated
                t_many.append(timed(lambda: model.greedy_decode_many(ms[:N], max_length=ml, batch=N), a.reps))
                assert model.last_decode_path == "lstm_loop"
                t_singles.append(timed(lambda: [model.greedy_decode(m, ln, max_length=ml, device_loop=True) for m in ms[:N]], max(2, a.reps // 3)))
            single[N] = min(t_many) / N
            say(f"    many, batch = {N:2d}: {min(t_many):.2f} ms = {min(t_many) / N:.3f} ms per utterance (runs {', '.join('%.2f' % v for v in t_many)}); "
                f"{N} single loop decodes {min(t_singles):.2f} ms = {min(t_singles) / N:.3f} per utterance; single / many = {min(t_singles) / min(t_many):.2f}")
        lo = min(single.values())
        say(f"    smallest batch within 10 % of the best time per utterance ({lo:.3f} ms): {min(N for N, v in single.items() if v <= 1.1 * lo)}")
    say("# not measured: the kernels one by one, other widths, text_ln, ragged batches, ordering a list by length")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
