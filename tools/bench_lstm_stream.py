#!/usr/bin/env python
"""Streaming greedy decode of an LSTMPredictor model at the reference's widths (config/basic_sp.yaml: S = V = 1024, E = Hd = 512,
O = H = 1024, L = 3, layer norm, eps 1e-3; no text_ln), the seeded model and blank-bias recipe of tools/bench_lstm_decode.py: a
1000-frame utterance per stream, pushed 50 frames and 1 frame at a time, every path in one process on one GPU:
  host    greedy_streams(n, device_loop=False): n HostGreedyLoops, one after the other within a push — for n = 1 what
          greedy_stream() of an LSTM model did before the device stream, for n > 1 what a server holding n such streams paid;
  device  greedy_streams(n, device_loop=True): rnnt_engine_greedy_stream_lstm_push, all n streams in lockstep, one synchronisation
          per push.
n = 1, 4, 8, 16, 32; every stream of a group gets frames in every push (its own utterance).  A run is the whole utterance: a host
clock around each push (a push ends in its own synchronisation), summed; the two paths alternate run by run, the first run of each is
dropped as warm-up.  Printed: the median over runs of the time per utterance and per stream, and the median over all pushes of all
runs of the time per push.  The frames are encoder outputs (PassThroughEncoder of the tests): the encoder is not measured.

    python tools/bench_lstm_stream.py [--reps 10] [--out profiles/lstm_stream_bench.txt]
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
GROUPS = (1, 4, 8, 16, 32)
T = 1000
PUSHES = (50, 1)


def run(model, mels, push, device_loop):
    """One utterance per stream, `push` frames at a time: (token lists, [ms per push])."""
    group = model.greedy_streams(len(mels), max_length=None, device_loop=device_loop)
    torch.cuda.synchronize()
    times = []
    for t in range(0, T, push):
        chunks = [m[..., t:t + push] for m in mels]
        t0 = time.perf_counter()
        group.push_encoded(chunks)
        times.append((time.perf_counter() - t0) * 1e3)
    assert group.last_path == ("lstm_stream" if device_loop else "host") and group.frames == [T] * len(mels)
    return group.tokens, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lstm_stream needs a HIP device"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/bench_lstm_stream.py on {torch.cuda.get_device_name(0)}; ms; S = V = {S}, E = Hd = {HD}, O = H = {O}, L = {L}, layer norm, "
        f"eps {EPS}, no text_ln; T = {T} frames per stream; launches per iteration: {5 + 2 * L}")
    torch.manual_seed(1)
    pred = rnnt_amd.LSTMPredictor(S, O, E, L, HD, lstm_layer_norm=True, lstm_layer_norm_epsilon=EPS, lstm_dropout=0.3)
    joint = rnnt_amd.JointNetwork(-1, -1, O, S)
    model = rnnt_amd.RNNTModel(pred, PassThroughEncoder(), joint).cuda().eval()
    g = torch.Generator().manual_seed(2)
    mels = [(torch.randn(1, O, T, generator=g) * 2.0).cuda() for _ in range(max(GROUPS))]
    lens = torch.tensor([T]).cuda()

    # the blank's bias at which the first utterance emits closest to 200 labels (tools/bench_lstm_decode.py's recipe)
    base = joint.joint_ln.bias.data[joint.blank_idx].item()
    best = None
    for step in range(0, 41):
        joint.joint_ln.bias.data[joint.blank_idx] = base + 0.25 * step
        n = len(model.greedy_decode(mels[0], lens, max_length=T + 1, device_loop=True))
        if best is None or abs(n - 200) < abs(best[1] - 200):
            best = (step, n)
        if n < 100:
            break
    joint.joint_ln.bias.data[joint.blank_idx] = base + 0.25 * best[0]
    say(f"blank bias raised by {0.25 * best[0]:.2f}: {best[1]} labels in the first utterance")
    want = [model.greedy_decode(m, lens, max_length=T + 1, device_loop=True) for m in mels[:4]]

    verdict = []
    for push in PUSHES:
        say(f"pushes of {push} frame{'s' if push > 1 else ''} ({T // push} pushes per utterance)")
        for n in GROUPS:
            reps = {True: a.reps, False: a.reps if n <= 4 else max(3, a.reps // 3)}  # (a host run of 32 streams takes seconds)
            total, per_push = {True: [], False: []}, {True: [], False: []}
            for r in range(a.reps + 1):  # alternated; run 0 of each path is the warm-up
                for path in ((False, True) if r % 2 == 0 else (True, False)):
                    if r > reps[path]:
                        continue
                    tokens, times = run(model, mels[:n], push, path)
                    assert tokens[:4] == want[:min(n, 4)], "a stream's token list differs from the offline decode"
                    if r > 0:
                        total[path].append(sum(times))
                        per_push[path] += times
            th, td = statistics.median(total[False]), statistics.median(total[True])
            ph, pd = statistics.median(per_push[False]), statistics.median(per_push[True])
            say(f"    n = {n:2d}: host {th:8.2f} ms = {th / n:7.2f} per stream, {ph:7.3f} per push (runs {len(total[False])}); "
                f"device {td:8.2f} ms = {td / n:7.2f} per stream, {pd:7.3f} per push (runs {len(total[True])}); host / device = {th / td:.2f}")
            verdict.append((push, n, th / td))
    worst = min(verdict, key=lambda v: v[2])
    say(f"# smallest host / device ratio: {worst[2]:.2f} (pushes of {worst[0]}, n = {worst[1]}); "
        f"the device stream is {'at or below' if worst[2] >= 1.0 else 'NOT at or below'} the host stream's time at every timed shape")
    say("# not measured: other widths, text_ln, ragged pushes (streams with different counts or sitting out), other label rates, "
        "the kernels one by one, an encoder in front")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
