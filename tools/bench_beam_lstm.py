#!/usr/bin/env python
"""Beam search of an LSTMPredictor model at the reference's widths (config/basic_sp.yaml: S = V = 1024, E = Hd = 512, O = H = 1024,
L = 3, layer norm, eps 1e-3; no text_ln), the seeded model and the blank-bias recipe of tools/bench_lstm_decode.py, every path in one
process on one GPU, medians of host-clock times around the call (each search ends in its own synchronisation), the paths alternating:
  host     beam_search(device_search=False): the host loop, one engine predictor step per new hypothesis from its parent's cached state;
  device   beam_search(device_search=True): rnnt_engine_beam_decode_lstm with one utterance;
  many N   beam_search_many(batch=N) of N utterances of the same length, N = 4, 8, 16, 32, against N single `device` searches.
T = 1000 and T = 100 frames, beam 4 and 8.  Also printed: the rounds that did work (state word 5), the launches per round
(6 + 2 L without text_ln: every round enqueues them all, the predictor's return at once in a round without a new label) and the
time per round.  The frames are encoder outputs (PassThroughEncoder of the tests): the encoder is not part of the measurement.

    python tools/bench_beam_lstm.py [--reps 5] [--host-reps 2] [--out profiles/beam_lstm_bench.txt]
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
BEAMS = (4, 8)


def timed(fn, reps, warmup=1):
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_beam_lstm needs a HIP device"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:  # (kept up to date: a long run leaves what it has measured)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    launches = 6 + 2 * L
    say(f"# tools/bench_beam_lstm.py on {torch.cuda.get_device_name(0)}; medians of n calls, ms; S = V = {S}, E = Hd = {HD}, O = H = {O}, "
        f"L = {L}, layer norm, eps {EPS}, no text_ln; launches per round: {launches}")
    torch.manual_seed(1)
    pred = rnnt_amd.LSTMPredictor(S, O, E, L, HD, lstm_layer_norm=True, lstm_layer_norm_epsilon=EPS, lstm_dropout=0.3)
    joint = rnnt_amd.JointNetwork(-1, -1, O, S)
    model = rnnt_amd.RNNTModel(pred, PassThroughEncoder(), joint).cuda().eval()
    g = torch.Generator().manual_seed(2)
    mels = {T: [(torch.randn(1, O, T, generator=g) * 2.0).cuda() for _ in range(max(BATCHES))] for T in (1000, 100)}
    lens = {T: torch.tensor([T]).cuda() for T in mels}
    ml = 1001  # no cap: the label count is the model's

    # the blank's bias at which the first utterance of T = 1000 emits closest to 200 labels (greedy; tools/bench_lstm_decode.py)
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
    say(f"blank bias raised by {0.25 * best[0]:.2f}: {best[1]} greedy labels in the first utterance of T = 1000")

    wins, pick = [], {}
    for T in (1000, 100):
        ms, ln = mels[T], lens[T]
        for beam in BEAMS:
            kw = dict(beam_size=beam, max_length=ml)
            dev = model.beam_search(ms[0], ln, device_search=True, **kw)
            assert model.last_beam_path == "lstm_device"
            host = model.beam_search(ms[0], ln, device_search=False, **kw)
            assert model.last_beam_path == "host"
            res = {"host": [], "device": []}
            for _ in range(2):  # alternated
                res["host"].append(timed(lambda: model.beam_search(ms[0], ln, device_search=False, **kw), a.host_reps, warmup=0))
                res["device"].append(statistics.mean(timed(lambda m=m: model.beam_search(m, ln, device_search=True, **kw), a.reps) for m in ms[:4]))
            t_host, t_dev = min(res["host"]), min(res["device"])
            wins.append(t_dev < t_host)
            state = rnnt_amd.engine.beam_decode_lstm([model._decode_frames(model.encoder(ms[0]).permute(0, 2, 1))], pred._decode_bundle(), None, None,
                                                     joint.joint_ln.weight, joint.joint_ln.bias, joint.blank_idx, ml, beam)[0]
            rounds = int(state[0, 5])
            say(f"T = {T}, beam {beam}: best entry {len(dev)} labels (host loop's list {'the same' if host == dev else 'DIFFERS'}); "
                f"host {t_host:.1f} ms (n = {a.host_reps}; runs {', '.join('%.1f' % v for v in res['host'])}); "
                f"device, n_utt = 1: {t_dev:.2f} ms (n = {a.reps}, mean of 4 utterances; runs {', '.join('%.2f' % v for v in res['device'])}); "
                f"host / device = {t_host / t_dev:.1f}")
            say(f"    device, first utterance: {rounds} rounds, {launches} launches each, {1e3 * t_dev / rounds:.1f} us per round "
                f"(host clock of the whole call over the rounds)")
            per = {}
            for N in BATCHES:
                t_many, t_singles = [], []
                for _ in range(2):  # alternated
                    t_many.append(timed(lambda: model.beam_search_many(ms[:N], batch=N, **kw), a.reps))
                    assert model.last_beam_path == "lstm_device"
                    t_singles.append(timed(lambda: [model.beam_search(m, ln, device_search=True, **kw) for m in ms[:N]], max(1, a.reps // 3)))
                per[N] = min(t_many) / N
                say(f"    many, batch = {N:2d}: {min(t_many):.2f} ms = {per[N]:.3f} ms per utterance (runs {', '.join('%.2f' % v for v in t_many)}); "
                    f"{N} single device searches {min(t_singles):.2f} ms = {min(t_singles) / N:.3f} per utterance; single / many = "
                    f"{min(t_singles) / min(t_many):.2f}")
            lo = min(per.values())
            pick[(T, beam)] = min(N for N, v in per.items() if v <= 1.1 * lo)
            say(f"    smallest batch within 10 % of the best time per utterance ({lo:.3f} ms): {pick[(T, beam)]}")
    say(f"# the device search beat the host loop at {sum(wins)} of {len(wins)} timed shapes; BEAM_LSTM_BATCH by the rule (within 10 % at both "
        f"lengths, every beam): {max(pick.values())}")
    say("# not measured: the kernels one by one, other widths, text_ln, ragged batches, beam 16, a context graph (host loop only)")


if __name__ == "__main__":
    main()
