#!/usr/bin/env python
"""The featurizer on the engine against the same module's torch path (rnnt_amd/featurizer.py), at the reference's sizes (n_fft 400,
hop 160, window 400, 201 bins, per-bin mean / invstddev, piecewise log), seeded noise, all paths in one process on one GPU, medians
(min) of host-clock times around a device synchronise, the paths alternated twice:
  engine   samples on the device -> features on the device (rnnt_engine_featurizer_fwd / _stream_push)
  torch    the torch.stft chain on the same device tensors
  host     the torch.stft chain on the CPU from samples in host memory, plus the upload of the features (what a caller without a
           device featurizer does).  `engine` and `torch` start from samples already on the device: the samples' own upload, 2 or 4
           bytes each against 201 floats per 160 of them, is not timed.
Shapes: a 1-frame push (160 samples onto 240 carried), an 8-frame push (1280 samples onto 240 carried), a 1000-frame utterance, each in
int16 and fp32; a ragged batch of 32 utterances of 500 .. 1000 frames (fp32 and int16).  Also printed per shape: the largest difference
between the engine's and the device torch path's features.

    python tools/bench_featurizer.py [--reps 200] [--out profiles/featurizer_bench.txt]
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
from tests.featurizer_cases import noise, per_bin, to_int16  # noqa: E402


def median_ms(fn, reps, warmup=10):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_featurizer needs a HIP device"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/bench_featurizer.py on {torch.cuda.get_device_name(0)}; medians (min) of n calls, ms; 400 / 160 / 400, 201 bins, per-bin "
        f"normalisation; torch {torch.__version__}, {torch.get_num_threads()} CPU threads")
    mean, inv = per_bin()
    mod = rnnt_amd.TFJSSpectrogram(400, 160, 400, True, mean, inv)
    host_mod = rnnt_amd.TFJSSpectrogram(400, 160, 400, True, mean, inv)

    def case(label, n_calls, make):
        """make(device, backend) -> a callable that runs one call and returns the features."""
        runs = {"engine": make("cuda", "engine"), "torch": make("cuda", "torch"), "host": make("cpu", "torch")}
        res = {}
        for name in ("torch", "engine", "host") * 2:  # alternate the paths
            res.setdefault(name, []).append(median_ms(runs[name], n_calls))
        best = {k: min(r[0] for r in v) for k, v in res.items()}
        diff = (runs["engine"]().float() - runs["torch"]().float()).abs().max().item()
        fmt = lambda k: f"{k} {best[k]:.3f} ms (runs {', '.join('%.3f (%.3f)' % r for r in res[k])})"
        say(f"{label}, n = {n_calls}: {fmt('engine')}; {fmt('torch')}; {fmt('host')}; torch / engine = {best['torch'] / best['engine']:.2f}, "
            f"host / engine = {best['host'] / best['engine']:.2f}; max|engine - torch| = {diff:.2e}")

    with torch.no_grad():
        for pcm in (True, False):
            kind = "int16" if pcm else "fp32"
            conv = to_int16 if pcm else (lambda t: t)
            carried = noise(240, 1)
            for frames, chunk_len in ((1, 160), (8, 1280)):
                chunk = conv(noise(chunk_len, 2 + frames))

                def make(device, backend, chunk=chunk):
                    m = mod if device == "cuda" else host_mod
                    c, st = chunk[None].to(device), carried[None].to(device)

                    def run():
                        m.backend = backend
                        y, _ = m.streaming_forward(c, st)
                        return y.cuda()  # (the host path's feature upload; a no-op for device results)
                    return run
                case(f"{frames}-frame push ({chunk_len} samples onto 240 carried), {kind}", a.reps, make)
            utt = conv(noise(400 + 999 * 160, 5))

            def make(device, backend, utt=utt):
                m = mod if device == "cuda" else host_mod
                x = utt[None].to(device)

                def run():
                    m.backend = backend
                    return m(x).cuda()
                return run
            case(f"1000-frame utterance ({len(utt)} samples), {kind}", max(20, a.reps // 4), make)
            lens = [400 + (499 + (i * 501) // 31) * 160 + 7 * i for i in range(32)]
            waves = [conv(noise(n, 10 + i)) for i, n in enumerate(lens)]

            def make(device, backend, waves=waves):
                m = mod if device == "cuda" else host_mod
                ws = [w.to(device) for w in waves]

                def run():
                    m.backend = backend
                    return m(ws)[0].cuda()
                return run
            case(f"ragged batch of 32 utterances, 500 .. 1000 frames ({sum(lens)} samples), {kind}", max(10, a.reps // 10), make)
    mod.backend = host_mod.backend = "auto"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
