#!/usr/bin/env python
"""AudioEncoder on the engine against the same module's torch path (rnnt_amd/encoder.py), at the widths of the reference's
basic_sp_convjs.yaml (F = 201; 256 / 384 / 512 channels, k = 11 / 13 / 25; epilogue 512, k = 29, dilation 2; 1024 out; ~43.6 M fp32
weights), seeded, N = 1, both paths in one process on one GPU, medians of host-clock times around a device synchronise (the number of
calls behind each median is printed with it):
  (a) whole-utterance forward of 1000 mel frames (norm instance_affine);
  (b) streaming_forward of 50-frame chunks = 25 rows (instance_affine), and a 1000-frame utterance through GreedyStream.push in 50-frame
      chunks with each encoder path (encoder + decode per push);
  (c) streaming_forward of 2-frame chunks = 1 row (norm batch: instance norm refuses one frame).
Per case also: the host's enqueue time and the device span per call (a run of calls back to back between two events, no synchronise
inside), which says whether a path is bound by the host or by the device.  Also printed: launches per push (2 per layer on the engine: conv + norm), the bytes a push streams (packed weights) and the rate that
makes of the push time, and the largest difference between the two paths' outputs on the timed inputs.

    python tools/bench_encoder.py [--reps 200] [--out profiles/encoder_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.encoder_cases import reference_width_encoder  # noqa: E402
from tests.helpers import DECODE_CASES, decode_case_arrays  # noqa: E402
from tests.stream_models import engine_model  # noqa: E402


# blank biases tried for the seeded joint behind (b'): the one whose offline greedy decode of the utterance's 500 encoder frames emits
# the number of labels closest to STREAM_TOKENS is used (an untrained joint without a bias emits the 10-per-frame cap on every frame,
# and the decode then dwarfs the encoder)
STREAM_BLANK_BIASES = (16.0, 24.0, 32.0, 34.0, 36.0, 38.0, 40.0, 45.0)
STREAM_TOKENS = 150


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


def spans_ms(fn, reps):
    """(host enqueue, device span) per call, ms: `reps` calls back to back between two events."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    host = (time.perf_counter() - t0) * 1e3 / reps
    torch.cuda.synchronize()
    return host, e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_encoder needs a HIP device"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/bench_encoder.py on {torch.cuda.get_device_name(0)}; medians (min) of n calls, ms; N = 1")
    g = torch.Generator().manual_seed(1)
    mel = torch.randn(1, 201, 1000, generator=g).cuda()
    for norm, cases in (("instance_affine", ("a", "b")), ("batch", ("c",))):
        enc = reference_width_encoder(norm, seed=3).cuda()
        flat = enc._flat()  # the engine's layer list
        wbytes = sum(c.weight.numel() * 4 for _, c, _, _ in flat)
        say(f"## norm {norm}: {len(flat)} layers, {wbytes / 1e6:.1f} MB of conv weights; engine launches per call = {2 * len(flat)} "
            f"(conv + norm per layer), no cat / slice / permute kernels")
        state0 = [s.cuda() for s in enc.streaming_init_state(1)]
        with torch.no_grad():
            for case in cases:
                if case == "a":
                    x, label = mel, "(a) forward, 1000 mel frames (500 rows)"
                    run = lambda: enc(x)
                else:
                    k = 50 if case == "b" else 2
                    x, label = mel[:, :, :k], f"({case}) streaming_forward, {k}-frame chunk ({k // 2} row{'s' if k > 2 else ''})"
                    # a steady-state push: the state a first push leaves
                    enc.backend = "torch"
                    _, st = enc.streaming_forward(x, state0)
                    st = [s.contiguous() for s in st]
                    run = lambda: enc.streaming_forward(x, st)
                res, span = {}, {}
                n_calls = a.reps if case != "a" else max(20, a.reps // 4)
                for backend in ("torch", "engine", "torch", "engine"):  # alternate the two
                    enc.backend = backend
                    y = run()
                    y = y[0] if isinstance(y, tuple) else y
                    med, lo = median_ms(run, n_calls)
                    res.setdefault(backend, []).append((med, lo, y.clone()))
                    span[backend] = spans_ms(run, n_calls)
                t_t = min(r[0] for r in res["torch"])
                t_e = min(r[0] for r in res["engine"])
                diff = (res["torch"][0][2] - res["engine"][0][2]).abs().max().item()
                say(f"{label}, n = {n_calls}: torch {t_t:.3f} ms  (runs {', '.join('%.3f (%.3f)' % r[:2] for r in res['torch'])}); "
                    f"engine {t_e:.3f} ms  (runs {', '.join('%.3f (%.3f)' % r[:2] for r in res['engine'])}); "
                    f"torch / engine = {t_t / t_e:.2f}; max|engine - torch| = {diff:.2e}")
                say("    per call, back to back: " + "; ".join(f"{b} host enqueue {span[b][0]:.3f} ms, device span {span[b][1]:.3f} ms"
                                                               for b in ("torch", "engine")))
                if case != "a":
                    say(f"    engine push streams {wbytes / 1e6:.1f} MB of weights in {t_e:.3f} ms = {wbytes / t_e / 1e9:.2f} TB/s "
                        f"(host-clock time of the whole push, launches included)")
        if norm == "instance_affine":
            spec = dict(DECODE_CASES["decode_ref_widths"])
            enc.backend = "torch"
            tried = {}
            for bias in STREAM_BLANK_BIASES:
                _, pred_sd, joint_sd = decode_case_arrays(spec, 4242, bias)
                m = engine_model(spec, pred_sd, joint_sd, encoder=enc)
                tried[bias] = len(m.greedy_decode(mel, torch.tensor([1000], device="cuda"), max_length=5001))
            bias = min(tried, key=lambda b: abs(tried[b] - STREAM_TOKENS))
            say(f"    (b') joint: blank bias {bias} of {tried} (labels of the offline greedy decode per bias)")
            _, pred_sd, joint_sd = decode_case_arrays(spec, 4242, bias)
            model = engine_model(spec, pred_sd, joint_sd, encoder=enc)

            def utterance():
                s = model.greedy_stream(max_length=None)
                n = 0
                for i in range(0, 1000, 50):
                    n += len(s.push(mel[..., i:i + 50]))
                return n
            res = {}
            for backend in ("torch", "engine", "torch", "engine"):
                enc.backend = backend
                ntok = utterance()
                res.setdefault(backend, []).append(median_ms(utterance, max(5, a.reps // 20), warmup=2) + (ntok,))
            t_t, t_e = min(r[0] for r in res["torch"]), min(r[0] for r in res["engine"])
            say(f"(b') 1000 mel frames through GreedyStream.push in 20 chunks of 50, n = {max(5, a.reps // 20)} utterances (encoder + decode, "
                f"{res['engine'][0][2]} tokens, "
                f"torch path {res['torch'][0][2]}): torch encoder {t_t:.2f} ms = {t_t / 20:.3f} per push; engine encoder {t_e:.2f} ms = "
                f"{t_e / 20:.3f} per push; ratio {t_t / t_e:.2f}")
        enc.backend = "auto"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
