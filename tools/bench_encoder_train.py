#!/usr/bin/env python
"""AudioEncoder TRAINING (forward + backward of the encoder alone) on the engine (backend "engine") against the same
module's torch path, in one process on the same inputs: the widths of the reference's basic_sp_convjs.yaml (F = 201; 256 / 384 / 512
channels, k = 11 / 13 / 25, 4 sub-blocks each; epilogue 512, k = 29, dilation 2; 1024 out; ~43.6 M fp32 weights), norm instance_affine,
train() mode with the blocks' dropout (0.2 / 0.2 / 0.3) on.  WITHOUT the config's `additional_context: 2` on the first block: neither
the reference's module nor either path here can run a whole utterance with look-ahead inside a JasperBlock (the residual add fails on
the lengths).  Shapes (N, mel frames) = (4, 1000), (32, 1000), (8, 4000); medians of host-clock times around a device synchronise,
after warm-up, the two paths alternating.  Also printed per shape: the bytes the engine's forward keeps for its backward, the FLOP of
the dW products (2 x rows x taps x cin x cout per layer; with a kernel-trace run's k_enc_dw time that is its rate against the fp32
MFMA peak), the largest difference between the two paths' gradients; and the step time of an RNNTModel (engine ConvPredictor and
joint at the reference's widths, V = 1024, U = 50) with either encoder at (4, 1000).

    python tools/bench_encoder_train.py [--reps 10] [--out profiles/encoder_train_bench.txt]
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_encoder_train.py --trace 32x1000     # engine only, 4 steps
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

SHAPES = ((4, 1000), (32, 1000), (8, 4000))
PEAK_TFLOPS = 157.3  # fp32 MFMA, MI355X


def median_ms(fn, reps, warmup):
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


def dw_flop(enc, N, L):
    rows, _ = enc._lengths(L, None)
    si, cur, total = 0, None, 0
    for holder, conv, _, role in enc._flat(allow_lookahead=True):
        if holder is not None:
            cur = rows[si][2]
            frames = cur
            si += 1
        else:
            frames = rows[si][0] if role == 4 else cur
        total += 2 * N * frames * conv.kernel_size[0] * conv.in_channels * conv.out_channels
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, metavar="NxFRAMES", help="engine only, 4 steps at that shape: for a kernel-trace run")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_encoder_train needs a HIP device"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    enc = reference_width_encoder("instance_affine", seed=3).cuda().train()
    g = torch.Generator().manual_seed(1)

    def step(mel, G):
        enc.zero_grad(set_to_none=True)
        (enc(mel) * G).sum().backward()

    if a.trace:
        N, L = (int(v) for v in a.trace.split("x"))
        enc.backend = "engine"
        mel = torch.randn(N, 201, L, generator=g).cuda()
        G = torch.randn(N, 1024, L // 2, generator=g).cuda()
        for _ in range(4):
            step(mel, G)
        torch.cuda.synchronize()
        print(f"traced: 4 steps at ({N}, {L}); dW FLOP per step {dw_flop(enc, N, L):.4e}")
        return

    say(f"# tools/bench_encoder_train.py on {torch.cuda.get_device_name(0)}; encoder forward + backward, medians (min) of {a.reps} steps, ms")
    say("# reference widths, instance_affine, train() with dropout on, no look-ahead (a JasperBlock with look-ahead runs on no path)")
    for N, L in SHAPES:
        mel = torch.randn(N, 201, L, generator=g).cuda()
        G = torch.randn(N, 1024, L // 2, generator=g).cuda()
        res = {}
        for backend in ("torch", "engine", "torch", "engine"):
            enc.backend = backend
            res.setdefault(backend, []).append(median_ms(lambda: step(mel, G), a.reps, 3))
            assert enc.last_backend == backend
        t_t, t_e = min(r[0] for r in res["torch"]), min(r[0] for r in res["engine"])
        # the same masks on both paths: the gradients' difference
        enc.backend = "engine"
        torch.manual_seed(7)
        y = enc(mel)
        masks = [m for m in y.grad_fn.call[4] if m is not None]
        enc.zero_grad(set_to_none=True)
        (y * G).sum().backward()
        ge = {k: p.grad.clone() for k, p in enc.named_parameters()}
        enc.backend = "torch"
        enc.zero_grad(set_to_none=True)
        (enc(mel, keep_masks=masks) * G).sum().backward()
        rel = max(float((ge[k] - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-30)) for k, p in enc.named_parameters()
                  if not k.endswith("conv.bias"))
        flop = dw_flop(enc, N, L)
        say(f"({N}, {L}): torch {t_t:.2f} ms (runs {', '.join('%.2f (%.2f)' % r for r in res['torch'])}); engine {t_e:.2f} ms "
            f"(runs {', '.join('%.2f (%.2f)' % r for r in res['engine'])}); torch / engine = {t_t / t_e:.2f}")
        say(f"    engine saved bytes {enc.last_saved_bytes / 1e6:.1f} MB; dW products {flop / 1e12:.3f} TFLOP per step "
            f"(at the {PEAK_TFLOPS} TFLOP/s fp32 MFMA peak: {flop / PEAK_TFLOPS / 1e9:.2f} ms); "
            f"max over tensors of max|g_engine - g_torch| / max|g_torch| (same masks, exactly zero conv biases left out) = {rel:.2e}")
        del ge, y, masks
        enc.zero_grad(set_to_none=True)
        torch.cuda.empty_cache()

    # the whole training step with either encoder
    from tests.helpers import DECODE_CASES, decode_case_arrays
    from tests.stream_models import engine_model
    spec = dict(DECODE_CASES["decode_ref_widths"])
    _, pred_sd, joint_sd = decode_case_arrays(spec, 4242, 0.0)
    model = engine_model(spec, pred_sd, joint_sd, encoder=enc).train()
    N, L, U = 4, 1000, 50
    mel = torch.randn(N, 201, L, generator=g).cuda()
    ids = torch.randint(0, spec["V"] - 1, (N, U), generator=g).cuda()
    mel_lens, id_lens = torch.full((N,), L).cuda(), torch.full((N,), U).cuda()

    def model_step():
        model.zero_grad(set_to_none=True)
        model(mel, mel_lens, ids, id_lens, spec["V"] - 1).backward()

    res = {}
    for backend in ("torch", "engine", "torch", "engine"):
        enc.backend = backend
        res.setdefault(backend, []).append(median_ms(model_step, a.reps, 3))
    t_t, t_e = min(r[0] for r in res["torch"]), min(r[0] for r in res["engine"])
    say(f"RNNTModel step (forward + backward, no optimizer) at ({N}, {L}), U = {U}, V = {spec['V']}: torch encoder {t_t:.2f} ms "
        f"(runs {', '.join('%.2f (%.2f)' % r for r in res['torch'])}); engine encoder {t_e:.2f} ms "
        f"(runs {', '.join('%.2f (%.2f)' % r for r in res['engine'])}); torch / engine = {t_t / t_e:.2f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
