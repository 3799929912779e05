#!/usr/bin/env python3
"""bench.py — RNN-T joint+loss lattice cells/s on MI355X (BASELINE.json metric).

A "step" = one fused forward+backward of the joint + transducer loss from resident inputs
(enc, pred, W, bias, targets, lengths) to (loss, grad_enc, grad_pred, grad_W, grad_bias):
ONE C-ABI call (rnnt_engine_joint_loss_fwd_bwd); with N>1 ranks the utterances are sharded by
batch (global batch fixed -> strong scaling) and one RCCL all-reduce of the flat
[dW | db | loss] buffer follows.

    python bench.py --gpus 1 --steps 5 --warmup 2
    python bench.py --gpus 1 --steps 5 --warmup 2 --dump-outputs DIR   # + the last timed step's outputs as DIR/*.npy
    python bench.py --gpus 1 --steps 5 --warmup 2 --full               # + everything the headline figure does not need
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, warms up, times the
steps, dumps (--dump-outputs) and prints.  --full adds, after the timed steps: "stages_ms" and "roofline"
(every stage and the dominant kernel vs the route's MFMA peak, timed live with HIP events on the launch
stream), "exact_fp32" and "bf16x3" (the other fp32-bar routes timed on the same inputs), "parity" (a
down-scaled twin against the fp64 oracle) and "cpu_baseline" (the CPU port of the same path on the host's
cores); each of them can be left out with its --no-* option.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CONFIGS = {
    # name: (B, T, U, H, V)  — BASELINE.json configs
    "cfg2": (32, 1000, 200, 512, 1024),
    "cfg4": (8, 4000, 600, 640, 1024),
    "cfg5": (16, 800, 150, 512, 16384),
    "small": (8, 200, 50, 512, 1024),
    # the reference's real joint width (hidden_features: 1024 in every rnnt/config/*.yaml):
    # BASELINE config 1's plumbing shape and a training-sized batch of it
    "cfg1": (2, 208, 50, 1024, 1024),
    "ref1024": (8, 500, 100, 1024, 1024),
    "ref512": (8, 500, 100, 512, 1024),     # the same lattice at H = 512: like-for-like with ref1024
    "ref1024b": (32, 500, 103, 1024, 1024),  # U1 = 104: no dead rows in 8- or 16-wide u tiles
    "ref512b": (32, 500, 103, 512, 1024),
    # one rank's batch under the reference's own training settings (config/basic_sp_convjs_fullcausal.yaml: pergpu_minibatch_size 4,
    # max_joint_size 160000 = B*T*U): the size a user of rnnt/train.py actually calls the engine with
    "train4": (4, 400, 100, 1024, 1024),
}
PEAK_F32_MFMA_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md, "Peak FP32 (matrix)"
PEAK_BF16_MFMA_TFLOPS = 2500.0  # same table: "Peak BF16/FP16 MFMA ~2.5 PF dense"; bf16x3 spends 6 bf16 products per fp32 product
PEAK_HBM_GBS = 8000.0
DUMP_MAX_BYTES = 64 * 10 ** 6  # --dump-outputs: every file together
DUMP_SEED = 2024  # --dump-outputs: the sample drawn from an array too large for its share


def synth(B, T, U, H, V, seed, device, permuted_enc=False):
    """Synthetic inputs of SURVEY.md §8d: unit-scale enc/pred, torch-Linear-default W/bias,
    targets uniform in [0,V-2], all lengths full so B*T*U is exact work.  permuted_enc: `enc` is the
    view the reference really hands over — `.permute(0, 2, 1)` of an (N,C,L) encoder output
    (rnnt/model.py:27-28): shape (B,T,H), t-stride 1, h-stride T, same values."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    k = 1.0 / (H ** 0.5)
    enc = torch.randn(B, T, H, generator=g)
    if permuted_enc:
        enc = enc.permute(0, 2, 1).contiguous().to(device).permute(0, 2, 1)  # (N,C,L) storage, (N,L,C) view
    pred = torch.randn(B, U + 1, H, generator=g)
    W = (torch.rand(V, H, generator=g) * 2 - 1) * k
    bias = (torch.rand(V, generator=g) * 2 - 1) * k
    targets = torch.randint(0, V - 1, (B, U), generator=g, dtype=torch.int32)
    ll = torch.full((B,), T, dtype=torch.int32)
    tl = torch.full((B,), U, dtype=torch.int32)
    return [x.to(device) for x in (enc, pred, W, bias, targets, ll, tl)]  # .to() keeps the permuted view's strides


def dump_outputs(out_dir, arrays, max_bytes=DUMP_MAX_BYTES, seed=DUMP_SEED):
    """Write each (name, array) of `arrays` to out_dir/<name>.npy in float32, all files together within max_bytes.
    Smallest first, every array gets an equal share of what is left; an array larger than its share is written as a
    fixed sample instead: its flattened values at sorted flat indices drawn without replacement by
    numpy.random.default_rng([seed, position in `arrays`]).  The same arguments draw the same indices, so the dumps of two
    builds compare element for element.  Returns {name: {"shape", "elements", "sampled"}}."""
    os.makedirs(out_dir, exist_ok=True)
    host = [(name, np.asarray(a, dtype=np.float32)) for name, a in arrays]
    left, info = max_bytes, {}
    order = sorted(range(len(host)), key=lambda i: host[i][1].size)
    for n, i in enumerate(order):
        name, a = host[i]
        keep = max(0, (left // (len(order) - n) - 4096) // a.itemsize)  # 4096: room for the .npy header
        sampled = a.size > keep
        if sampled:
            idx = np.sort(np.random.default_rng([seed, i]).choice(a.size, size=keep, replace=False))
            a = a.reshape(-1)[idx]
        path = os.path.join(out_dir, name + ".npy")
        np.save(path, a)
        left -= os.path.getsize(path)
        info[name] = {"shape": list(host[i][1].shape), "elements": int(a.size), "sampled": sampled}
    return info


def cpu_baseline(T, U, H, V, budget_s=40.0):
    """CPU port of the same path on this box's host cores, the two legs timed separately:
    joint — the reference's own torch-CPU op sequence (oracle/torch_check.joint_torch == rnnt/joint.py:32-39)
    forward + torch autograd backward, all torch threads; loss — the C restatement standing in for torchaudio
    (absent from the image): rnnt_oracle_loss_par_f32, fp32, OpenMP over the (b,t,u) rows of the whole sample
    for the log-softmax and gradient loops (every core busy), one utterance per thread for the small
    alpha/beta recurrences."""
    from oracle import cpu_oracle
    from oracle.torch_check import joint_torch
    cpu_oracle.build()
    threads = torch.get_num_threads()

    def one(B, Tq):
        enc, pred, W, bias, targets, ll, tl = synth(B, Tq, U, H, V, 99, "cpu")
        enc.requires_grad_(True); pred.requires_grad_(True)
        W.requires_grad_(True); bias.requires_grad_(True)
        t0 = time.perf_counter()
        logits = joint_torch(enc, pred, W, bias)
        t1 = time.perf_counter()
        costs, grad = cpu_oracle.rnnt_loss_par_f32(logits.detach().numpy(), targets.numpy(), ll.numpy(), tl.numpy())
        t2 = time.perf_counter()
        logits.backward(torch.from_numpy(grad) / B)
        t3 = time.perf_counter()
        return t3 - t0, (t1 - t0) + (t3 - t2), t2 - t1

    one(1, max(8, T // 50))  # warm-up (thread pools, allocator)
    t_probe = one(1, max(8, T // 10))[0]
    est_full = t_probe * 10.0  # one utterance at full T
    # BASELINE.md §3 protocol: 1 warm-up, median of 3 runs; the three together are the ~10-30 s of
    # CPU work (the probe over-estimates: thread pools warm up), so each run gets a third
    B = int(max(1, min(8, round(budget_s / 3.0 / max(est_full, 1e-3)))))
    runs = sorted(one(B, T) for _ in range(3))
    dt, joint_s, loss_s = runs[1]
    omp = int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))
    return {"value": B * T * U / dt, "unit": "cells/s", "cores": threads, "kind": "port",
            "joint_s": joint_s, "loss_s": loss_s,
            "joint_cells_per_s": B * T * U / joint_s, "loss_cells_per_s": B * T * U / loss_s,
            "threads_busy": {"joint": threads, "loss_rows": omp, "loss_lattice": min(B, omp)},
            "sample": f"B={B},T={T},U={U},H={H},V={V} fp32, median of 3 runs ({runs[0][0]:.2f}/{runs[1][0]:.2f}/{runs[2][0]:.2f} s): "
                      f"joint fwd+bwd (torch CPU, {threads} threads) {joint_s:.2f} s + loss fwd+grad (C port, OpenMP over "
                      f"all {B * T * (U + 1)} (b,t,u) rows on {omp} threads; alpha/beta one utterance per thread) {loss_s:.2f} s",
            "runs_s": [r[0] for r in runs], "os_cpu_count": os.cpu_count()}


def parity_twin(H, V, device, dtype="fp32"):
    """Loss / gradient error of a down-scaled twin of the workload against the fp64 oracle
    (bf16 route: the oracle with the same bf16 rounding points, tests/helpers.py)."""
    import rnnt_amd
    from tests.helpers import make_inputs, oracle_fused, oracle_fused_bf16
    d = make_inputs(2, 48, 12, H, V, seed=7)
    t = {k: torch.from_numpy(v).to(device) for k, v in d.items()}
    outs = rnnt_amd.engine.joint_loss_fwd_bwd(t["enc"], t["pred"], t["W"], t["bias"], t["targets"],
                                              t["logit_lens"], t["target_lens"], V - 1, 0.5,
                                              dtype=dtype)
    torch.cuda.synchronize()
    ref = oracle_fused_bf16(d) if dtype == "bf16" else oracle_fused(d)  # bf16x3: the plain fp64 oracle, fp32's bar
    loss = float(outs[0].double().mean())
    gerr = max(float(np.abs(o.cpu().numpy() - ref[k]).max() / (np.abs(ref[k]).max() + 1e-30))
               for o, k in zip(outs[1:], ("grad_enc", "grad_pred", "grad_W", "grad_bias")))
    return {"loss_rel_err": abs(loss - ref["loss"]) / abs(ref["loss"]), "grad_rel_err": gerr,
            "twin": "B=2,T=48,U=12 ragged, same H,V, vs fp64 oracle" +
                    (" with bf16 rounding points" if dtype == "bf16" else "")}


def self_launch(n):
    """`python bench.py --gpus N` with no launcher around it (WORLD_SIZE unset): start the N rank
    processes here, one per GPU — the process layout of reference rnnt/train.py:25-33 (mp.spawn,
    one rank per device, "nccl").  The parent launches no GPU work: the ranks are FRESH child processes
    (Popen, never a re-exec of this one), so whatever torch.cuda.device_count() does to count the devices
    stays in the parent; it refuses to run fewer ranks than asked for.  A parent that is told to stop
    (SIGTERM / SIGINT, e.g. the driver's timeout) takes its ranks with it — none is left blocked in a
    collective holding a GPU and the rendezvous port."""
    import signal
    import subprocess
    have = torch.cuda.device_count()
    single = os.environ.get("BENCH_SINGLE_DEVICE") == "1"  # rehearsal: every rank on cuda:0
    if have < n and not (single and have >= 1):
        print(json.dumps({"error": f"--gpus {n} requested but hipGetDeviceCount() = {have}; refusing to "
                                   "benchmark fewer GPUs than asked for", "hipGetDeviceCount": have,
                          "n_gpus_requested": n}), flush=True)
        raise SystemExit(3)
    # rendezvous of the self-launched ranks: a FILE store in a fresh private directory (one node, one file system) — no TCP port to pick.
    # ("bind to port 0, read the number, close, hand it to the children" leaves a window in which anything on the box — RCCL's own
    # bootstrap sockets included — can take the port before rank 0's store binds it.)
    import tempfile
    rdzv_dir = tempfile.mkdtemp(prefix="rnnt_bench_rdzv_")
    procs = []

    def stop_ranks(grace=5.0):
        for p in procs:
            if p.poll() is None:
                p.terminate()
        t_end = time.time() + grace
        for p in procs:
            try:
                p.wait(timeout=max(0.0, t_end - time.time()))
            except subprocess.TimeoutExpired:
                p.kill()

    def on_signal(signum, _frame):
        stop_ranks()
        raise SystemExit(128 + signum)

    old = {sig: signal.signal(sig, on_signal) for sig in (signal.SIGTERM, signal.SIGINT)}
    rc = 0
    try:
        for r in range(n):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), BENCH_INIT_FILE=os.path.join(rdzv_dir, "store"),
                       HSA_ENABLE_IPC_MODE_LEGACY="0")
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                          stdout=None if r == 0 else subprocess.DEVNULL))
        live = list(procs)
        while live:  # a rank that dies would leave the others waiting in a collective: stop them
            time.sleep(0.2)
            for p in list(live):
                code = p.poll()
                if code is None:
                    continue
                live.remove(p)
                if code != 0 and rc == 0:
                    rc = code
                    for q in live:
                        q.terminate()
    finally:  # whatever ends this loop (a signal, an exception): no rank outlives the parent
        stop_ranks()
        for sig, h in old.items():
            signal.signal(sig, h)
        import shutil
        shutil.rmtree(rdzv_dir, ignore_errors=True)
    raise SystemExit(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)   # >= 5 warm-ups, median of >= 20
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="cfg2", choices=sorted(CONFIGS))
    ap.add_argument("--dtype", default="f16x2", choices=["fp32", "bf16", "bf16x3", "f16x2"],
                    help="f16x2 (default, round 4) = fp32-class results from THREE fp16 MFMA products of power-of-two-scaled, 2-way split "
                         "operands (RNNT_DTYPE_F32_F16X2: 22 significant bits per operand, the fp32 route's 1e-4 parity bar, every fp32 "
                         "parity test runs on it, half the matrix work of bf16x3); bf16x3 = fp32-ACCURATE results from six bf16 MFMA products of 3-way split operands "
                         "(RNNT_DTYPE_F32_BF16X3: the fp32 route's 1e-4 parity bar, every fp32 parity test runs on it); "
                         "fp32 = exact fp32 products on v_mfma_f32_32x32x2_f32 (1/16 of the bf16 matrix rate); "
                         "bf16 = BASELINE config 3's arithmetic (bf16-rounded GEMM operands, fp32 accumulate)")
    ap.add_argument("--permuted-enc", action="store_true",
                    help="hand `enc` over as the reference does: the permute(0,2,1) view of an (N,C,L) tensor "
                         "(rnnt/model.py:27-28); the engine's tiled transpose is then part of every step")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure what the headline figure does not need: per-stage timing and the "
                         "roofline, the exact-fp32 and bf16x3 routes, the parity twin and the CPU baseline (the --no-* options "
                         "below leave parts of it out); without it the run only sets up, warms up, times, dumps and prints")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-stage-timing", action="store_true", help="--full without the per-stage timing and roofline")
    ap.add_argument("--no-exact-fp32", action="store_true",
                    help="--full without the secondary `exact_fp32` and `bf16x3` objects (the other routes timed in the same run)")
    ap.add_argument("--no-parity", action="store_true",
                    help="--full without the down-scaled parity twin of the CPU leg (it also goes with --no-cpu-baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last timed step computed to DIR/<name>.npy (float32): loss, "
                         "costs, grad_enc, grad_pred, grad_W, grad_bias (rank 0's shard of costs / grad_enc / grad_pred); at most "
                         "64 MB in all, an array too large for its share as a fixed seeded sample (dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args.gpus)  # never returns
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    import torch.distributed as dist
    # rehearsal knobs (not used by the driver): BENCH_SINGLE_DEVICE=1 maps every rank to cuda:0 and
    # BENCH_BACKEND=gloo swaps RCCL for gloo, so the N>1 code path can run on a one-GPU box
    single = os.environ.get("BENCH_SINGLE_DEVICE") == "1"
    backend = os.environ.get("BENCH_BACKEND", "nccl")
    device = torch.device("cuda", 0 if single else local_rank)
    torch.cuda.set_device(device)
    # BENCH_FORCE_DIST=1: run the N>1 code path (process group, broadcast, all-reduce, barriers)
    # with a single rank, so the RCCL calls can be exercised on a one-GPU box
    dist_on = world > 1 or os.environ.get("BENCH_FORCE_DIST") == "1"
    if dist_on:
        # rendezvous: the launcher's (torchrun / the driver: MASTER_ADDR + MASTER_PORT in the environment, init_method env://); a file store
        # for ranks this script launched itself (BENCH_INIT_FILE, self_launch) and for a single forced rank with no launcher at all
        # (BENCH_FORCE_DIST=1: a private temporary file — a one-rank group needs no TCP port, and a fixed default port or one picked by
        # bind-close-reuse can be taken by the time the store binds it)
        init_file = os.environ.get("BENCH_INIT_FILE")
        own_dir = None
        if init_file is None and "MASTER_PORT" not in os.environ:
            if world != 1:
                raise SystemExit("WORLD_SIZE > 1 without MASTER_PORT or BENCH_INIT_FILE: launch through torchrun or `bench.py --gpus N`")
            import tempfile
            own_dir = tempfile.mkdtemp(prefix="rnnt_bench_rdzv_")
            init_file = os.path.join(own_dir, "store")
        kw = dict(init_method="file://" + init_file, rank=rank, world_size=world) if init_file else {}
        if not init_file:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device, **kw)  # "nccl" is RCCL on ROCm
        else:
            dist.init_process_group(backend, **kw)
        if own_dir is not None:
            import atexit
            import shutil
            atexit.register(shutil.rmtree, own_dir, ignore_errors=True)

    import rnnt_amd
    from rnnt_amd import engine
    engine.lib()

    B, T, U, H, V = CONFIGS[args.config]
    if B % world != 0:
        raise SystemExit(f"global batch {B} not divisible by {world} ranks")
    Bl = B // world  # contiguous batch shard per rank (strong scaling: global batch fixed)
    enc, pred, W, bias, targets, ll, tl = synth(Bl, T, U, H, V, 1234 + rank, device, permuted_enc=args.permuted_enc)
    if dist_on:  # parameters are replicated: rank 0's W/bias everywhere
        dist.broadcast(W, 0); dist.broadcast(bias, 0)
    scale = 1.0 / B
    # flat [dW | db | loss] buffer: grad_W / grad_bias are views, so the all-reduce needs no copy
    from rnnt_amd.parallel import FlatGrad
    fg = FlatGrad(V, H, device)
    flat, gW, gb = fg.flat, fg.grad_W, fg.grad_bias
    costs = torch.empty(Bl, dtype=torch.float32, device=device)
    ge = torch.empty(Bl, T, H, dtype=torch.float32, device=device)
    gp = torch.empty(Bl, U + 1, H, dtype=torch.float32, device=device)
    outs = (costs, ge, gp, gW, gb)

    # transport of the one all-reduce: torch.distributed's "nccl" backend (= RCCL; default), or with
    # BENCH_COMM=engine the C entry rnnt_engine_allreduce on a communicator of the bench's own
    comm = None
    if dist_on and backend == "nccl" and os.environ.get("BENCH_COMM") == "engine":
        from rnnt_amd.parallel import RcclComm
        comm = RcclComm(rank, world, device)

    def step():
        engine.joint_loss_fwd_bwd(enc, pred, W, bias, targets, ll, tl, V - 1, scale, outs=outs,
                                  dtype=args.dtype)
        fg.set_loss(costs, scale)
        fg.all_reduce(comm=comm)  # N>1: one RCCL all-reduce over xGMI of dW, db and the loss

    for _ in range(args.warmup):
        step()
    if dist_on:
        dist.barrier()
    torch.cuda.synchronize()
    # The contract's number: EXACTLY K steps between two (barrier + synchronize) brackets, wall clock, max over
    # ranks.  Beside it, SURVEY §8d's protocol: a HIP-event pair around every one of those K steps on the launch
    # stream (torch's current stream IS the stream the engine enqueues on), median reported.
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    t0 = time.perf_counter()
    for e0, e1 in evs:
        e0.record()
        step()
        e1.record()
    torch.cuda.synchronize()
    if dist_on:
        dist.barrier()
    dt = time.perf_counter() - t0
    step_ms = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
    med_ms = step_ms[len(step_ms) // 2] if len(step_ms) % 2 else 0.5 * (step_ms[len(step_ms) // 2 - 1] + step_ms[len(step_ms) // 2])
    tmax = torch.tensor([dt, med_ms], dtype=torch.float64, device=device)
    if dist_on:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt, med_ms = float(tmax[0].item()), float(tmax[1].item())
    loss = float(flat[V * H + V].item())
    # what the last timed step computed, copied off the device before the stage timing below reuses `outs`
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, [(k, t.cpu().numpy()) for k, t in (
            ("loss", fg.loss), ("costs", costs), ("grad_enc", ge), ("grad_pred", gp), ("grad_W", gW), ("grad_bias", gb))])

    # ---- per-stage timing with HIP events on the launch stream (torch's current stream IS the
    # stream every kernel was enqueued on: engine._stream()).
    stage_ms = None
    if args.full and not args.no_stage_timing:
        names = ["producers_hidden_wpack", "joint_fwd_gemm", "lattice_sweep", "grad_coef_make_g",
                 "dhidden_gemm", "dhidden_reduce", "dw_gemm", "dw_reduce"]
        # as many repetitions per stage as timed steps (default 20): the three GEMM stages then keep the GPU busy
        # for seconds, long enough for an external utilisation sampler to see the run
        reps = max(2, args.steps)
        stage_ms = {}
        for s, name in enumerate(names):
            engine.joint_loss_fwd_bwd(enc, pred, W, bias, targets, ll, tl, V - 1, scale, outs=outs, stage=s,
                                      dtype=args.dtype)
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                engine.joint_loss_fwd_bwd(enc, pred, W, bias, targets, ll, tl, V - 1, scale, outs=outs, stage=s,
                                          dtype=args.dtype)
            e1.record(); e1.synchronize()
            stage_ms[name] = e0.elapsed_time(e1) / reps

    # ---- the other fp32-bar routes timed in the same run, so that one driver-run line carries every arithmetic form of the
    # fp32-accurate path (N = 1, default route only): exact fp32 products (v_mfma_f32_32x32x2_f32) and the bf16x3 route
    def time_route(dt, arith, peak):
        n = max(3, args.steps // 2)
        for _ in range(2):
            engine.joint_loss_fwd_bwd(enc, pred, W, bias, targets, ll, tl, V - 1, scale, outs=outs, dtype=dt)
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for e0, e1 in evs:
            e0.record()
            engine.joint_loss_fwd_bwd(enc, pred, W, bias, targets, ll, tl, V - 1, scale, outs=outs, dtype=dt)
            e1.record()
        torch.cuda.synchronize()
        ts = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
        m = ts[len(ts) // 2]
        tf = 6.0 * H * V * Bl * T * (U + 1) / (m * 1e-3) / 1e12
        loss_r = float(outs[0].double().sum().item() * scale)
        # the route's own kernel roofline (round-5 verdict item 7): its three GEMM stages timed one by one (HIP events on the launch
        # stream, mean of `reps` back-to-back launches), the slowest of them priced at 2 H V flop per cell against the route's peak
        reps = max(3, n // 2)
        gemm_ms = {}
        for s_idx, name in ((1, "joint_fwd_gemm"), (4, "dhidden_gemm"), (6, "dw_gemm")):
            engine.joint_loss_fwd_bwd(enc, pred, W, bias, targets, ll, tl, V - 1, scale, outs=outs, stage=s_idx, dtype=dt)
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                engine.joint_loss_fwd_bwd(enc, pred, W, bias, targets, ll, tl, V - 1, scale, outs=outs, stage=s_idx, dtype=dt)
            e1.record(); e1.synchronize()
            gemm_ms[name] = e0.elapsed_time(e1) / reps
        dom_r = max(gemm_ms, key=gemm_ms.get)
        ach_r = 2.0 * H * V * Bl * T * (U + 1) / (gemm_ms[dom_r] * 1e-3) / 1e12
        return {"ms_per_step": m, "value": B * T * U / (m * 1e-3), "unit": "cells/s", "steps": n, "arith": arith, "path_tflops": tf,
                "peak": peak, "frac": tf / peak, "loss": loss_r,
                "roofline": {"bound": "mfma", "kernel": dom_r, "ms": gemm_ms[dom_r], "achieved": ach_r, "peak": peak, "unit": "TFLOP/s",
                             "frac": ach_r / peak, "gemm_stage_ms": gemm_ms,
                             "note": "2*H*V flop per cell per GEMM launch / HIP-event time of that stage"},
                "timing": f"hipEventElapsedTime per step, median of {n}, same process and inputs as the headline"}

    exact_fp32 = route_bf16x3 = None
    if args.full and world == 1 and args.dtype in ("f16x2", "bf16x3") and not args.no_exact_fp32:
        exact_fp32 = time_route("fp32", "v_mfma_f32_32x32x2_f32 (exact fp32 products)", PEAK_F32_MFMA_TFLOPS)
        if args.dtype == "f16x2":
            route_bf16x3 = time_route("bf16x3", "6 x v_mfma_f32_32x32x16_bf16 per fp32 product (operands split hi+mid+lo)", PEAK_BF16_MFMA_TFLOPS / 6.0)

    if rank != 0:
        if dist_on:
            dist.destroy_process_group()
        return

    cells_local = Bl * T * U
    cells_global = B * T * U
    ms = dt / args.steps * 1e3
    out = {
        "metric": "RNN-T joint+loss fwd+bwd lattice cells/s (B*T*U/s)",
        "value": cells_global * args.steps / dt,
        "unit": "cells/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms,
        # SURVEY §8d protocol beside the contract's wall-clock mean: HIP-event pair per step, median (max over ranks)
        "ms_per_step_median": med_ms, "ms_per_step_min": step_ms[0], "ms_per_step_max": step_ms[-1],
        "value_at_median": cells_global / (med_ms * 1e-3),
        "timing": f"value/ms_per_step: wall clock over {args.steps} steps between barrier+synchronize brackets, max over "
                  f"ranks; ms_per_step_median: hipEventElapsedTime per step, median of {args.steps}",
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        # dtype = the arithmetic the path computes in, named honestly (round-4 verdict item 1e): "f32" ONLY for exact fp32
        # products; the split routes say what their operands hold — "f32(f16x2)": fp32 tensors in and out, fp32 accumulation,
        # products formed from 22-bit operands (2 fp16 pieces), held to the fp32 route's 1e-4 bar by tests/ and `parity` below;
        # "f32(bf16x3)": 24-bit operands (3 bf16 pieces).  `exact_fp32` in this line is the strict-fp32 number.  arith = how
        # the products are formed
        "dtype": {"fp32": "f32", "f16x2": "f32(f16x2)", "bf16x3": "f32(bf16x3)", "bf16": "bf16"}[args.dtype], "data": "synthetic",
        "arith": {"fp32": "v_mfma_f32_32x32x2_f32 (exact fp32 products)",
                  "bf16x3": "6 x v_mfma_f32_32x32x16_bf16 per fp32 product (operands split hi+mid+lo), fp32 accumulate",
                  "f16x2": "3 x v_mfma_f32_32x32x16_f16 per fp32 product (operands scaled by powers of two and split hi+mid: 22 significant bits), fp32 accumulate",
                  "bf16": "v_mfma_f32_32x32x16_bf16 on bf16-rounded operands, fp32 accumulate, fp16 logits"}[args.dtype],
        "config": {"workload": f"{args.config}: B={B},T={T},U={U},H={H},V={V} " +
                               {"fp32": "fp32", "bf16": "bf16", "bf16x3": "fp32-accurate (bf16x3 arithmetic)", "f16x2": "fp32-class (f16x2 arithmetic)"}[args.dtype] +
                               " joint+loss fwd+bwd" +
                               (", enc = permuted (N,C,L) view" if args.permuted_enc else ""),
                   "enc_layout": "permute(0,2,1) view of (N,C,L), as rnnt/model.py:27-28" if args.permuted_enc else "contiguous (B,T,H)",
                   "global_batch": B, "per_gpu_batch": Bl, "parallelism": f"dp{world}",
                   "cells_BTU1": B * T * (U + 1)},
        "loss": loss,
        # what actually ran: devices the runtime sees, ranks in the RCCL communicator
        "hipGetDeviceCount": torch.cuda.device_count(),
        # ranks of the process group, under the name of the transport that carried the all-reduce: `rccl_ranks` only
        # when the backend is nccl (= RCCL), `dist_ranks` for a gloo rehearsal
        ("rccl_ranks" if (dist_on and backend == "nccl") or not dist_on else "dist_ranks"): dist.get_world_size() if dist_on else 0,
        "dist_backend": (("rccl" if backend == "nccl" else backend) if dist_on else None),  # "nccl" is RCCL on ROCm; gloo only in rehearsals
        "allreduce_via": ("rnnt_engine_allreduce" if comm is not None else "torch.distributed") if dist_on else None,
    }
    flops_cell = 6.0 * H * V  # 2HV fwd + 2HV dHidden + 2HV dW per lattice cell
    cells1 = Bl * T * (U + 1)  # cells the GEMMs actually process per launch (U+1 columns)
    out["path_tflops"] = flops_cell * cells1 / (dt / args.steps) / 1e12
    if stage_ms:
        gemms = {k: stage_ms[k] for k in ("joint_fwd_gemm", "dhidden_gemm", "dw_gemm")}
        dom = max(gemms, key=gemms.get)
        ach = 2.0 * H * V * cells1 / (gemms[dom] * 1e-3) / 1e12
        peak = {"bf16x3": PEAK_BF16_MFMA_TFLOPS / 6.0, "f16x2": PEAK_BF16_MFMA_TFLOPS / 3.0}.get(args.dtype, PEAK_F32_MFMA_TFLOPS)
        out["roofline"] = {"bound": "mfma", "kernel": dom, "achieved": ach,
                           "peak": peak, "unit": "TFLOP/s",
                           "frac": ach / peak, "traffic": None,
                           "flops_per_launch": 2.0 * H * V * cells1, "ms_per_launch": gemms[dom]}
        if args.dtype == "f16x2":
            out["roofline"]["peak_note"] = "dense fp16 MFMA peak 2500 TFLOP/s / 3 fp16 products per fp32 product (fp32-equivalent flops)"
            # the other roofline of this route's kernels: algorithmic HBM bytes per cell (rnnt_amd/csrc/x2.hip: two fp16 planes per
            # operand; fwd 4H + 4V, dHidden 4V + 4V, dW 4V + 4H) over the same launch time
            per_cell = {"joint_fwd_gemm": 4 * H + 4 * V, "dhidden_gemm": 8 * V, "dw_gemm": 4 * V + 4 * H}
            gbs = per_cell[dom] * cells1 / (gemms[dom] * 1e-3) / 1e9
            out["roofline"]["hbm"] = {"achieved": gbs, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": gbs / PEAK_HBM_GBS,
                                      "bytes_per_launch": per_cell[dom] * cells1}
        if args.dtype == "bf16x3":
            out["roofline"]["peak_note"] = "dense bf16 MFMA peak 2500 TFLOP/s / 6 bf16 products per fp32 product (fp32-equivalent flops)"
        if args.dtype == "bf16":
            # 16x the matrix rate: every kernel of this route is HBM-bound.  Algorithmic bytes per
            # cell (rnnt_amd/csrc/bf16.hip header; logits stored fp16): fwd 2H+2V, dHidden 2V+2V+2H, dW 2V+2H
            per_cell = {"joint_fwd_gemm": 2 * H + 2 * V, "dhidden_gemm": 4 * V + 2 * H, "dw_gemm": 2 * V + 2 * H}
            gbs = per_cell[dom] * cells1 / (gemms[dom] * 1e-3) / 1e9
            out["roofline"] = {"bound": "hbm", "kernel": dom, "achieved": gbs, "peak": PEAK_HBM_GBS,
                               "unit": "GB/s", "frac": gbs / PEAK_HBM_GBS, "traffic": None,
                               "bytes_per_launch": per_cell[dom] * cells1, "ms_per_launch": gemms[dom],
                               "mfma_tflops": ach}
        # HBM traffic of that kernel: not measurable from inside the process; taken from the PMC
        # profile committed for this config (profiles/r01_traffic.json), else null
        try:
            key = args.config if args.dtype == "fp32" else args.config + "_" + args.dtype
            tfile = sorted(f for f in os.listdir(os.path.join(ROOT, "profiles")) if f.endswith("_traffic.json"))[-1]
            tr = json.load(open(os.path.join(ROOT, "profiles", tfile)))[key][dom]
            if world == 1:
                # MI355X_MICROARCH.md §HBM: on gfx950 FETCH_SIZE reports half the bytes of 16 B/lane
                # streams (every load of these kernels is 16 B/lane) -> doubled; WRITE_SIZE is exact
                out["roofline"]["traffic"] = 2 * tr["fetch_raw"] + tr["write"]
                # REPLAYED from the committed PMC profile of this config, not measured in this run
                out["roofline"]["traffic_source"] = {"file": "profiles/" + tfile, "replayed": True,
                                                     "commit": tr.get("commit") or json.load(open(os.path.join(ROOT, "profiles", tfile))).get("commit")}
                if tr.get("mfma_busy") is not None:
                    # SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 x 1024 SIMDs) of this kernel in the committed SQ
                    # counter pass — REPLAYED like `traffic`, not measured in this run
                    out["roofline"]["mfma_busy"] = tr["mfma_busy"]
                    out["roofline"]["mfma_busy_source"] = {"file": tr.get("mfma_busy_file"), "replayed": True}
                out["roofline"]["traffic_note"] = ("bytes/launch = 2 x FETCH_SIZE + WRITE_SIZE (rocprofv3 PMC, separate "
                                                   "passes, KB x 1024; gfx950 half-count correction for 16 B/lane loads), "
                                                   "profiles/%s; algorithmic HBM bytes %.3g" % (tfile, tr["algorithmic"]))
        except Exception:  # noqa: BLE001
            pass
        sweep_bytes = 24.0 * cells1
        out["stages_ms"] = stage_ms
        out["lattice_sweep"] = {"achieved_GBs": sweep_bytes / (stage_ms["lattice_sweep"] * 1e-3) / 1e9,
                                "peak_GBs": PEAK_HBM_GBS, "bytes": sweep_bytes,
                                "frac": sweep_bytes / (stage_ms["lattice_sweep"] * 1e-3) / 1e9 / PEAK_HBM_GBS}
    if exact_fp32 is not None:
        out["exact_fp32"] = exact_fp32
    if route_bf16x3 is not None:
        out["bf16x3"] = route_bf16x3  # round 3's default route (six bf16 products of 3-way split operands) on the same inputs
    if args.full and world == 1 and not args.no_cpu_baseline:
        # the CPU leg (rank 0, N = 1 only; the one place bench.py touches oracle/): the oracle as checker of a
        # down-scaled twin of the workload, then the CPU port timed on this box's host cores
        if not args.no_parity:
            try:
                out["parity"] = parity_twin(H, V, device, args.dtype)
            except Exception as e:  # noqa: BLE001
                out["parity"] = {"error": repr(e)}
        engine.release_workspaces()
        out["cpu_baseline"] = cpu_baseline(T, U, H, V)
        out["gpu_over_cpu"] = out["value"] / out["cpu_baseline"]["value"]
    if dumped is not None:
        out["dump_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
    print(json.dumps(out), flush=True)
    if dist_on:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
