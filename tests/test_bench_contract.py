"""CPU test: the bench line committed under profiles/ (produced by `python bench.py` on an MI355X)
carries every field the bench contract names, with consistent values."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(name):
    text = open(os.path.join(ROOT, "profiles", name)).read().strip().splitlines()[-1]
    return json.loads(text)


def _check(d, dtype):
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "cells/s" and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["scaling"] == "strong" and d["data"] == "synthetic" and d["dtype"] == dtype and d["n_gpus"] == 1
    assert "workload" in d["config"] and "model" not in d["config"]
    B, T, U = 32, 1000, 200  # BASELINE configs[1]
    assert abs(d["value"] - B * T * U / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert 0.0 < r["frac"] < 1.0
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["unit"] == "cells/s" and c["cores"] >= 1


import pytest


@pytest.mark.parametrize("rnd", ["r01", "r02"])
def test_committed_fp32_bench_line(rnd):
    d = _line(f"{rnd}_bench_default.json")
    _check(d, "f32")
    assert d["roofline"]["bound"] == "mfma" and d["roofline"]["peak"] == 157.3
    if rnd != "r01":
        assert d["roofline"]["traffic"] > 0 and d["hipGetDeviceCount"] >= 1 and d["rccl_ranks"] == 0
        assert "median of 3 runs" in d["cpu_baseline"]["sample"]


@pytest.mark.parametrize("rnd", ["r01", "r02"])
def test_committed_bf16_bench_line(rnd):
    d = _line(f"{rnd}_bf16_bench_default.json")
    _check(d, "bf16")
    assert d["roofline"]["bound"] == "hbm" and d["roofline"]["peak"] == 8000.0
    if rnd != "r01":
        assert d["steps"] == 20


def test_committed_round4_bf16x3_bench_line():
    """Round 4's first default (bf16x3 arithmetic, fp32-accurate; kept as profiles/r04_bf16x3_bench_default.json): the line
    carries the exact-fp32 route timed in the same run, the MFMA-busy figure replayed from the committed SQ counter pass, and
    names its ranks by transport."""
    d = _line("r04_bf16x3_bench_default.json")
    _check(d, "f32")
    r = d["roofline"]
    assert r["bound"] == "mfma" and abs(r["peak"] - 2500.0 / 6.0) < 1e-6 and r["traffic"] > 0
    assert 0.3 < r["mfma_busy"] < 1.0 and r["mfma_busy_source"]["replayed"] is True
    assert os.path.exists(os.path.join(ROOT, r["mfma_busy_source"]["file"])) and os.path.exists(os.path.join(ROOT, r["traffic_source"]["file"]))
    e = d["exact_fp32"]
    assert e["peak"] == 157.3 and abs(e["frac"] - e["path_tflops"] / 157.3) < 1e-9 and e["ms_per_step"] > d["ms_per_step"]
    assert abs(e["loss"] - d["loss"]) <= 1e-4 * abs(d["loss"])  # the two arithmetic forms agree on the same inputs
    assert d["rccl_ranks"] == 0 and "dist_ranks" not in d and d["steps"] == 20
    assert d["parity"]["loss_rel_err"] < 1e-4 and d["parity"]["grad_rel_err"] < 1e-4
    c4 = _line("r04_cfg4_bf16x3_bench.json")  # config 4 on that route: a kept record
    assert "cfg4" in c4["config"]["workload"] and "bf16x3" in c4["config"]["workload"] and c4["ms_per_step"] > 0


def test_committed_round4_default_bench_line():
    """The shipped default (f16x2 arithmetic: three fp16 products of scaled, 2-way split operands, fp32-class): the line carries
    the exact-fp32 route AND the bf16x3 route timed in the same run on the same inputs (all three agree on the loss), both
    rooflines of the dominant kernel, the replayed PMC figures, the CPU baseline."""
    d = _line("r04_bench_default.json")
    _check(d, "f32")
    assert "f16x2" in d["config"]["workload"] and "v_mfma_f32_32x32x16_f16" in d["arith"]
    r = d["roofline"]
    assert r["bound"] == "mfma" and abs(r["peak"] - 2500.0 / 3.0) < 1e-6 and r["traffic"] > 0
    assert 0.2 < r["mfma_busy"] < 1.0 and r["mfma_busy_source"]["replayed"] is True
    assert os.path.exists(os.path.join(ROOT, r["mfma_busy_source"]["file"])) and os.path.exists(os.path.join(ROOT, r["traffic_source"]["file"]))
    assert 0.0 < r["hbm"]["frac"] < 1.0 and r["hbm"]["peak"] == 8000.0
    e, x3 = d["exact_fp32"], d["bf16x3"]
    assert e["peak"] == 157.3 and e["ms_per_step"] > x3["ms_per_step"] > d["ms_per_step"]
    for other in (e, x3):  # the three arithmetic forms agree on the same inputs
        assert abs(other["loss"] - d["loss"]) <= 1e-4 * abs(d["loss"])
    assert d["rccl_ranks"] == 0 and "dist_ranks" not in d and d["steps"] == 20
    assert d["parity"]["loss_rel_err"] < 1e-4 and d["parity"]["grad_rel_err"] < 1e-4
    assert d["ms_per_step"] < 85.0  # round-3 verdict item 1's target for config 2
    for name in ("cfg4", "cfg5"):  # configs 4 and 5 on the shipped default route: kept records
        c = _line(f"r04_{name}_f16x2_bench.json")
        assert name in c["config"]["workload"] and "f16x2" in c["config"]["workload"] and c["ms_per_step"] > 0


def test_committed_round5_default_bench_line():
    """Round 5: the same shipped route with an HONEST dtype label — "f32(f16x2)" (22-bit operands), never plain "f32", which the line
    keeps for `exact_fp32` — the round-5 kernels' own PMC figures replayed, and config 4 with its last 128 dHidden columns on
    k_dhidden_x2r (step <= 225 ms, dHidden <= 78 ms: the round-4 verdict's targets)."""
    d = _line("r05_bench_default.json")
    _check(d, "f32(f16x2)")
    assert "f16x2" in d["config"]["workload"] and "v_mfma_f32_32x32x16_f16" in d["arith"]
    r = d["roofline"]
    assert r["bound"] == "mfma" and abs(r["peak"] - 2500.0 / 3.0) < 1e-6 and r["traffic"] > 0 and r["frac"] > 0.37
    assert os.path.exists(os.path.join(ROOT, r["mfma_busy_source"]["file"])) and os.path.exists(os.path.join(ROOT, r["traffic_source"]["file"]))
    e, x3 = d["exact_fp32"], d["bf16x3"]
    assert e["peak"] == 157.3 and e["ms_per_step"] > x3["ms_per_step"] > d["ms_per_step"]
    for other in (e, x3):
        assert abs(other["loss"] - d["loss"]) <= 1e-4 * abs(d["loss"])
    assert d["parity"]["loss_rel_err"] < 1e-4 and d["parity"]["grad_rel_err"] < 1e-4
    assert d["ms_per_step"] < 58.0  # (round 4: 58.2-59.6)
    c4 = _line("r05_cfg4_f16x2_bench.json")
    assert "cfg4" in c4["config"]["workload"] and c4["ms_per_step"] <= 225.0 and c4["stages_ms"]["dhidden_gemm"] <= 78.0
    b = _line("r05_bf16_bench.json")
    assert b["dtype"] == "bf16" and b["ms_per_step"] < 26.0  # (round 4: 26.45)


def test_bench_refuses_to_run_fewer_gpus_than_asked():
    """`python bench.py --gpus N` with no launcher (WORLD_SIZE unset) starts the N ranks itself and
    must exit non-zero — never fall through to a 1-GPU run — when fewer than N devices exist."""
    import subprocess
    import sys

    import pytest
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("this box has >= 2 GPUs: the self-launch would really run")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode != 0
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert "error" in line and line["n_gpus_requested"] == 2 and line["hipGetDeviceCount"] < 2


def test_dump_outputs_fits_the_budget_and_samples_reproducibly(tmp_path):
    """bench.py --dump-outputs writes through bench.dump_outputs: float32 .npy files, all together within the byte budget;
    arrays that fit are written whole, a larger one as a sample whose indices depend on the seed only, so two dumps of
    the same arguments compare element for element."""
    import numpy as np

    import bench
    rng = np.random.default_rng(0)
    big = rng.standard_normal((300, 1000)).astype(np.float32)
    small = rng.standard_normal((4, 5))
    arrays = [("loss", np.float32(3.5)), ("big", big), ("small", small)]
    budget = 600_000
    info = bench.dump_outputs(str(tmp_path / "a"), arrays, max_bytes=budget)
    bench.dump_outputs(str(tmp_path / "b"), arrays, max_bytes=budget)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "loss.npy", "small.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= budget
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float32 and np.array_equal(x, y)
    assert not info["loss"]["sampled"] and not info["small"]["sampled"] and info["big"]["sampled"]
    assert info["big"]["shape"] == [300, 1000]
    loss = np.load(tmp_path / "a" / "loss.npy")
    assert loss.shape == () and loss == np.float32(3.5)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "small.npy"), small.astype(np.float32))
    sample = np.load(tmp_path / "a" / "big.npy")
    assert sample.shape == (info["big"]["elements"],) and 100_000 < sample.size < 150_000
    flat = big.reshape(-1)
    pos = np.searchsorted(np.sort(flat), sample)
    assert np.array_equal(np.sort(flat)[pos], sample)  # every sampled value is one of the array's
    # the default budget holds for the largest headline output (config 4's grad_enc: 82 MB in float32)
    B, T, U, H, V = bench.CONFIGS["cfg4"]
    info = bench.dump_outputs(str(tmp_path / "c"), [("grad_enc", np.zeros((B, T, H), np.float32)),
                                                   ("grad_pred", np.zeros((B, U + 1, H), np.float32))])
    assert info["grad_enc"]["sampled"] and not info["grad_pred"]["sampled"]
    assert sum(os.path.getsize(tmp_path / "c" / f) for f in os.listdir(tmp_path / "c")) <= bench.DUMP_MAX_BYTES


def test_bench_inputs_are_the_same_every_run():
    """The benchmark's inputs come from a seeded generator: the same arguments give the same tensors, so the outputs
    --dump-outputs writes for two builds are comparable."""
    import torch

    import bench
    a = bench.synth(2, 30, 7, 64, 128, 1234, "cpu")
    b = bench.synth(2, 30, 7, 64, 128, 1234, "cpu")
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_bench_refuses_zero_steps():
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "--steps" in out.stderr


@pytest.mark.gpu
def test_bench_dump_outputs_are_what_the_timed_step_computed(tmp_path):
    """`bench.py --dump-outputs DIR` on a small config: the result line reports the number of timed steps asked for and
    ms_per_step, and DIR holds the loss, costs and four gradients of the fused step on the bench's seeded inputs, equal
    to one call of the engine on the same inputs."""
    import subprocess
    import sys

    import numpy as np
    import torch

    import bench
    import rnnt_amd
    d = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "small", "--steps", "3",
                          "--warmup", "1", "--no-cpu-baseline", "--no-stage-timing", "--no-exact-fp32", "--dump-outputs", str(d)],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-1500:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    names = ["loss", "costs", "grad_enc", "grad_pred", "grad_W", "grad_bias"]
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in names)
    assert sum(os.path.getsize(d / (n + ".npy")) for n in names) <= bench.DUMP_MAX_BYTES
    B, T, U, H, V = bench.CONFIGS["small"]
    enc, pred, W, bias, targets, ll, tl = bench.synth(B, T, U, H, V, 1234, "cuda")
    ref = rnnt_amd.engine.joint_loss_fwd_bwd(enc, pred, W, bias, targets, ll, tl, V - 1, 1.0 / B, dtype="f16x2")
    torch.cuda.synchronize()
    ref = [r.cpu().numpy() for r in ref]
    for name, r in zip(names[1:], ref):
        got = np.load(d / (name + ".npy"))
        assert got.dtype == np.float32 and got.shape == r.shape, name
        np.testing.assert_allclose(got, r, rtol=0, atol=1e-6 * np.abs(r).max(), err_msg=name)
    loss = float(np.load(d / "loss.npy"))
    assert abs(loss - float(ref[0].astype(np.float64).sum()) / B) <= 1e-5 * abs(loss)


def _bench_line(*args):
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "small", "--steps", "3",
                          "--warmup", "1"] + list(args), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-1500:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_full_run_carries_the_rest():
    """A plain run prints the headline line only; --full on the same arguments adds the per-stage timing and roofline, the
    other fp32-bar routes, the parity twin and the CPU baseline.  Both time the same steps on the same inputs: the headline
    fields are there in both and the losses agree."""
    import bench
    B, T, U, H, V = bench.CONFIGS["small"]
    plain = _bench_line()
    full = _bench_line("--full")
    extras = ("stages_ms", "roofline", "lattice_sweep", "exact_fp32", "bf16x3", "parity", "cpu_baseline", "gpu_over_cpu")
    for k in extras:
        assert k not in plain, k
        assert k in full, k
    for d in (plain, full):
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "loss"):
            assert k in d, k
        assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "cells/s" and d["higher_is_better"] is True
        assert d["dtype"] == "f32(f16x2)" and d["ms_per_step"] > 0
        assert abs(d["value"] - B * T * U / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    assert abs(plain["loss"] - full["loss"]) <= 1e-6 * abs(full["loss"])
    assert set(full["stages_ms"]) >= {"joint_fwd_gemm", "lattice_sweep", "dhidden_gemm", "dw_gemm"}
    assert 0.0 < full["roofline"]["frac"] < 1.0
    for route in ("exact_fp32", "bf16x3"):
        assert abs(full[route]["loss"] - full["loss"]) <= 1e-4 * abs(full["loss"])
    assert full["parity"]["loss_rel_err"] < 1e-4 and full["parity"]["grad_rel_err"] < 1e-4
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["kind"] == "port"
