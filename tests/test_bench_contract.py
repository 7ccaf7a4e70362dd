"""bench.py's launch contract: `--gpus N` starts N ranks by itself when no launcher did, the N > 1
path runs (gloo stand-in for RCCL on a single-GPU box: all ranks share device 0), a plain run times the
headline alone, and with `--full` the one JSON line carries the headline, `roofline`, `cpu_baseline`, `configs`
and `boundary_inclusive`."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env=None, timeout=900):
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout,
                          env=dict(os.environ, **(env or {})), cwd=ROOT)


def _json_line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0])


def test_bench_fails_loudly_without_a_gpu_or_with_too_few():
    """No CPU fallback: without a device (this container) every form of the command exits non-zero with a
    message; on a GPU box asking for more GPUs than the node has does."""
    import torch
    if torch.cuda.is_available():
        r = _run(["--gpus", str(torch.cuda.device_count() + 1), "--steps", "1", "--warmup", "0"])
        assert r.returncode != 0 and "GPU(s) visible" in (r.stderr + r.stdout)
    else:
        for a in (["--steps", "1"], ["--gpus", "2", "--steps", "1"], ["--full", "--steps", "1"]):
            r = _run(a)
            assert r.returncode != 0 and "needs an MI355X" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_bench_gpus_2_launches_its_own_ranks():
    r = _run(["--gpus", "2", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-configs"],
             env={"MI_BENCH_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-3000:]
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "weak"
    assert d["config"]["global_batch"] == 2048 and d["value"] > 0
    one = _json_line(_run(["--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-configs"]).stdout)
    assert one["n_gpus"] == 1 and one["config"]["global_batch"] == 1024
    # weak scaling: every rank solves 1024 problems per step (its block of the 2048-problem global draw), so
    # rank 0's iterations per step stay within a few percent of the single-rank batch's
    assert abs(d["iterations_per_step_rank0"] - one["iterations_per_step_rank0"]) < 0.05 * one["iterations_per_step_rank0"]
    assert d["converged_rank0"] == 1024


@pytest.mark.gpu
def test_bench_line_carries_every_config_and_the_boundary():
    r = _run(["--full", "--steps", "5", "--warmup", "2", "--cpu-sample", "4"])
    assert r.returncode == 0, r.stderr[-3000:]
    d = _json_line(r.stdout)
    assert d["full"] is True and d["value_cold_clock"] > 0 and d["ms_per_step_cold_clock"] > 0
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "configs", "boundary_inclusive"):
        assert k in d, k
    assert d["dtype"] == "f64" and d["vs_baseline"] is None and "workload" in d["config"]
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and rf["kernel_ms"] > 0
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] >= 1 and d["cpu_baseline"]["value"] > 0
    names = [c["name"][:2] for c in d["configs"]]
    assert names[:5] == ["C1", "C3", "C4", "C5", "C5"]
    for c in d["configs"]:
        assert c["iterations_per_s"] > 0 and c["ms_per_solve"] > 0 and c["kernel_ms_per_solve"] > 0 and 0 < c["hbm_frac"] < 1
        assert c["converged"] == c["batch"] or c["name"].startswith("C4")       # (C4: long contact solves may hit no cap, all converge too)
    assert d["configs"][3]["backward_fp64_TFLOPs_per_gpu"] > 0
    b = d["boundary_inclusive"]
    assert b["ms_per_solve"] > d["ms_per_step"] and b["bytes_out"] > b["bytes_in"]
    assert b["pinned_results_shared_guess"]["ms_per_solve"] > d["ms_per_step"] and b["pinned_results_shared_guess"]["bytes_in"] < b["bytes_in"]
    assert d["clock_ramp_steps"] >= 0 and "order" in d and "kernel_ms_source" in rf
    cb = d["concurrent_batches"]["runs"]
    assert [r_["handles"] for r_ in cb] == [2, 4] and all(r_["iterations_per_s"] > 0.8 * d["value"] for r_ in cb)


PLAIN_OVERHEAD_S = 30.0     # what a plain run may spend outside its warm-up and timed steps


@pytest.mark.gpu
def test_bench_plain_run_times_the_headline_alone():
    """`bench.py --gpus 1 --steps K --warmup W` without --full: set-up, warm-up, the K timed steps and the line - the headline's
    keys as ever, null for everything that has runs of its own (they are --full's), the counters from the committed passes, and
    at most PLAIN_OVERHEAD_S of the whole process (start to exit) outside its K + W steps."""
    steps, warmup = 20, 3
    t0 = time.perf_counter()
    r = _run(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)])
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    d = _json_line(r.stdout)
    assert d["metric"] == "iLQR iterations/sec (batch, whole node)" and d["unit"] == "iterations/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["converged_rank0"] == 1024
    assert abs(d["value"] - d["iterations_per_step_rank0"] / (d["ms_per_step"] * 1e-3)) < 1e-9 * d["value"]
    assert d["full"] is False
    for k in ("cpu_baseline", "configs", "boundary_inclusive", "concurrent_batches", "value_cold_clock", "ms_per_step_cold_clock",
              "strong_scaling", "value_strong"):
        assert d[k] is None, k
    rf = d["roofline"]
    assert rf["kernel_ms"] > 0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    assert rf["traffic_source"] is None or rf["traffic_source"].startswith("committed ")
    assert d["roofline_compute"] is None or d["roofline_compute"]["source"].startswith("committed ")
    outside = wall - (steps + warmup) * d["ms_per_step"] * 1e-3
    print(f"plain run: {wall:.2f} s start to exit, {outside:.2f} s outside its {steps} + {warmup} steps")
    assert outside <= PLAIN_OVERHEAD_S, (wall, outside)


def test_dump_outputs_samples_a_fixed_subset_above_the_cap(tmp_path, monkeypatch):
    """dump_outputs on a stand-in for the solver: below the cap every problem is written; above it a fixed, sorted sample of
    problems that fits the cap, the same on every call, with its indices in problem_index.npy."""
    import types
    import numpy as np
    import bench
    B, n, m, N = 1000, 2, 1, 50
    rng = np.random.default_rng(5)
    s = types.SimpleNamespace(B=B, x_bar=rng.standard_normal((B, n, N)), u_bar=rng.standard_normal((B, m, N - 1)),
                              cost=rng.standard_normal(B), iterations=np.arange(B, dtype=np.int32), status=np.zeros(B, np.int32))
    bench.dump_outputs(s, str(tmp_path / "all"))
    assert np.array_equal(np.load(tmp_path / "all" / "x_bar.npy"), s.x_bar) and not (tmp_path / "all" / "problem_index.npy").exists()
    cap = 200 * 1024
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", cap)
    for d in ("a", "b"):
        bench.dump_outputs(s, str(tmp_path / d))
    files = sorted((tmp_path / "a").iterdir())
    assert sum(f.stat().st_size - 128 for f in files) <= cap                  # (.npy header: 128 bytes)
    idx = np.load(tmp_path / "a" / "problem_index.npy")
    assert 0 < len(idx) < B and np.all(np.diff(idx) > 0) and idx.dtype == np.float64
    assert np.array_equal(idx, np.load(tmp_path / "b" / "problem_index.npy"))
    i = idx.astype(int)
    assert np.array_equal(np.load(tmp_path / "a" / "u_bar.npy"), s.u_bar[i])
    assert np.array_equal(np.load(tmp_path / "a" / "iterations.npy"), i.astype(np.float64))


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_last_steps_results(tmp_path):
    """--dump-outputs DIR: the last timed step's x_bar, u_bar, cost, iterations, status of the 1024 problems as float64 .npy
    files, 64 MB at most.  --steps sets the timed steps; every step is a cold-start solve of the same seeded inputs, so runs
    with another step count leave the same results, bit for bit, and the iterations they hold are the line's."""
    import numpy as np
    got = {}
    for steps in (3, 5):
        out = tmp_path / f"s{steps}"
        r = _run(["--steps", str(steps), "--warmup", "1", "--no-cpu-baseline", "--no-configs", "--dump-outputs", str(out)])
        assert r.returncode == 0, r.stderr[-3000:]
        d = _json_line(r.stdout)
        assert d["steps"] == steps and d["ms_per_step"] > 0
        names = sorted(p.name for p in out.iterdir())
        assert names == ["cost.npy", "iterations.npy", "status.npy", "u_bar.npy", "x_bar.npy"], names
        arrs = {n[:-4]: np.load(out / n) for n in names}
        assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
        assert all(a.dtype == np.float64 for a in arrs.values())
        assert arrs["x_bar"].shape == (1024, 2, 200) and arrs["u_bar"].shape == (1024, 1, 199) and arrs["cost"].shape == (1024,)
        assert np.isfinite(arrs["x_bar"]).all() and (arrs["status"] == 0).all()
        assert arrs["iterations"].sum() == d["iterations_per_step_rank0"]
        got[steps] = arrs
    for k in got[3]:
        assert np.array_equal(got[3][k], got[5][k]), k


_ONE_RANK = {}


def _one_rank_configs():
    """The single-rank run with every config (cached for the sharded runs to be compared with)."""
    if "d" not in _ONE_RANK:
        r = _run(["--full", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"])
        assert r.returncode == 0, r.stderr[-3000:]
        _ONE_RANK["d"] = _json_line(r.stdout)
    return _ONE_RANK["d"]


@pytest.mark.gpu
# (at most 3 ranks: with this test process and bench.py's own launcher, 5 processes then hold the device, and a shared GPU
#  node allows no more than 6; 3 ranks also give uneven shards: C3's 512 -> 171/171/170, C5's 64 -> 22/21/21)
@pytest.mark.parametrize("world", [2, 3])
def test_bench_sharded_configs_do_exactly_the_whole_batchs_work(world):
    """`bench.py --full --gpus N` WITH every config (C1, C3 ... C6b through run_config's shard path: C3 at 512 / N problems per rank, C5 at
    64 / N, C1's single problem on rank 0 alone), N ranks over gloo sharing this box's GPU - the form of the run a multi-GPU
    node executes over RCCL.  Problems are independent and every kernel's result is independent of its batch,
    so the ranks together must do EXACTLY the single-rank run's work: the same iterations per config (rank-summed), every problem
    converged, batch_per_gpu = ceil(B / N); the line says how many ranks and which collective."""
    one = _one_rank_configs()
    r = _run(["--full", "--gpus", str(world), "--steps", "2", "--warmup", "1", "--no-cpu-baseline"], env={"MI_BENCH_BACKEND": "gloo"}, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _json_line(r.stdout)
    assert d["n_gpus"] == world and d["scaling"] == "weak" and d["config"]["global_batch"] == 1024 * world
    assert d["config"]["parallelism"] == f"batch-shard x{world}" and "all_reduce(MIN)" in d["config"]["collective"]
    # round 6: the N > 1 line checks itself - the communicator's rank count, every rank's own iteration sum, the strong-scaling
    # figure (C2's 1024 problems sharded over the ranks) beside the weak one, and why the library's own communicator was not
    # used (gloo ranks share this box's one GPU; on the driver's node it is, after a self-check)
    assert d["communicator_ranks"] == world and "share a device" in d["config"]["collective_fallback_reason"]
    ipr = d["iterations_per_rank"]
    assert len(ipr) == world and all(v > 0 for v in ipr) and abs(sum(ipr) - d["value"] * d["ms_per_step"] * 1e-3 * d["steps"]) < 1e-6 * sum(ipr)
    sg = d["strong_scaling"]
    assert d["value_strong"] == sg["value"] > 0 and sg["global_batch"] == 1024 and len(sg["iterations_per_rank"]) == world
    # the shards of the single-GPU run's own batch do exactly its work: K steps x the single-rank run's iterations per step
    assert abs(sum(sg["iterations_per_rank"]) - d["steps"] * one["iterations_per_step_rank0"]) < 0.5
    ref = {c["name"]: c for c in one["configs"]}
    names = [c["name"] for c in d["configs"]]
    assert [n[:3].strip() for n in names] == ["C1", "C3", "C4", "C5", "C5q", "C5q", "C6", "C6b"], names     # (the B = 8 shard line is a 1-rank entry)
    for c in d["configs"]:
        o = ref[c["name"]]
        assert c["batch"] == o["batch"] and c["batch_per_gpu"] == -(-c["batch"] // world), c["name"]
        assert c["iterations"] == o["iterations"], (c["name"], c["iterations"], o["iterations"])
        assert c["converged"] == o["converged"] and (c["converged"] == c["batch"] or c["name"].startswith("C4")), (c["name"], c["converged"], o["converged"])
        assert c["max_iterations_per_problem"] == o["max_iterations_per_problem"]
        assert c["iterations_per_s"] > 0 and c["ms_per_solve"] > 0
    assert d["boundary_inclusive"] is not None and d["concurrent_batches"] is None
    # headline: weak scaling, rank 0 solves its 1024-problem block of the 1024 N drawn with one seed (another draw than the single-rank batch)
    assert abs(d["iterations_per_step_rank0"] - one["iterations_per_step_rank0"]) < 0.05 * one["iterations_per_step_rank0"] and d["converged_rank0"] == 1024


@pytest.mark.gpu
def test_bench_native_rccl_communicator_two_ranks():
    """MI_BENCH_NATIVE_RCCL=1: the best-cost reduction through the LIBRARY's communicator (mi_ilqr_comm_create over librccl, the C
    caller's path), the ranks and the 128-byte id shipped by torch.distributed.  With two GPUs it runs; on a one-GPU box RCCL
    refuses two ranks on one device - the run must then stop with the library's own message, not hang or fall back."""
    import torch
    r = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-configs"],
             env={"MI_BENCH_BACKEND": "gloo", "MI_BENCH_NATIVE_RCCL": "1"}, timeout=600)
    if torch.cuda.device_count() >= 2:
        assert r.returncode == 0, r.stderr[-3000:]
        assert "mi_ilqr_allreduce_min_start" in _json_line(r.stdout)["config"]["collective"]
    else:
        assert r.returncode != 0
        assert "ncclCommInitRank failed" in r.stderr and "mi_ilqr_comm_create" in r.stderr, r.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("stall", [False, True])
def test_bench_falls_back_when_the_library_communicator_fails_or_never_answers(stall):
    """The default N > 1 run tries the library's own communicator first.  Two ranks on this box's one GPU: RCCL refuses the second
    rank (an error), or - MI_BENCH_NATIVE_TEST_STALL - the attempt never returns (a bootstrap that hangs); either way every rank
    agrees on torch.distributed, the reason is in the line and the run finishes."""
    import torch
    if torch.cuda.device_count() >= 2 and not stall:
        pytest.skip("two GPUs: the communicator comes up (test_bench_native_rccl_communicator_two_ranks)")
    env = {"MI_BENCH_BACKEND": "gloo", "MI_BENCH_NATIVE_RCCL": "try"}
    if stall:
        env.update(MI_BENCH_NATIVE_TEST_STALL="1", MI_BENCH_NATIVE_DEADLINE_S="5")
    r = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-configs"], env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _json_line(r.stdout)
    assert "torch.distributed all_reduce(MIN)" in d["config"]["collective"]
    why = d["config"]["collective_fallback_reason"]
    assert ("no answer from librccl within" in why) if stall else ("mi_ilqr_comm_create: RCCL error" in why), why
    assert d["n_gpus"] == 2 and d["value"] > 0
