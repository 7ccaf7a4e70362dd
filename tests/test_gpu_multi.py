"""Multi-GPU readiness: every rank on its own GPU on a node with >= 2 GPUs.

* the library's own RCCL communicator with world = 2..N ranks contributing different values (min, not avg);
* the shard partitioning: all-reduce(min) over the shards' best costs == min over the whole batch on one GPU;
* `bench.py --gpus N` on the nccl (= RCCL) backend: n_gpus, weak-scaling batch, rank-summed iterations.

RCCL refuses two ranks of one node on one device, so on a one-GPU node the ranks share device 0 and reduce through
torch.distributed over gloo (the path bench.py falls back to), and the library's communicator is held to refusing them
with its own error instead of hanging."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _n_gpus():
    try:
        import torch
        return torch.cuda.device_count() if torch.cuda.is_available() else 0
    except Exception:  # pragma: no cover
        return 0


# ranks started at once: with this test process (and bench.py's launcher) the processes holding a GPU stay at 6 at most
MAX_RANKS = 4


def _worlds():
    n = min(_n_gpus(), MAX_RANKS)
    return sorted({w for w in (2, 4, n) if 2 <= w <= n}) or [2]


@pytest.mark.gpu
@pytest.mark.parametrize("world", _worlds())
def test_native_rccl_min_and_sharded_solve(world, tmp_path):
    """`world` ranks, one GPU each, reducing through the library's communicator - on a node with fewer GPUs than ranks they
    share device 0 and reduce through torch.distributed (gloo).  Same assertions either way."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    mode = [] if _n_gpus() >= world else ["gloo"]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_multi_worker.py"), str(r), str(world), str(tmp_path)] + mode,
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{o[-3000:]}"
    res = [json.load(open(tmp_path / f"ok.{r}")) for r in range(world)]
    assert len({x["best"] for x in res}) == 1                       # every rank holds the same global best cost
    assert sum(x["iters"] for x in res) == res[0]["whole_iters"]    # shards do exactly the whole batch's iterations
    assert res[0]["lo"] == 0 and res[-1]["hi"] == 64 and all(a["hi"] == b["lo"] for a, b in zip(res, res[1:]))


@pytest.mark.gpu
def test_native_rccl_min_with_two_ranks_on_one_gpu(tmp_path):
    """The library's communicator with world = 2 on a ONE-GPU box: both ranks (two processes) on device 0.  Ranks contribute
    different values to mi_ilqr_allreduce_min (min - not avg, not sum), then each solves its shard and the reduced best cost
    equals the whole batch's.  RCCL builds that refuse two ranks of one node on one device ("Duplicate GPU", invalid usage)
    must make the library say so: every rank then stops in mi_ilqr_comm_create with RCCL's error - none hangs, none goes on."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", NCCL_DEBUG=os.environ.get("NCCL_DEBUG", "WARN"))
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_multi_worker.py"), str(r), "2", str(tmp_path), "same"],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=300)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    if any(p.returncode != 0 for p in procs):
        text = "\n".join(outs)
        markers = ("Duplicate GPU", "duplicate GPU", "invalid usage", "ncclInvalidUsage")
        assert any(m in text for m in markers), "rank(s) failed:\n" + text[-4000:]
        for r, (p, o) in enumerate(zip(procs, outs)):                 # the refusal: every rank, through the library's own error
            assert p.returncode != 0 and "mi_ilqr_comm_create" in o and not os.path.exists(tmp_path / f"ok.{r}"), (r, o[-3000:])
        return
    res = [json.load(open(tmp_path / f"ok.{r}")) for r in range(2)]
    assert res[0]["best"] == res[1]["best"] and res[0]["iters"] + res[1]["iters"] == res[0]["whole_iters"]
    assert (res[0]["lo"], res[0]["hi"], res[1]["lo"], res[1]["hi"]) == (0, 32, 32, 64)


@pytest.mark.gpu
def test_bench_on_rccl_all_gpus():
    """`bench.py --gpus N` over up to MAX_RANKS GPUs on RCCL; on a one-GPU node two ranks share it over gloo."""
    n = min(_n_gpus(), MAX_RANKS)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    if n < 2:
        n, env["MI_BENCH_BACKEND"] = 2, "gloo"
    tail = ["--steps", "8", "--warmup", "2", "--no-cpu-baseline", "--no-configs"]
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + tail,
                         env=env, capture_output=True, text=True, timeout=900)
    assert one.returncode == 0, one.stdout[-2000:] + one.stderr[-2000:]
    many = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n)] + tail,
                          env=env, capture_output=True, text=True, timeout=900)
    assert many.returncode == 0, many.stdout[-2000:] + many.stderr[-2000:]
    j1 = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][-1])
    jn = json.loads([l for l in many.stdout.splitlines() if l.startswith("{")][-1])
    assert jn["n_gpus"] == n and jn["scaling"] == "weak"
    assert jn["config"]["global_batch"] == n * j1["config"]["global_batch"]
    # weak scaling of independent shards: the ranks' summed iterations per step = N x one rank's (different seeds
    # of the same distribution: within 5 %)
    per_step = lambda j: j["value"] * j["ms_per_step"] * 1e-3          # iterations of all ranks in one step
    assert abs(per_step(jn) - n * per_step(j1)) <= 0.05 * n * per_step(j1)
    assert "all_reduce" in jn["config"]["collective"] or "all-reduce" in jn["config"]["collective"]
