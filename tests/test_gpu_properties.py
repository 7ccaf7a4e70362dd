"""GPU tests at BASELINE.json's full sizes through size-independent properties, plus the edge
cases of the reference's control flow (line-search exhaustion, iteration cap, warm starts,
SaveSolution), all through the C ABI."""
import os

import numpy as np
import pytest

from common import assert_flip_budget

from test_gpu_parity import make_solver

pytestmark = pytest.mark.gpu


def c2_setup(B, **kw):
    from drake_ddp_amd import workloads as W
    prob = W.pendulum_problem()
    x0 = W.pendulum_batch_x0(1024)[:B]
    s = make_solver(prob, B=B, jac="fd", **kw)
    s.SetInitialState(x0)
    s.SetInitialGuess(np.zeros((1, prob["N"] - 1)))
    return prob, x0, s


def test_c2_full_batch_properties():
    """B=1024 (config C2): every problem converges, costs decrease monotonically, the solution is a
    fixed point of the dynamics, batch element i == the same problem solved alone or in a different
    batch position (bitwise: problems never interact), and two 512-problem shards == the full batch."""
    from drake_ddp_amd import workloads as W
    from oracle import models_np as M
    prob, x0, s = c2_setup(1024)
    x, u, _, L = s.Solve()
    it, st = s.iterations, s.status
    assert (st == 0).all() and it.min() >= 2 and it.max() < 64
    h = s.history
    for b in range(0, 1024, 37):
        costs = h[b, :it[b], 0]
        assert np.all(np.diff(costs) < 0)                               # accepted steps only ever decrease L
        assert abs(costs[-1] - L[b]) == 0
        assert costs[-2] - costs[-1] <= prob["delta"]                   # termination rule (ilqr.py:692)
    # returned trajectory satisfies x_{t+1} = f(x_t,u_t) under the oracle's model to round-off
    model = M.Model(prob["model_id"], prob["dt"])
    for b in (0, 511, 1023):
        xr = x[b][:, 0].copy()
        assert np.array_equal(xr, x0[b])
        for t in range(prob["N"] - 1):
            xr = model.step(xr, u[b][:, t])
            assert np.max(np.abs(xr - x[b][:, t + 1])) < 1e-9
    # every one of the 1024 problems against the C oracle (pinned to the reference's goldens)
    from oracle import c_oracle
    r = c_oracle.solve_batch(model, prob, x0, np.zeros((1, prob["N"] - 1)))
    assert np.array_equal(r["iters"], it) and np.array_equal(r["ls"], s.ls_trials) and (r["status"] == 0).all()
    assert np.max(np.abs(L - r["cost"]) / np.abs(r["cost"])) < 5e-8       # both sides central FD: 1e-16/h round-off amplification
    assert np.max(np.abs(x - r["x_bar"])) < 1e-6 and np.max(np.abs(u - r["u_bar"])) < 1e-6
    assert np.max(np.abs(s.K - r["K"])) / np.max(np.abs(r["K"])) < 1e-6
    # permutation / position invariance, bitwise
    perm = np.random.default_rng(0).permutation(1024)
    _, _, s2 = c2_setup(1024)
    s2.SetInitialState(x0[perm])
    x2, u2, _, L2 = s2.Solve()
    assert np.array_equal(L2, L[perm]) and np.array_equal(x2, x[perm]) and np.array_equal(s2.K, s.K[perm])
    # shard invariance (what the multi-GPU path relies on): two handles of 512 == one of 1024
    from drake_ddp_amd.dist import shard_range
    for r in range(2):
        lo, hi = shard_range(1024, r, 2)
        _, _, sh = c2_setup(hi - lo)
        sh.SetInitialState(x0[lo:hi])
        xs, us, _, Ls = sh.Solve()
        assert np.array_equal(Ls, L[lo:hi]) and np.array_equal(xs, x[lo:hi]) and np.array_equal(us, u[lo:hi])
    # single-problem class == batch element
    from drake_ddp_amd.ilqr import IterativeLinearQuadraticRegulator
    from drake_ddp_amd.models import ModelSystem
    one = IterativeLinearQuadraticRegulator(ModelSystem(prob["model_id"], prob["dt"]), prob["N"], delta=prob["delta"],
                                            beta=prob["beta"], gamma=prob["gamma"], jacobian_mode="fd", verbose=False)
    one.SetTargetState(prob["x_nom"]); one.SetRunningCost(prob["Q"], prob["R"]); one.SetTerminalCost(prob["Qf"])
    one.SetInitialState(x0[77]); one.SetInitialGuess(np.zeros((1, prob["N"] - 1)))
    x1, u1, _, L1 = one.Solve()
    assert L1 == L[77] and np.array_equal(x1, x[77]) and np.array_equal(u1, u[77])
    assert x1.shape == (2, 200) and u1.shape == (1, 199) and one.K.shape == (1, 2, 199)


@pytest.mark.parametrize("B,N", [(1, 4), (3, 5), (65, 17)])
def test_ragged_sizes_vs_oracle(B, N):
    from drake_ddp_amd import workloads as W
    from common import make_oracle, rel_err
    prob = dict(W.pendulum_problem(), N=N)
    x0 = W.pendulum_batch_x0(128, seed=3)[:B]
    s = make_solver(prob, B=B, jac="ad")
    s.SetInitialState(x0)
    s.SetInitialGuess(np.zeros((1, N - 1)))
    x, u, _, L = s.Solve()
    for b in range(0, B, max(1, B // 4)):
        o = make_oracle(prob)
        o.set_problem(x0[b], prob["x_nom"], prob["Q"], prob["R"], prob["Qf"], np.zeros((1, N - 1)))
        xo, uo, Lo, hist = o.solve()
        assert len(hist) == s.iterations[b] and abs(L[b] - Lo) < 1e-9 * abs(Lo)
        assert rel_err(x[b], xo) < 1e-9 and rel_err(s.K[b], o.K) < 1e-7


def test_linesearch_exhaustion_and_iteration_cap():
    """ilqr.py:337: RuntimeError after eps < 1e-8; the batch reports it per problem instead."""
    from drake_ddp_amd import workloads as W
    from drake_ddp_amd.ilqr import IterativeLinearQuadraticRegulator
    from drake_ddp_amd.models import ModelSystem
    prob = dict(W.acrobot_problem())                         # beta = 0.5 -> 27 valid eps values
    x0 = W.acrobot_batch_x0(4)
    x0[2, 0] = np.nan                                        # NaN state -> cost NaN -> never accepted
    s = make_solver(prob, B=4, jac="fd")
    s.SetInitialState(x0)
    s.SetInitialGuess(np.zeros((1, prob["N"] - 1)))
    s.Solve()
    st = s.status
    assert st[2] == 2 and (np.delete(st, 2) == 0).all()     # one failed lane does not abort the batch
    assert s.ls_trials[2] == 27 and s.iterations[2] == 0
    assert s.stats.n_ls_failed == 1 and s.stats.n_converged == 3
    one = IterativeLinearQuadraticRegulator(ModelSystem(prob["model_id"], prob["dt"]), prob["N"], beta=0.5, verbose=False)
    one.SetTargetState(prob["x_nom"]); one.SetRunningCost(prob["Q"], prob["R"]); one.SetTerminalCost(prob["Qf"])
    one.SetInitialState(x0[2]); one.SetInitialGuess(np.zeros((1, prob["N"] - 1)))
    with pytest.raises(RuntimeError, match="linesearch failed after 27 iterations"):
        one.Solve()
    # iteration cap (the reference has none; the device needs one)
    capped = make_solver(prob, B=2, jac="fd", max_iters=2)
    capped.SetInitialState(W.acrobot_batch_x0(2))
    capped.SetInitialGuess(np.zeros((1, prob["N"] - 1)))
    capped.Solve()
    assert (capped.status == 1).all() and (capped.iterations == 2).all()


def test_history_cap_and_resolve_semantics(tmp_path):
    """More iterations than hist_cap rows must not corrupt anything; a second Solve() without
    SetInitialGuess continues from the stored u_bar and gains (ilqr.py:375);
    SaveSolution writes the reference's npz keys/shapes (ilqr.py:712-733)."""
    from drake_ddp_amd import workloads as W
    from drake_ddp_amd.ilqr import IterativeLinearQuadraticRegulator
    from drake_ddp_amd.models import ModelSystem
    prob = W.cartpole_wall_problem(N=100)
    s = IterativeLinearQuadraticRegulator(ModelSystem(prob["model_id"], prob["dt"]), prob["N"], beta=prob["beta"],
                                          jacobian_mode="ad", hist_cap=4, verbose=False)
    s.SetTargetState(prob["x_nom"]); s.SetRunningCost(prob["Q"], prob["R"]); s.SetTerminalCost(prob["Qf"])
    s.SetInitialState(np.array([0, np.pi + 0.5, 0, 0.0])); s.SetInitialGuess(np.zeros((1, 99)))
    x, u, _, L = s.Solve()
    assert s.iterations[0] > 4 and np.isfinite(L) and np.all(np.isfinite(s.history[0]))
    x2, u2, _, L2 = s.Solve()                                # warm re-solve from the converged point
    # the first rollout of a re-solve applies the stale gains and is accepted unconditionally (L_last = inf,
    # SURVEY F10), so the cost may tick up before it descends again: same basin, not monotone across solves
    assert s.iterations[0] >= 1 and L2 < 1.05 * L
    f = os.path.join(tmp_path, "sol.npz")
    s.SaveSolution(f)
    z = np.load(f)
    assert sorted(z.files) == ["K", "t", "u_bar", "x_bar"]
    assert z["x_bar"].shape == (4, 99) and z["u_bar"].shape == (1, 99) and z["K"].shape == (1, 4, 99)
    assert z["t"].shape == (99,) and abs(z["t"][1] - prob["dt"]) < 1e-15


def test_c3_c4_c5_configs_converge_at_full_size():
    from drake_ddp_amd import workloads as W
    # C3: acrobot MPC, B=512, 1 + 5 receding-horizon re-solves on the device
    a = W.acrobot_problem()
    s = make_solver(a, B=512, jac="fd")
    s.SetInitialState(W.acrobot_batch_x0(512)); s.SetInitialGuess(np.zeros((1, a["N"] - 1)))
    s.Solve()
    first = s.cost.copy()
    for _ in range(5):
        s.MPCShift(2)
        st = s.solve_resident()
        assert st.n_converged == 512
    assert np.all(np.isfinite(s.cost)) and np.all(np.abs(s.cost - first) < 0.2 * np.abs(first))
    # C4: cart-pole with wall, B=256, FD Jacobians
    c = W.cartpole_wall_problem()
    s = make_solver(c, B=256, jac="fd", hist_cap=8)
    s.SetInitialState(W.cartpole_wall_batch_x0(256)); s.SetInitialGuess(np.zeros((1, c["N"] - 1)))
    _, _, _, L = s.Solve()
    assert (s.status == 0).all() and np.all(L < 200.0) and s.ls_trials.sum() > s.iterations.sum()
    # C5: cheetah-shaped, B=64
    q = W.synth36_problem()
    s = make_solver(q, B=64, jac="fd")
    s.SetInitialState(W.synth36_batch_x0(64)); s.SetInitialGuess(W.synth36_u_guess(q["N"]))
    _, _, _, L = s.Solve()
    assert (s.status == 0).all() and np.all(np.isfinite(L))


@pytest.mark.parametrize("script", ["swingup_pendulum.py", "mpc_acrobot.py", "wall_cartpole.py", "mpc_many_legs.py",
                                    "mpc_planar_quadruped.py", "mpc_mini_cheetah_3d.py", "arm_reach.py", "swingup_cartpole.py",
                                    "arm_push_scenarios.py", "arm_reach.py --coupled"])
def test_example_scripts_run(script):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script, *flags = script.split()
    out = subprocess.run([sys.executable, os.path.join(root, "examples", script)] + flags, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert any(k in out.stdout for k in ("Optimal cost: 0.23997", "device loop", "derivatives evaluated at", "iLQR iterations in the re-solves",
                                         "Optimal cost: 1.15064", "Optimal cost: 3.49189"))
    assert "all converged: False" not in out.stdout


def test_long_horizon_falls_back_to_streaming_kernel():
    """acrobot.py's literal horizon (T=3, dt=0.004 -> N=750, acrobot.py:19-20) does not fit LDS;
    AUTO serves it with the HBM-streaming kernel.  Checked against the oracle."""
    from drake_ddp_amd import workloads as W
    from common import make_oracle, rel_err
    prob = W.acrobot_problem(N=750)
    s = make_solver(prob, B=2, jac="ad", hist_cap=128)
    x0 = np.zeros((2, 4)); x0[1] = [0.05, -0.03, 0.0, 0.0]
    s.SetInitialState(x0)
    s.SetInitialGuess(np.zeros((1, 749)))
    x, u, _, L = s.Solve()
    assert (s.status == 0).all()
    o = make_oracle(prob)
    o.set_problem(x0[1], prob["x_nom"], prob["Q"], prob["R"], prob["Qf"], np.zeros((1, 749)))
    xo, uo, Lo, hist = o.solve()
    assert len(hist) == s.iterations[1]
    assert abs(L[1] - Lo) < 1e-8 * abs(Lo) and rel_err(x[1], xo) < 1e-6


@pytest.mark.parametrize("kp", [("adaptiveJerk", 3, 25, 1e-4, 0.0), ("iterativeError", 4, 0, 0.0, 1e-7), ("setInterval", 7, 0, 0.0, 0.0)])
def test_long_horizon_with_keypoints_vs_c_oracle(kp):
    """acrobot.py's literal N = 750 with the key-point methods (ilqr.py:417-593): does not fit LDS, and until round 3 the
    streaming kernel refused key-points - the combination was E_UNSUPPORTED.  Now served by the lane-per-problem KP
    instantiation: every lane its own key-point list.  Iterations, trials, the key-point count of every iteration and the
    last key-point list exactly the C oracle's on 70 starts (a ragged wave)."""
    from drake_ddp_amd import workloads as W
    from oracle import c_oracle, models_np as M
    prob = W.acrobot_problem(N=750)
    B = 70
    x0 = 0.2 * W.acrobot_batch_x0(512)[:B]
    ug = np.zeros((1, 749))
    s = make_solver(prob, B=B, keypoint=kp, jac="fd", hist_cap=128)
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    x, u, _, L = s.Solve()
    r = c_oracle.solve_batch(M.Model(prob["model_id"], prob["dt"]), prob, x0, ug, keypoint=kp, hist_cap=128)
    same = (s.status == r["status"]) & (s.iterations == r["iters"]) & (s.ls_trials == r["ls"])
    print(f"{kp[0]}: {int(same.sum())}/{B} with the oracle's decisions; converged {int((s.status == 0).sum())}; key-points {s.keypoint_count.min()}..{s.keypoint_count.max()} of 749")
    assert same.all()
    h, nk, kl = s.history, s.keypoint_count, s.keypoint_list
    # (a jerk / an interpolation error within round-off of its threshold - libm against the device's sin / cos - may fall
    # on the other side: at most a key-point or two in an iteration of a few problems, the decisions above unchanged)
    off = 0
    for b in range(B):
        it = min(int(r["iters"][b]), 128)
        mine, ref = np.round(h[b, :it, 3] * 749 / 100.0), r["hist"][b, :it, 3]
        exact = np.array_equal(mine, ref) and nk[b] == r["kp_count"][b] and np.array_equal(kl[b][:nk[b]], r["kp_list"][b][:nk[b]])
        off += not exact
        assert np.abs(mine - ref).max() <= 2 and (mine != ref).sum() <= 2, (b, mine - ref)
    print(f"  key-point counts of every iteration and the last list exact on {B - off}/{B} problems")
    assert off <= 3
    # costs: 749 steps x up to 128 iterations of a swing-up amplify round-off; the yardstick is the C oracle against itself
    # with x0 one ulp away (same decisions), the device may be 10 x that far from the oracle
    ok = s.status == 0
    rel = np.abs(L - r["cost"]) / np.abs(r["cost"])
    own = np.zeros(B)
    for direction in (np.inf, -np.inf):
        xq = x0.copy()
        xq[:, 0] = np.nextafter(xq[:, 0], direction)
        rq = c_oracle.solve_batch(M.Model(prob["model_id"], prob["dt"]), prob, xq, ug, keypoint=kp, hist_cap=128)
        agree = (rq["iters"] == r["iters"]) & (rq["ls"] == r["ls"])
        own = np.maximum(own, np.where(agree, np.abs(rq["cost"] - r["cost"]) / np.abs(r["cost"]), np.inf))
    print(f"  cost: device - oracle max {rel[ok].max():.1e} (median {np.median(rel[ok]):.1e}); oracle - oracle(x0 +- 1 ulp) max {own[np.isfinite(own)].max():.1e} "
          f"(median {np.median(own[np.isfinite(own)]):.1e}), {int((~np.isfinite(own)).sum())} problems change their decisions")
    assert ok.mean() > 0.5 and rel[ok].max() <= max(1e-7, 10 * own[np.isfinite(own)].max())


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_randomized_configs_vs_c_oracle(seed):
    """Random cost weights / beta / gamma / horizons on random batches, every problem compared with the
    C oracle (iterations and line-search trial counts exact, cost 1e-8): exercises backtracking with
    stored candidates, re-rolled winners, gamma > 0 acceptance and ragged batches."""
    from drake_ddp_amd import workloads as W
    from oracle import c_oracle, models_np as M
    rng = np.random.default_rng(100 + seed)
    model_id = [0, 1, 2, 0][seed]
    n = [2, 4, 4, 2][seed]
    N = int(rng.integers(20, 90))
    B = int(rng.integers(40, 150))
    dt = [0.02, 0.01, 0.02, 0.03][seed]
    prob = dict(model_id=model_id, dt=dt, N=N, x_nom=np.concatenate([[np.pi], np.zeros(n - 1)]) if model_id != 2 else np.array([0, np.pi, 0, 0.0]),
                Q=dt * np.diag(rng.uniform(0.0, 2.0, n)), R=dt * np.diag(rng.uniform(0.05, 0.5, 1)),
                Qf=np.diag(rng.uniform(1.0, 50.0, n)), delta=1e-3, beta=float(rng.choice([0.5, 0.7, 0.9])),
                gamma=float(rng.choice([0.0, 0.1])))
    x0 = rng.uniform(-1.0, 1.0, (B, n))
    if model_id == 2:
        x0[:, 1] += np.pi
    ug = rng.uniform(-0.5, 0.5, (B, 1, N - 1))
    s = make_solver(prob, B=B, jac="fd", hist_cap=8)
    s.SetInitialState(x0)
    s.SetInitialGuess(ug)
    x, u, _, L = s.Solve()
    r = c_oracle.solve_batch(M.Model(model_id, dt), prob, x0, ug)
    assert np.array_equal(s.status, r["status"]) and (s.status == 0).all()       # every problem converges on both sides
    it, ls = s.iterations, s.ls_trials
    same = (it == r["iters"]) & (ls == r["ls"])
    # a long or ill-conditioned solve may flip one line-search decision at round-off level: rare (none on these
    # seeds today), and such a problem must still land on the oracle's optimum
    assert_flip_budget(f"randomized_{seed}", same, (it[~same][:10], r["iters"][~same][:10]))
    rel = np.abs(L - r["cost"]) / np.abs(r["cost"])
    assert np.max(rel[same]) < 1e-7
    assert np.all(rel[~same] < 1e-3)
    assert np.max(np.abs(x[same] - r["x_bar"][same])) < 1e-4


@pytest.mark.parametrize("cfg,B", [("pendulum", 300), ("wall", 5)])
def test_helper_wavefronts_do_not_change_results(cfg, B, tmp_path):
    """The team linearization (helper wavefronts, one or three per problem) computes the same items
    with the same code: every output must be bitwise identical to the single-wave kernel.  (n = 2 only gets helpers
    when its time-parallel rollout - whose final pass differentiates the steps it holds itself, the faster form - is
    switched off: MI_ILQR_SEQ_ROLLOUT=1 on both sides of the pendulum case.)"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = f"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {os.path.join(root, 'tests')!r})
from drake_ddp_amd import workloads as W
from test_gpu_parity import make_solver
prob = {{'pendulum': W.pendulum_problem, 'wall': W.cartpole_wall_problem}}[{cfg!r}]()
x0 = {{'pendulum': W.pendulum_batch_x0, 'wall': W.cartpole_wall_batch_x0}}[{cfg!r}](1024)[:{B}]
s = make_solver(prob, B={B}, jac='fd')
s.SetInitialState(x0); s.SetInitialGuess(np.zeros((1, prob['N'] - 1)))
x, u, _, L = s.Solve()
np.savez(sys.argv[1], x=x, u=u, L=L, K=s.K, kappa=s.kappa, fx=s.fx, fu=s.fu, it=s.iterations, ls=s.ls_trials, kp=s.keypoint_count, kpl=s.keypoint_list)
"""
    outs = []
    common = {"MI_ILQR_SEQ_ROLLOUT": "1"} if cfg == "pendulum" else {}
    for tag, env in (("team", {}), ("solo", {"MI_ILQR_NO_HELPER": "1"})):
        f = str(tmp_path / f"{tag}.npz")
        r = subprocess.run([sys.executable, "-c", script, f], capture_output=True, text=True, timeout=300, env=dict(os.environ, **common, **env))
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(np.load(f))
    for k in outs[0].files:
        assert np.array_equal(outs[0][k], outs[1][k]), k


def _run_variant(script, env, out_file, tmp_path):
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", script, out_file], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out_file)


def test_time_parallel_passes_match_the_sequential_ones(tmp_path):
    """n = 2: the Riccati sweep runs as an associative scan over the horizon and the eps = 1 trial as
    Newton's method on the whole trajectory.  Against the same kernels forced to the sequential forms
    (MI_ILQR_SEQ_BACKWARD / MI_ILQR_SEQ_ROLLOUT): identical iteration and line-search-trial counts for
    every problem; costs, trajectories and gains equal to round-off amplified by up to 12 iterations
    (typically 1e-11 relative on the cost, ~1e-8 at worst over the batch: both sides differentiate by
    central differences, which amplifies round-off by 1/h) - inside the end-to-end
    tolerances of test_gpu_parity.py."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = f"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {os.path.join(root, 'tests')!r})
from drake_ddp_amd import workloads as W
from test_gpu_parity import make_solver
prob = W.pendulum_problem()
x0 = W.pendulum_batch_x0(1024)[:512]
s = make_solver(prob, B=512, jac='fd')
s.SetInitialState(x0); s.SetInitialGuess(np.zeros((1, prob['N'] - 1)))
x, u, _, L = s.Solve()
np.savez(sys.argv[1], x=x, u=u, L=L, K=s.K, kappa=s.kappa, dV=s.dV_coeff, it=s.iterations, ls=s.ls_trials)
"""
    par = _run_variant(script, {}, str(tmp_path / "par.npz"), tmp_path)
    seq = _run_variant(script, {"MI_ILQR_SEQ_BACKWARD": "1", "MI_ILQR_SEQ_ROLLOUT": "1"}, str(tmp_path / "seq.npz"), tmp_path)
    assert np.array_equal(par["it"], seq["it"]) and np.array_equal(par["ls"], seq["ls"])
    rel_L = np.abs(par["L"] - seq["L"]) / np.abs(seq["L"])
    assert np.max(rel_L) < 5e-8 and np.median(rel_L) < 1e-10       # worst case: the C-oracle bound of the C2 test
    assert np.max(np.abs(par["x"] - seq["x"])) < 1e-6 and np.max(np.abs(par["u"] - seq["u"])) < 1e-6
    assert np.max(np.abs(par["K"] - seq["K"])) < 1e-5 * np.max(np.abs(seq["K"]))


@pytest.mark.parametrize("N", [4, 5, 64, 66, 130, 254, 257, 258, 300])
def test_pendulum_horizons_around_the_lane_chunk_edges(N):
    """The time-parallel passes deal 1..4 consecutive steps to each lane (up to N = 257; longer
    horizons take the sequential rollout and a longer-chunk sweep): horizons that leave lanes empty,
    fill them exactly, or spill over - every problem against the C oracle."""
    from oracle import c_oracle, models_np as M
    rng = np.random.default_rng(N)
    dt = 2.0 / 200
    prob = dict(model_id=0, dt=dt, N=N, x_nom=np.array([np.pi, 0.0]), Q=dt * 0.01 * np.diag([0.0, 1.0]),
                R=dt * 0.01 * np.eye(1), Qf=100.0 * np.eye(2), delta=1e-3, beta=0.8, gamma=0.0)
    B = 48
    x0 = np.stack([rng.uniform(-np.pi, np.pi, B), rng.uniform(-1, 1, B)], axis=1)
    ug = rng.uniform(-0.2, 0.2, (B, 1, N - 1))
    s = make_solver(prob, B=B, jac="fd")
    s.SetInitialState(x0)
    s.SetInitialGuess(ug)
    x, u, _, L = s.Solve()
    r = c_oracle.solve_batch(M.Model(0, dt), prob, x0, ug)
    assert np.array_equal(s.status, r["status"]) and (s.status == 0).all()
    same = (s.iterations == r["iters"]) & (s.ls_trials == r["ls"])
    assert_flip_budget("short_horizons", same, (s.iterations[~same][:8], r["iters"][~same][:8]))
    rel = np.abs(L - r["cost"]) / np.abs(r["cost"])
    assert np.max(rel[same]) < 1e-7 and np.all(rel[~same] < 1e-3)          # a flipped decision still reaches the same optimum
    # (the shortest horizons need controls ~1e3 to reach the target in 3 steps: relative to the largest entry)
    for got, want in ((x, r["x_bar"]), (u, r["u_bar"]), (s.K, r["K"])):
        assert np.max(np.abs(got[same] - want[same])) < 1e-6 * max(1.0, np.max(np.abs(want[same])))


def test_pendulum_mpc_on_device_time_parallel_vs_sequential(tmp_path):
    """MPCRun on the n = 2 path: every re-solve moves x0 off the stored nominal trajectory (the
    predictor and the Newton sweeps start from x0 - x_bar_0 != 0) and restarts with L = inf.  Same
    iteration counts and logs as the kernels forced to the sequential passes."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = f"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {os.path.join(root, 'tests')!r})
from test_gpu_parity import make_solver
dt = 0.02
prob = dict(model_id=0, dt=dt, N=60, x_nom=np.array([np.pi, 0.0]), Q=dt * np.diag([1.0, 0.1]), R=dt * 0.05 * np.eye(1),
            Qf=20.0 * np.eye(2), delta=1e-3, beta=0.7, gamma=0.0)
rng = np.random.default_rng(7)
B = 40
x0 = np.stack([rng.uniform(-np.pi, np.pi, B), rng.uniform(-1, 1, B)], axis=1)
s = make_solver(prob, B=B, jac='fd')
s.SetInitialState(x0); s.SetInitialGuess(np.zeros((1, prob['N'] - 1)))
s.Solve()
s.MPCRun(12, 3)
np.savez(sys.argv[1], log=s.mpc_log, x=s.x_bar, u=s.u_bar, K=s.K, it=s.iterations, ls=s.ls_trials)
"""
    par = _run_variant(script, {}, str(tmp_path / "par.npz"), tmp_path)
    seq = _run_variant(script, {"MI_ILQR_SEQ_BACKWARD": "1", "MI_ILQR_SEQ_ROLLOUT": "1"}, str(tmp_path / "seq.npz"), tmp_path)
    same = (par["it"] == seq["it"]) & (par["ls"] == seq["ls"])
    assert_flip_budget("pendulum_mpc_par_vs_seq", same)
    # (a problem whose counts differ flipped one decision in one of 12 re-solves: its final costs still agree)
    assert np.allclose(par["log"][~same][:, -1, -2], seq["log"][~same][:, -1, -2], rtol=1e-3)
    assert np.allclose(par["log"][same], seq["log"][same], rtol=1e-7, atol=1e-9)
    assert np.max(np.abs(par["x"][same] - seq["x"][same])) < 1e-6 and np.max(np.abs(par["u"][same] - seq["u"][same])) < 1e-6


def test_async_solves_keep_their_own_statistics():
    """mi_ilqr_solve_async x k then mi_ilqr_collect_stats_n: every enqueued solve ran in full and left
    its own record (the bench pipelines its steps this way); more than the ring holds is refused."""
    from drake_ddp_amd._capi import MiIlqrError
    prob, x0, s = c2_setup(64)
    x, u, _, L = s.Solve()
    ref = s.stats
    for _ in range(5):
        s.rearm(cold=True)
        s.solve_resident_async()
    got = s.collect(5)
    for st in got:
        assert st.total_iters == ref.total_iters and st.total_ls_trials == ref.total_ls_trials
        assert st.n_converged == 64 and st.best_cost == ref.best_cost and st.kernel_ms > 0
    assert np.array_equal(s.x_bar, x) and np.array_equal(s.cost, L)
    with pytest.raises(MiIlqrError):
        s.collect(33)


def test_auto_kernel_selection_at_large_batches():
    """AUTO keeps the n = 2 models on the wave-per-problem kernel at any batch size (its time-parallel
    passes make it the faster one) and moves the other small-state models to the lane-per-problem
    kernel at B >= 8192; both serve the same batch with the same results."""
    from drake_ddp_amd import workloads as W
    from drake_ddp_amd._capi import MiIlqrError
    prob = W.pendulum_problem()
    B = 8192
    x0 = W.pendulum_batch_x0(B)
    res = {}
    for mode in ("auto", "throughput"):
        s = make_solver(prob, B=B, jac="fd", kernel_mode=mode, hist_cap=2)
        s.SetInitialState(x0)
        s.SetInitialGuess(np.zeros((1, prob["N"] - 1)))
        x, u, _, L = s.Solve()
        res[mode] = (L, s.iterations.copy())
        if mode == "auto":
            s.stage_backward()                         # stage-level entries: wave-per-problem kernels only
        else:
            with pytest.raises(MiIlqrError):
                s.stage_backward()
    assert np.array_equal(res["auto"][1], res["throughput"][1])
    assert np.max(np.abs(res["auto"][0] - res["throughput"][0]) / np.abs(res["throughput"][0])) < 5e-8   # both central FD
    a = make_solver(W.acrobot_problem(), B=B, jac="ad", kernel_mode="auto", hist_cap=2)
    with pytest.raises(MiIlqrError):
        a.stage_backward()                             # n = 4 at B >= 8192: lane-per-problem kernel


def test_in_kernel_and_separate_statistics_agree(tmp_path):
    """The batch statistics come from the solve kernel's own epilogue (small batches) or from
    stats_kernel: same aggregate either way, for a batch with converged, capped and failed problems."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = f"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {os.path.join(root, 'tests')!r})
from drake_ddp_amd import workloads as W
from test_gpu_parity import make_solver
prob = W.pendulum_problem()
x0 = W.pendulum_batch_x0(1024)[:200]
s = make_solver(prob, B=200, jac='fd', max_iters=7)
s.SetInitialState(x0); s.SetInitialGuess(np.zeros((1, prob['N'] - 1)))
s.Solve()
st = s.stats
np.savez(sys.argv[1], v=np.array([st.total_iters, st.total_ls_trials, st.n_converged, st.n_max_iters, st.n_ls_failed,
                                  st.max_iters_seen, st.best_index, st.best_cost]), it=s.iterations, status=s.status, cost=s.cost)
"""
    a = _run_variant(script, {"MI_ILQR_STATS_KERNEL": "0"}, str(tmp_path / "a.npz"), tmp_path)
    b = _run_variant(script, {"MI_ILQR_STATS_KERNEL": "1"}, str(tmp_path / "b.npz"), tmp_path)
    assert np.array_equal(a["v"], b["v"]) and np.array_equal(a["it"], b["it"])
    v, it, status, cost = a["v"], a["it"], a["status"], a["cost"]
    assert v[0] == it.sum() and v[2] == (status == 0).sum() and v[3] == (status == 1).sum() and v[3] > 0 and v[5] == it.max()
    conv = np.where(status == 0)[0]
    assert int(v[6]) == conv[np.argmin(cost[conv])] and v[7] == cost[conv].min()


@pytest.mark.parametrize("model_id,N", [(2, 160), (1, 200), (3, 200)])
def test_n4_long_horizon_scan_matches_the_sequential_sweep(model_id, N, tmp_path):
    """n = 4, N > 128: the backward pass runs as the time-parallel scan (4x4 elements, unpivoted inverse
    with a pivot guard, outlined into its own function).  Against the sequential MFMA sweep
    (MI_ILQR_SEQ_BACKWARD=1) on forward-mode Jacobians: one backward pass from identical inputs agrees
    to 1e-9 in the gains, and the first five iterations of a solve (these swing-ups take 20-500 and
    amplify any difference ~10x per iteration) agree in their line-search decisions and to 1e-6 in the
    cost (1e-5 on the stiff contact model)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = f"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {os.path.join(root, 'tests')!r})
from test_gpu_parity import make_solver
model_id, N = {model_id}, {N}
dt = 0.01
rng = np.random.default_rng(5 + model_id)
x_nom = np.array([0, np.pi, 0, 0.0]) if model_id >= 2 else np.array([np.pi, 0, 0, 0.0])
prob = dict(model_id=model_id, dt=dt, N=N, x_nom=x_nom, Q=dt * np.diag([0.5, 1.0, 0.05, 0.05]), R=dt * 0.05 * np.eye(1),
            Qf=np.diag([30.0, 30.0, 3.0, 3.0]), delta=1e-3, beta=0.6, gamma=0.0)
B = 24
x0 = rng.uniform(-0.3, 0.3, (B, 4))
if model_id >= 2: x0[:, 1] += np.pi
s = make_solver(prob, B=B, jac='ad', max_iters=5)
s.SetInitialState(x0); s.SetInitialGuess(rng.uniform(-0.2, 0.2, (B, 1, N - 1)))
s.stage_forward(np.inf)                       # one trajectory + its linearization, then ONE backward pass
s.stage_backward()
K1, k1, dV1 = s.K.copy(), s.kappa.copy(), s.dV_coeff.copy()
x, u, _, L = s.Solve()
np.savez(sys.argv[1], K1=K1, k1=k1, dV1=dV1, L=L, it=s.iterations, ls=s.ls_trials, x=x, K=s.K, status=s.status)
"""
    par = _run_variant(script, {}, str(tmp_path / "par.npz"), tmp_path)
    seq = _run_variant(script, {"MI_ILQR_SEQ_BACKWARD": "1"}, str(tmp_path / "seq.npz"), tmp_path)
    for f in ("K1", "k1", "dV1"):
        assert np.max(np.abs(par[f] - seq[f])) < 1e-9 * max(1.0, np.max(np.abs(seq[f]))), f
    same = (par["it"] == seq["it"]) & (par["ls"] == seq["ls"])
    assert_flip_budget("scan_vs_seq_backward", same, (par["ls"], seq["ls"]))
    # (the stiff contact model amplifies faster: 1e-5 there)
    assert np.max(np.abs(par["L"][same] - seq["L"][same]) / np.abs(seq["L"][same])) < (1e-5 if model_id == 3 else 1e-6)


def test_set_control_limits_is_the_reference_stub():
    """SetControlLimits (ilqr.py:158-159) is `pass` in the reference: calling it, with any limits, changes nothing - results
    bitwise those of a solver that never heard of it (both classes; nothing is pinned against limits because the reference has
    no semantics for them)."""
    from drake_ddp_amd import workloads as W
    p = W.pendulum_problem()
    x0 = W.pendulum_batch_x0(32)
    out = []
    for limits in (None, (-0.1, 0.1)):
        s = make_solver(p, B=32, jac="fd")
        if limits is not None:
            assert s.SetControlLimits(np.full(1, limits[0]), np.full(1, limits[1])) is None
        s.SetInitialState(x0); s.SetInitialGuess(np.zeros((1, p["N"] - 1)))
        x, u, _, L = s.Solve()
        out.append((x.copy(), u.copy(), L.copy(), s.K.copy(), s.iterations.copy()))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert np.abs(out[1][1]).max() > 0.1                      # (the "limits" were well inside what the solution uses)
    one = make_solver(p, jac="fd", single=True)
    one.SetControlLimits(-1.0, 1.0)
    one.SetInitialState(x0[0]); one.SetInitialGuess(np.zeros((1, p["N"] - 1)))
    x1, u1, _, L1 = one.Solve()
    assert np.array_equal(x1, out[0][0][0]) and L1 == out[0][2][0]


@pytest.mark.parametrize("N", [2, 3])
def test_shortest_horizons_vs_c_oracle(N):
    """The reference takes any num_timesteps >= 2 (ilqr.py:51); until round 4 mi_ilqr_create refused N < 4 without a
    reason.  One and two control steps on every kernel family (wave-per-problem, lane-per-problem, mid-size and n = 36
    workgroup-per-problem) against the C oracle: costs to round-off and the same trajectories.  (The iteration / trial COUNTS
    are not compared: a one-step problem is solved by its first iteration and every later cost comparison, L_last - L > 0 with
    gamma = 0, is a tie decided by the last bit - the reference's own line search is a coin flip there.)"""
    from drake_ddp_amd import workloads as W
    from oracle import c_oracle, models_np as M
    B = 70
    for name, prob, x0, m, modes in (("pendulum", W.pendulum_problem(), W.pendulum_batch_x0(128)[:B], 1, ("auto", "throughput")),
                                     ("acrobot", W.acrobot_problem(), W.acrobot_batch_x0(128)[:B], 1, ("auto", "throughput")),
                                     ("cart-pole + wall", W.cartpole_wall_problem(), W.cartpole_wall_batch_x0(128)[:B], 1, ("auto",)),
                                     ("36-state chain", W.synth36_problem(), W.synth36_batch_x0(B), 12, ("auto",)),
                                     ("arm + ball", W.arm27_problem(), W.arm27_batch_x0(B), 7, ("auto",))):
        p = dict(prob, N=N)
        ug = 0.1 * np.random.default_rng(1).standard_normal((B, m, N - 1))
        r = c_oracle.solve_batch(M.Model(p["model_id"], p["dt"]), p, x0, ug)
        for mode in modes:
            s = make_solver(p, B=B, jac="fd", kernel_mode=mode)
            s.SetInitialState(x0); s.SetInitialGuess(ug)
            s.Solve()                                    # (the batched class reports a line search that ran out of step sizes on a tie
            assert s.stats.n_internal == 0               #  per problem; it RAISES for an aborted kernel - which round 6 found this test
            rel = np.abs(s.cost - r["cost"]) / np.abs(r["cost"])   #  had been swallowing: clustered launches at N = 3, lds_layout.hpp: kIntRowMin)
            xe = np.abs(s.x_bar - r["x_bar"]).max()
            print(f"N = {N} {name} ({mode}): cost {rel.max():.1e}, x {xe:.1e}")
            assert np.isfinite(s.x_bar).all() and rel.max() < 1e-11 and xe < 2e-5
        if m > 2:
            # the workgroup-per-problem kernels at a batch that is CLUSTERED by default (8 problems: 8 workgroups each; round 6:
            # their hand-shake state lives in the integer scratch, whose rows were N ints long - three at N = 3, one short)
            s = make_solver(p, B=8, jac="fd")
            s.SetInitialState(x0[:8]); s.SetInitialGuess(ug[:8])
            s.Solve()
            rel = np.abs(s.cost - r["cost"][:8]) / np.abs(r["cost"][:8])
            assert s.stats.n_internal == 0 and s.cluster_stats[:, 0].max() > 0 and rel.max() < 1e-11 and np.abs(s.x_bar - r["x_bar"][:8]).max() < 2e-5


def test_longest_horizons_of_the_workgroup_kernels_vs_c_oracle():
    """The workgroup-per-problem kernels keep the cost gradients of the whole horizon in LDS next to their fixed buffers; the
    horizon that still fits: N = 148 for (36, 12), 96 for (37, 12), 319 for the arm + ball's (27, 7).  At
    those horizons (three times the reference scripts' 40 - 50 steps) and at twice to three times that - where the gradients
    move to HBM (large_lds_bytes_hbm: refused at create until round 4) - against the C oracle, costs within 10 x the oracle's
    own one-ulp sensitivity.  What still bounds the horizon is the key-point code's integer scratch: MI_ILQR_E_UNSUPPORTED at
    create, never a launch failure."""
    from drake_ddp_amd import workloads as W, _capi
    from drake_ddp_amd._capi import MiIlqrError
    from oracle import c_oracle, models_np as M
    B = 6
    for name, prob, x0, ugf, horizons in (("36-state chain", W.synth36_problem(), W.synth36_batch_x0(B), W.synth36_u_guess, (148, 149, 400)),
                                          ("3-D quadruped", W.quad3d_problem(), W.quad3d_batch_x0(B), W.quad3d_u_guess, (96, 97, 200)),
                                          ("planar quadruped", dict(W.planar_quad_problem(), dt=2e-4), W.planar_quad_batch_x0(B), W.planar_quad_u_guess, (148, 149, 260)),
                                          # (a short step: with dt = 4e-3 the standing guess falls within 148 steps, and with 1.5e-3 the Riccati recursion through
                                          #  this stiff contact model amplifies round-off by ~10 x every 12 steps - DESIGN section 8 - so that beyond N ~ 110
                                          #  neither the device nor the fp64 reference has a digit left)
                                          ("arm + ball", W.arm27_problem(), W.arm27_batch_x0(B), W.arm27_u_guess, (319, 320, 420))):
        for N in horizons:
            p = dict(prob, N=N)
            ug = ugf(N)
            s = make_solver(p, B=B, jac="fd", hist_cap=256)
            s.SetInitialState(x0); s.SetInitialGuess(ug)
            s.Solve()
            model = M.Model(p["model_id"], p["dt"])
            r = c_oracle.solve_batch(model, p, x0, ug)
            rel = np.abs(s.cost - r["cost"]) / np.abs(r["cost"])
            same = (s.iterations == r["iters"]) & (s.ls_trials == r["ls"]) & (s.status == r["status"])
            own, flips = 0.0, 0
            for d in (np.inf, -np.inf):
                xq = x0.copy()
                xq[:, 0] = np.nextafter(xq[:, 0], d)
                rq = c_oracle.solve_batch(model, p, xq, ug)
                keep = (rq["iters"] == r["iters"]) & (rq["ls"] == r["ls"])
                flips = max(flips, int((~keep).sum()))
                own = max(own, float((np.abs(rq["cost"] - r["cost"]) / np.abs(r["cost"]))[keep].max()) if keep.any() else 0.0)
            fin = np.isfinite(r["cost"])                      # (a quadruped that falls within a long horizon: L = inf on both sides)
            worst = float(rel[same & fin].max()) if (same & fin).any() else 0.0
            print(f"{name} N = {N}: same decisions {int(same.sum())}/{B} (the oracle against itself: {B - flips}/{B}), cost {worst:.1e} (its own one-ulp sensitivity {own:.1e})")
            assert (~same).sum() <= flips and worst < max(1e-7, 10 * own) and np.array_equal(np.isfinite(s.cost)[same], fin[same])
    with pytest.raises(MiIlqrError) as e:                   # (what still bounds the horizon: the key-point code's integers in LDS)
        make_solver(dict(W.synth36_problem(), N=20000), B=B, jac="fd")
    assert e.value.code == _capi.E_UNSUPPORTED


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_randomized_configs_of_the_workgroup_kernels_vs_c_oracle(seed):
    """test_randomized_configs_vs_c_oracle for the workgroup-per-problem families: random horizon (5 .. 60), beta (0.3 .. 0.85),
    gamma (0, 0.1, 0.3: the expected-improvement side of the test of ilqr.py:330, also inside the four-candidate passes of
    the mid-size kernels), random positive weights, on the arm + ball (backtracks), the 36-state chain and the 3-D quadruped.
    Decisions (status, iterations, trials) against the C oracle with at most the flips the oracle shows against itself (x0 one
    ulp away) + 1; costs of the agreeing problems within 10 x its own deviation (at least 1e-8)."""
    from drake_ddp_amd import workloads as W
    from oracle import c_oracle, models_np as M
    rng = np.random.default_rng(500 + seed)
    name = ["arm", "arm", "synth36", "quad3d", "arm", "synth36"][seed]
    base, x0f, ugf = {"arm": (W.arm27_problem(), W.arm27_batch_x0, W.arm27_u_guess), "synth36": (W.synth36_problem(), W.synth36_batch_x0, W.synth36_u_guess),
                      "quad3d": (W.quad3d_problem(), W.quad3d_batch_x0, W.quad3d_u_guess)}[name]
    n, m = base["Q"].shape[0], base["R"].shape[0]
    N = int(rng.integers(5, 61))
    B = int(rng.integers(3, 40))
    def scale(M_):                                   # D M D with a random positive diagonal D: symmetric, as definite as M
        d_ = np.sqrt(10.0 ** rng.uniform(-0.5, 0.5, M_.shape[0]))
        return M_ * d_[:, None] * d_[None, :]
    prob = dict(base, N=N, Q=scale(base["Q"]), R=scale(base["R"]), Qf=scale(base["Qf"]),
                beta=float(rng.choice([0.3, 0.5, 0.7, 0.85])), gamma=float(rng.choice([0.0, 0.1, 0.3])))
    x0, ug = x0f(B), ugf(N)
    s = make_solver(prob, B=B, jac="fd", hist_cap=8)
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    s.Solve()
    model = M.Model(prob["model_id"], prob["dt"])
    r = c_oracle.solve_batch(model, prob, x0, ug)
    same = (s.status == r["status"]) & (s.iterations == r["iters"]) & (s.ls_trials == r["ls"])
    flips, own = 0, 0.0
    for d in (np.inf, -np.inf):
        xq = x0.copy()
        xq[:, 0] = np.nextafter(xq[:, 0], d)
        rq = c_oracle.solve_batch(model, prob, xq, ug)
        keep = (rq["iters"] == r["iters"]) & (rq["ls"] == r["ls"]) & (rq["status"] == r["status"])
        flips = max(flips, int((~keep).sum()))
        if keep.any():
            own = max(own, float((np.abs(rq["cost"] - r["cost"]) / np.abs(r["cost"]))[keep].max()))
    rel = np.abs(s.cost - r["cost"]) / np.abs(r["cost"])
    print(f"{name} N = {N} B = {B} beta {prob['beta']} gamma {prob['gamma']}: {int(r['ls'].sum())} trials in {int(r['iters'].sum())} iterations, statuses {np.unique(r['status']).tolist()}; "
          f"{int((~same).sum())} problems decide differently (the oracle against itself: {flips}); cost {rel[same].max() if same.any() else 0:.1e} (own {own:.1e})")
    assert int((~same).sum()) <= flips + 1
    assert same.any() and rel[same].max() <= max(1e-8, 10 * own)


def test_a_poisoned_problem_fails_alone():
    """NaN in one problem's x0: the reference's line search would run out of step sizes on it (every cost comparison with NaN
    is false, ilqr.py:330-337) - status LINESEARCH_FAILED for that problem, no hang, and its batch neighbours come out
    bitwise as from a clean batch, on every kernel family.  An infinite initial guess fails the same way; NaN cost matrices
    are refused by the workgroup-per-problem families at set_cost and fail every problem's first search elsewhere."""
    from drake_ddp_amd import workloads as W, _capi
    for name, prob, x0, ug, kw in (("pendulum", W.pendulum_problem(), W.pendulum_batch_x0(70), np.zeros((1, 199)), {}),
                                   ("pendulum, lane per problem", W.pendulum_problem(), W.pendulum_batch_x0(70), np.zeros((1, 199)), {"kernel_mode": "throughput"}),
                                   ("cart-pole + wall", W.cartpole_wall_problem(), W.cartpole_wall_batch_x0(70), np.zeros((1, 199)), {}),
                                   ("36-state chain", W.synth36_problem(), W.synth36_batch_x0(9), W.synth36_u_guess(40), {}),
                                   ("3-D quadruped", W.quad3d_problem(), W.quad3d_batch_x0(9), W.quad3d_u_guess(40), {}),
                                   ("arm + ball", W.arm27_problem(), W.arm27_batch_x0(9), W.arm27_u_guess(50), {})):
        B = len(x0)
        clean = make_solver(prob, B=B, jac="fd", **kw)
        clean.SetInitialState(x0); clean.SetInitialGuess(ug)
        xc, uc, _, Lc = clean.Solve()
        bad = x0.copy()
        bad[3, 0] = np.nan
        s = make_solver(prob, B=B, jac="fd", **kw)
        s.SetInitialState(bad); s.SetInitialGuess(ug)
        x, u, _, L = s.Solve()
        others = np.arange(B) != 3
        assert s.status[3] == _capi.STATUS_LINESEARCH_FAILED and (s.status[others] == clean.status[others]).all(), name
        assert np.array_equal(x[others], xc[others]) and np.array_equal(u[others], uc[others]) and np.array_equal(L[others], Lc[others]), name
        assert np.array_equal(s.iterations[others], clean.iterations[others]), name
        g = np.broadcast_to(np.asarray(ug, dtype=float), (B,) + np.asarray(ug).shape[-2:]).copy()
        g[5, 0, 0] = np.inf
        t = make_solver(prob, B=B, jac="fd", **kw)
        t.SetInitialState(x0); t.SetInitialGuess(g)
        t.Solve()
        assert t.status[5] == _capi.STATUS_LINESEARCH_FAILED and (np.delete(t.status, 5) == np.delete(clean.status, 5)).all(), name
        print(f"{name}: the poisoned problem stops with status 2, the other {B - 1} are bitwise the clean batch's")


@pytest.mark.parametrize("replan", ["1", "N-2"])
def test_mpc_loop_replan_extremes_vs_c_oracle(replan):
    """The receding-horizon loop (acrobot.py:145-155) with the shortest and the longest shift the reference's warm start allows
    - one step, and N - 2 steps (all but one control of the new guess is the repeated last one) - three re-solves, on the
    wave-per-problem (pendulum), lane-per-problem (acrobot, host loop), n = 36 and mid-size workgroup kernels: per-re-solve
    iteration counts and x0's against oracle_mpc_batch; a shift of N - 1 is refused."""
    from drake_ddp_amd import workloads as W, _capi
    from drake_ddp_amd._capi import MiIlqrError
    from oracle import c_oracle, models_np as M
    for name, prob, x0, ug, kw in (("pendulum", dict(W.pendulum_problem(), N=60), W.pendulum_batch_x0(40), np.zeros((1, 59)), {}),
                                   ("acrobot, lane per problem", W.acrobot_problem(), W.acrobot_batch_x0(70), np.zeros((1, 39)), {"kernel_mode": "throughput"}),
                                   ("36-state chain", W.synth36_problem(), W.synth36_batch_x0(6), W.synth36_u_guess(40), {}),
                                   ("arm + ball", dict(W.arm27_problem(), N=20), W.arm27_batch_x0(6), W.arm27_u_guess(20), {})):
        N, n = prob["N"], prob["Q"].shape[0]
        r_ = 1 if replan == "1" else N - 2
        s = make_solver(prob, B=len(x0), jac="fd", **kw)
        s.SetInitialState(x0); s.SetInitialGuess(ug)
        s.Solve()
        first_it = s.iterations.copy()
        s.MPCRun(3, r_)
        log = s.mpc_log
        r = c_oracle.mpc_batch(M.Model(prob["model_id"], prob["dt"]), prob, x0, ug, 3, r_)
        assert np.array_equal(first_it, r["first"][:, 1].astype(int)), name
        same = (log[:, :, -1] == r["log"][:, :, -1]).all(axis=1)
        relL = np.abs(log[:, :, -2] - r["log"][:, :, -2]) / np.abs(r["log"][:, :, -2])
        dx = np.abs(log[:, :, :n] - r["log"][:, :, :n]).max()
        print(f"{name} replan {r_}: {int(same.sum())}/{len(x0)} problems with the oracle's iteration counts in every re-solve, costs {relL[same].max():.1e}, x0 of the re-solves {dx:.1e}")
        # (a shift of N - 2 steps applies gains far from where they were computed, SURVEY F10: round-off grows by the re-solve -
        #  5e-9, 1e-8, 4e-6 on the pendulum - while every count stays the oracle's)
        assert same.mean() >= 0.9 and relL[same].max() < (1e-6 if r_ == 1 else 1e-4) and np.abs(log[same][:, :, :n] - r["log"][same][:, :, :n]).max() < 1e-4
        with pytest.raises(MiIlqrError) as e:
            s.MPCRun(1, N - 1)
        assert e.value.code == _capi.E_BAD_ARG


@pytest.mark.parametrize("seed", list(range(8)))
def test_randomized_keypoint_configs_vs_c_oracle(seed):
    """The three key-point methods (ilqr.py:417-593) with random minN / maxN / thresholds on every kernel family - wave per
    problem, lane per problem (per-lane lists), mid-size and n = 36 workgroup kernels: statuses, iterations, trials, the
    key-point count of every iteration and the last key-point list against the C oracle.  A jerk or an interpolation error within
    round-off of its threshold may fall on the other side (libm against the device's sin / cos): at most two problems of a case
    may differ from the oracle, every other one is exact."""
    from drake_ddp_amd import workloads as W
    from oracle import c_oracle, models_np as M
    rng = np.random.default_rng(900 + seed)
    name, prob, x0f, ugf, kw = [("pendulum", W.pendulum_problem(), lambda B: W.pendulum_batch_x0(128)[:B], lambda N: np.zeros((1, N - 1)), {}),
                                ("acrobot, lane per problem", W.acrobot_problem(), lambda B: W.acrobot_batch_x0(128)[:B], lambda N: np.zeros((1, N - 1)), {"kernel_mode": "throughput"}),
                                ("arm + ball", W.arm27_problem(), W.arm27_batch_x0, W.arm27_u_guess, {}),
                                ("36-state chain", W.synth36_problem(), W.synth36_batch_x0, W.synth36_u_guess, {}),
                                ("acrobot", W.acrobot_problem(), lambda B: W.acrobot_batch_x0(128)[:B], lambda N: np.zeros((1, N - 1)), {}),
                                ("pendulum, lane per problem", W.pendulum_problem(), lambda B: W.pendulum_batch_x0(128)[:B], lambda N: np.zeros((1, N - 1)), {"kernel_mode": "throughput"}),
                                ("arm + ball", W.arm27_problem(), W.arm27_batch_x0, W.arm27_u_guess, {}),
                                ("3-D quadruped", W.quad3d_problem(), W.quad3d_batch_x0, W.quad3d_u_guess, {})][seed]
    method = ["adaptiveJerk", "iterativeError", "iterativeError", "adaptiveJerk", "setInterval", "adaptiveJerk", "setInterval", "iterativeError"][seed]
    N = int(rng.integers(12, 70)) if prob["Q"].shape[0] > 4 else int(rng.integers(30, 200))
    minN = int(rng.integers(1, 6))
    kp = (method, minN, minN + int(rng.integers(1, 12)), float(10.0 ** rng.uniform(-6, -3)), float(10.0 ** rng.uniform(-9, -5)))
    B = 24 if prob["Q"].shape[0] > 4 else 70
    p = dict(prob, N=N)
    x0, ug = x0f(B), ugf(N)
    s = make_solver(p, B=B, keypoint=kp, jac="fd", hist_cap=64, **kw)
    s.SetInitialState(x0); s.SetInitialGuess(ug)
    s.Solve()
    r = c_oracle.solve_batch(M.Model(p["model_id"], p["dt"]), p, x0, ug, keypoint=kp, hist_cap=64)
    h, nk, kl = s.history, s.keypoint_count, s.keypoint_list
    exact = np.zeros(B, bool)
    for b in range(B):
        it = min(int(r["iters"][b]), 64)
        exact[b] = (s.status[b] == r["status"][b] and s.iterations[b] == r["iters"][b] and s.ls_trials[b] == r["ls"][b]
                    and np.array_equal(np.round(h[b, :it, 3] * (N - 1) / 100.0), r["hist"][b, :it, 3])
                    and nk[b] == r["kp_count"][b] and np.array_equal(kl[b][:nk[b]], r["kp_list"][b][:nk[b]]))
    # (long stiff solves - the plain cart-pole over 190 steps - amplify round-off by the iteration: the yardstick is again the
    #  oracle against itself with x0 one ulp away)
    flips = 0
    if (~exact).sum() > 2:
        for d in (np.inf, -np.inf):
            xq = x0.copy()
            xq[:, 1] = np.nextafter(xq[:, 1], d)
            rq = c_oracle.solve_batch(M.Model(p["model_id"], p["dt"]), p, xq, ug, keypoint=kp, hist_cap=64)
            flips = max(flips, int(((rq["iters"] != r["iters"]) | (rq["ls"] != r["ls"]) | (rq["kp_count"] != r["kp_count"])).sum()))
    print(f"{name} N = {N} {kp}: {int(exact.sum())}/{B} problems exact (statuses {np.unique(r['status']).tolist()}, key-points {r['kp_count'].min()}..{r['kp_count'].max()} of {N - 1})"
          + (f"; the oracle against itself, x0 one ulp away: {flips} problems differ" if flips else ""))
    assert (~exact).sum() <= 2 + flips
    ok = exact & (r["status"] == 0)
    assert ok.any() and (np.abs(s.cost - r["cost"]) / np.abs(r["cost"]))[ok].max() < 1e-6


@pytest.mark.parametrize("fd_step", [1e-4, 1e-6])
def test_other_difference_steps_vs_c_oracle(fd_step):
    """The central-difference step is a constructor option (default 1e-5, BASELINE's north_star); with 1e-4 and 1e-6 on every
    kernel family the decisions are the C oracle's with the same step, costs to 1e-7."""
    from drake_ddp_amd import workloads as W
    from oracle import c_oracle, models_np as M
    for name, prob, x0, ug, kw in (("pendulum", W.pendulum_problem(), W.pendulum_batch_x0(70), np.zeros((1, 199)), {}),
                                   ("acrobot, lane per problem", W.acrobot_problem(), W.acrobot_batch_x0(70), np.zeros((1, 39)), {"kernel_mode": "throughput"}),
                                   ("36-state chain", W.synth36_problem(), W.synth36_batch_x0(8), W.synth36_u_guess(40), {}),
                                   ("3-D quadruped", W.quad3d_problem(), W.quad3d_batch_x0(8), W.quad3d_u_guess(40), {}),
                                   ("arm + ball", W.arm27_problem(), W.arm27_batch_x0(8), W.arm27_u_guess(50), {})):
        s = make_solver(prob, B=len(x0), jac="fd", fd_step=fd_step, **kw)
        s.SetInitialState(x0); s.SetInitialGuess(ug)
        s.Solve()
        r = c_oracle.solve_batch(M.Model(prob["model_id"], prob["dt"]), prob, x0, ug, fd_h=fd_step)
        same = (s.status == r["status"]) & (s.iterations == r["iters"]) & (s.ls_trials == r["ls"])
        rel = np.abs(s.cost - r["cost"]) / np.abs(r["cost"])
        print(f"{name} h = {fd_step:g}: {int(same.sum())}/{len(x0)} with the oracle's decisions, costs {rel[same].max():.1e}")
        assert same.sum() >= len(x0) - 1 and rel[same].max() < 1e-7


def test_other_model_parameters_vs_c_oracle():
    """Every built-in model with its physical parameters scaled by random factors in [0.8, 1.25] (masses, lengths, damping,
    contact stiffness ...: mi_ilqr_desc.model_params, the `params` argument of drake_ddp_amd.models): decisions against the C
    oracle run with the same parameters, costs to 1e-7."""
    from drake_ddp_amd import workloads as W
    from oracle import c_oracle, models_np as M
    rng = np.random.default_rng(77)
    for name, prob, x0, ug, kw in (("pendulum", W.pendulum_problem(), W.pendulum_batch_x0(70), np.zeros((1, 199)), {}),
                                   ("acrobot", W.acrobot_problem(), W.acrobot_batch_x0(70), np.zeros((1, 39)), {}),
                                   ("acrobot, lane per problem", W.acrobot_problem(), W.acrobot_batch_x0(70), np.zeros((1, 39)), {"kernel_mode": "throughput"}),
                                   ("cart-pole + wall", dict(W.cartpole_wall_problem(), N=60), W.cartpole_wall_batch_x0(70), np.zeros((1, 59)), {}),
                                   ("36-state chain", W.synth36_problem(), W.synth36_batch_x0(8), W.synth36_u_guess(40), {}),
                                   ("3-D quadruped", W.quad3d_problem(), W.quad3d_batch_x0(8), W.quad3d_u_guess(40), {}),
                                   ("arm + ball", W.arm27_problem(), W.arm27_batch_x0(8), W.arm27_u_guess(50), {})):
        base = M.Model(prob["model_id"], prob["dt"]).params
        params = base * rng.uniform(0.8, 1.25, base.size)
        p = dict(prob, params=params)
        s = make_solver(p, B=len(x0), jac="fd", **kw)
        s.SetInitialState(x0); s.SetInitialGuess(ug)
        s.Solve()
        r = c_oracle.solve_batch(M.Model(prob["model_id"], prob["dt"], params), p, x0, ug)
        same = (s.status == r["status"]) & (s.iterations == r["iters"]) & (s.ls_trials == r["ls"])
        fin = same & np.isfinite(r["cost"])
        rel = (np.abs(s.cost - r["cost"]) / np.abs(r["cost"]))[fin]
        print(f"{name}: {int(same.sum())}/{len(x0)} with the oracle's decisions (statuses {np.unique(r['status']).tolist()}), costs {rel.max() if rel.size else 0:.1e}")
        assert same.sum() >= len(x0) - 1 and (rel.size == 0 or rel.max() < 1e-7)


def test_pipelined_cold_and_warm_solves_on_every_kernel_family():
    """mi_ilqr_solve_async on the workgroup-per-problem (mid-size with its four-candidate passes, n = 36) and lane-per-problem
    kernels: a cold / warm / warm / cold sequence enqueued back to back returns, solve by solve, the statistics of the same
    sequence run with a collect after each - warm re-solves start from the persistent gains and take fewer
    iterations, a cold one repeats the first."""
    from drake_ddp_amd import workloads as W
    for name, prob, x0, ug, kw in (("arm + ball", W.arm27_problem(), W.arm27_batch_x0(24), W.arm27_u_guess(50), {}),
                                   ("36-state chain", W.synth36_problem(), W.synth36_batch_x0(24), W.synth36_u_guess(40), {}),
                                   ("acrobot, lane per problem", W.acrobot_problem(), W.acrobot_batch_x0(200), np.zeros((1, 39)), {"kernel_mode": "throughput"})):
        s = make_solver(prob, B=len(x0), jac="fd", **kw)
        s.SetInitialState(x0); s.SetInitialGuess(ug)
        s.Solve()
        ref = []
        for cold in (True, False, False, True):
            if cold:
                s.rearm(cold=True)
            s.solve_resident_async()
            st = s.collect(1)[0]
            ref.append((st.total_iters, st.total_ls_trials, st.n_converged, st.best_cost, st.best_index, s.iterations.copy(), s.cost.copy()))
        assert ref[0][:5] == ref[3][:5] and ref[1][0] < ref[0][0], name
        for cold in (True, False, False, True):
            if cold:
                s.rearm(cold=True)
            s.solve_resident_async()
        got = s.collect(4)
        for g, r in zip(got, ref):
            assert (g.total_iters, g.total_ls_trials, g.n_converged, g.best_cost, g.best_index) == r[:5], name
        assert np.array_equal(s.iterations, ref[3][5]) and np.array_equal(s.cost, ref[3][6])
        print(f"{name}: iterations of the cold / warm / warm / cold solves {[r[0] for r in ref]}")
