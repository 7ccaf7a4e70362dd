"""The comparands of the key-point edge tests, on the CPU: the NumPy restatement builds the lists ilqr.py:417-593 builds at the
edges (tests/keypoint_edges.py) and leaves the rows it does not touch as they were; the C restatement takes the same
decisions over whole solves (lists, counts and trials of every iteration) and refuses adaptiveJerk with
maxN < 1 like mi_ilqr_create does."""
import numpy as np
import pytest

from common import make_oracle
from keypoint_edges import crafted_x_bar, edge_configs, expected_list, fx_sentinel, fu_sentinel, iterations_before_roundoff, short_configs


def _pendulum(N):
    from drake_ddp_amd import workloads as W
    return dict(W.pendulum_problem(), N=N, delta=1e-3)


def _acrobot(N):
    from drake_ddp_amd import workloads as W
    return W.acrobot_problem(N)


def _x0(model, B):
    from drake_ddp_amd import workloads as W
    return W.pendulum_batch_x0(B) if model == "pendulum" else W.acrobot_batch_x0(B)


PROBLEMS = {"pendulum": _pendulum, "acrobot": _acrobot}


def _alternating_list(N, phase, minN, maxN):
    """adaptiveJerk on crafted_x_bar: the jerk at t is +1 where t + phase is even, else -1 (threshold 0)."""
    kp, since = [0], 0
    for t in range(N - 3):
        since += 1
        if since >= minN and (t + phase) % 2 == 0:
            kp.append(t); since = 0
        if since >= maxN:
            kp.append(t); since = 0
    kp[-1] = N - 2
    return kp


@pytest.mark.parametrize("model", ["pendulum", "acrobot"])
def test_numpy_oracle_builds_the_reference_lists_at_the_edges(model):
    """Every edge configuration on crafted trajectories: the list is the one the reference's loops give (written out
    independently in keypoint_edges.expected_list), percentage_derivs follows it, rows the list and its interpolation never
    reach keep their old values bit for bit, every other row changed."""
    prob_f = PROBLEMS[model]
    rng = np.random.default_rng(11)
    for N in (40, 2, 3, 4, 5):
        cfgs = edge_configs(N) if N >= 6 else short_configs()
        prob = prob_f(N)
        n = prob["Q"].shape[0]
        x0 = np.tile(prob["x_nom"], (1, 1)) + 0.3 * rng.standard_normal((1, n))
        x = crafted_x_bar(x0, N, rng)[0]
        u = 0.2 * rng.standard_normal((1, N - 1))
        for label, cfg in cfgs.items():
            o = make_oracle(prob, keypoint=cfg, jacobian="ad")
            o.fx, o.fu = fx_sentinel(1, n, N)[0].copy(), fu_sentinel(1, n, 1, N)[0].copy()
            kp = o.linearize(x, u)
            want = expected_list(cfg, N)
            if label == "aj_alternating":
                dof = n // 2
                vel = x[dof:2 * dof]
                jerk = (vel[:, 2:] - vel[:, 1:-1]) - (vel[:, 1:-1] - vel[:, :-2])
                phase = 0 if jerk[0, 0] > 0 else 1
                assert np.all(np.abs(np.abs(jerk) - 1.0) < 1e-12)
                want = _alternating_list(N, phase, cfg[1], cfg[2])
            assert want is not None, label
            assert kp == want, (model, N, label, kp, want)
            assert o.percentage_derivs == len(want) / (N - 1) * 100
            touched = set(want)
            if not (cfg[0] == "setInterval" and cfg[1] == 1):
                for a, b in zip(want[:-1], want[1:]):
                    touched.update(range(a, b))
            for t in range(N - 1):
                stale = np.array_equal(o.fx[:, :, t], fx_sentinel(1, n, N)[0, :, :, t])
                assert stale == (t not in touched), (model, N, label, t)
                assert np.array_equal(o.fu[:, :, t], fu_sentinel(1, n, 1, N)[0, :, :, t]) == stale


def _numpy_solve(prob, cfg, x0, max_iters):
    """(oracle, cost, history, status) of the NumPy restatement with the C oracle's status codes: 0 converged, 1 stopped at
    max_iters with the improvement still above delta, 2 line search failed."""
    from oracle.ilqr_np import LinesearchFailed
    o = make_oracle(prob, keypoint=cfg, jacobian="fd", fd_step=1e-5)
    o.max_iters = max_iters
    o.set_problem(x0, prob["x_nom"], prob["Q"], prob["R"], prob["Qf"], np.zeros((1, prob["N"] - 1)))
    try:
        _, _, L, hist = o.solve()
    except LinesearchFailed:
        return o, None, None, 2
    last_improvement = hist[-2][0] - hist[-1][0] if len(hist) > 1 else np.inf
    return o, L, hist, int(len(hist) == max_iters and last_improvement > o.delta)


CASES = [(model, N, label) for model in ("pendulum", "acrobot") for N in (30,) for label in edge_configs(N)] + \
        [("pendulum", N, label) for N in (2, 3, 4, 5) for label in short_configs()]


@pytest.mark.parametrize("model,N,label", CASES)
def test_c_oracle_matches_numpy_oracle_at_the_edges(model, N, label):
    """Whole solves from cold, central differences on both sides: status, iterations, trials and key-point count of every
    iteration, and the last list, exact.  Costs to 1e-10 (pendulum, observed 8e-12) and 1e-9 (acrobot, observed 1.1e-10 on
    its flat optimum; test_c_oracle.py holds both to 1e-10 on the goldens): the two restatements' central differences differ
    at round-off.  Each solve stops before its first iteration decided at round-off
    (keypoint_edges.iterations_before_roundoff)."""
    from oracle import c_oracle, models_np as M
    prob = PROBLEMS[model](N)
    cfg = (edge_configs(N) if N >= 6 else short_configs())[label]
    x0 = _x0(model, 2)
    model_ = M.Model(prob["model_id"], prob["dt"])
    ug = np.zeros((1, N - 1))
    full = c_oracle.solve_batch(model_, prob, x0, ug, keypoint=cfg, hist_cap=64, max_iters=64)
    caps = [iterations_before_roundoff(full["hist"][b, :min(int(full["iters"][b]), 64), 0]) for b in range(2)]
    for b in range(2):
        cap = max(1, caps[b])
        r = c_oracle.solve_batch(model_, prob, x0[b:b + 1], ug, keypoint=cfg, hist_cap=cap, max_iters=cap)
        r = {k: v[0] for k, v in r.items() if k != "threads"}
        o, L, hist, status = _numpy_solve(prob, cfg, x0[b], cap)
        if status == 2:
            assert r["status"] == 2, (b, r["status"])
            continue
        it = len(hist)
        assert r["iters"] == it and r["status"] == status, (b, r["iters"], it, r["status"], status)
        hist = np.array(hist)
        h = r["hist"][:it]
        assert np.array_equal(h[:, 1:3], hist[:, 1:3]), b
        assert np.array_equal(h[:, 3], np.round(hist[:, 3] * (N - 1) / 100.0)), b
        nk = int(r["kp_count"])
        assert nk == len(o.keypoints) and np.array_equal(r["kp_list"][:nk], o.keypoints), b
        assert abs(r["cost"] - L) <= (1e-9 if model == "acrobot" else 1e-10) * abs(L), (b, r["cost"], L)


def test_c_oracle_refuses_adaptive_jerk_with_maxN_below_one():
    """The reference's list can outgrow N - 1 there (ilqr.py:452-463): refused, as mi_ilqr_create refuses it; maxN stays
    free for the two methods that never read it."""
    from oracle import c_oracle, models_np as M
    prob = _pendulum(20)
    model = M.Model(prob["model_id"], prob["dt"])
    x0 = _x0("pendulum", 1)
    for maxN in (0, -1):
        with pytest.raises(ValueError):
            c_oracle.solve_batch(model, prob, x0, None, keypoint=("adaptiveJerk", 1, maxN, 0.0, 0.0), hist_cap=4)
    for cfg in (("setInterval", 2, 0, 0.0, 0.0), ("iterativeError", 2, -1, 0.0, 1e-6), ("adaptiveJerk", 1, 1, 0.0, 0.0)):
        r = c_oracle.solve_batch(model, prob, x0, None, keypoint=cfg, hist_cap=4, max_iters=3)
        assert r["iters"][0] >= 1
