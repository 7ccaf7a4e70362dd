"""The backward passes of the wave-per-problem kernels (csrc/ilqr_small.hpp) against the reference's recursion in extended
precision - the yardstick of test_gpu_conditioning.py (tests/common.py: backward_extended), unchanged:
    status == 0, every output finite, e_dev < max(1e-11, 20 x the fp64 NumPy pass's own distance).
One backward pass per case, B = 8 seeded problems per launch, on inputs the NumPy oracle made (riccati_scan_np.trajectories:
its rollout of a random control guess from a random start and its forward-mode Jacobians), so the device and the references
see identical x_bar, u_bar, fx, fu.  Forms and the smallest shapes that reach them:
    n = 2 scan, chunks held in registers   pendulum N = 5 (lanes past the horizon), 64 (one element per lane), 66 (chunk 2, the
                                           terminal element among the live lanes), 257 (chunk 4, the last held horizon)
    n = 2 scan, chunks re-read             pendulum N = 300
    n = 2 backward_scalar                  pendulum N = 66: MI_ILQR_SEQ_BACKWARD=1 (a child process) and the exact form (a Q that
                                           is asymmetric by one ulp)
    n = 4 backward_mfma                    acrobot, cart-pole, cart-pole with wall at N = 40, 128; the cart-pole at its own N = 100
    n = 4 scan (LongHorizon kernels)       acrobot, cart-pole with wall at N = 130 (first chunk of 3), 200; the same shapes with
                                           MI_ILQR_SEQ_BACKWARD=1: backward_mfma inside the LongHorizon kernels
    Limited<M> (box-QP pass)               pendulum N = 66, cart-pole N = 40, limits too wide to clamp anything
(The host's model table puts four built-in models on this kernel family - pendulum, acrobot, cart-pole, cart-pole with wall - all
with m = 1; the m = 2 form of backward_scalar is reached by plug-in models only.)
Cost scalings per form: R x {1, 1e-3, 1e-6} and Qf x {1, 100} on the workload's Q, one dense Qf, for n = 2 also R x 1e-9.  The
seeds are chosen such that the fp64 NumPy pass keeps e_ref < 1e-6 everywhere (test_riccati_scan_oracle.py checks it on the CPU).
Measured when these tests were written (MI355X; DESIGN 8.1 has the table): the sequential forms are inside the yardstick
everywhere (worst e_dev / bound 0.36); the scans as they were - no check of their own result - missed it in 8 of 45 (n = 2:
R x 1e-9 at every held horizon, e_dev 5.8e-8 against e_ref 1.1e-11) and 20 of 28 cases (n = 4: every acrobot case, 8.5 x the
bound on its own cost at N = 130, 1.2e5 x with R x 1e-6, Qf x 100 at N = 200 where the gains were off by 1.8e-2).  The scans now
check themselves and hand such passes to the sequential sweep (backward_scan, phase (4)); what they keep is inside at 0.29."""
import json
import os
import sys

import numpy as np
import pytest

import riccati_scan_np as RS
from test_gpu_parity import make_solver

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N2_SCAN = [("pendulum", N) for N in (5, 64, 66, 257, 300)]
N4_MFMA = [(mdl, N) for mdl in ("acrobot", "cartpole", "cartpole_wall") for N in (40, 128)] + [("cartpole", 100)]
N4_SCAN = [(mdl, N) for mdl in ("acrobot", "cartpole_wall") for N in (130, 200)]
LIMITED = [("pendulum", 66), ("cartpole", 40)]


def _with_costs(shapes):
    return [(mdl, N, lab) for mdl, N in shapes for lab in RS.cost_labels(mdl)]


def _id(case):
    return "-".join(str(v) for v in case)


def device_pass(model, N, label, asym=False, limited=False):
    """One backward pass of the device on the case's inputs: (K (B, m, n, N-1), kappa, dV_coeff, status)."""
    prob = RS.problem(model, N)
    Q, R, Qf = RS.cost_matrices(prob, label)
    if asym:
        Q = RS.asymmetric(Q)
    x0, ug, xb, fx, fu = RS.trajectories(model, N)
    kw = dict(control_limits="enforce") if limited else {}
    s = make_solver(dict(prob, Q=Q, R=R, Qf=Qf), B=RS.B, jac="ad", **kw)
    if limited:
        s.SetControlLimits(-1e6, 1e6)
    s.SetInitialState(x0)
    s.SetInitialGuess(ug)
    s.set_state(x_bar=xb, u_bar=ug, fx=fx, fu=fu)
    s.stage_backward()
    return s.K, s.kappa, s.dV_coeff, s.status.copy()


def judge(form, case, out, asym=False):
    """The yardstick on every problem of a case; prints the worst problem's figures and the restatement's cond(P) on it."""
    model, N, label = case
    K, kappa, dV, status = out
    refs, e_ref, cond = RS.reference(model, N, label, asym)
    e_dev = np.array([RS.distance((K[b], kappa[b], dV[b]), refs[b]) for b in range(RS.B)])
    bound = np.maximum(1e-11, 20 * e_ref)
    b = int(np.argmax(e_dev / bound))
    sc = RS.Scan(RS.oracle_for(model, N, label, b, asym)).run()
    print(f"{form} {model} N = {N} {label}: e_dev {e_dev[b]:.2e}, e_ref {e_ref[b]:.2e}, ratio {e_dev[b] / max(e_ref[b], 1e-300):.3g}, "
          f"e_dev / bound {e_dev[b] / bound[b]:.3g}; restatement cond(P) {sc.cond_P:.1e}, min pivot {sc.min_pivot:.1e}; "
          f"max cond(Quu) {cond.max():.1e}; status {status.tolist()}")
    assert (e_ref < 1e-6).all(), e_ref
    assert (status == 0).all(), status
    assert all(np.isfinite(a).all() for a in (K, kappa, dV))
    assert (e_dev < bound).all(), (e_dev, e_ref)
    return e_dev, e_ref


# ------------------------------------------------------------------------------------------------------------------------
# The forced sequential forms (MI_ILQR_SEQ_BACKWARD=1 is read once per process): one child process runs every case.
# ------------------------------------------------------------------------------------------------------------------------
SEQ_CASES = _with_costs(N2_SCAN + N4_SCAN)


@pytest.fixture(scope="module")
def sequential(tmp_path_factory):
    import subprocess
    out = str(tmp_path_factory.mktemp("seq") / "seq.npz")
    script = f"""
import json, sys, numpy as np
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
from test_gpu_small_backward import device_pass
res = {{}}
for i, case in enumerate(json.loads(sys.argv[2])):
    K, kappa, dV, status = device_pass(*case)
    res.update({{f"K{{i}}": K, f"k{{i}}": kappa, f"d{{i}}": dV, f"s{{i}}": status}})
np.savez(sys.argv[1], **res)
"""
    r = subprocess.run([sys.executable, "-c", script, out, json.dumps(SEQ_CASES)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, MI_ILQR_SEQ_BACKWARD="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    return {case: (z[f"K{i}"], z[f"k{i}"], z[f"d{i}"], z[f"s{i}"]) for i, case in enumerate(SEQ_CASES)}


@pytest.mark.parametrize("case", _with_costs(N2_SCAN), ids=_id)
def test_n2_scan(case):
    judge("n2-scan", case, device_pass(*case))


@pytest.mark.parametrize("case", _with_costs(N2_SCAN), ids=_id)
def test_n2_sequential(case, sequential):
    """backward_scalar through MI_ILQR_SEQ_BACKWARD=1 (N = 66 is the shape the form needs; the other horizons are the
    sequential side of test_scan_falls_back_to_the_sequential_sweep)."""
    judge("n2-scalar-seq", case, sequential[case])


@pytest.mark.parametrize("case", _with_costs([("pendulum", 66)]), ids=_id)
def test_n2_exact_form(case):
    """backward_scalar as the exact form (mode 2): Q asymmetric by one ulp of its largest entry."""
    judge("n2-scalar-exact", case, device_pass(*case, asym=True), asym=True)


@pytest.mark.parametrize("case", _with_costs(N4_MFMA), ids=_id)
def test_n4_mfma(case):
    judge("n4-mfma", case, device_pass(*case))


@pytest.mark.parametrize("case", _with_costs(N4_SCAN), ids=_id)
def test_n4_scan(case):
    judge("n4-scan", case, device_pass(*case))


@pytest.mark.parametrize("case", _with_costs(N4_SCAN), ids=_id)
def test_n4_long_horizon_sequential(case, sequential):
    judge("n4-mfma-long", case, sequential[case])


FIRING = [("acrobot", 130, "R1e-6_Qf100"), ("cartpole_wall", 200, "R1e-3_Qf100"), ("pendulum", 5, "R1e-9"), ("pendulum", 66, "R1e-9"),
          ("pendulum", 257, "R1e-9"), ("pendulum", 300, "R1e-9_Qf100")]
SILENT = [("pendulum", 66, "own"), ("pendulum", 257, "own"), ("pendulum", 300, "own"), ("cartpole_wall", 130, "own"),
          ("cartpole_wall", 200, "own")]


@pytest.mark.parametrize("case", FIRING, ids=_id)
def test_scan_falls_back_to_the_sequential_sweep(case, sequential):
    """Where the scan's own check fires (backward_scan, phase (4): the restatement's guard quantity is 1e2 .. 1e9 x its threshold
    on these inputs) the pass is redone by the sequential sweep: K, kappa, dV equal the MI_ILQR_SEQ_BACKWARD=1
    child's BIT FOR BIT.  That the equality is the fallback's doing and not the scan's: before the guard the scan's gains on
    these inputs were 5e-8 (pendulum, R x 1e-9) to 2e-2 (acrobot) away from the extended-precision pass, the sequential sweep's
    < 1e-8, and test_scan_stays_on_benign_inputs shows that a scan that ran does differ in its last bits."""
    out, seq = device_pass(*case), sequential[case]
    sc = RS.Scan(RS.oracle_for(*case, 0)).run()
    v, tol = sc.guard()
    print(f"{_id(case)}: restatement's guard quantity {v:.1e} (threshold {tol:g})")
    assert v > 10 * tol
    assert (out[3] == 0).all()
    for a, b in zip(out[:3], seq[:3]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("case", SILENT, ids=_id)
def test_scan_stays_on_benign_inputs(case, sequential):
    """On the workloads' own matrices the guard is silent: the result is the scan's, which differs from the sequential sweep's in
    its last bits (and only there: 1e-11)."""
    out, seq = device_pass(*case), sequential[case]
    assert any(not np.array_equal(a, b) for a, b in zip(out[:3], seq[:3]))
    for a, b in zip(out[:3], seq[:3]):
        assert np.max(np.abs(a - b)) <= 1e-11 * np.max(np.abs(b))


@pytest.mark.parametrize("case", _with_costs(LIMITED), ids=_id)
def test_limited_pass_with_inactive_limits(case):
    """Limited<M>: the box-QP backward pass with limits no step reaches must meet the free pass's yardstick."""
    judge("limited", case, device_pass(*case, limited=True))
