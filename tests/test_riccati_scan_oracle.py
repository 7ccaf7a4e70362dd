"""The NumPy statement of the time-parallel backward pass (riccati_scan_np.Scan) against the NumPy oracle and the
extended-precision recursion, on the CPU: that the restatement states the same pass as oracle.backward() on the workloads' own
matrices, that the committed seeds of test_gpu_small_backward.py leave the fp64 reference its digits (e_ref < 1e-6), and - printed -
what the restatement predicts for every scan case of that file: its distance from the yardstick, and whether the device's guard
fires (asserted: it fires wherever the restatement is outside the yardstick)."""
import numpy as np
import pytest

import riccati_scan_np as RS

OWN = [("pendulum", N) for N in (5, 64, 66, 200, 257, 300)] + [("cartpole_wall", N) for N in (130, 200)]


@pytest.mark.parametrize("model,N", OWN)
def test_restatement_agrees_with_the_oracle_on_the_workloads_own_matrices(model, N):
    """Every problem of the case: the scan's gains within max(1e-11, 20 e_ref) of the extended-precision pass, and directly against
    oracle.backward() at the same bound."""
    refs, e_ref, _ = RS.reference(model, N, "own")
    for b in range(RS.B):
        o = RS.oracle_for(model, N, "own", b)
        sc = RS.Scan(o).run()
        o.backward()
        e_scan = RS.distance((sc.K, sc.kappa, sc.dV), refs[b])
        d_np = RS.distance((sc.K, sc.kappa, sc.dV), (o.K, o.kappa, o.dV))
        bound = max(1e-11, 20 * e_ref[b])
        assert e_scan < bound and d_np < 2 * bound, (b, e_scan, d_np, e_ref[b], sc.cond_P)
        assert np.isfinite(sc.K).all() and not sc.fires()                             # (the device's guard stays silent)


def test_inversion_choice_does_not_matter_on_a_benign_input():
    """The device's inversions of P (adjugate, unpivoted Gauss-Jordan) and np.linalg.inv give the same pass where P is benign."""
    for model, N in (("pendulum", 66), ("cartpole_wall", 130)):
        o = RS.oracle_for(model, N, "own", 0)
        a, b = RS.Scan(o, "device").run(), RS.Scan(o, "inv").run()
        assert RS.distance((a.K, a.kappa, a.dV), (b.K, b.kappa, b.dV)) < 1e-11


def _cases():
    import test_gpu_small_backward as G
    shapes = sorted(set(G.N2_SCAN + G.N4_MFMA + G.N4_SCAN + G.LIMITED))
    return [(mdl, N, lab) for mdl, N in shapes for lab in RS.cost_labels(mdl)]


def test_committed_seeds_leave_the_reference_its_digits():
    """e_ref < 1e-6 on every problem of every case of the GPU file (its pass/fail rule never rests on a reference without digits)."""
    worst = 0.0
    for mdl, N, lab in _cases():
        _, e_ref, _ = RS.reference(mdl, N, lab)
        worst = max(worst, float(e_ref.max()))
        assert (e_ref < 1e-6).all(), (mdl, N, lab, e_ref)
    _, e_ref, _ = RS.reference("pendulum", 66, "R1e-9_Qf100", True)
    assert (e_ref < 1e-6).all()
    print(f"largest e_ref over the committed cases: {worst:.2e}")


def test_print_the_restatements_prediction():
    """The table of the scan cases (problems 0 and 1 of each, the worse one): the restatement's distance from the extended-precision
    pass, the fp64 pass's, their ratio, the smallest unpivoted pivot and the largest cond(P) of any composition, and the
    quantities the device's guard looks at (Scan.edge_gap for n = 2, Scan.gain_gap for n = 4; Scan.guard()).  Asserted: whatever the guard lets
    through is inside the yardstick.  Run with -s to read it."""
    import test_gpu_small_backward as G
    print(f"\n{'input':44s} {'scan':>8s} {'NumPy':>8s} {'ratio':>8s} {'min piv':>8s} {'cond(P)':>8s} {'edge gap':>8s} {'gain gap':>8s}  within the yardstick / guard")
    for mdl, N in G.N2_SCAN + G.N4_SCAN:
        for lab in RS.cost_labels(mdl):
            refs, e_ref, _ = RS.reference(mdl, N, lab)
            rows = []
            for b in range(2):
                sc = RS.Scan(RS.oracle_for(mdl, N, lab, b)).run()
                e = RS.distance((sc.K, sc.kappa, sc.dV), refs[b])
                rows.append((e / max(1e-11, 20 * e_ref[b]), e, e_ref[b], sc))
            r, e, er, sc = max(rows, key=lambda v: v[0])
            print(f"{mdl + ' N = ' + str(N) + ' ' + lab:44s} {e:8.1e} {er:8.1e} {e / er:8.2g} {sc.min_pivot:8.1e} {sc.cond_P:8.1e} "
                  f"{sc.edge_gap:8.1e} {sc.gain_gap:8.1e}  {'yes' if r < 1 else 'NO'} / {'fires' if sc.fires() else 'silent'}")
            assert all(r_ < 1 or sc_.fires() for r_, _, _, sc_ in rows), (mdl, N, lab, r, sc.guard())
