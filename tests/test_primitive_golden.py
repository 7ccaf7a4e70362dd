"""The fixtures of the primitive tests (tests/golden/prim_<name>.npz, written by oracle/gen_primitive_golden.py) are what their
generator writes today: the inputs rebuilt from the seed are the ones the truth was computed at (digest), and a fixed sample of
every array, regenerated with mpmath, is equal to what is stored."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import primitive_probes as P  # noqa: E402

SAMPLE = 61                       # every 61st point of every array (a prime: no phase with the segments' sizes)


@pytest.mark.parametrize("prim", P.PRIMS)
def test_inputs_rebuilt_from_the_seed_are_the_stored_ones(prim):
    g = P.load(prim)
    x = P.inputs(prim)
    assert x.size >= 2 ** 16 and g["hi"].size == x.size
    assert str(g["x_sha1"]) == P.digest(x) and str(g["fd_x_sha1"]) == P.digest(P.fd_inputs(prim))
    m = P.measured(prim)
    assert np.isfinite(g["hi"][m]).all() and np.isnan(g["hi"][~m & ~np.isfinite(x)]).all()
    assert np.abs(g["lo"]).max() <= 0.5 + 1e-6 or prim in ("exp", "softplus")      # (below 2^-1074 hi = 0 and lo counts the rest)
    lo, hi, _ = P.FD_RANGE[prim]
    xf = P.fd_inputs(prim)
    assert xf.min() >= lo and xf.max() <= hi and np.array_equal((xf + P.FD_H) - xf, np.full(xf.size, P.FD_H)) \
        and np.array_equal(xf - (xf - P.FD_H), np.full(xf.size, P.FD_H))                # x +- h exact


@pytest.mark.parametrize("prim", P.PRIMS)
def test_a_sample_of_every_fixture_regenerates_bit_for_bit(prim):
    pytest.importorskip("mpmath")
    from oracle import gen_primitive_golden as G
    g = P.load(prim)
    new = G.arrays(prim, sample=SAMPLE)
    assert set(new) == set(g)
    for k, v in new.items():
        if v.ndim == 0:
            assert str(v) == str(g[k]), k
        else:
            assert v.dtype == g[k].dtype and np.array_equal(v, g[k][::SAMPLE], equal_nan=True), (prim, k)


def test_probe_packing_round_trips():
    """pack() / unpack(): every input of every primitive reaches a slot that evaluates that primitive, and comes back in order."""
    rng = np.random.default_rng(0)
    for name, (n, m, fam, slots) in P.PROBES.items():
        pools = {p: rng.standard_normal(1000 + 37 * i) for i, p in enumerate(P.PRIMS)}
        x0, where = P.pack(slots, pools, 64)
        assert x0.shape[1:] == (64, n)
        back = P.unpack(x0, where, pools)
        for p in P.PRIMS:
            if p in slots:
                assert np.array_equal(back[p], pools[p]), (name, p)
            else:
                assert p not in back
    covered = set(P.PROBES["probe_small_a"][3]) | set(P.PROBES["probe_small_b"][3])
    assert covered == set(P.PRIMS) and set(P.PROBES["probe_mid"][3]) == set(P.PRIMS) and set(P.PROBES["probe_large"][3]) == set(P.PRIMS)


def test_the_stored_multiples_of_half_pi_are_the_nearest_doubles():
    pytest.importorskip("mpmath")
    from oracle import gen_primitive_golden as G
    new = G.kpi()
    with np.load(os.path.join(P.GOLDEN, "prim_kpi.npz")) as z:
        assert np.array_equal(new["near"], z["near"]) and np.array_equal(new["far"], z["far"])
    assert new["near"][2048] == 0.0 and new["near"][2049] == np.pi / 2 and new["far"].size == 1538
