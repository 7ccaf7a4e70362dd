"""Every documented primitive of the open model interface (drake_ddp_amd/plugin.py: + - * / and mi_sin, mi_cos, mi_rcp, mi_exp,
mi_log1p, mi_sqrt, mi_softplus) has an overload for every scalar type a kernel family instantiates step() with: double, Dual1,
and - for n = 2, m = 1, the time-parallel Newton rollout - Dual2.  Compile-only: needs hipcc, no GPU.  Before Dual2 had
operator/, mi_exp, mi_log1p, mi_sqrt and mi_softplus the n = 2, m = 1 case failed ("candidate template ignored: substitution
failure [with T = Dual2]") while the other three shapes built."""
import concurrent.futures
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# one body for any (n, m): every primitive, and / in its three forms
ALL_PRIMITIVES_BODY = """    const T q = x[0], v = x[1];
    const T w = q * q;
    T a = u[0] - mi_sin(q) - 0.1 * (v / (2.0 + w)) - 0.05 * mi_softplus(q - 1.0);
    a = a + 0.01 * mi_exp(-w) - 0.01 * mi_log1p(w) + 0.01 * (mi_sqrt(1.0 + v * v) - 1.0) * mi_cos(q);
    a = a + 0.01 * mi_rcp(1.0 + w) + 0.001 * (1.0 / (3.0 + v * v)) + 0.001 * (q / 4.0);
    const T vn = v + dt * a;
    xn[1] = vn; xn[0] = q + dt * vn;
    for (int i = 2; i < n; ++i) xn[i] = 0.9 * x[i] + dt * u[i % m];"""

SHAPES = [(2, 1, "small"), (2, 2, "small"), (4, 1, "small"), (8, 3, "large")]


def test_one_body_with_every_primitive_compiles_at_every_shape_class():
    from drake_ddp_amd import plugin
    with concurrent.futures.ThreadPoolExecutor(4) as ex:
        futs = {sh: ex.submit(plugin.compile_model, "allprims_%d_%d" % sh[:2], sh[0], sh[1], ALL_PRIMITIVES_BODY, (), sh[2]) for sh in SHAPES}
    errors = {}
    for sh, f in futs.items():
        try:
            assert os.path.exists(f.result())
        except RuntimeError as e:
            errors[sh] = str(e)[-1500:]
    assert not errors, errors
