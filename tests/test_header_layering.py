"""The layering of the native headers (drake_ddp_amd/csrc/*.hpp; DESIGN.md, "Source layout"): every header compiles as the only
include of a translation unit, and the `#include "..."` lines keep the kernel families apart - no family header includes
another, the host (host.hpp, host_internal.hpp and every host unit) includes none of them, policy_rollout.hpp names what it uses.  Compile-only
(-fsyntax-only) and text checks: needs hipcc, no GPU.  At the end, the same for the Python front end: which module of
drake_ddp_amd/{argcheck, results, ilqr}.py may import which."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from drake_ddp_amd import build  # noqa: E402

FAMILY = {"ilqr_small.hpp", "ilqr_large.hpp", "ilqr_batch.hpp", "policy_rollout.hpp"}
HEADERS = sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hpp"))


def includes(name):
    """The quoted includes of csrc/<name>, as written."""
    with open(os.path.join(build.CSRC, name)) as f:
        return re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M)


def test_the_headers_the_rules_speak_of_exist():
    assert FAMILY <= set(HEADERS)
    assert {"host.hpp", "kernel_args.hpp", "lds_layout.hpp", "wave_ops.hpp", "cost_terms.hpp", "model_traits.hpp", "models.hpp",
            "fastmath.hpp", "launch_small.hpp", "launch_large.hpp", "launch_batch.hpp"} <= set(HEADERS)


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_as_the_only_include(header, tmp_path):
    src = tmp_path / ("only_" + header[:-4] + ".hip")
    src.write_text('#include "%s"\n' % os.path.join(build.CSRC, header))
    r = subprocess.run([build.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]


@pytest.mark.parametrize("header", sorted(FAMILY))
def test_no_family_header_includes_another(header):
    assert not (set(includes(header)) & FAMILY), includes(header)


def test_the_shared_headers_include_no_family_header_and_no_launch_templates():
    for name in ("kernel_args.hpp", "lds_layout.hpp", "wave_ops.hpp", "cost_terms.hpp", "host.hpp"):
        inc = set(includes(name))
        assert not (inc & FAMILY) and not any(i.startswith("launch_") for i in inc), (name, sorted(inc))


def test_kernel_args_knows_no_model_and_no_keypoint_code():
    assert includes("kernel_args.hpp") == ["../../include/mi_ilqr.h"]
    with open(os.path.join(build.CSRC, "kernel_args.hpp")) as f:
        assert sorted(re.findall(r"^\s*#\s*include\s+<([^>]+)>", f.read(), re.M)) == ["hip/hip_runtime.h", "stdint.h"]


def test_host_takes_the_kernel_arguments_from_their_own_header():
    assert "kernel_args.hpp" in includes("host.hpp")


def test_policy_rollout_names_what_it_uses():
    assert {"host.hpp", "fastmath.hpp", "model_traits.hpp", "models.hpp"} <= set(includes("policy_rollout.hpp"))


HOST_UNITS = sorted(os.path.basename(s) for s in build.host_sources())
INTERNAL = "host_internal.hpp"


def test_the_host_units_are_the_units_that_are_no_kernel_units():
    units = sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip"))
    assert HOST_UNITS == [f for f in units if not f.startswith("k_")]
    assert "mi_ilqr.hip" in HOST_UNITS and all(f == "mi_ilqr.hip" or f.startswith("h_") for f in HOST_UNITS), HOST_UNITS
    assert len(HOST_UNITS) >= 2


@pytest.mark.parametrize("unit", HOST_UNITS)
def test_no_host_unit_includes_a_family_header_or_kernel_templates(unit):
    inc = set(includes(unit))
    assert INTERNAL in inc or "host.hpp" in inc, sorted(inc)
    assert not (inc & FAMILY) and not any(i.startswith("launch_") for i in inc), sorted(inc)


def test_the_abi_unit_includes_the_interface_and_no_kernel_templates():
    inc = set(includes("mi_ilqr.hip"))
    assert {"host.hpp", INTERNAL, "kernel_args.hpp", "lds_layout.hpp", "models.hpp"} <= inc
    assert not (inc & FAMILY) and not any(i.startswith("launch_") for i in inc), sorted(inc)


def test_the_internal_header_is_the_host_units_own():
    """host_internal.hpp: included by host units only - no kernel unit, no header, not the plugin template - and it includes host.hpp
    and no family header or launch templates."""
    inc = set(includes(INTERNAL))
    assert "host.hpp" in inc and not (inc & FAMILY) and not any(i.startswith("launch_") for i in inc), sorted(inc)
    for name in sorted(os.listdir(build.CSRC)):
        if (name.endswith(".hip") or name.endswith(".hpp")) and name not in HOST_UNITS:
            assert INTERNAL not in includes(name), name
    from drake_ddp_amd import plugin
    for family in ("small", "large"):
        assert INTERNAL not in plugin.source("t", 2, 1, "xn[0] = x[0]; xn[1] = x[1] + dt * u[0];", [], family)


def test_the_communicator_alone_includes_rccl_and_dlfcn():
    for name in sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip") or f.endswith(".hpp")):
        with open(os.path.join(build.CSRC, name)) as f:
            system = set(re.findall(r"^\s*#\s*include\s+<([^>]+)>", f.read(), re.M))
        assert not (system & {"rccl/rccl.h", "dlfcn.h"}) or name == "h_comm.hip", name


def test_each_launch_header_serves_one_family():
    for launch, family in (("launch_small.hpp", "ilqr_small.hpp"), ("launch_large.hpp", "ilqr_large.hpp"), ("launch_batch.hpp", "ilqr_batch.hpp")):
        assert set(includes(launch)) & FAMILY == {family}, (launch, includes(launch))


# ---------------------------------------------------------------- the Python front end ("The Python side")
PACKAGE = os.path.join(ROOT, "drake_ddp_amd")
MOVED = ("check_model_params", "check_target_trajectory", "check_rollout_args", "check_noise_args", "check_plant_args", "check_mc_args",
         "check_mc_observe", "check_seed_args", "check_mppi_args", "MC_DISTS", "PolicySamples", "MPPIResult", "SeedSelection",
         "PolicyEnvelope", "PolicySafety", "PolicyStats", "PlantLog", "PolicyRollout", "_chan")


def python_imports(module):
    """-> (modules imported from outside the package, names imported from the package) by drake_ddp_amd/<module>.py, anywhere in it."""
    import ast
    with open(os.path.join(PACKAGE, module + ".py")) as f:
        tree = ast.parse(f.read())
    outside, inside = set(), set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            outside |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom) and node.level == 0:
            (inside if node.module.split(".")[0] == "drake_ddp_amd" else outside).add(node.module)
        elif isinstance(node, ast.ImportFrom):
            inside |= {node.module} if node.module else {a.name for a in node.names}
    return outside, inside


def test_results_and_argcheck_need_neither_the_library_nor_ctypes():
    assert python_imports("results") == ({"numpy"}, set())
    assert python_imports("argcheck") == ({"numpy"}, {"_capi"})
    with open(os.path.join(PACKAGE, "argcheck.py")) as f:
        assert "load(" not in f.read()
    child = ("import sys; import drake_ddp_amd.argcheck, drake_ddp_amd.results; from drake_ddp_amd import _capi; "
             "assert _capi._lib is None; assert 'drake_ddp_amd.ilqr' not in sys.modules")
    r = subprocess.run([sys.executable, "-c", child], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]


def test_ilqr_hands_on_every_name_that_moved():
    from drake_ddp_amd import argcheck, ilqr, results
    for name in MOVED:
        home = argcheck if name.startswith("check_") or name == "MC_DISTS" else results
        assert getattr(ilqr, name) is getattr(home, name), name
    for name in ("shard_range", "allreduce_min", "allreduce_min_async", "_PinnedBlock", "BatchedIterativeLQR", "IterativeLinearQuadraticRegulator"):
        assert hasattr(ilqr, name), name
    assert {"argcheck", "results"} <= python_imports("ilqr")[1]
