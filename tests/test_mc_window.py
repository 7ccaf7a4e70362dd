"""The window arithmetic of the on-device Monte-Carlo (drake_ddp_amd/csrc/mc_window.hpp: mc_window, what run_policy_mc plans its
passes with) as a host-only program: compiled here with the host compiler, run on a table of inputs, and checked against a Python
restatement of the arithmetic and against the invariants every plan has to keep.  No GPU, no HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drake_ddp_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include "mc_window.hpp"
int main() {
  unsigned long long G, B, group_bytes, traj_group_bytes;
  int forced;
  while (std::scanf("%llu %llu %llu %llu %d", &G, &B, &group_bytes, &traj_group_bytes, &forced) == 5) {
    const mi_host::McWindow w = mi_host::mc_window(G, (size_t)B, (size_t)group_bytes, (size_t)traj_group_bytes, forced);
    std::printf("%llu %llu\n", w.k, w.passes);
  }
  std::printf("caps %llu %llu %llu\n", (unsigned long long)mi_host::kMcWindowBytes, (unsigned long long)mi_host::kMcTrajWindowBytes,
              mi_host::kMcEventPairs);
  return 0;
}
"""

WINDOW, TRAJ_WINDOW, FIELDS, INT_MAX = 64 << 20, 1 << 30, 10, 0x7fffffff


def host_compiler():
    for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(c)
        if path:
            return path
    pytest.fail("no host C++ compiler")


def run_bytes(S, B, n, m, N, n_params, samples, keep_x, env_u):
    """G, and the bytes of a group of 64 samples as run_policy_mc counts them: the partials and the optional sample buffers; the
    optional trajectory windows (0: the run observes nothing)."""
    SW = n + n_params + 2
    group = FIELDS * B * 8 + (2 * B * 64 * SW * 8 if samples else 0)
    traj = B * 64 * 8 * ((N * n if keep_x else 0) + ((N - 1) * m if env_u else 0))
    return (S + 63) // 64, group, traj


def window_py(G, B, group, traj, forced):
    """The arithmetic as run_policy_mc did it in place before it had a function of its own."""
    k = max(1, WINDOW // group)
    if traj:
        k = min(k, max(1, TRAJ_WINDOW // traj))
    if forced > 0:
        k = forced
    k = min(min(k, G), max(1, INT_MAX // B))
    return k, (G + k - 1) // k


def table():
    rows = []
    for forced in (0, 1, 3, 7, 4000, 10 ** 6):
        for S, B, n, m, N, npar in ((1, 1, 2, 1, 50, 3), (64, 3, 2, 1, 50, 3), (65, 3, 4, 1, 101, 4), (5000, 7, 2, 1, 50, 0),
                                    (2 ** 32, 1, 2, 1, 50, 3), (2 ** 32, 4096, 4, 2, 200, 10), (320000, 1 << 20, 2, 1, 50, 3),
                                    (10 ** 6, INT_MAX, 2, 1, 3, 0), (10 ** 6, INT_MAX // 2, 2, 1, 3, 0), (10 ** 6, 10 ** 6, 2, 1, 50, 3),
                                    (100000, 64, 36, 12, 4001, 4), (100000, 1000, 27, 7, 300, 15)):
            for samples in (False, True):
                for keep_x, env_u in ((False, False), (True, False), (False, True), (True, True)):
                    G, group, traj = run_bytes(S, B, n, m, N, npar, samples, keep_x, env_u)
                    rows.append((G, B, group, traj, forced))
    return rows


def test_the_window_function_against_its_restatement_and_its_invariants(tmp_path):
    src, exe = tmp_path / "mc_window_table.cpp", tmp_path / "mc_window_table"
    src.write_text(PROGRAM)
    r = subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    rows = table()
    out = subprocess.run([str(exe)], input="".join("%d %d %d %d %d\n" % row for row in rows), stdout=subprocess.PIPE, text=True, check=True)
    lines = out.stdout.split("\n")
    assert lines[len(rows)] == "caps %d %d 32" % (WINDOW, TRAJ_WINDOW)
    seen = set()
    for (G, B, group, traj, forced), line in zip(rows, lines):
        k, passes = (int(v) for v in line.split())
        case = (G, B, group, traj, forced, k, passes)
        assert (k, passes) == window_py(G, B, group, traj, forced), case
        assert 1 <= k <= G and k * B <= INT_MAX and passes == -(-G // k), case
        if forced > 0:
            assert k == min(forced, G, max(1, INT_MAX // B)), case                     # honoured up to the caps
        else:
            assert k == 1 or (k * group <= WINDOW and k * traj <= TRAJ_WINDOW), case      # more than one group: within both windows
        if group > WINDOW or traj > TRAJ_WINDOW:
            assert forced > 0 or k == 1, case
        seen |= {("G1", G == 1), ("int31", INT_MAX // B < G), ("group", group > WINDOW), ("traj", traj > TRAJ_WINDOW), ("traj0", traj == 0),
                 ("forced>G", forced > G), ("capped", forced > 0 and k < min(forced, G)), ("many", forced == 0 and k > 1 and passes > 1)}
    assert seen == {(name, flag) for name in ("G1", "int31", "group", "traj", "traj0", "forced>G", "capped", "many") for flag in (False, True)}
