"""Build libmi_ilqr.so (HIP, gfx950) in-tree with hipcc.

    python -m drake_ddp_amd.build [--force] [--resource-usage]

One translation unit per model's kernels (csrc/k_<model>.hip) plus the host side of the C ABI, a unit per
concern (csrc/mi_ilqr.hip and csrc/h_<concern>.hip: host_sources()), compiled in parallel and linked into drake_ddp_amd/lib/libmi_ilqr.so (git-ignored,
but it travels to the GPU box with the gpurun snapshot).  hipcc cross-compiles without a GPU.
Objects are cached in drake_ddp_amd/lib/obj, each beside the dependency file the compiler wrote for it (<obj>.d), and rebuilt
when their source, a file it includes or the flags change.
"""
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
OBJDIR = os.path.join(LIBDIR, "obj")
LIB = os.path.join(LIBDIR, "libmi_ilqr.so")

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -amdgpu-mfma-vgpr-form: MFMA accumulators / results in the architectural VGPRs (gfx90a+ has one register file) instead of the
# AGPRs the compiler's heuristic picks - in the backward passes every MFMA result feeds VALU work (Vxx' = H + 2Q - ..., stores)
# and 29 % of the arm's hottest MFMA loop were v_accvgpr moves.  Same-box A/B, round 5: backward step of the arm 5.5 k -> 5.15 k
# cycles, C5 350 k -> 359 k, C6 166 k -> 171 k, C3 18.7 M -> 19.1 M it/s; results bitwise unchanged (same instructions, other registers).
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math",
         "-ffp-contract=fast", "-Wall", "-Wno-unused-function", "-mllvm", "-amdgpu-mfma-vgpr-form=1"]


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def host_sources():
    """The host units: every unit that is not a kernel unit (k_*.hip)."""
    return [s for s in sources() if not os.path.basename(s).startswith("k_")]


def headers():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")) + \
        [os.path.join(HERE, "..", "include", "mi_ilqr.h")]


def _obj(src, tag):
    return os.path.join(OBJDIR, os.path.basename(src)[:-4] + tag + ".o")


def _deps(obj):
    """The files `obj` was compiled from, out of the compiler's dependency file (-MD -MF obj.d), or None when there is none."""
    try:
        with open(obj + ".d") as f:
            text = f.read()
    except (OSError, UnicodeDecodeError):
        return None
    words = re.split(r"(?<!\\)\s+", text.replace("\\\n", " ").strip())      # (a space inside a path is written "\ ")
    colon = next((i for i, w in enumerate(words) if w.endswith(":")), None)
    return None if colon is None else [w.replace("\\ ", " ") for w in words[colon + 1:]]


def _stale(obj, src):
    """An object is rebuilt when its source or a file it includes is newer - or gone - or when it has no dependency file."""
    deps = _deps(obj)
    if not os.path.exists(obj) or deps is None:
        return True
    t = os.path.getmtime(obj)
    return any(not os.path.exists(d) or os.path.getmtime(d) > t for d in [src] + deps)


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(d) > t for d in sources() + headers() if os.path.exists(d))


def _compile(src, obj, flags, verbose):
    cmd = [HIPCC] + flags + ["-MD", "-MF", obj + ".d", "-c", src, "-o", obj]
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return src, r.returncode, r.stdout


def build(force=False, verbose=True, extra=(), lib=LIB):
    """Compile (in parallel) and link.  `extra`: additional compiler flags (they get their own object cache);
    `lib`: output path."""
    os.makedirs(OBJDIR, exist_ok=True)
    if not force and not extra and lib == LIB and not needs_build():
        return lib
    flags = FLAGS + list(extra)
    tag = ("-" + hashlib.sha1(" ".join(extra).encode()).hexdigest()[:8]) if extra else ""
    jobs = [(s, _obj(s, tag)) for s in sources()]
    todo = [(s, o) for s, o in jobs if force or _stale(o, s)]
    logs = {}
    if todo:
        workers = max(1, min(len(todo), os.cpu_count() or 4))
        with concurrent.futures.ThreadPoolExecutor(workers) as ex:
            for src, rc, out in ex.map(lambda so: _compile(so[0], so[1], flags, verbose), todo):
                logs[src] = out
                if rc != 0:
                    sys.stderr.write(out)
                    raise subprocess.CalledProcessError(rc, [HIPCC, src])
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC"] + [o for _, o in jobs] + ["-o", lib, "-ldl"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    if "-Rpass-analysis=kernel-resource-usage" in extra:
        with open(os.path.join(LIBDIR, "resource_usage.txt"), "w") as f:
            for s in sorted(logs):
                f.write(logs[s])
    return lib


ASAN_LIB = os.path.join(LIBDIR, "libmi_ilqr_asan.so")
ASAN_RT = "/opt/rocm/lib/llvm/lib/clang/22/lib/linux/libclang_rt.asan-x86_64.so"


def build_asan(verbose=False):
    """libmi_ilqr_asan.so: the HOST side of the C ABI (host_sources()) instrumented with AddressSanitizer, linked
    with the regular kernel objects (device code cannot be instrumented on gfx950).  tests/test_gpu_asan.py drives it."""
    build(verbose=verbose)
    flags = [f for f in FLAGS if f != "-O3"] + ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address", "-shared-libsan", "-Wno-option-ignored"]
    host = [(s, _obj(s, "-asan")) for s in host_sources()]
    for src, obj in host:
        if _stale(obj, src):
            _, rc, out = _compile(src, obj, flags, verbose)
            if rc != 0:
                sys.stderr.write(out)
                raise subprocess.CalledProcessError(rc, [HIPCC, src])
    if not os.path.exists(ASAN_LIB) or os.path.getmtime(ASAN_LIB) < max([os.path.getmtime(o) for _, o in host] + [os.path.getmtime(LIB)]):
        objs = [_obj(s_, "") for s_ in sources() if s_ not in host_sources()]
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-fsanitize=address", "-shared-libsan", "-Wno-option-ignored"] +
                              [o for _, o in host] + objs + ["-o", ASAN_LIB, "-ldl"])
    return ASAN_LIB


if __name__ == "__main__":
    ex = ["-Rpass-analysis=kernel-resource-usage"] if "--resource-usage" in sys.argv else []
    build(force="--force" in sys.argv, extra=ex)
    if "--asan" in sys.argv or os.path.exists(ASAN_LIB):      # (an existing sanitizer build follows the headers: a stale one refuses plugins)
        build_asan(verbose="--asan" in sys.argv)
