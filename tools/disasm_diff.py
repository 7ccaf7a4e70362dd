"""Device instruction text of two builds, function by function: python tools/disasm_diff.py OBJDIR_A OBJDIR_B

For every k_*.o / mi_ilqr.o present in both object directories (drake_ddp_amd/lib/obj of two checkouts): take the gfx950 code object
out of the host object's .hip_fatbin section, disassemble it and compare the text of each device function.  Exit status 1 when a
function differs or exists on one side only.  How "the built-in kernels do not change" is checked for a change to the shared headers."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def functions(obj, tmp):
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co, "--unbundle"])
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^<(.*)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None and line.strip():
            out[name].append(line.strip())
    return out


def main(a, b):
    names = sorted(f for f in os.listdir(a) if re.match(r"(k_.*|mi_ilqr)\.o$", f) and os.path.exists(os.path.join(b, f)))
    total = diff = 0
    with tempfile.TemporaryDirectory() as tmp:
        for f in names:
            fa, fb = functions(os.path.join(a, f), tmp), functions(os.path.join(b, f), tmp)
            bad = sorted(k for k in set(fa) | set(fb) if fa.get(k) != fb.get(k))
            total += len(set(fa) | set(fb))
            diff += len(bad)
            print("%-28s %3d functions%s" % (f, len(fa), "" if not bad else ", DIFFERENT: " + ", ".join(bad[:4])))
    print("%d device functions in %d objects, %d differ" % (total, len(names), diff))
    return 1 if diff or not names else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
