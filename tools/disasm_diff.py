"""Device instruction text of two builds, function by function: python tools/disasm_diff.py OBJDIR_A OBJDIR_B

For every object of the two object directories (drake_ddp_amd/lib/obj of two checkouts): take the gfx950 code object out of the
host object's .hip_fatbin section and disassemble it; then compare the text of each device function of the two builds BY NAME,
whatever object holds it - a kernel that moved to another unit is still compared with its old self.  Exit status 1 when a function
differs or exists on one side only.  How "the built-in kernels do not change" is checked for a change to the shared headers or to
the split of the units."""
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
    if os.path.getsize(fat) == 0 or TARGET not in subprocess.check_output(
            [os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--input=" + fat, "--list"], text=True).split():
        return {}                                                  # a host unit without a kernel
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co, "--unbundle"])
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^<(.*)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None and line.strip() and line.strip() != "...":       # ("...": the padding behind a function)
            out[name].append(re.sub(r"\s*// [0-9A-F]{12}: ", "  // ", line.strip()))     # (the encoding stays, the address goes: it moves with the unit)
    return out


def union(objdir, tmp):
    """Every device function of every object of `objdir` by name: the objects that hold it (a template kernel instantiated in two
    units has two) and, in the same order, its texts."""
    out = {}
    for f in sorted(os.listdir(objdir)):
        if re.match(r"[A-Za-z0-9_]+\.o$", f):                    # (not the objects of other flag sets: <unit>-<tag>.o)
            for name, text in functions(os.path.join(objdir, f), tmp).items():
                objs, texts = out.setdefault(name, ([], []))
                objs.append(f)
                texts.append(text)
    return out


def main(a, b):
    with tempfile.TemporaryDirectory() as tmp:
        fa, fb = union(a, tmp), union(b, tmp)
    none = ([], [])
    bad = sorted(k for k in set(fa) | set(fb) if sorted(fa.get(k, none)[1]) != sorted(fb.get(k, none)[1]))
    moved = sorted(k for k in set(fa) & set(fb) if fa[k][0] != fb[k][0])
    for k in moved:
        print("moved      %s: %s -> %s" % (k, ", ".join(fa[k][0]), ", ".join(fb[k][0])))
    for k in bad:
        print("DIFFERENT  %s (%s | %s)" % (k, ", ".join(fa.get(k, none)[0]) or "-", ", ".join(fb.get(k, none)[0]) or "-"))
    units = lambda u: len({o for objs, _ in u.values() for o in objs})
    print("%d device functions in %d | %d objects, %d moved, %d differ" % (len(set(fa) | set(fb)), units(fa), units(fb), len(moved), len(bad)))
    return 1 if bad or not fa else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
