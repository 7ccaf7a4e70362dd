"""The compile-time switches of the native sources: besides the header guard, only the three instrumented builds
(MI_PROF_BACKWARD, MI_PROF_BACKWARD_LIGHT, MI_PROF_NEWTON), and each of those is used by a tool.  An A/B variant that has been
measured leaves the source; its numbers belong to DESIGN.md, docs/ and profiles/.  CPU only."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE_DIRS = (os.path.join(ROOT, "drake_ddp_amd", "csrc"), os.path.join(ROOT, "include"))
TOOLS = os.path.join(ROOT, "tools")
PROFILING = {"MI_PROF_NEWTON", "MI_PROF_BACKWARD", "MI_PROF_BACKWARD_LIGHT"}


def _texts(top):
    for d, _, names in os.walk(top):
        for f in names:
            path = os.path.join(d, f)
            with open(path, errors="replace") as fh:
                yield os.path.relpath(path, ROOT), fh.read()


def test_sources_test_only_the_header_guard_and_the_profiling_switches():
    found = {}                                                   # MI_* name -> files whose preprocessor conditionals test it
    for top in SOURCE_DIRS:
        for rel, text in _texts(top):
            for line in re.sub(r"\\\n", " ", text).splitlines():   # (a continued directive is one line)
                if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                    for name in re.findall(r"\bMI_[A-Za-z0-9_]+", line):
                        found.setdefault(name, set()).add(rel)
    allowed = {"MI_ILQR_H"} | PROFILING
    extra = {k: sorted(v) for k, v in found.items() if k not in allowed}
    assert not extra, "compile-time switches beyond the instrumented builds: %r" % extra
    assert set(found) == allowed, "no longer tested anywhere: %r" % sorted(allowed - set(found))
    tools = [text for _, text in _texts(TOOLS)]
    for name in sorted(PROFILING):
        # (as -DNAME or bare; not as the prefix of a longer name)
        assert any(re.search(r"%s(?![A-Za-z0-9_])" % name, t) for t in tools), "%s: no file under tools/ names it" % name
