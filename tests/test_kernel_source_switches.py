"""CPU: the product sources under lammps-ani_amd/csrc carry no compile-time experiment switches.

The rule: experiments are built from a branch or a tool, not switched inside product sources.  A conditional in csrc may name
an include guard, the compiler's own __HIPCC__, the build option ANI_NO_ROCTX (Makefile) or one of the three stamp switches of
the measurement builds (tools/bwd_stamps.py, tools/mlpf_stamps.py, behind the exported ani_debug_fused_stamps) -- nothing else.
A timing ablation, an alternative that was measured slower or a numeric `#ifndef X / #define X n` knob fails this test: the
finding goes into a comment at the code it informs, the value into a constexpr."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lammps-ani_amd", "csrc")

ALLOWED = {
    "PAIR_CLASS", "LMP_PAIR_ANI_HIP_H",                 # pair_ani.h: the LAMMPS style registration and its include guard
    "__HIPCC__",                                        # ani_fused_ring.h: host + device header
    "ANI_NO_ROCTX",                                     # Makefile option: build without the profiler SDK
    "ABLB_STAMPS", "ABLB_STAMPS_VM", "ABLF_STAMPS",     # stamp instrumentation of the measurement builds
}
DIRECTIVE = re.compile(r"^\s*#\s*(ifdef|ifndef|if|elif)\b(.*)$")


def conditionals():
    """(file, line number, directive, macros it names) of every #if / #ifdef / #ifndef / #elif line of csrc/*.{hip,h,cpp}"""
    out = []
    files = sorted(f for ext in ("hip", "h", "cpp") for f in glob.glob(os.path.join(CSRC, "*." + ext)))
    assert len(files) >= 20, files
    for path in files:
        for no, line in enumerate(open(path, encoding="utf-8"), 1):
            m = DIRECTIVE.match(line)
            if not m:
                continue
            expr = re.sub(r"//.*|/\*.*?\*/", "", m.group(2))
            names = set(re.findall(r"[A-Za-z_]\w*", expr)) - {"defined"}
            if m.group(1) in ("ifdef", "ifndef"):
                names = set(expr.split()[:1])
            out.append((os.path.basename(path), no, line.strip(), names))
    return out


def test_conditionals_name_only_allowed_macros():
    """Experiments are built from a branch or a tool, not switched inside product sources: every preprocessor conditional of
    csrc names allow-listed macros only."""
    found = conditionals()
    assert len(found) >= 8     # the guards, the roctx option and the stamp sites are there: the scan sees the sources
    bad = [f"{f}:{no}: {text}" for f, no, text, names in found if not names or not names <= ALLOWED]
    assert not bad, "experiment switches in product sources (build experiments from a branch or a tool):\n" + "\n".join(bad)
    assert {n for _, _, _, names in found for n in names} == ALLOWED   # an entry nothing uses any more leaves the list
