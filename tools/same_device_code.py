#!/usr/bin/env python3
"""Per-kernel comparison of gfx950 device assembly, for tools/same_device_code.sh --per-kernel (kernels that moved between files).

usage: same_device_code.py OLD.s [OLD.s ...] -- NEW.s [NEW.s ...]

Every file is cut into functions, from `-- Begin function` to `-- End function`: the instructions and, for a kernel, its
.amdhsa_kernel descriptor.  Comments go, and the number that the compiler gives a function inside its translation unit
(.LBB<n>_, .Lfunc_end<n>, .Ltmp<n>) becomes a constant: it changes when a function's neighbours change, nothing else does.
Prints one line per symbol -- identical / DIFFERS / only old / only new -- and exits 0 only when both sides have the same
symbols and every one is identical."""
import re
import sys

BEGIN = re.compile(r"-- Begin function (\S+)")
END = re.compile(r"-- End function")
LOCAL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp)\d+")


def functions(path):
    """{symbol: normalised lines} of one assembly file"""
    out, name, body = {}, None, []
    for line in open(path, encoding="utf-8", errors="replace"):
        m = BEGIN.search(line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if END.search(line):
            assert name not in out, f"{path}: {name} twice"
            out[name], name = body, None
            continue
        text = LOCAL.sub(r".\g<1>N", line.split(";", 1)[0]).strip()
        if text:
            body.append(text)
    assert name is None, f"{path}: {name} has no end"
    return out


def side(paths):
    merged = {}
    for p in paths:
        for sym, body in functions(p).items():
            assert sym not in merged, f"{sym} in two files of one side"
            merged[sym] = body
    return merged


def main(argv):
    if "--" not in argv:
        sys.exit(__doc__)
    cut = argv.index("--")
    old, new = side(argv[:cut]), side(argv[cut + 1:])
    bad = nkernels = 0
    for sym in sorted(set(old) | set(new)):
        if sym not in new:
            verdict = "only old"
        elif sym not in old:
            verdict = "only new"
        else:
            verdict = "identical" if old[sym] == new[sym] else "DIFFERS"
        bad += verdict != "identical"
        body = new.get(sym, old.get(sym))
        kernel = any(line.startswith(".amdhsa_kernel ") for line in body)
        nkernels += kernel
        print(f"{verdict:9s} {sym}  ({len(body)} lines{', kernel' if kernel else ''})")
    print(f"{len(old)} symbols old, {len(new)} new ({nkernels} kernels in all), {bad} not identical")
    return 1 if bad or not old else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
