#!/usr/bin/env python3
"""Are the kernels of two sets of gfx950 assembly listings the same machine code?

    python tools/isa_identity.py BEFORE.s [...] -- AFTER.s [...] [--may-differ 'sell_fill' ...]

Listings: hipcc $(CXXFLAGS) $(HIPFLAGS) --cuda-device-only -S FILE.hip.  Every kernel whose demangled name contains none of the
--may-differ texts must exist on both sides under the same mangled name, with the same instruction body line for line -- local
labels (.LBB<n>_<k>) carry the function's index in its file and are renumbered -- and the same kernel descriptor and kernel info
(registers, LDS, scratch, kernarg size, occupancy).  Kernels that match a --may-differ text are listed, not compared.  Exit
status 0 when nothing else differs.  Text only: no GPU.
"""
import re
import sys

from isa_waits import demangle, kernels


def normal(body):
    """the body without comments, local labels renumbered in order of appearance"""
    seen, out = {}, []
    for ln in body:
        code = ln.split(";")[0].rstrip()
        if not code.strip():
            continue
        out.append(re.sub(r"\.L[A-Za-z_]+\d+_\d+", lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), code))
    return out


def load(paths):
    ks = {}
    for p in paths:
        ks.update(kernels(open(p).read()))
    return ks


def main(argv):
    sides, loose, cur = [[], []], [], 0
    args = iter(argv[1:])
    for a in args:
        if a == "--":
            cur = 1
        elif a == "--may-differ":
            loose.append(next(args))
        else:
            sides[cur].append(a)
    if not sides[0] or not sides[1]:
        print(__doc__)
        return 2
    before, after = load(sides[0]), load(sides[1])
    pretty = demangle(sorted(set(before) | set(after)))
    is_loose = lambda n: any(t in pretty[n] for t in loose)
    a, b = set(n for n in before if not is_loose(n)), set(n for n in after if not is_loose(n))
    bad = ["only before: " + pretty[n] for n in sorted(a - b)] + ["only after: " + pretty[n] for n in sorted(b - a)]
    same = 0
    for n in sorted(a & b):
        if normal(before[n][0]) != normal(after[n][0]):
            bad.append("body differs: " + pretty[n])
        elif before[n][1] != after[n][1]:
            bad.append("descriptor differs: " + pretty[n])
        else:
            same += 1
    print("kernels before: %d, after: %d" % (len(before), len(after)))
    print("compared (same mangled name on both sides): %d, identical in body and descriptor: %d" % (len(a & b), same))
    for ln in bad:
        print("DIFFERENT  " + ln)
    for side, ks in (("before", before), ("after", after)):
        free = sorted(pretty[n] for n in ks if is_loose(n))
        print("not compared, %s (%d):" % (side, len(free)))
        for n in free:
            print("  " + n)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
