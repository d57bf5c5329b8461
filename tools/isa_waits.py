#!/usr/bin/env python3
"""The memory skeleton of one kernel in a gfx950 assembly listing (hipcc --save-temps: *-hip-amdgcn-*.s).

    python tools/isa_waits.py FILE.s 'sell_mv_short_kernel<double, 5, 4, 2, false, 2>' [more names ...]

For every kernel whose DEMANGLED name contains the given text: its scalar loads, vector (global / flat / buffer / scratch)
loads and stores, LDS accesses, barriers, branches, labels and waits in program order -- runs of the same kind of
instruction folded into one line with a count -- followed by the integer-division markers (v_rcp_* / v_cvt_f32_u32), the
register counts, scratch, LDS and occupancy from the kernel's metadata.  It reads text only: no GPU, no network; names are
demangled with c++filt or llvm-cxxfilt when one is on PATH (else the mangled name is matched).
"""
import re
import shutil
import subprocess
import sys


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin")
    if not tool or not names:
        return dict((n, n) for n in names)
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, out)) if len(out) == len(names) else dict((n, n) for n in names)


def kernels(text):
    """{mangled name: (body lines, metadata dict)} of every .amdhsa_kernel in the listing"""
    lines = text.splitlines()
    start = {}
    for k, ln in enumerate(lines):
        m = re.match(r"^([A-Za-z_$][\w$.]*):\s*(;.*)?$", ln)
        if m and not m.group(1).startswith(".L"):
            start[m.group(1)] = k
    out = {}
    for k, ln in enumerate(lines):
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m or m.group(1) not in start:
            continue
        name, meta, end = m.group(1), {}, k
        for j in range(k, len(lines)):
            if ".end_amdhsa_kernel" in lines[j]:
                end = j
                break
            mm = re.match(r"^\s*\.(amdhsa_\w+)\s+(\S+)", lines[j])
            if mm:
                meta[mm.group(1)] = mm.group(2)
        # the "; Kernel info:" comments behind the descriptor (NumVgprs, ScratchSize, Occupancy, ...)
        for cl in lines[end:end + 80]:
            if ".amdhsa_kernel" in cl:
                break
            mm = re.match(r"^\s*;\s*(NumVgprs|NumAgprs|NumSgprs|ScratchSize|Occupancy|LDSByteSize|TotalNumVgprs|codeLenInByte):?\s*(\d+)", cl)
            if mm:
                meta[mm.group(1)] = mm.group(2)
        body = []
        for bl in lines[start[name] + 1:]:
            if re.match(r"^\s*\.(section|size)\b", bl) or ".Lfunc_end" in bl:
                break
            body.append(bl)
        out[name] = (body, meta)
    return out


KINDS = [
    ("scalar load", r"^s_(buffer_)?load_"),
    ("vector load", r"^(global|flat|buffer|scratch)_load_"),
    ("vector store", r"^(global|flat|buffer|scratch)_store_"),
    ("vector atomic", r"^(global|flat|buffer)_atomic_"),
    ("lds write", r"^ds_(write|store)"),
    ("lds read", r"^ds_(read|load)"),
    ("barrier", r"^s_barrier"),
    ("wait", r"^s_waitcnt"),
    ("branch", r"^s_c?branch"),
    ("end", r"^s_endpgm"),
]


def skeleton(body):
    events = []  # (kind, text)
    division = 0
    for ln in body:
        code = ln.split(";")[0].strip()
        if not code:
            continue
        lab = re.match(r"^(\.L\w+):", code)
        if lab:
            events.append(("label", lab.group(1)))
            continue
        op = code.split()[0]
        if re.match(r"^v_(rcp_|cvt_f32_u32)", op):
            division += 1
        for kind, pat in KINDS:
            if re.match(pat, op):
                if kind in ("wait", "branch"):
                    events.append((kind, code))
                else:
                    events.append((kind, op))
                break
    folded = []
    for kind, txt in events:
        if folded and folded[-1][0] == kind and kind not in ("wait", "branch", "label", "barrier", "end"):
            folded[-1][1].append(txt)
        else:
            folded.append((kind, [txt]))
    return folded, division


def report(name, pretty, body, meta):
    folded, division = skeleton(body)
    print("== %s" % pretty)
    if pretty != name:
        print("   (%s)" % name)
    for kind, txts in folded:
        if kind in ("wait", "branch", "label", "barrier", "end"):
            print("  %-13s %s" % (kind, txts[0]))
        else:
            ops = {}
            for t in txts:
                ops[t] = ops.get(t, 0) + 1
            print("  %-13s %3d   %s" % (kind, len(txts), ", ".join("%s x%d" % kv for kv in ops.items())))
    counts = {}
    for kind, txts in folded:
        counts[kind] = counts.get(kind, 0) + len(txts)
    print("  -- totals: " + ", ".join("%s %d" % (k, counts[k]) for k in sorted(counts) if k not in ("label", "end")))
    print("  -- integer-division markers (v_rcp_* / v_cvt_f32_u32): %d" % division)
    keys = ["NumVgprs", "NumAgprs", "TotalNumVgprs", "NumSgprs", "ScratchSize", "LDSByteSize", "Occupancy", "codeLenInByte"]
    print("  -- " + ", ".join("%s %s" % (k, meta[k]) for k in keys if k in meta))
    if "amdhsa_next_free_vgpr" in meta:
        print("  -- .amdhsa_next_free_vgpr %s, .amdhsa_private_segment_fixed_size %s, .amdhsa_group_segment_fixed_size %s" % (
            meta.get("amdhsa_next_free_vgpr"), meta.get("amdhsa_private_segment_fixed_size", "?"),
            meta.get("amdhsa_group_segment_fixed_size", "?")))
    print()


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    ks = kernels(open(argv[1]).read())
    pretty = demangle(list(ks))
    found = 0
    for want in argv[2:]:
        for name in sorted(ks, key=lambda n: pretty[n]):
            if want in pretty[name] or want in name:
                report(name, pretty[name], *ks[name])
                found += 1
    if not found:
        print("no kernel matches; the listing has:", file=sys.stderr)
        for n in sorted(pretty.values()):
            print("  " + n, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
