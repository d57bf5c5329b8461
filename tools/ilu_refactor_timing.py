#!/usr/bin/env python
"""What does the ILU(0) factorisation of a handle cost again after a value change -- and from which row length on does the
binary search for the updated position beat the scan?

Inputs, double precision, base 0, made diagonally dominant (off-diagonals in +-[0.8, 1.2], diagonal = sum |off-diagonals| + 1):
  shell      the shell-like stand-in at a tenth of its full size (tools/standins.py: shell_like(n=150000), ~35 entries per row)
  laplace    the 1000 x 1000 5-point Laplacian (1 M rows)
  band<k>    banded matrices of --band-rows rows with half-bandwidth k / 2: about 20, 40, 80 and 140 entries per row
Per input, the median of --repeats runs after one warm-up, with the spread (max - min) / median:
  baseline   (--baseline: runs on the commit BEFORE ?ilu0_refactor_device existed, and on this one) a fresh handle's first
             aoclsparse_dilu_smoother: the library's phase "ilu: factorise on the GPU" (AOCLSPARSE_MI355_TIMING=1: the host loop over
             the rows for the levels, the upload of the level order and of the values, the factorisation, the download), and the wall
             clock of what a caller without the refactorisation pays per value change: destroy + create + that first smoother call
  scan       aoclsparse_mi355_dilu0_refactor_device after aoclsparse_mi355_dupdate_values_device, option ilu_search = 0: wall clock
  search     the same with option ilu_search = 1
The factor of the last scan run and of the last search run are compared bit for bit.  --parent reads the --baseline output of the
parent commit and puts it next to this commit's columns."""
import argparse
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as entry  # noqa: E402
from clean_device_timing import stderr_lines  # noqa: E402

PHASE = "ilu: factorise on the GPU"


def dominant(m, rp, ci, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.8, 1.2, len(ci)) * rng.choice([-1.0, 1.0], len(ci))
    dg = ci == np.repeat(np.arange(m, dtype=np.int64), np.diff(rp))
    v[dg] = 0
    v[dg] = np.add.reduceat(np.abs(v), rp[:-1]) + 1.0
    return v


def banded(m, hb):
    i = np.arange(m, dtype=np.int64)
    lo, hi = np.maximum(0, i - hb), np.minimum(m, i + hb + 1)
    rp = np.concatenate([[0], np.cumsum(hi - lo)])
    ci = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)])
    return rp.astype(np.int32), ci.astype(np.int32)


def inputs(names, band_rows):
    import standins

    for name in names:
        if name == "shell":
            m, rp, ci, _ = standins.shell_like(n=150000)
        elif name == "laplace":
            m, rp, ci, _ = entry.laplace5(1000)
        else:
            m = band_rows
            rp, ci = banded(m, int(name[4:]) // 2)
        rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
        yield name, m, rp, ci, dominant(m, rp, ci, 5)


def stats(ts):
    med = float(np.median(ts))
    return med, (max(ts) - min(ts)) / med


def cell(ts):
    med, spread = stats(ts)
    return "%9.2f ms +-%4.1f%%" % (med, 100 * spread)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="shell,laplace,band20,band40,band80,band140")
    ap.add_argument("--band-rows", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline", action="store_true", help="the smoother's first factorisation alone: runs on the parent commit too")
    ap.add_argument("--parent", default=None, help="the --baseline output of the parent commit")
    ap.add_argument("--out", default=None, help="default: profiles/r26/ilu_refactor.txt, with --baseline ilu_refactor_baseline.txt")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r26", "ilu_refactor_baseline.txt" if a.baseline else "ilu_refactor.txt")
    os.environ["AOCLSPARSE_MI355_TIMING"] = "1"
    import ctypes

    import torch

    P = entry.load_package()
    L = P.lib()
    assert torch.cuda.is_available(), "needs a GPU"
    d = P.Descr()
    out = []

    def say(line):
        print(line, flush=True)
        out.append(line)

    def smoother(A, b):
        pv, x = ctypes.c_void_p(), np.zeros(A.m)
        assert L.aoclsparse_dilu_smoother(P.OP_NONE, A.h, d.h, ctypes.byref(pv), None, P._ptr(x), P._ptr(b)) == 0
        return pv.value

    def factor(A, address):
        return np.ctypeslib.as_array(ctypes.cast(ctypes.c_void_p(address), ctypes.POINTER(ctypes.c_double)), (A.nnz,)).copy()

    parent = {}
    if a.parent:
        for ln in open(a.parent):
            mt = re.match(r"^baseline (\S+)\s+phase\s+([\d.]+) ms \+-\s*([\d.]+)%\s+recreate\s+([\d.]+) ms \+-\s*([\d.]+)%", ln)
            if mt:
                parent[mt.group(1)] = [float(g) for g in mt.groups()[1:]]
    say("# %s, %d repeats after one warm-up: median +- (max - min) / median" % (torch.cuda.get_device_name(0), a.repeats))
    for name, m, rp, ci, v in inputs(a.inputs.split(","), a.band_rows):
        b = np.random.default_rng(7).uniform(-1, 1, m)
        vals = [v, np.ascontiguousarray(v * np.random.default_rng(6).uniform(0.8, 1.2, len(v)))]
        if a.baseline:
            phase, wall, A = [], [], None
            for r in range(a.repeats + 1):
                t0 = time.perf_counter()
                A = None  # (destroys the previous handle)
                with stderr_lines() as err:
                    A = P.Matrix(0, m, m, rp, ci, vals[r & 1].copy())
                    smoother(A, b)
                t1 = time.perf_counter()
                ms = [float(ln.split()[-2]) for ln in err.lines if PHASE in ln]
                assert len(ms) == 1, err.lines
                if r:
                    phase.append(ms[0]), wall.append(1e3 * (t1 - t0))
            say("baseline %-8s phase %s   recreate %s   (%d rows, %d entries)" % (name, cell(phase), cell(wall), m, len(v)))
            continue
        row, facs = {}, {}
        for opt, key in ((0, "scan"), (1, "search")):
            assert L.aoclsparse_mi355_set_option(P.OPTION_ILU_SEARCH, opt) == 0
            A = P.Matrix(0, m, m, rp, ci, vals[0].copy())
            with stderr_lines():
                address = smoother(A, b)
            assert L.aoclsparse_mi355_set_option(P.OPTION_ILU_SEARCH, -1) == 0
            dv = [torch.from_numpy(w).cuda() for w in vals]
            ts = []
            for r in range(a.repeats + 1):
                assert A.update_values_device(dv[(r + 1) & 1]) == 0
                torch.cuda.synchronize()
                with stderr_lines():
                    t0 = time.perf_counter()
                    st, _ = A.ilu0_refactor_device()
                    t1 = time.perf_counter()
                assert st == 0, P.STATUS.get(st, st)
                if r:
                    ts.append(1e3 * (t1 - t0))
            info = A.ilu_info()
            assert info.search == opt and info.analyses == 1, (info.search, info.analyses)
            row[key], facs[key] = ts, factor(A, address)
        assert facs["scan"].tobytes() == facs["search"].tobytes(), name
        (ms, ss), (mq, sq) = stats(row["scan"]), stats(row["search"])
        line = "%-8s rows %8d  max_row %4d  levels %7d  %s  scan %s  search %s  search/scan %.3f" % (
            name, m, info.max_row, info.levels, "sync-free" if info.syncfree else "per level", cell(row["scan"]), cell(row["search"]),
            mq / ms)
        if name in parent:
            p = parent[name]
            line += "  | parent: phase %9.2f ms +-%4.1f%% (scan/phase %.3f)  destroy+create+smoother %9.2f ms +-%4.1f%% (scan/that %.3f)" % (
                p[0], p[1], ms / p[0], p[2], p[3], ms / p[2])
        say(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
