#!/usr/bin/env python
"""What does the first product after a value change in HBM cost, with the SELL-64 structure kept and without?

One input per process (--input), a handle over arrays in HBM with the keep_value_maps flag, an mv hint and aoclsparse_optimize:
  laplace-d   the g x g 5-point Laplacian (default g = 4096), double: a table of two, one-byte words, records, a periodic range
  laplace-s   the same in float
  shell       the shell-like stand-in of tools/standins.py with random values, double: PACK 4, shared lists, no table, no records
Wall clock in ms around aoclsparse_mi355_synchronize: aoclsparse_mi355_?revalue_device, then the first ?mv.  One warm-up repeat,
then --repeats (at least 5) timed ones; the median and the range are reported.  Two series of new values:
  x2          the values alternate between v and 2 v (on this commit: the periodic range is carried over, no search)
  two-cell    the values alternate between v and v with one cell changed in one row of two slices (the search runs)
--tree names the checkout whose package and library are measured (default: this one).  A checkout from before
aoclsparse_mi355_get_sell_keep_info rebuilds the copy in that first product: that is (a); this commit's run is (b).  Under
AOCLSPARSE_MI355_TIMING=1 (set here) the library's laps of the stages and the refill kernel's device-event time are collected
from stderr; the refill's bytes (row pointer and values read, cells written) over that time are set against the 6.29 TB/s
device-to-device copy rate.  After the last repeat the product is compared, bit for bit, with a fresh handle's.
The result is appended to --out as one block of text."""
import argparse
import contextlib
import importlib.util
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPY_RATE = 6.29e12  # bytes/s
LAPS = ["sell: structure (with the table pass)", "sell: values (fill, flags, range)", "sell: values (structure kept)",
        "sell kept: table pass", "sell kept: table + cell buffers", "sell kept: refill, flags, compare",
        "sell: periodic range of the records", "sell: refill kernel events"]


class stderr_lines:
    """the library's diagnostic lines (file descriptor 2) of the calls made inside the block"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        self.lines = []
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.lines = self.tmp.read().decode(errors="replace").splitlines()
        self.tmp.close()


def load_package(tree):
    spec = importlib.util.spec_from_file_location("aocl_sparse_amd", os.path.join(tree, "aocl-sparse_amd", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(tree, "aocl-sparse_amd")])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["aocl_sparse_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def fmt(key, ts, unit="ms"):
    return "%-64s median %9.3f %s   range %.3f - %.3f   [%s]" % (key, statistics.median(ts), unit, min(ts), max(ts),
                                                                 ", ".join("%.3f" % t for t in ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", choices=["laplace-d", "laplace-s", "shell"], default="laplace-d")
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--label", default=None, help="what to call the tree in the output (default: its path)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r28", "sell_revalue.txt"))
    a = ap.parse_args()
    assert a.repeats >= 5, "the median of at least 5 runs"
    os.environ["AOCLSPARSE_MI355_TIMING"] = "1"
    import torch

    sys.path.insert(0, os.path.join(HERE, "tools"))
    P = load_package(os.path.abspath(a.tree))
    L = P.lib()
    assert torch.cuda.is_available(), "needs a GPU"
    has_info = hasattr(P.Matrix, "sell_keep_info")
    d = P.Descr()

    def sync():
        assert L.aoclsparse_mi355_synchronize() == 0

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        sync()
        return (time.perf_counter() - t0) * 1e3, r

    if a.input == "shell":
        import standins
        m, rp, ci, _ = standins.shell_like()
        v = np.random.default_rng(28).uniform(-1.0, 1.0, len(ci))
        what = "shell-like stand-in, %d rows, random values" % m
    else:
        rp, ci, v = None, None, None
        m = a.grid * a.grid
        r = np.arange(m, dtype=np.int64)
        i, j = r // a.grid, r % a.grid
        cols = np.stack([r - a.grid, r - 1, r, r + 1, r + a.grid], axis=1)
        ok = np.stack([i > 0, j > 0, np.ones(m, bool), j < a.grid - 1, i < a.grid - 1], axis=1)
        rp = np.zeros(m + 1, np.int64)
        rp[1:] = np.cumsum(ok.sum(axis=1))
        rp, ci = rp.astype(np.int32), cols[ok].astype(np.int32)
        v = np.broadcast_to(np.array([-1.0, -1.0, 4.0, -1.0, -1.0]), (m, 5))[ok]
        del r, i, j, cols, ok
        what = "%d x %d 5-point Laplacian, %d rows" % (a.grid, a.grid, m)
    dtype = np.float32 if a.input == "laplace-s" else np.float64
    v = np.ascontiguousarray(v, dtype=dtype)
    nnz, vsize = len(v), v.dtype.itemsize
    v_two = v.copy()
    for s in (m // 64 // 3, 2 * (m // 64) // 3):  # one cell in one row of two slices takes another value of the input
        e = rp[64 * s + 5] + 1
        v_two[e] = v[rp[64 * s + 5]] if v[e] != v[rp[64 * s + 5]] else v[e + 1]
    t_rp, t_ci = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda()
    vals = {"v": torch.from_numpy(v).cuda(), "x2": torch.from_numpy((2 * v).astype(dtype)).cuda(), "two-cell": torch.from_numpy(v_two).cuda()}
    x = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, m).astype(dtype)).cuda()
    mv = P.dmv if dtype == np.float64 else P.smv
    torch.cuda.synchronize()

    def product(A):
        y = torch.zeros(m, dtype=x.dtype, device="cuda")
        assert mv(P.OP_NONE, 1.0, A, d, x, 0.0, y) == 0
        return y

    def fresh(t_val, flag):
        A = P.Matrix.from_device(0, m, m, nnz, t_rp, t_ci, t_val)
        assert A.status == 0, A.status
        if flag:
            assert A.keep_value_maps() == 0
        assert L.aoclsparse_set_mv_hint(A.h, P.OP_NONE, d.h, 100) == 0 and L.aoclsparse_optimize(A.h) == 0
        product(A)
        sync()
        return A

    lines = ["", "# tools/sell_revalue_timing.py --input %s --repeats %d  tree: %s  (%s)" % (a.input, a.repeats, a.label or a.tree, P.device_info()[3]),
             "# %s, %d entries, %s; wall clock in ms around aoclsparse_mi355_synchronize; one warm-up repeat, then the repeats listed" % (what, nnz, v.dtype)]
    with stderr_lines() as err:
        A = fresh(vals["v"], True)
    for lap in LAPS[:2]:
        q = [w for w in (re.search(r"%s\s+([\d.]+) ms" % re.escape(lap), ln) for ln in err.lines) if w]
        if q:
            lines.append("first build: %-50s %9.3f ms" % (lap, float(q[0].group(1))))
    info = A.spmv_info()
    packing = A.sell_packing()
    lines.append("plan: kernel %d, %d slices, %d stored cells, table %d, packing %s, period %s" % (
        info.kernel, info.sell_slices, info.stored_cells, A.sell_values(), packing, A.sell_period()))
    # what the refill kernel reads and writes: the row pointer and the values; the cells in the plan's encoding
    mpad = (info.sell_slices * 64)
    written = mpad * packing[1] if packing[0] else (info.stored_cells if A.sell_values() else info.stored_cells * vsize)
    refill_bytes = 4.0 * (m + 1) + nnz * vsize + written
    for series in ("x2", "two-cell"):
        tot, rev, first, routes = [], [], [], []
        laps = {k: [] for k in LAPS}
        skipped = 0
        for k in range(a.repeats + 1):
            new = vals[series] if k % 2 == 0 else vals["v"]
            with stderr_lines() as err:
                t0, st = clock(lambda: A.revalue_device(new))
                assert st == 0, st
                t1, y = clock(lambda: product(A))
            if k == 0:
                continue  # warm-up
            tot.append(t0 + t1), rev.append(t0), first.append(t1)
            for lap in LAPS:
                q = [w for w in (re.search(r"%s\s+([\d.]+) ms" % re.escape(lap), ln) for ln in err.lines) if w]
                if q:
                    laps[lap].append(float(q[0].group(1)))
            skipped += any("search skipped" in ln for ln in err.lines)
            if has_info:
                routes.append(A.sell_keep_info().last_route)
        lines.append(fmt("(%s) revalue_device + first mv" % series, tot))
        lines.append(fmt("(%s)     revalue_device" % series, rev))
        lines.append(fmt("(%s)     first mv (the copy is brought up to date here)" % series, first))
        for lap in LAPS:
            if laps[lap]:
                lines.append(fmt("(%s)        lap: %s" % (series, lap), laps[lap]))
        ev = laps["sell: refill kernel events"]
        if ev:
            t = statistics.median(ev)
            lines.append("(%s)        refill kernel: %.1f MB in %.3f ms = %.2f TB/s = %.2f of the %.2f TB/s copy rate" % (
                series, refill_bytes / 1e6, t, refill_bytes / (t * 1e-3) / 1e12, refill_bytes / (t * 1e-3) / COPY_RATE, COPY_RATE / 1e12))
        if has_info:
            lines.append("(%s)     last_route of every repeat: %s; searches skipped in %d of %d" % (series, routes, skipped, a.repeats))
        # the handle holds `new` of the last repeat: a fresh handle over the same values gives the same bits
        T = fresh(new, False)
        assert torch.equal(y.view(torch.int64 if dtype == np.float64 else torch.int32),
                           product(T).view(torch.int64 if dtype == np.float64 else torch.int32)), "differs from a fresh handle"
        T.destroy()
        lines.append("(%s)     the last product equals a fresh handle's, bit for bit" % series)
    if has_info:
        i = A.sell_keep_info()
        lines.append("kept: structure_builds %d, value_fills %d, searches_skipped %d, kept_bytes %d" % (
            i.structure_builds, i.value_fills, i.searches_skipped, i.kept_bytes))
    A.destroy()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
