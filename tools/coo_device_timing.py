#!/usr/bin/env python
"""How long do unordered triplets in HBM take to become a matrix handle?

The g x g 5-point Laplacian (default g = 4096: 16.8 M rows, 83.9 M triplets), its triplets shuffled with a fixed seed and resident
in HBM.  Wall clock around aoclsparse_mi355_synchronize, the minimum of --repeats with the range:
  (a) host route + first dmv     what a caller had before aoclsparse_mi355_create_?csr_from_coo_device: the three arrays copied to
                                 the host, aoclsparse_create_dcoo, aoclsparse_convert_csr (a single-threaded counting sort),
                                 aoclsparse_export_dcsr, aoclsparse_create_dcsr on the exported arrays, the first aoclsparse_dmv
                                 (which uploads them again) -- and its parts
  (b) from_coo_device(keep) + first dmv, and its parts
  (c) from_coo_device(sum) + first dmv on the triplets with every tenth one repeated (8.4 M more)
and, from the library's own events (AOCLSPARSE_MI355_TIMING=1, set here before the library is loaded), the time of the sort's
kernels alone: the radix passes, and what follows them (row counts, gathers / run sums, scans).  A pass reads and writes
8 bytes per entry (key and position); the fraction of the 6.29 TB/s copy rate of the MI355X that this traffic reaches is
printed next to the time.  x and y are device tensors; making and shuffling the triplets is not timed.
Writes the lines to --out and prints them."""
import argparse
import ctypes
import os
import re
import sys
import tempfile
import time
from ctypes import byref, c_int, c_int32, c_void_p

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s: the MI355X's measured device-to-device copy rate


class stderr_lines:
    """the library's diagnostic lines (written to file descriptor 2) of the calls made inside the block"""

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
        for ln in self.lines:
            sys.stderr.write(ln + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true", help="leave (a) out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "coo_device.txt"))
    a = ap.parse_args()
    os.environ["AOCLSPARSE_MI355_TIMING"] = "1"
    import torch

    P = entry.load_package()
    L = P.lib()
    assert torch.cuda.is_available(), "needs a GPU"
    m, rp, ci, v = entry.laplace5(a.grid)
    nnz = len(v)
    rng = np.random.default_rng(19)
    perm = rng.permutation(nnz)
    row = np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))[perm]
    col = ci[perm]
    val = (v * rng.uniform(0.5, 1.5, nnz))[perm]
    # (c): every tenth triplet once more, somewhere else in the arrays
    rep = np.arange(0, nnz, 10)
    perm2 = rng.permutation(nnz + len(rep))
    row2, col2 = np.concatenate([row, row[rep]])[perm2], np.concatenate([col, col[rep]])[perm2]
    val2 = np.concatenate([val, 0.25 * val[rep]])[perm2]
    del perm, perm2
    d = P.Descr()
    x = torch.ones(m, dtype=torch.float64, device="cuda")
    y = torch.zeros(m, dtype=torch.float64, device="cuda")
    trow, tcol, tval = (torch.from_numpy(t).cuda() for t in (row, col, val))
    trow2, tcol2, tval2 = (torch.from_numpy(t).cuda() for t in (row2, col2, val2))
    nnz2 = len(val2)
    del row2, col2, val2
    torch.cuda.synchronize()

    def sync():
        assert L.aoclsparse_mi355_synchronize() == 0

    def dmv(A):
        assert P.dmv(P.OP_NONE, 1.0, A, d, x, 0.0, y) == 0
        sync()

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        return (time.perf_counter() - t0) * 1e3, r

    keys = ["(a) host route + first dmv", "    a: device-to-host copy", "    a: create_dcoo", "    a: convert_csr", "    a: export_dcsr + create_dcsr",
            "    a: first dmv", "(b) from_coo_device(keep) + first dmv", "    b: create alone", "    b: first dmv", "    b: sort kernels (radix passes)",
            "    b: sort kernels (count, gathers, scan)", "(c) from_coo_device(sum) + first dmv", "    c: create alone", "    c: first dmv",
            "    c: sort kernels (radix passes)", "    c: sort kernels (gathers, run sums, scans)"]
    rows = {k: [] for k in keys}
    passes = {}
    y_host = None

    laps = {}

    def sort_events(lines, tag):
        laps[tag] = [ln for ln in lines if "[mi355 timing]" in ln]
        for ln in lines:
            g = re.search(r"coo sort kernels: (\d+) passes\s+([\d.]+) ms, .*?([\d.]+) ms", ln)
            if g:
                passes[tag] = int(g.group(1))
                return float(g.group(2)), float(g.group(3))
        raise AssertionError("no event line from the library")

    for _ in range(a.repeats):
        if not a.skip_host:
            t_copy, (hr, hc, hv) = clock(lambda: tuple(t.cpu().numpy() for t in (trow, tcol, tval)))
            h, c = c_void_p(), c_void_p()
            t_coo, st = clock(lambda: L.aoclsparse_create_dcoo(byref(h), 0, m, m, nnz, P._ptr(hr), P._ptr(hc), P._ptr(hv)))
            assert st == 0
            t_conv, st = clock(lambda: L.aoclsparse_convert_csr(h, P.OP_NONE, byref(c)))
            assert st == 0

            def export_create():
                base, mm, nn, zz = c_int(), c_int32(), c_int32(), c_int32()
                a1, a2, a3 = c_void_p(), c_void_p(), c_void_p()
                assert L.aoclsparse_export_dcsr(c, byref(base), byref(mm), byref(nn), byref(zz), byref(a1), byref(a2), byref(a3)) == 0
                erp = np.ctypeslib.as_array(ctypes.cast(a1, ctypes.POINTER(c_int32)), (m + 1,))
                eci = np.ctypeslib.as_array(ctypes.cast(a2, ctypes.POINTER(c_int32)), (nnz,))
                ev = np.ctypeslib.as_array(ctypes.cast(a3, ctypes.POINTER(ctypes.c_double)), (nnz,))
                A = P.Matrix(0, m, m, erp, eci, ev)  # (aliases the converted handle's arrays: it stays alive until A is gone)
                assert A.status == 0
                return A
            t_exp, A = clock(export_create)
            t_dmv, _ = clock(lambda: dmv(A))
            for k, t in zip(keys[:6], (t_copy + t_coo + t_conv + t_exp + t_dmv, t_copy, t_coo, t_conv, t_exp, t_dmv)):
                rows[k].append(t)
            y_host = y.clone()
            A.destroy()
            L.aoclsparse_destroy(byref(c))
            L.aoclsparse_destroy(byref(h))
            del hr, hc, hv

        with stderr_lines() as err:
            t0, D = clock(lambda: P.Matrix.from_coo_device(0, m, m, nnz, trow, tcol, tval, duplicates=P.COO_KEEP))
        assert D.status == 0
        t1, _ = clock(lambda: dmv(D))
        s0, s1 = sort_events(err.lines, "b")
        for k, t in zip(keys[6:11], (t0 + t1, t0, t1, s0, s1)):
            rows[k].append(t)
        if y_host is not None:
            assert torch.equal(y, y_host), "handle from device triplets: other bits than the host route"
        D.destroy()

        with stderr_lines() as err:
            t0, S = clock(lambda: P.Matrix.from_coo_device(0, m, m, nnz2, trow2, tcol2, tval2, duplicates=P.COO_SUM))
        assert S.status == 0 and S.nnz == nnz, (S.status, S.nnz)
        t1, _ = clock(lambda: dmv(S))
        s0, s1 = sort_events(err.lines, "c")
        for k, t in zip(keys[11:], (t0 + t1, t0, t1, s0, s1)):
            rows[k].append(t)
        S.destroy()

    st, dev_id, cus, name = P.device_info()
    lines = ["# tools/coo_device_timing.py --grid %d --repeats %d  (%s, %d CUs)" % (a.grid, a.repeats, name, cus),
             "# laplace5(%d): m = %d, %d triplets shuffled (seed 19); (c): %d triplets, every tenth repeated" % (a.grid, m, nnz, nnz2),
             "# wall clock in ms around aoclsparse_mi355_synchronize; sort kernels: device events; min of the repeats [all]"]
    for k in keys:
        ts = rows[k]
        if not ts:
            lines.append("%-48s not measured" % k)
            continue
        extra = ""
        if "radix passes" in k:
            tag, n = k.strip()[0], (nnz if k.strip()[0] == "b" else nnz2)
            byts = 16.0 * n * passes[tag]  # every pass: 8 bytes read and 8 bytes written per entry by the scatter
            extra = "   %d passes, %.2f GB of pair traffic: %.1f %% of the 6.29 TB/s copy rate" % (
                passes[tag], byts / 1e9, 100.0 * byts / (min(ts) * 1e-3) / COPY_RATE)
        lines.append("%-48s %10.2f ms   [%s]%s" % (k, min(ts), ", ".join("%.2f" % t for t in ts), extra))
    lines += ["#", "# where a creation goes (AOCLSPARSE_MI355_TIMING=1, the library's own laps of the last repeat: keep, then sum)"]
    lines += ["# " + ln for tag in ("b", "c") for ln in laps.get(tag, [])]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
