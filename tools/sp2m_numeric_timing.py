#!/usr/bin/env python
"""What does a time step cost whose matrix product C = A * A gets new values on a fixed pattern: with
aoclsparse_sp2m(stage_finalize) into C, and with aoclsparse_mi355_sp2m_numeric_device?

One input per process (--input), double:
  laplace     A = the g x g 5-point Laplacian (default g = 2048): C has 54.5 M entries
  shell       A = the shell-like stand-in of tools/standins.py with random values
A is a host-created handle; C is the result handle of a full computation, resident, with the keep_value_maps flag and the clean
CSR of aoclsparse_mi355_clean_csr_device, and has done one dmv and one lower dtrsv.  A step is:
aoclsparse_mi355_drevalue_device(A) with other values, the product again into C, then the next dmv and lower dtrsv with C.
Wall clock in ms around aoclsparse_mi355_synchronize, every part and their sum; one warm-up step,
then --repeats (at least 5) timed ones; the median and the range are reported.  The values alternate between two independent draws.
--tree names the checkout whose package and library are measured (default: this one).  A checkout from before
aoclsparse_mi355_sp2m_numeric_device takes the finalize route: that is (a); this commit's run is (b).  --route finalize measures
(a) on this commit too.  Under AOCLSPARSE_MI355_TIMING=1 (set here) the library's laps of the numeric call and of the commit, and
the numeric kernels' device-event time, are collected from stderr.  --fill-trace instead runs one finalize call under
AOCLSPARSE_MI355_SP2M_TRACE=1 and reports the library's phases of it: the fill pass's kernels next to the numeric kernels'.
After the last repeat C is compared, bit for bit, with a fresh full computation.  The result is appended to --out as one block of
text.  The tool sets no time limit of its own: the caller wraps every process in `timeout`, one per (tree, input), and starts the
next only when the one before ended well.
Without aoclsparse_mi355_clean_csr_device C's clean CSR would be the copy the first solve builds on the host, which records no
value map: the commit then drops C's TRSV plans on either route and the step is the solve's analysis."""
import argparse
import contextlib
import ctypes
import os
import re
import statistics
import sys
import time
from ctypes import byref, c_int, c_void_p

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from sell_revalue_timing import fmt, load_package, stderr_lines  # noqa: E402

LAPS = ["sp2m_numeric: operands + mirror", "sp2m_numeric: plan build", "sp2m_numeric: kernel events",
        "sp2m_numeric: kernels + verdict", "sp2m_numeric: commit", "revalue_device: values to host view + mirror",
        "revalue_device: clean gather + copy back", "revalue_device: diagonal + plan gathers"]


def laplacian(g):
    m = g * g
    r = np.arange(m, dtype=np.int64)
    i, j = r // g, r % g
    cols = np.stack([r - g, r - 1, r, r + 1, r + g], axis=1)
    ok = np.stack([i > 0, j > 0, np.ones(m, bool), j < g - 1, i < g - 1], axis=1)
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum(ok.sum(axis=1))
    k = np.broadcast_to(np.arange(5), (m, 5))[ok]
    return m, rp.astype(np.int32), cols[ok].astype(np.int32), k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", choices=["laplace", "shell"], default="laplace")
    ap.add_argument("--grid", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--label", default=None, help="what to call the tree in the output (default: its path)")
    ap.add_argument("--route", choices=["auto", "finalize", "numeric"], default="auto")
    ap.add_argument("--fill-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r29", "sp2m_numeric.txt"))
    a = ap.parse_args()
    assert a.repeats >= 5, "the median of at least 5 runs"
    os.environ["AOCLSPARSE_MI355_TIMING"] = "1"
    if a.fill_trace:
        os.environ["AOCLSPARSE_MI355_SP2M_TRACE"] = "1"
    import torch

    P = load_package(os.path.abspath(a.tree))
    L = P.lib()
    assert torch.cuda.is_available(), "needs a GPU"
    has_numeric = "aoclsparse_mi355_sp2m_numeric_device" in P.SIGNATURES
    route = ("numeric" if has_numeric else "finalize") if a.route == "auto" else a.route
    assert route == "finalize" or has_numeric, "this tree has no numeric entry point"
    d = P.Descr()
    dl = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=P.FILL_LOWER)
    N = P.OP_NONE

    def sync():
        assert L.aoclsparse_mi355_synchronize() == 0

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        sync()
        return (time.perf_counter() - t0) * 1e3, r

    rng = np.random.default_rng(29)
    if a.input == "shell":
        import standins
        m, rp, ci, _ = standins.shell_like()
        vals = [rng.uniform(-1.0, 1.0, len(ci)) for _ in range(2)]
        what = "A = the shell-like stand-in, %d rows, random values" % m
    else:
        m, rp, ci, k = laplacian(a.grid)
        vals = [np.where(k == 2, 4.0, -1.0) * (1.0 + rng.uniform(0.0, 0.25, len(ci))) for _ in range(2)]
        what = "A = the %d x %d 5-point Laplacian, %d rows, values (4, -1) x (1 + e), e drawn in [0, 0.25)" % (a.grid, a.grid, m)
    dvals = [torch.from_numpy(v).cuda() for v in vals]
    x = torch.from_numpy(rng.uniform(-1, 1, m)).cuda()
    torch.cuda.synchronize()

    def full(A):
        h = c_void_p()
        st = L.aoclsparse_sp2m(N, d.h, A.h, N, d.h, A.h, P.STAGE_FULL, byref(h))
        assert st == 0, P.STATUS[st]
        return h

    hip = ctypes.CDLL(P.hip_runtime_path()[1])
    hip.hipMemcpy.argtypes = [c_void_p, c_void_p, ctypes.c_size_t, ctypes.c_int]

    def view(h):
        """(nnz, row_ptr, col_ind, val) of the handle's arrays as they stand in HBM (aoclsparse_mi355_export_csr_device: the
        handle's own CSR; aoclsparse_export_?csr shows the clean copy once a solve has made one), copied to the host"""
        base, mm, nn, nnz = c_int(), c_int(), c_int(), c_int()
        p, i, v = c_void_p(), c_void_p(), c_void_p()
        st = L.aoclsparse_mi355_export_csr_device(h, byref(base), byref(mm), byref(nn), byref(nnz), byref(p), byref(i), byref(v))
        assert st == 0, P.STATUS[st]
        out = [nnz.value]
        for q, n, dt in ((p, mm.value + 1, np.int32), (i, nnz.value, np.int32), (v, nnz.value, np.int64)):
            host = np.zeros(max(n, 1), dt)
            assert hip.hipMemcpy(P._ptr(host), q, n * host.itemsize, 2) == 0  # hipMemcpyDeviceToHost
            out.append(host[:n])
        return out

    A = P.Matrix(0, m, m, rp, ci, vals[0].copy())
    assert A.status == 0
    lines = ["", "# tools/sp2m_numeric_timing.py --input %s --repeats %d%s  tree: %s  route: %s  (%s)" % (
        a.input, a.repeats, " --fill-trace" if a.fill_trace else "", a.label or a.tree, "finalize, traced" if a.fill_trace else route,
        P.device_info()[3])]
    with stderr_lines() as err:
        t_full, hC = clock(lambda: full(A))
    nz = c_int()
    assert L.aoclsparse_export_dcsr(hC, byref(c_int()), byref(c_int()), byref(c_int()), byref(nz), byref(c_void_p()), byref(c_void_p()),
                                    byref(c_void_p())) == 0
    nnz_c = nz.value
    lines.append("# %s, %d entries; C = A A: %d entries; full computation %.1f ms" % (what, len(ci), nnz_c, t_full))
    if a.fill_trace:
        with stderr_lines() as err:
            for _ in range(2):  # (the second call: warm staging slots)
                st = L.aoclsparse_sp2m(N, d.h, A.h, N, d.h, A.h, P.STAGE_FINALIZE, byref(hC))
                assert st == 0, P.STATUS[st]
        seen = [ln for ln in err.lines if ln.startswith("sp2m ")]
        lines += ["finalize, phases of the second call (each synchronised: AOCLSPARSE_MI355_SP2M_TRACE):"] + [
            "    " + ln for ln in seen[len(seen) // 2:]]
    else:
        C = P.Matrix.__new__(P.Matrix)  # (a wrapper without from_handle's copies of the arrays)
        C.h, C.double, C.status, C.row_ptr, C.col_ind, C.val = hC, True, 0, None, None, None
        C.m, C.n, C.nnz, C.base = m, m, nnz_c, 0
        # the flag, and the clean CSR built in HBM: it records the value maps that carry it and the TRSV plans through a commit
        assert C.keep_value_maps() == 0 and C.clean_device() == 0

        def after(C):
            y, z = torch.zeros(m, dtype=torch.float64, device="cuda"), torch.zeros(m, dtype=torch.float64, device="cuda")
            t_mv, st = clock(lambda: P.dmv(N, 1.0, C, d, x, 0.0, y))
            assert st == 0, P.STATUS[st]
            t_sv, st = clock(lambda: P.dtrsv(N, 1.0, C, dl, x, z))
            assert st == 0, P.STATUS[st]
            return t_mv, t_sv

        t_mv, t_sv = after(C)
        lines.append("first dmv %.1f ms, first lower dtrsv %.1f ms (analysis included)" % (t_mv, t_sv))

        def product():
            if route == "numeric":
                return L.aoclsparse_mi355_sp2m_numeric_device(N, d.h, A.h, N, d.h, A.h, C.h)
            return L.aoclsparse_sp2m(N, d.h, A.h, N, d.h, A.h, P.STAGE_FINALIZE, byref(C.h))

        parts = {k: [] for k in ("step", "revalue_device(A)", "product", "next dmv", "next dtrsv")}
        laps = {k: [] for k in LAPS}
        first_laps = {}
        for k in range(a.repeats + 1):
            new = dvals[(k + 1) % 2]
            t0, st = clock(lambda: A.revalue_device(new))
            assert st == 0, P.STATUS[st]
            with stderr_lines() as err:
                t1, st = clock(product)
            assert st == 0, P.STATUS[st]
            t2, t3 = after(C)
            found = {}
            for lap in LAPS:
                q = [w for w in (re.search(r"%s\s+([\d.]+) ms" % re.escape(lap), ln) for ln in err.lines) if w]
                if q:
                    found[lap] = float(q[-1].group(1))
            if k == 0:
                first_laps = found
                continue  # warm-up
            for name, t in zip(parts, (t0 + t1 + t2 + t3, t0, t1, t2, t3)):
                parts[name].append(t)
            for lap, t in found.items():
                laps[lap].append(t)
        tag = "(a)" if route == "finalize" else "(b)"
        for name, ts in parts.items():
            lines.append(fmt("%s %s%s" % (tag, "" if name == "step" else "    ", name), ts))
        if "sp2m_numeric: plan build" in first_laps:
            lines.append("%s         first call only: plan build %.3f ms" % (tag, first_laps["sp2m_numeric: plan build"]))
        for lap, ts in laps.items():
            if ts:
                lines.append(fmt("%s         lap: %s" % (tag, lap), ts))
        if has_numeric:
            i = C.sp2m_plan_info()
            lines.append("plan: kept %d, rows per bin %s, builds %d, numeric runs %d, refused %d, %d bytes" % (
                i.kept, list(i.rows_in_bin), i.plan_builds, i.numeric_runs, i.refused, i.plan_bytes))
        vm = C.value_map_info()
        lines.append("C: TRSV plan builds %d, clean builds %d since creation" % (vm.plan_builds, vm.clean_builds))
        # C holds the product of `new` of the last repeat: a fresh full computation over the same values gives the same bits
        T = P.Matrix(0, m, m, rp, ci, vals[(a.repeats + 1) % 2].copy())
        hT = full(T)
        for got, want in zip(view(C.h), view(hT)):
            assert np.array_equal(got, want), "C differs from a fresh full computation"
        L.aoclsparse_destroy(byref(hT))
        lines.append("C equals a fresh full computation bit for bit (row_ptr, col_ind, val in HBM)")
        C.destroy()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
