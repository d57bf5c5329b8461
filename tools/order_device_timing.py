#!/usr/bin/env python
"""What does it cost to put the rows of a CSR handle that lives in HBM into column order?

Two inputs, both resident before anything is timed:
  shuffled   the g x g 5-point Laplacian (default g = 4096: 16.8 M rows, 83.9 M entries) with the entries of every row shuffled by a
             fixed seed, created with aoclsparse_mi355_create_dcsr_device
  sp2m       the result of aoclsparse_sp2m of the g/2 x g/2 Laplacian with itself, whose rows are in first-touch order
Wall clock around aoclsparse_mi355_synchronize, the minimum of --repeats with the range; every repeat starts from a fresh unsorted
handle that has run one dmv (making it is not timed):
  (a) aoclsparse_order_mat + next dmv               the host route: a single-threaded std::stable_sort per row over the host view,
                                                    then the next product uploads all three arrays again
  (b) aoclsparse_mi355_order_mat_device + next dmv  the rows sorted in HBM, one copy back into the host view, the product uploads
                                                    nothing.  The sort kernels' own time from the library's events and the copy
                                                    back from its lap timer (AOCLSPARSE_MI355_TIMING=1, set here before the library
                                                    is loaded), the kernels' bytes / time as a fraction of the 6.29 TB/s copy rate.
                                                    The bytes: the flag pass reads every column (4 per entry) and 4 per row of
                                                    row_ptr and writes 4 per row; the lane-per-row sort reads 8 per row and reads
                                                    and writes the 12 bytes of every entry of a row it sorts.
--only-a measures (a) alone and needs nothing newer than create_dcsr_device: run on the commit before order_mat_device existed, its
output is what --parent-a reads to put (a) of that commit, and the ratio (a) / (b) against it, next to this commit's.
Both routes must leave the same arrays: the device arrays of (b) are compared with the host export of (a) once per input."""
import argparse
import ctypes
import os
import re
import sys
import tempfile
import time

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


def fmt(key, ts, extra=""):
    return "%-58s %10.2f ms   [%s]%s" % (key, min(ts), ", ".join("%.2f" % t for t in ts), extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only-a", action="store_true", help="measure (a) alone: runs on a commit without order_mat_device")
    ap.add_argument("--parent-a", default=None, help="the --only-a output of the commit before order_mat_device existed")
    ap.add_argument("--out", default=None, help="default: profiles/r23/order_device.txt, with --only-a order_device_parent_a.txt")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r23", "order_device_parent_a.txt" if a.only_a else "order_device.txt")
    os.environ["AOCLSPARSE_MI355_TIMING"] = "1"
    import torch

    P = entry.load_package()
    L = P.lib()
    assert torch.cuda.is_available(), "needs a GPU"
    d = P.Descr()

    def sync():
        assert L.aoclsparse_mi355_synchronize() == 0

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        sync()
        return (time.perf_counter() - t0) * 1e3, r

    # ---- the two inputs: a function that makes a fresh, resident, unsorted handle --------------------------------------------
    m, rp, ci, v = entry.laplace5(a.grid)
    nnz = len(v)
    g = torch.Generator(device="cuda")
    g.manual_seed(23)
    t_rp = torch.from_numpy(rp).cuda()
    rows = torch.repeat_interleave(torch.arange(m, device="cuda"), t_rp[1:] - t_rp[:-1])
    perm = torch.argsort(rows.double() + torch.rand(nnz, device="cuda", dtype=torch.float64, generator=g) * 0.999)
    t_ci = torch.from_numpy(ci).cuda()[perm].contiguous()
    t_v = (torch.from_numpy(v).cuda() * (0.5 + torch.rand(nnz, device="cuda", dtype=torch.float64, generator=g)))[perm].contiguous()
    del rows, perm, ci, v
    torch.cuda.synchronize()

    def make_shuffled():
        A = P.Matrix.from_device(0, m, m, nnz, t_rp, t_ci, t_v)
        assert A.status == 0, A.status
        return A

    m2, rp2, ci2, v2 = entry.laplace5(a.grid // 2)
    B = P.Matrix(0, m2, m2, rp2, ci2, v2 * np.random.default_rng(8).uniform(0.5, 1.5, len(v2)))
    assert B.status == 0

    def make_sp2m():
        C = ctypes.c_void_p()
        assert L.aoclsparse_sp2m(P.OP_NONE, d.h, B.h, P.OP_NONE, d.h, B.h, P.STAGE_FULL, ctypes.byref(C)) == 0
        return P.Matrix.from_handle(C, True)

    inputs = {"shuffled": (make_shuffled, m), "sp2m": (make_sp2m, m2)}
    res, shape = {}, {}
    for tag, (make, rows_) in inputs.items():
        x = torch.ones(rows_, dtype=torch.float64, device="cuda")
        y = torch.zeros(rows_, dtype=torch.float64, device="cuda")

        def dmv(A):
            assert P.dmv(P.OP_NONE, 1.0, A, d, x, 0.0, y) == 0

        r = res[tag] = {k: [] for k in ("a", "a_order", "a_dmv", "b", "b_order", "b_dmv", "b_kernel", "b_copy")}
        ref = None
        for k in range(a.repeats):
            with stderr_lines():
                A = make()
                dmv(A)
                sync()
            assert A.spmv_info().device_resident == 1
            with stderr_lines():
                t0, st = clock(lambda: L.aoclsparse_order_mat(A.h))
                assert st == 0, st
                t1, _ = clock(lambda: dmv(A))
            r["a"].append(t0 + t1), r["a_order"].append(t0), r["a_dmv"].append(t1)
            if k == a.repeats - 1 and not a.only_a:
                e = A.export()
                ref = (e["col_ind"], e["val"], y.clone())
                shape[tag] = (e["m"], e["nnz"])
            elif tag not in shape:
                shape[tag] = (A.m, A.nnz)
            A.destroy()
        if a.only_a:
            continue
        for k in range(a.repeats):
            with stderr_lines():
                A = make()
                dmv(A)
                sync()
            with stderr_lines() as err:
                t0, st = clock(A.order_device)
            assert st == 0, st
            assert A.spmv_info().device_resident == 1
            with stderr_lines():
                t1, _ = clock(lambda: dmv(A))
            kern = [q for q in (re.search(r"order rows kernels:\s+([\d.]+) ms", ln) for ln in err.lines) if q]
            copy = [q for q in (re.search(r"order_mat_device: host view\s+([\d.]+) ms", ln) for ln in err.lines) if q]
            assert kern and copy, "no event line from the library"
            r["b"].append(t0 + t1), r["b_order"].append(t0), r["b_dmv"].append(t1)
            r["b_kernel"].append(float(kern[0].group(1))), r["b_copy"].append(float(copy[0].group(1)))
            if k == a.repeats - 1:
                e = A.export_device()
                assert e["status"] == 0
                n_ = e["nnz"]
                dc = torch.empty(n_, dtype=torch.int32, device="cuda")
                dv = torch.empty(n_, dtype=torch.float64, device="cuda")
                hip = ctypes.CDLL(P.hip_runtime_path()[1])
                hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
                assert hip.hipMemcpy(dc.data_ptr(), e["col_ind"], 4 * n_, 3) == 0 and hip.hipMemcpy(dv.data_ptr(), e["val"], 8 * n_, 3) == 0
                assert np.array_equal(dc.cpu().numpy(), ref[0]) and np.array_equal(dv.cpu().numpy().view(np.uint64), ref[1].view(np.uint64)), \
                    "the device route left other arrays than the host route"
                assert torch.equal(y, ref[2]), "the product after the device route has other bits"
            A.destroy()

    parent = {}
    if a.parent_a:
        for ln in open(a.parent_a):
            q = re.match(r"\((shuffled|sp2m)\) \(a\) order_mat \+ next dmv\s+([\d.]+) ms\s+\[(.*?)\]", ln)
            if q:
                parent[q.group(1)] = [float(t) for t in q.group(3).split(",")]
    st, dev_id, cus, name = P.device_info()
    lines = ["# tools/order_device_timing.py --grid %d --repeats %d%s  (%s, %d CUs)" % (a.grid, a.repeats, " --only-a" if a.only_a else "", name, cus),
             "# shuffled: laplace5(%d), the entries of every row shuffled (seed 23); sp2m: laplace5(%d) times itself, rows in first-touch order"
             % (a.grid, a.grid // 2),
             "# wall clock in ms around aoclsparse_mi355_synchronize; sort kernels: device events; copy back: the library's lap timer; min [all]"]
    for tag in inputs:
        r = res[tag]
        mm, nz = shape[tag]
        lines.append("(%s) %d rows, %d entries" % (tag, mm, nz))
        lines.append(fmt("(%s) (a) order_mat + next dmv" % tag, r["a"]))
        lines.append(fmt("(%s)     a: aoclsparse_order_mat" % tag, r["a_order"]))
        lines.append(fmt("(%s)     a: next dmv (uploads the three arrays)" % tag, r["a_dmv"]))
        if a.only_a:
            continue
        if tag in parent:
            lines.append(fmt("(%s) (a) on the commit before, from --parent-a" % tag, parent[tag]))
        byts = 4.0 * nz + 16.0 * mm + 24.0 * nz
        frac = byts / (min(r["b_kernel"]) * 1e-3) / COPY_RATE
        lines.append(fmt("(%s) (b) order_mat_device + next dmv" % tag, r["b"]))
        lines.append(fmt("(%s)     b: aoclsparse_mi355_order_mat_device" % tag, r["b_order"]))
        lines.append(fmt("(%s)     b: next dmv (uploads nothing)" % tag, r["b_dmv"]))
        lines.append(fmt("(%s)     b: sort kernels (flag pass .. last kernel)" % tag, r["b_kernel"],
                         "   %.2f GB if every row is sorted: %.1f %% of the 6.29 TB/s copy rate" % (byts / 1e9, 100.0 * frac)))
        lines.append(fmt("(%s)     b: copy back into the host view" % tag, r["b_copy"],
                         "   %.0f %% of (b)" % (100.0 * min(r["b_copy"]) / min(r["b"]))))
        a_ref = parent.get(tag, r["a"])
        lines.append("(%s) (a) / (b) = %.2f  (%s)" % (tag, min(a_ref) / min(r["b"]),
                                                      "(a) of the commit before" if tag in parent else "(a) of this commit"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
