#!/usr/bin/env python
"""What does the clean CSR (rows in group order, a full diagonal, idiag / iurow) of a handle that lives in HBM cost?

Three inputs, all resident before anything is timed:
  shuffled   the g x g 5-point Laplacian (default g = 4096: 16.8 M rows, 83.9 M entries) with the entries of every row shuffled by a
             fixed seed: case 3 with a full diagonal (sort, then a copy without insertions)
  nodiag     the same Laplacian fully sorted, every 10th diagonal entry removed: case 2 (mark, scan and expand alone)
  sp2m       the result of aoclsparse_sp2m of the g/2 x g/2 Laplacian with itself, whose rows are in first-touch order: case 3
Wall clock around aoclsparse_mi355_synchronize, the minimum of --repeats with the range; every repeat starts from a fresh handle
that is resident and has run one dmv (making it is not timed):
  (a) aoclsparse_optimize          the host route, csr_optimize.  aoclsparse_optimize returns at once without a pending hint, so the
                                   handle gets (untimed) the one hint that asks for the clean CSR and nothing else: a forward SOR sweep
  (b) aoclsparse_mi355_clean_csr_device   the same result built in HBM; its parts from the library's lap timer
                                   (AOCLSPARSE_MI355_TIMING=1, set here before the library is loaded): the check kernels, the sort,
                                   mark + scan, the host allocations, expand + finish, the copy back
--only-a measures (a) alone and needs nothing newer than create_dcsr_device: run on the commit before clean_csr_device existed, its
output is what --parent-a reads to put (a) of that commit next to this commit's.
Both routes must leave the same clean CSR: aoclsparse_export_dcsr and aoclsparse_mi355_export_diag of (b) are compared with those
of (a), bit for bit, once per input."""
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

LAPS = ["mirror + check", "sort", "mark + scan", "host arrays", "expand + finish", "copy back"]


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
    ap.add_argument("--only-a", action="store_true", help="measure (a) alone: runs on a commit without clean_csr_device")
    ap.add_argument("--parent-a", default=None, help="the --only-a output of the commit before clean_csr_device existed")
    ap.add_argument("--out", default=None, help="default: profiles/r24/clean_device.txt, with --only-a clean_device_parent_a.txt")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r24", "clean_device_parent_a.txt" if a.only_a else "clean_device.txt")
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

    # ---- the three inputs: a function that makes a fresh, resident handle ----------------------------------------------------
    m, rp, ci, v = entry.laplace5(a.grid)
    nnz = len(v)
    g = torch.Generator(device="cuda")
    g.manual_seed(24)
    t_rp = torch.from_numpy(rp).cuda()
    rows = torch.repeat_interleave(torch.arange(m, device="cuda"), t_rp[1:] - t_rp[:-1])
    perm = torch.argsort(rows.double() + torch.rand(nnz, device="cuda", dtype=torch.float64, generator=g) * 0.999)
    s_ci, s_v = torch.from_numpy(ci).cuda(), torch.from_numpy(v).cuda() * (0.5 + torch.rand(nnz, device="cuda", dtype=torch.float64, generator=g))
    t_ci, t_v = s_ci[perm].contiguous(), s_v[perm].contiguous()
    keep = ~((s_ci == rows) & (rows % 10 == 0))
    n_ci, n_v = s_ci[keep].contiguous(), s_v[keep].contiguous()
    n_rp = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
    n_rp[1:] = torch.cumsum(torch.bincount(rows[keep], minlength=m), 0).to(torch.int32)
    n_nnz = int(n_ci.numel())
    del rows, perm, keep, s_ci, s_v, ci, v
    torch.cuda.synchronize()

    def make_shuffled():
        A = P.Matrix.from_device(0, m, m, nnz, t_rp, t_ci, t_v)
        assert A.status == 0, A.status
        return A

    def make_nodiag():
        A = P.Matrix.from_device(0, m, m, n_nnz, n_rp, n_ci, n_v)
        assert A.status == 0, A.status
        return A

    m2, rp2, ci2, v2 = entry.laplace5(a.grid // 2)
    B = P.Matrix(0, m2, m2, rp2, ci2, v2 * np.random.default_rng(8).uniform(0.5, 1.5, len(v2)))
    assert B.status == 0

    def make_sp2m():
        C = ctypes.c_void_p()
        assert L.aoclsparse_sp2m(P.OP_NONE, d.h, B.h, P.OP_NONE, d.h, B.h, P.STAGE_FULL, ctypes.byref(C)) == 0
        return P.Matrix.from_handle(C, True)

    def clean_of(A):
        e, dg = A.export(), A.export_diag()
        assert e["status"] == 0 and dg["status"] == 0
        return [e["base"], e["row_ptr"], e["col_ind"], e["val"].view(np.uint64), dg["idiag"], dg["iurow"], dg["is_internal"]]

    inputs = {"shuffled": (make_shuffled, m), "nodiag": (make_nodiag, m), "sp2m": (make_sp2m, m2)}
    res, shape = {}, {}
    for tag, (make, rows_) in inputs.items():
        x = torch.ones(rows_, dtype=torch.float64, device="cuda")
        y = torch.zeros(rows_, dtype=torch.float64, device="cuda")

        def fresh():
            with stderr_lines():
                A = make()
                assert P.dmv(P.OP_NONE, 1.0, A, d, x, 0.0, y) == 0
                sync()
            assert A.spmv_info().device_resident == 1
            return A

        r = res[tag] = {k: [] for k in ["a", "b"] + LAPS}
        ref = None
        for k in range(a.repeats):
            A = fresh()
            assert L.aoclsparse_set_sorv_hint(A.h, d.h, 0, 1) == 0  # aoclsparse_sor_forward
            with stderr_lines():
                t0, st = clock(lambda: L.aoclsparse_optimize(A.h))
            assert st == 0, st
            r["a"].append(t0)
            shape[tag] = (A.m, A.nnz)
            if k == a.repeats - 1 and not a.only_a:
                ref = clean_of(A)
            A.destroy()
        if a.only_a:
            continue
        for k in range(a.repeats):
            A = fresh()
            with stderr_lines() as err:
                t0, st = clock(A.clean_device)
            assert st == 0, st
            assert A.spmv_info().device_resident == 1
            r["b"].append(t0)
            for lap in LAPS:
                q = [w for w in (re.search(r"clean_csr_device: %s\s+([\d.]+) ms" % re.escape(lap), ln) for ln in err.lines) if w]
                r[lap].append(float(q[0].group(1)) if q else 0.0)
            if k == a.repeats - 1:
                got = clean_of(A)
                assert got[0] == ref[0] and got[6] == ref[6] and all(np.array_equal(p, q) for p, q in zip(got[1:6], ref[1:6])), \
                    "the device route left another clean CSR than the host route"
                shape[tag] += (len(got[2]),)
            A.destroy()

    parent = {}
    if a.parent_a:
        for ln in open(a.parent_a):
            q = re.match(r"\((\w+)\) \(a\) aoclsparse_optimize\s+([\d.]+) ms\s+\[(.*?)\]", ln)
            if q:
                parent[q.group(1)] = [float(t) for t in q.group(3).split(",")]
    st, dev_id, cus, name = P.device_info()
    lines = ["# tools/clean_device_timing.py --grid %d --repeats %d%s  (%s, %d CUs)" % (a.grid, a.repeats, " --only-a" if a.only_a else "", name, cus),
             "# shuffled: laplace5(%d), the entries of every row shuffled (seed 24); nodiag: the same sorted, every 10th diagonal entry removed;"
             % a.grid,
             "# sp2m: laplace5(%d) times itself, rows in first-touch order.  double precision, base 0" % (a.grid // 2),
             "# wall clock in ms around aoclsparse_mi355_synchronize; the parts of (b): the library's lap timer (host clock, the stream",
             "# synchronised at every lap); min [all]"]
    for tag in inputs:
        r = res[tag]
        lines.append("(%s) %d rows, %d entries%s" % ((tag,) + shape[tag][:2] + (", %d in the clean CSR" % shape[tag][2] if len(shape[tag]) > 2 else "",)))
        lines.append(fmt("(%s) (a) aoclsparse_optimize" % tag, r["a"]))
        if a.only_a:
            continue
        if tag in parent:
            lines.append(fmt("(%s) (a) on the commit before, from --parent-a" % tag, parent[tag]))
        lines.append(fmt("(%s) (b) aoclsparse_mi355_clean_csr_device" % tag, r["b"]))
        for lap in LAPS:
            lines.append(fmt("(%s)     b: %s" % (tag, lap), r[lap], "   %.0f %% of (b)" % (100.0 * min(r[lap]) / min(r["b"]))))
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
