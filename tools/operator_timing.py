#!/usr/bin/env python
"""What does the operator of a symmetric descriptor cost: built by the first product on the host or by
aoclsparse_mi355_build_operator_device in HBM, and after a value change in HBM dropped and rebuilt or kept?

Input: the g x g 5-point Laplacian (default g = 4096: 16.8 M rows, 83.9 M entries), base 0, resident in HBM, its clean CSR made by
aoclsparse_mi355_clean_csr_device before anything is timed (the handle's own arrays); the operator is that of the symmetric
descriptor with the lower fill.  Wall clock around aoclsparse_mi355_synchronize, in ms, the minimum of --repeats with all values:
  (a) a fresh handle's first symmetric ?mv: the host loop build_derived, the upload, the SELL-64 build, the product
  (b) aoclsparse_mi355_build_operator_device on a fresh handle (kernels, the copy back of the host view, plan and SELL-64 build),
      and the first symmetric ?mv behind it
  (c) ?revalue_device + the next symmetric ?mv with an operator a product built: dropped, and built again as in (a)
  (d) the same with the operator build_operator_device built under keep_value_maps: one gather, one copy back, the SELL-64 refill
  (e) ?revalue_device alone on a handle without operators, and the general ?mv behind it (its own SELL-64 refill)
After the last repeat of (d) the product is compared bit for bit with (c)'s on the same values.  --timing also sets
AOCLSPARSE_MI355_TIMING=1, so that the library's laps go to stderr."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def fmt(what, ts):
    return "%-84s %10.2f ms  [%s]" % (what, min(ts), ", ".join("%.2f" % t for t in ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dtype", default="float64", choices=["float64", "float32"])
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.timing:
        os.environ["AOCLSPARSE_MI355_TIMING"] = "1"
    import torch

    P = entry.load_package()
    L = P.lib()
    assert torch.cuda.is_available(), "needs a GPU"
    tdt = torch.float64 if a.dtype == "float64" else torch.float32
    mvf = P.dmv if a.dtype == "float64" else P.smv
    sym, gen = P.Descr(mtype=P.TYPE_SYMMETRIC, fill=P.FILL_LOWER), P.Descr()

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        assert L.aoclsparse_mi355_synchronize() == 0
        return (time.perf_counter() - t0) * 1e3, r

    m, rp, ci, v = entry.laplace5(a.grid, dtype=a.dtype)
    nnz = len(v)
    g = torch.Generator(device="cuda")
    g.manual_seed(30)
    t_rp, t_ci, t_v = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(v).cuda()
    vals = [(t_v * (0.5 + torch.rand(nnz, device="cuda", dtype=tdt, generator=g))).contiguous() for _ in range(2)]
    x = torch.rand(m, device="cuda", dtype=tdt, generator=g)
    del ci, v
    torch.cuda.synchronize()

    def fresh(maps):
        A = P.Matrix.from_device(0, m, m, nnz, t_rp, t_ci, vals[0])
        assert A.status == 0, A.status
        if maps:
            assert A.keep_value_maps() == 0
        assert A.clean_device() == 0
        return A

    def product(A, d):
        y = torch.zeros(m, device="cuda", dtype=tdt)
        assert mvf(P.OP_NONE, 1.0, A, d, x, 0.0, y) == 0
        return y

    r = {k: [] for k in ("a", "b", "b mv", "c", "c revalue", "c mv", "d", "d revalue", "d mv", "e revalue", "e mv")}
    for _ in range(a.repeats):
        A = fresh(False)
        r["a"].append(clock(lambda: product(A, sym))[0])
        assert A.operator_info(sym).host_builds == 1
        A.destroy()
        A = fresh(True)
        t, st = clock(lambda: A.build_operator_device(sym))
        assert st == 0 and A.operator_info(sym).built_on_device == 1, st
        r["b"].append(t), r["b mv"].append(clock(lambda: product(A, sym))[0])
        A.destroy()
    C, D, E = fresh(True), fresh(True), fresh(True)
    product(C, sym)
    assert D.build_operator_device(sym) == 0
    product(D, sym), product(E, gen), product(E, gen)
    yc = yd = None
    for k in range(a.repeats):
        new = vals[(k + 1) % 2]
        for tag, X, d in (("c", C, sym), ("d", D, sym), ("e", E, gen)):
            t0, st = clock(lambda: X.revalue_device(new))
            assert st == 0, st
            t1, y = clock(lambda: product(X, d))
            r[tag + " revalue"].append(t0), r[tag + " mv"].append(t1)
            if tag != "e":
                r[tag].append(t0 + t1)
            yc, yd = (y, yd) if tag == "c" else (yc, y) if tag == "d" else (yc, yd)
    ic, idv = C.operator_info(sym), D.operator_info(sym)
    assert (ic.built_on_device, ic.host_builds) == (0, a.repeats + 1) and (idv.built_on_device, idv.device_builds, idv.host_builds, idv.followed) == (1, 1, 0, 1)
    assert torch.equal(yc, yd), "the product on the kept operator differs from the rebuilt one's"
    st, dev_id, cus, name = P.device_info()
    lines = ["# tools/operator_timing.py --grid %d --repeats %d --dtype %s  (%s, %d CUs)" % (a.grid, a.repeats, a.dtype, name, cus),
             "# laplace5(%d): %d rows, %d entries; symmetric descriptor, lower fill: an operator of %d entries; wall clock, min [all]"
             % (a.grid, m, nnz, idv.nnz),
             fmt("(a) first symmetric mv of a fresh handle: host build, upload, SELL-64 build, product", r["a"]),
             fmt("(b) build_operator_device", r["b"]), fmt("    the first symmetric mv behind it", r["b mv"]),
             fmt("(c) revalue_device + symmetric mv, operator built by a product (dropped, rebuilt)", r["c"]),
             fmt("    c: revalue_device", r["c revalue"]), fmt("    c: the mv", r["c mv"]),
             fmt("(d) revalue_device + symmetric mv, operator kept (gather, copy back, SELL-64 refill)", r["d"]),
             fmt("    d: revalue_device", r["d revalue"]), fmt("    d: the mv", r["d mv"]),
             fmt("(e) revalue_device alone, no operator on the handle", r["e revalue"]),
             fmt("    e: the general mv behind it (refills the handle's own SELL-64 copy)", r["e mv"]),
             "(a) / (b) = %.1f    (c) / (d) = %.1f    (d) / ((e) revalue + mv) = %.2f    operator map %.1f MB, SELL-64 refills %d"
             % (min(r["a"]) / min(r["b"]), min(r["c"]) / min(r["d"]), min(r["d"]) / (min(r["e revalue"]) + min(r["e mv"])),
                idv.map_bytes / 1e6, idv.sell_value_fills)]
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
