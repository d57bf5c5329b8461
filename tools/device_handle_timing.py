#!/usr/bin/env python
"""How long does a matrix take to get into the library, from host arrays and from arrays in HBM?

Four wall-clock figures on the g x g 5-point Laplacian (default g = 4096: 16.8 M rows, 83.9 M non-zeros), each ending in
aoclsparse_mi355_synchronize:
  create_host + first dmv      aoclsparse_create_dcsr on numpy arrays, then aoclsparse_dmv (which uploads the arrays)
  create_device + first dmv    aoclsparse_mi355_create_dcsr_device on device tensors (check kernels, device copy, copy back to
                               the host view), then aoclsparse_dmv
  update_host + next dmv       aoclsparse_dupdate_values from a numpy array, then aoclsparse_dmv (uploads all three arrays again)
  update_device + next dmv     aoclsparse_mi355_dupdate_values_device from a device tensor, then aoclsparse_dmv
x and y are device tensors throughout; the upload of the caller's device tensors is not timed (they are "already on the GPU").
The device route is also split into its parts (create alone / first dmv alone).  Writes the lines to --out and prints them."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r7", "device_handles.txt"))
    a = ap.parse_args()
    import torch

    P = entry.load_package()
    L = P.lib()
    assert torch.cuda.is_available(), "needs a GPU"
    m, rp, ci, v = entry.laplace5(a.grid)
    nnz = len(v)
    v2 = np.ascontiguousarray(v * 1.5)
    d = P.Descr()
    x = torch.ones(m, dtype=torch.float64, device="cuda")
    y = torch.zeros(m, dtype=torch.float64, device="cuda")
    trp, tci, tv, tv2 = (torch.from_numpy(t).cuda() for t in (rp, ci, v, v2))
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

    rows = {k: [] for k in ("create_host+dmv", "create_device+dmv", "create_device alone", "first dmv after create_device",
                            "update_host+dmv", "update_device+dmv", "update_device alone")}
    for _ in range(a.repeats):
        vh = v.copy()  # (the handle aliases it and ?update_values writes into it)

        def host():
            A = P.Matrix(0, m, m, rp, ci, vh)
            assert A.status == 0
            dmv(A)
            return A
        t, A = clock(host)
        rows["create_host+dmv"].append(t)
        y_host = y.clone()

        def upd_host():
            assert L.aoclsparse_dupdate_values(A.h, nnz, P._ptr(v2)) == 0
            dmv(A)
        rows["update_host+dmv"].append(clock(upd_host)[0])
        y_host2 = y.clone()
        A.destroy()

        t0, D = clock(lambda: P.Matrix.from_device(0, m, m, nnz, trp, tci, tv))
        assert D.status == 0
        t1, _ = clock(lambda: dmv(D))
        rows["create_device alone"].append(t0)
        rows["first dmv after create_device"].append(t1)
        rows["create_device+dmv"].append(t0 + t1)
        assert torch.equal(y, y_host), "device-created handle: other bits"
        t2, st = clock(lambda: D.update_values_device(tv2))
        assert st == 0
        t3, _ = clock(lambda: dmv(D))
        rows["update_device alone"].append(t2)
        rows["update_device+dmv"].append(t2 + t3)
        assert torch.equal(y, y_host2), "device-updated handle: other bits"
        D.destroy()

    st, dev_id, cus, name = P.device_info()
    lines = ["# tools/device_handle_timing.py --grid %d --repeats %d  (%s, %d CUs)" % (a.grid, a.repeats, name, cus),
             "# laplace5(%d): m = %d, nnz = %d; wall clock in ms around aoclsparse_mi355_synchronize; min of the repeats [all]" % (a.grid, m, nnz)]
    for k, ts in rows.items():
        lines.append("%-32s %10.2f ms   [%s]" % (k, min(ts), ", ".join("%.2f" % t for t in ts)))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
