#!/usr/bin/env python
"""What does a new set of values cost a handle that was created from triplets in HBM?

The g x g 5-point Laplacian (default g = 4096: 16.8 M rows, 83.9 M triplets), its triplets shuffled with a fixed seed and resident
in HBM (`keep`), and the same with every tenth coordinate repeated (`sum`: 8.4 M triplets more).  An assembly loop produces the
same coordinates with other values every step.  Wall clock around aoclsparse_mi355_synchronize, the minimum of --repeats with the
range, for both cases:
  (a) destroy + create + first dmv    the only route without a kept map: aoclsparse_destroy, create_dcsr_from_coo_device on the new
                                      values (the whole sort again), the first aoclsparse_dmv
  (b) refresh + next dmv              a handle created once with aoclsparse_mi355_coo_keep_map, then
                                      aoclsparse_mi355_drefresh_values_from_coo_device on the new values and the next aoclsparse_dmv;
                                      the refresh kernel's own time from the library's events (AOCLSPARSE_MI355_TIMING=1, set here
                                      before the library is loaded) and its bytes / time as a fraction of the 6.29 TB/s copy rate.
                                      The bytes: 4 of the map's position + one value read per triplet, one value written per entry,
                                      in `sum` mode 4 more per entry for the run starts.
  (c) update_values_device + next dmv for scale: nnz values already in CSR order, which `keep` callers could produce themselves
                                      and `sum` callers could not
--only-a measures (a) alone and needs nothing newer than create_dcsr_from_coo_device: run on the commit before the refresh existed,
its output is what --parent-a reads to put (a) of that commit, and the ratio (a) / (b) against it, next to this commit's.
x and y are device tensors; making and shuffling the triplets is not timed.  Writes the lines to --out and prints them."""
import argparse
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
    return "%-52s %10.2f ms   [%s]%s" % (key, min(ts), ", ".join("%.2f" % t for t in ts), extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only-a", action="store_true", help="measure (a) alone: runs on a commit without the refresh")
    ap.add_argument("--parent-a", default=None, help="the --only-a output of the commit before the refresh existed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "coo_refresh.txt"))
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
    rep = np.arange(0, nnz, 10)  # `sum`: every tenth triplet once more, somewhere else in the arrays
    perm2 = rng.permutation(nnz + len(rep))
    row2, col2 = np.concatenate([row, row[rep]])[perm2], np.concatenate([col, col[rep]])[perm2]
    val2 = np.concatenate([val, 0.25 * val[rep]])[perm2]
    del perm, perm2, rp, ci, v
    d = P.Descr()
    x = torch.ones(m, dtype=torch.float64, device="cuda")
    y = torch.zeros(m, dtype=torch.float64, device="cuda")
    cases = {}
    for tag, (r_, c_, v_) in (("keep", (row, col, val)), ("sum", (row2, col2, val2))):
        tr, tc, tv = (torch.from_numpy(t).cuda() for t in (r_, c_, v_))
        cases[tag] = dict(row=tr, col=tc, val=tv, new=tv * 1.5 + 0.125, triplets=len(v_),
                          mode=P.COO_KEEP if tag == "keep" else P.COO_SUM)
    del row, col, val, row2, col2, val2
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

    def create(c, vals, flag=0):
        A = P.Matrix.from_coo_device(0, m, m, c["triplets"], c["row"], c["col"], vals, duplicates=c["mode"] | flag)
        assert A.status == 0 and A.nnz == nnz, (A.status, A.nnz)
        return A

    lines = []
    res = {}
    for tag, c in cases.items():
        r = res[tag] = {k: [] for k in ("a", "a_create", "a_dmv", "b", "b_refresh", "b_dmv", "b_kernel", "c", "c_update", "c_dmv")}
        # (a): the handle of the previous step goes, a new one is sorted from the new values
        with stderr_lines():
            A = create(c, c["val"])
            dmv(A)
            for k in range(a.repeats):
                vals = c["new"] if k % 2 == 0 else c["val"]

                def recreate():
                    A.destroy()
                    return create(c, vals)
                t0, A = clock(recreate)
                t1, _ = clock(lambda: dmv(A))
                r["a"].append(t0 + t1), r["a_create"].append(t0), r["a_dmv"].append(t1)
            y_a = y.clone() if a.repeats % 2 == 1 else None  # (the product on the NEW values, when the last repeat used them)
            A.destroy()
        if a.only_a:
            continue
        # (b): one creation that keeps the map, then values only
        with stderr_lines():
            R = create(c, c["val"], P.COO_KEEP_MAP)
            dmv(R)
        info = R.coo_map_info()
        assert info.kept == 1 and info.triplets == c["triplets"] and info.entries == nnz
        for k in range(a.repeats):
            vals = c["new"] if k % 2 == 0 else c["val"]
            with stderr_lines() as err:
                t0, st = clock(lambda: R.refresh_from_coo_device(vals))
            assert st == 0, st
            t1, _ = clock(lambda: dmv(R))
            g = [re.search(r"coo refresh kernel \(%s\):\s+([\d.]+) ms" % tag, ln) for ln in err.lines]
            g = [q for q in g if q]
            assert g, "no event line from the library"
            r["b"].append(t0 + t1), r["b_refresh"].append(t0), r["b_dmv"].append(t1), r["b_kernel"].append(float(g[0].group(1)))
        if y_a is not None:
            assert torch.equal(y, y_a), "refreshed handle: other bits than a fresh creation"
        assert R.spmv_info().device_resident == 1
        # (c): values that are in CSR order already
        tn = torch.full((nnz,), 0.5, dtype=torch.float64, device="cuda")
        for k in range(a.repeats):
            t0, st = clock(lambda: R.update_values_device(tn))
            assert st == 0, st
            t1, _ = clock(lambda: dmv(R))
            r["c"].append(t0 + t1), r["c_update"].append(t0), r["c_dmv"].append(t1)
        r["map_bytes"] = int(info.map_bytes)
        R.destroy()
        del tn

    parent = {}
    if a.parent_a:
        for ln in open(a.parent_a):
            g = re.match(r"\((keep|sum)\) \(a\) destroy \+ create \+ first dmv\s+([\d.]+) ms\s+\[(.*?)\]", ln)
            if g:
                parent[g.group(1)] = [float(t) for t in g.group(3).split(",")]
    st, dev_id, cus, name = P.device_info()
    lines = ["# tools/coo_refresh_timing.py --grid %d --repeats %d%s  (%s, %d CUs)" % (a.grid, a.repeats, " --only-a" if a.only_a else "", name, cus),
             "# laplace5(%d): m = %d; keep: %d triplets shuffled (seed 19); sum: %d triplets, every tenth coordinate repeated; %d entries both"
             % (a.grid, m, cases["keep"]["triplets"], cases["sum"]["triplets"], nnz),
             "# wall clock in ms around aoclsparse_mi355_synchronize; refresh kernel: device events; min of the repeats [all]"]
    for tag, c in cases.items():
        r = res[tag]
        lines.append(fmt("(%s) (a) destroy + create + first dmv" % tag, r["a"]))
        lines.append(fmt("(%s)     a: destroy + create" % tag, r["a_create"]))
        lines.append(fmt("(%s)     a: first dmv" % tag, r["a_dmv"]))
        if a.only_a:
            continue
        if tag in parent:
            lines.append(fmt("(%s) (a) on the commit before, from --parent-a" % tag, parent[tag]))
        byts = 12.0 * c["triplets"] + 8.0 * nnz + (4.0 * (nnz + 1) if tag == "sum" else 0.0)
        frac = byts / (min(r["b_kernel"]) * 1e-3) / COPY_RATE
        lines.append(fmt("(%s) (b) refresh + next dmv" % tag, r["b"]))
        lines.append(fmt("(%s)     b: refresh_values_from_coo_device" % tag, r["b_refresh"]))
        lines.append(fmt("(%s)     b: next dmv" % tag, r["b_dmv"]))
        lines.append(fmt("(%s)     b: refresh kernel" % tag, r["b_kernel"],
                         "   %.2f GB of map, values in and values out: %.1f %% of the 6.29 TB/s copy rate" % (byts / 1e9, 100.0 * frac)))
        lines.append(fmt("(%s) (c) update_values_device + next dmv" % tag, r["c"]))
        lines.append(fmt("(%s)     c: update_values_device" % tag, r["c_update"]))
        lines.append(fmt("(%s)     c: next dmv" % tag, r["c_dmv"]))
        a_ref = parent.get(tag, r["a"])
        lines.append("(%s) (a) / (b) = %.2f  (%s)   (b) - (c) = %.2f ms   map kept on the handle: %.1f MB"
                     % (tag, min(a_ref) / min(r["b"]), "(a) of the commit before" if tag in parent else "(a) of this commit",
                        min(r["b"]) - min(r["c"]), r["map_bytes"] / 1e6))
        if frac < 0.5:
            # a shuffled gather reads 8-byte values out of 64-byte sectors
            moved = (4.0 + 64.0) * c["triplets"] + 8.0 * nnz + (4.0 * (nnz + 1) if tag == "sum" else 0.0)
            lines.append("#   (%s) sector amplification: the positions are a random permutation here, so every 8-byte value read fetches a 64-byte"
                         % tag)
            lines.append("#   sector: %.2f GB cross the memory interface, %.1f %% of the copy rate.  Worst case; element-ordered assembly is mild."
                         % (moved / 1e9, 100.0 * moved / (min(r["b_kernel"]) * 1e-3) / COPY_RATE))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
