#!/usr/bin/env python
"""What does a solve after a value change in HBM cost, with and without value maps?

Two inputs, double precision, base 0, solved with a lower-triangular descriptor:
  sorted     the g x g 5-point Laplacian (default g = 4096: 16.8 M rows, 83.9 M entries): the clean CSR is the handle's own arrays
  shuffled   the same with the entries of every row shuffled by a fixed seed, cleaned by aoclsparse_mi355_clean_csr_device: case 3,
             the clean CSR is a copy
Wall clock around aoclsparse_mi355_synchronize, the minimum of --repeats with the range.  The handle is resident and has solved
once before anything is timed, and every repeat leaves it so for the next one (the values alternate between two sets):
  (a) aoclsparse_mi355_dupdate_values_device, then the next aoclsparse_dtrsv: the clean copy, the diagonal and the plan are built again
  (b) aoclsparse_mi355_keep_value_maps + aoclsparse_mi355_drevalue_device, then the next aoclsparse_dtrsv; the parts of the revalue
      from the library's lap timer (AOCLSPARSE_MI355_TIMING=1, set here before the library is loaded; host clock, the stream
      synchronised at every lap): the values to the host view and the mirror, the clean gather with its copy back, the diagonal's
      and the plans' gathers; and the gather kernels alone from the device events the library records under the same switch
--only-a measures (a) alone and needs nothing newer than ?update_values_device and clean_csr_device: run on the commit before
?revalue_device existed, its output is what --parent-a reads to put (a) of that commit next to this commit's (b).
After the last repeat of (b) the solution is compared, bit for bit, with that of a fresh handle created with the same values."""
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
from clean_device_timing import fmt, stderr_lines  # noqa: E402

LAPS = ["values to host view + mirror", "clean gather + copy back", "diagonal + plan gathers"]
EVENTS = ["clean gather events", "plan gather events"]  # device events around the gather kernels alone (hipEventElapsedTime)
COPY_RATE = 6.29e12  # bytes/s, the device-to-device copy rate the DESIGN tables refer to


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only-a", action="store_true", help="measure (a) alone: runs on a commit without ?revalue_device")
    ap.add_argument("--parent-a", default=None, help="the --only-a output of the commit before ?revalue_device existed")
    ap.add_argument("--out", default=None, help="default: profiles/r25/revalue_device.txt, with --only-a revalue_device_parent_a.txt")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r25", "revalue_device_parent_a.txt" if a.only_a else "revalue_device.txt")
    os.environ["AOCLSPARSE_MI355_TIMING"] = "1"
    import torch

    P = entry.load_package()
    L = P.lib()
    assert torch.cuda.is_available(), "needs a GPU"
    d = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=P.FILL_LOWER)

    def sync():
        assert L.aoclsparse_mi355_synchronize() == 0

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        sync()
        return (time.perf_counter() - t0) * 1e3, r

    m, rp, ci, v = entry.laplace5(a.grid)
    nnz = len(v)
    g = torch.Generator(device="cuda")
    g.manual_seed(25)
    t_rp = torch.from_numpy(rp).cuda()
    rows = torch.repeat_interleave(torch.arange(m, device="cuda"), t_rp[1:] - t_rp[:-1])
    perm = torch.argsort(rows.double() + torch.rand(nnz, device="cuda", dtype=torch.float64, generator=g) * 0.999)
    s_ci, s_v = torch.from_numpy(ci).cuda(), torch.from_numpy(v).cuda()
    scale = [0.5 + torch.rand(nnz, device="cuda", dtype=torch.float64, generator=g) for _ in range(2)]
    inputs = {"sorted": (s_ci, [(s_v * s).contiguous() for s in scale], False),
              "shuffled": (s_ci[perm].contiguous(), [(s_v * s)[perm].contiguous() for s in scale], True)}
    strict = int((s_ci < rows).sum().item())
    del rows, perm, ci, v
    b = torch.ones(m, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def solve(A):
        x = torch.zeros(m, dtype=torch.float64, device="cuda")
        assert P.dtrsv(P.OP_NONE, 1.0, A, d, b, x) == 0
        return x

    res, notes = {}, {}
    for tag, (t_ci, vals, clean) in inputs.items():
        def fresh(k, maps):
            with stderr_lines():
                A = P.Matrix.from_device(0, m, m, nnz, t_rp, t_ci, vals[k])
                assert A.status == 0, A.status
                if maps:
                    assert A.keep_value_maps() == 0
                if clean:
                    assert A.clean_device() == 0
                solve(A)
                sync()
            assert A.spmv_info().device_resident == 1
            return A

        r = res[tag] = {k: [] for k in ["a", "a update", "a solve", "b", "b revalue", "b solve"] + LAPS + EVENTS}
        A = fresh(0, False)
        for k in range(a.repeats):
            with stderr_lines():
                t0, st = clock(lambda: A.update_values_device(vals[(k + 1) % 2]))
                assert st == 0, st
                if clean:  # (the clean copy was dropped: the time-stepping code of DESIGN 5.6 builds it in HBM again)
                    t1, st = clock(A.clean_device)
                    assert st == 0, st
                    t0 += t1
                t2, _ = clock(lambda: solve(A))
            r["a"].append(t0 + t2), r["a update"].append(t0), r["a solve"].append(t2)
        A.destroy()
        if a.only_a:
            continue
        A = fresh(0, True)
        for k in range(a.repeats):
            i0 = A.value_map_info()
            with stderr_lines() as err:
                t0, st = clock(lambda: A.revalue_device(vals[(k + 1) % 2]))
                assert st == 0, st
                t2, x = clock(lambda: solve(A))
            i1 = A.value_map_info()
            assert (i1.plan_builds, i1.clean_builds, i1.last_kept_plans) == (i0.plan_builds, i0.clean_builds, 1), "something was rebuilt"
            r["b"].append(t0 + t2), r["b revalue"].append(t0), r["b solve"].append(t2)
            for lap in LAPS + EVENTS:
                q = [w for w in (re.search(r"revalue_device: %s\s+([\d.]+) ms" % re.escape(lap), ln) for ln in err.lines) if w]
                r[lap].append(float(q[0].group(1)) if q else 0.0)
        info, ti = A.value_map_info(), A.trsv_info(P.FILL_LOWER)
        layouts = (info.map_bytes - 4 * m - (4 * nnz if clean else 0)) // (4 * max(strict, 1))
        notes[tag] = "%d plan kept, %d layout(s), %d levels, %d blocks, schedule %d, maps %.1f MB" % (
            info.plans_mapped, layouts, ti.levels, ti.blocks, ti.schedule, info.map_bytes / 1e6)
        # bytes the diagonal's and the plan's gathers move: 4 (map) + 8 (value read) + 8 (value written) per item
        r["gather bytes"] = 20.0 * (m + layouts * strict)
        r["clean bytes"] = 20.0 * nnz if clean else 0.0
        T = fresh(a.repeats % 2, False)
        assert torch.equal(x, solve(T)), "the solve after ?revalue_device differs from a fresh handle's"
        T.destroy(), A.destroy()

    parent = {}
    if a.parent_a:
        for ln in open(a.parent_a):
            q = re.match(r"\((\w+)\) \(a\) update_values_device.*?\s+([\d.]+) ms\s+\[(.*?)\]", ln)
            if q:
                parent[q.group(1)] = [float(t) for t in q.group(3).split(",")]
    st, dev_id, cus, name = P.device_info()
    lines = ["# tools/revalue_timing.py --grid %d --repeats %d%s  (%s, %d CUs)" % (a.grid, a.repeats, " --only-a" if a.only_a else "", name, cus),
             "# sorted: laplace5(%d), %d rows, %d entries, %d in the strict lower triangle; shuffled: the entries of every row shuffled" % (a.grid, m, nnz, strict),
             "# (seed 25), cleaned by clean_csr_device.  double precision, base 0, lower-triangular descriptor, op = N, non-unit",
             "# wall clock in ms around aoclsparse_mi355_synchronize; the parts of the revalue: the library's lap timer (host clock, the",
             "# stream synchronised at every lap); the gather kernels alone: device events (hipEventElapsedTime); min [all]"]
    for tag, (_, _, clean) in inputs.items():
        r = res[tag]
        what = "update_values_device%s + dtrsv" % (" + clean_csr_device" if clean else "")
        lines.append(fmt("(%s) (a) %s" % (tag, what), r["a"]))
        lines.append(fmt("(%s)     a: the update%s" % (tag, " and the clean copy" if clean else ""), r["a update"]))
        lines.append(fmt("(%s)     a: the solve (builds the diagonal and the plan)" % tag, r["a solve"]))
        if a.only_a:
            continue
        if tag in parent:
            lines.append(fmt("(%s) (a) on the commit before, from --parent-a" % tag, parent[tag]))
        lines.append(fmt("(%s) (b) revalue_device + dtrsv" % tag, r["b"]))
        lines.append(fmt("(%s)     b: revalue_device" % tag, r["b revalue"]))
        for lap in LAPS:
            lines.append(fmt("(%s)        revalue: %s" % (tag, lap), r[lap]))
        lines.append(fmt("(%s)     b: the solve" % tag, r["b solve"]))
        lines.append("(%s)     %s" % (tag, notes[tag]))
        for ev, nbytes in (("clean gather events", r["clean bytes"]), ("plan gather events", r["gather bytes"])):
            t = min(r[ev])
            if t > 0 and nbytes > 0:
                lines.append(fmt("(%s)        revalue: %s" % (tag, ev), r[ev]))
                lines.append("(%s)        %s: %.1f MB (4 B map + 8 B read + 8 B written per item) in %.3f ms = %.2f TB/s = %.2f of the %.2f TB/s copy rate"
                             % (tag, ev, nbytes / 1e6, t, nbytes / (t * 1e-3) / 1e12, nbytes / (t * 1e-3) / COPY_RATE, COPY_RATE / 1e12))
        a_ref = parent.get(tag, r["a"])
        lines.append("(%s) (a) / (b) = %.2f  (%s)" % (tag, min(a_ref) / min(r["b"]), "(a) of the commit before" if tag in parent else "(a) of this commit"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
