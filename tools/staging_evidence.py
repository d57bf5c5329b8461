"""Hashes and staging footprints for comparing two builds of the library: run once per build, each in a fresh process
(AOCLSPARSE_MI355_LIB selects the build), and diff the outputs.

  python tools/staging_evidence.py hashes      ->  <case> <output>=<sha256[:16]> ...   (host-pointer call of every case of
  python tools/staging_evidence.py footprint   ->  <case> <bytes aoclsparse_mi355_release_staging frees after one call>  tests/pointer_cases.py)
  python tools/staging_evidence.py products    ->  <case> row_ptr=.. col_ind=.. val=.. staging=<bytes freed after the call(s)>
                                                   for a fixed list of sparse-product calls (sp2m, syrk, sypr; double and cdouble)
"""
import ctypes
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]  # (the test modules import the oracle package of the root)


def main(what):
    from pointer_cases import CASES, P, bits, run_case

    L = P.lib()
    freed = ctypes.c_size_t()
    for name in sorted(CASES):
        assert L.aoclsparse_mi355_release_staging(ctypes.byref(freed)) == 0
        out, check = run_case(name, "host")
        if what == "hashes":
            print(name, " ".join("%s=%s" % (k, hashlib.sha256(bits(out[k]).tobytes()).hexdigest()[:16]) for k in sorted(out)))
        else:
            assert L.aoclsparse_mi355_release_staging(ctypes.byref(freed)) == 0
            print(name, freed.value)


def products():
    """Operands: tests/spgemm_edges.py (sp2m) and the SHAPES of tests/test_sy_sparse_gpu.py (syrk, sypr).  Every case starts from
    released staging and fresh operand handles, so a line depends on nothing but its own calls."""
    import numpy as np

    import spgemm_edges as E
    import test_sy_sparse_gpu as S
    from test_sy_sparse_cpu import COUNT, FINAL, FULL, H, N, T, Handle, Result, export, sym_descr

    P = S.P
    L = P.lib()
    freed = ctypes.c_size_t()
    names = {N: "N", T: "T", H: "H"}
    requests = (("full", (FULL,)), ("count+finalize", (COUNT, FINAL)))

    def case(name, t, call, sequences=requests):
        """call(request, Result) -> status, once per request of each sequence, on the same Result"""
        for label, seq in sequences:
            assert L.aoclsparse_mi355_release_staging(ctypes.byref(freed)) == 0
            r, t0 = Result(), time.perf_counter()
            for request in seq:
                st = call(request, r)
                assert st == 0, (name, label, P.STATUS[st])
            print("%s %s %s: %.3f s" % (name, t, label, time.perf_counter() - t0), file=sys.stderr, flush=True)
            assert L.aoclsparse_mi355_release_staging(ctypes.byref(freed)) == 0
            x = export(r.h, t)
            sha = " ".join("%s=%s" % (k, hashlib.sha256(np.ascontiguousarray(x[k]).view(np.uint8).tobytes()).hexdigest()[:16])
                           for k in ("row_ptr", "col_ind", "val"))
            print("%s %s %s %dx%d nnz=%d %s staging=%d" % (name, t, label, x["m"], x["n"], x["nnz"], sha, freed.value), flush=True)

    # A^T * A and A * A^T leave the "over" rows out: 8,193 entries in one column make one row of the product cost ~10^8 steps
    every, light = E.edge_operands(9000), E.edge_operands(9000, tuple(f for f in E.FAMILIES if f != "over"))
    d0 = P.Descr()
    for t in ("d", "z"):
        def vals(v):
            return v.astype(np.complex128) + 1j * np.roll(v, 1) if t == "z" else v

        def fresh(ops):
            (pa, ia, va), (pb, ib, vb) = ops.A, ops.B
            return Handle(0, ops.m, ops.k, pa, ia, vals(va)), Handle(0, ops.k, ops.n, pb, ib, vals(vb))

        tr = (T, H) if t == "z" else (T,)
        pairs = [(N, N, every, 0, 1)] + [p for o in tr for p in ((o, N, light, 0, 0), (N, o, light, 0, 0), (o, o, every, 1, 0))]
        for oa, ob, ops, ix, iy in pairs:  # A * B, A^T * A, A * A^T, B^T * A^T
            h = fresh(ops)
            case("sp2m(%s,%s)" % (names[oa], names[ob]), t,
                 lambda rq, r: L.aoclsparse_sp2m(oa, d0.h, h[ix].h, ob, d0.h, h[iy].h, rq, ctypes.byref(r.h)))
        # a result handle as the transposed operand: (A B)^T * A
        h = fresh(every)
        C0 = Result()
        assert L.aoclsparse_sp2m(N, d0.h, h[0].h, N, d0.h, h[1].h, FULL, ctypes.byref(C0.h)) == 0
        for o in tr:
            case("sp2m(%s,N) of a result handle" % names[o], t,
                 lambda rq, r: L.aoclsparse_sp2m(o, d0.h, C0.h, N, d0.h, h[0].h, rq, ctypes.byref(r.h)))
        for shape in S.SHAPES:
            for csc in (False, True):
                m, n, ptr, ind, val = S.arrays(shape, csc, t)
                for op in S.legal_ops(t):
                    Hd = Handle(0, m, n, ptr, ind, val, csc=csc)
                    path = "dense rows" if S.takes_dense_row_path(csc, op, m, n, len(ind)) else "walk"
                    name = "syrk(%s) %s %dx%d %s" % (names[op], "csc" if csc else "csr", m, n, path)
                    case(name, t, lambda rq, r: L.aoclsparse_syrk(op, Hd.h, ctypes.byref(r.h)), requests[:1])  # (no request argument)
        for shape in S.SHAPES[:2]:
            for csc in (False, True):
                m, n, ptr, ind, val = S.arrays(shape, csc, t)
                for op in S.legal_ops(t):
                    for lower in (True, False):
                        k = n if op == N else m
                        bptr, bind, _, bval = S.b_input(k, t, lower)
                        Hd, Bh = Handle(0, m, n, ptr, ind, val, csc=csc), Handle(1, k, k, bptr + 1, bind + 1, bval)
                        d = sym_descr(t, 1, P.FILL_LOWER if lower else P.FILL_UPPER)
                        name = "sypr(%s) %s %dx%d %s" % (names[op], "csc" if csc else "csr", m, n, "lower" if lower else "upper")
                        case(name, t, lambda rq, r: L.aoclsparse_sypr(op, Hd.h, Bh.h, d.h, ctypes.byref(r.h), rq))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "hashes"
    products() if mode == "products" else main(mode)
