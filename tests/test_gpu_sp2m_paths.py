"""aoclsparse_sp2m on the two operand paths that no other test reaches in staged form, on tiny matrices (40 x 30, 30 x 40 and
40 x 40, at most 8 entries per row, bases 0 and 1).

1. A transposed operand that is a RESULT handle: it owns its arrays, so its transpose is built per call on the host and travels
   through the staging slots, values included only when the request fills.  The same call on a handle made by create_?csr over a
   copy of the same arrays uses the handle's kept transpose and its resident device copy.  Both must give the same bits, as a
   full computation and as count then finalize (the count call of the staged path is the one that sends no values).
2. op(A) * op(A) with op = T (and H on complex types) and A square: computed as (A A)^T, both operands the same arrays, sent
   once.  Full computation, and count then finalize twice on the same C, give the same bits; the full computation is compared
   to the oracle as tests/test_gpu_parity.py::test_complex_sp2m does: row_ptr and col_ind bit for bit those of the oracle's
   product of the patterns (transposed by its csr2csc), double values bit for bit, the other types within (terms + 4) eps of
   the dense product of absolute values (terms <= 8, the longest row).
3. The C of a count-only op(A) * op(A) as a transposed operand: see the last test."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from test_sy_sparse_cpu import COUNT, DT, FINAL, FULL, H, N, T, Handle, Result, export
from util import EPS32, EPS64, pkg, random_csr

pytestmark = pytest.mark.gpu
P = pkg()
L = P.lib()
OPS = {"s": (T,), "d": (T,), "z": (T, H)}


@functools.lru_cache(maxsize=None)
def arrays(seed, m, n, t):
    """zero-based sorted CSR of at most 8 entries per row (shared: never modified)"""
    ptr, ind, vr = random_csr(seed, m, n, lambda r, i: r.integers(0, 9))
    if t == "z":
        return ptr, ind, (vr + 1j * np.random.default_rng(seed + 1000).uniform(-1, 1, len(vr))).astype(DT[t])
    return ptr, ind, vr.astype(DT[t])


def handle(seed, m, n, t, base):
    ptr, ind, val = arrays(seed, m, n, t)
    return Handle(base, m, n, ptr + base, ind + base, val)


def sp2m(opa, da, A, opb, db, B, request, C=None):
    r = C or Result()
    st = L.aoclsparse_sp2m(opa, da.h, A, opb, db.h, B, request, ctypes.byref(r.h))
    assert st == 0, P.STATUS[st]
    return r


def same_bits(x, y):
    return (x["m"], x["n"], x["base"], x["nnz"]) == (y["m"], y["n"], y["base"], y["nnz"]) \
        and np.array_equal(x["row_ptr"], y["row_ptr"]) and np.array_equal(x["col_ind"], y["col_ind"]) \
        and np.array_equal(x["val"].view(np.uint8), y["val"].view(np.uint8))


def dense(x, wide=np.complex128):
    D = np.zeros((x["m"], x["n"]), wide)
    np.add.at(D, (np.repeat(np.arange(x["m"]), np.diff(x["row_ptr"])), x["col_ind"] - x["base"]), x["val"])
    return D


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("t", ["d", "z"])
def test_transposed_result_handle_staged_equals_created_handle_resident(t, base):
    m, k = 40, 30
    A, B, A2 = handle(1, m, k, t, base), handle(2, k, m, t, base), handle(3, m, k, t, base)
    d0, db = P.Descr(base=0), P.Descr(base=base)
    C0 = sp2m(N, db, A.h, N, db, B.h, FULL)  # 40 x 40, zero-based, owns its arrays
    c0 = export(C0.h, t)
    assert (c0["m"], c0["n"], c0["base"]) == (m, m, 0) and c0["nnz"] > m
    R = Handle(0, m, m, c0["row_ptr"], c0["col_ind"], c0["val"])  # aliases the exported copies: keeps its transpose
    for op in OPS[t]:
        got = {}
        for name, h in (("staged", C0.h), ("resident", R.h)):
            full = sp2m(op, d0, h, N, db, A2.h, FULL)
            two = sp2m(op, d0, h, N, db, A2.h, COUNT)
            counted = export(two.h, t)
            assert sp2m(op, d0, h, N, db, A2.h, FINAL, two) is two
            got[name] = (export(full.h, t), counted, export(two.h, t))
        for s, r in zip(got["staged"], got["resident"]):
            assert (s["m"], s["n"], s["base"], s["nnz"]) == (r["m"], r["n"], r["base"], r["nnz"]) == (m, k, 0, s["nnz"])
            assert np.array_equal(s["row_ptr"], r["row_ptr"])
        assert same_bits(got["staged"][0], got["resident"][0]), (op, "full")
        assert same_bits(got["staged"][2], got["resident"][2]), (op, "count + finalize")
        if t == "d":  # C0^T * A2 by the oracle's csr2csc and csr2m
            pa, ia, va = arrays(3, m, k, t)
            st, tp, ti, tv = oracle.dcsr2csc(m, m, c0["nnz"], 0, 0, c0["row_ptr"], c0["col_ind"], c0["val"])
            so, pc, ic, vc = oracle.dcsr2m(m, k, 0, tp, ti.astype(np.int32), tv, 0, pa, ia, va)
            x = got["staged"][0]
            assert st == 0 and so == 0
            assert np.array_equal(x["row_ptr"], pc) and np.array_equal(x["col_ind"], ic) and np.array_equal(x["val"], vc)


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("t", ["d", "s", "z"])
def test_both_operands_transposed_and_the_same_handle(t, base):
    m = 40
    ptr, ind, val = arrays(4, m, m, t)
    A, d = handle(4, m, m, t, base), P.Descr(base=base)
    # the oracle's product of the patterns (real parts), transposed: (A A)^T
    vr = np.ascontiguousarray(val.real, np.float64)
    so, pc, ic, vc = oracle.dcsr2m(m, m, 0, ptr, ind, vr, 0, ptr, ind, vr)
    st, tp, ti, tv = oracle.dcsr2csc(m, m, len(ic), 0, 0, pc, ic, vc)
    assert so == 0 and st == 0 and len(ic) > m
    D = dense(dict(m=m, n=m, base=0, row_ptr=ptr, col_ind=ind, val=val))
    eps = EPS32 if t == "s" else EPS64
    for op in OPS[t]:
        one = sp2m(op, d, A.h, op, d, A.h, FULL)
        full = export(one.h, t)
        two = sp2m(op, d, A.h, op, d, A.h, COUNT)
        c = export(two.h, t)
        assert (c["m"], c["n"], c["base"]) == (m, m, 0)  # (the row pointer of a transposed-back product comes with finalize)
        for _ in range(2):
            assert sp2m(op, d, A.h, op, d, A.h, FINAL, two) is two
            assert same_bits(export(two.h, t), full), op
        assert (full["m"], full["n"], full["base"], full["nnz"]) == (m, m, 0, len(ic))
        assert np.array_equal(full["row_ptr"], tp) and np.array_equal(full["col_ind"], ti)
        if t == "d":
            assert np.array_equal(full["val"], tv)
        X = D.T if op == T else D.conj().T
        bound = (np.abs(X) @ np.abs(X)) * (12 * eps) + 1e-300
        assert np.all(np.abs(dense(full) - X @ X) <= bound), op


def test_a_counted_but_unfilled_transposed_product_is_an_empty_operand():
    """The C of a count-only sp2m(T, T) holds nnz, a row pointer that is still all base and no column indices until finalize.  As a
    transposed operand it is read through its row pointer alone, so it is an empty matrix and the product the valid empty result;
    C itself is left alone and finalizes as usual.  (The one case in this file that the code before the shared host transpose did
    not define: it read the unwritten indices.)"""
    m, k, t = 40, 30, "d"
    A, A2, d = handle(4, m, m, t, 0), handle(3, m, k, t, 0), P.Descr()
    full = sp2m(T, d, A.h, T, d, A.h, FULL)
    C = sp2m(T, d, A.h, T, d, A.h, COUNT)
    E = sp2m(T, d, C.h, N, d, A2.h, FULL)
    e = export(E.h, t)
    assert (e["m"], e["n"], e["base"], e["nnz"]) == (m, k, 0, 0) and not e["row_ptr"].any()
    assert sp2m(T, d, A.h, T, d, A.h, FINAL, C) is C
    assert same_bits(export(C.h, t), export(full.h, t))
