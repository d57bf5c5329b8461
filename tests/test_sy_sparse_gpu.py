"""aoclsparse_syrk / aoclsparse_sypr on the GPU against the restatement of tests/test_sy_sparse_cpu.py.

Structure (shape, base, nnz, row_ptr, col_ind in order) must equal the restatement for all four types, both bases, handles made
from CSR and from CSC arrays and every legal op.  Values: double precision bit for bit; the other three types within the
componentwise bound |got - exact| <= (L + 4) u S of tests/test_sy_dense_gpu.py with alpha = 1, beta = 0: S the same product
formed from absolute values, L the longest chain (for sypr the sum of the two nested chains: the longest row of op(A) plus the
longest row of the symmetrised B with its inserted diagonal zeros), u the real type's epsilon, doubled for complex types;
`exact` is evaluated one precision up.  The single and complex-single structures are those of the double restatements of the same
pattern (the pattern does not depend on the values: nothing cancels on random data)."""
import functools
import glob
import os
import subprocess

import numpy as np
import pytest

from test_sy_dense_gpu import WIDER, pattern, values
from test_sy_sparse_cpu import (COUNT, DT, FINAL, FULL, H, KATS, N, OPS, T, TYPES, Handle, check_against_dense, export, herm, kat_handle,
                                restated_sypr, restated_syrk, sym_descr, symmetric_input, sypr, syrk, takes_dense_row_path, values_of)
from util import ROOT, pkg

pytestmark = pytest.mark.gpu
P = pkg()
SHAPES = ((45, 70), (70, 45), (20, 60))
IDS = ["45x70", "70x45", "20x60"]
WIDE = {"s": "d", "c": "z", "d": "d", "z": "z"}  # whose restatement gives a type its structure


@functools.lru_cache(maxsize=None)
def stored(shape, t):
    """zero-based sorted CSR arrays of a shape[0] x shape[1] matrix: the patterns of tests/test_sy_dense_gpu.py; 20 x 60 holds 12
    to 15 entries in every row, so that nnz > 10 m keeps it off the dense-row path although m < n (60 x 20, whose arrays serve as
    the CSC arrays of a 20 x 60 matrix: 4 or 5 per row)"""
    m, n = shape
    if 20 in shape:
        rng = np.random.default_rng(100 * m + n)
        lo, hi = (12, 16) if n == 60 else (4, 6)
        rows = [sorted(rng.choice(n, size=int(rng.integers(lo, hi)), replace=False).tolist()) for _ in range(m)]
        ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        ind = np.array([c for r in rows for c in r], np.int32)
    else:
        ptr, ind = pattern(m, n)
    return ptr, ind, values(len(ind), DT[t], m)


def arrays(shape, csc, t):
    """-> (caller's m, n, ptr, ind, val): csc hands the CSR arrays of the n x m pattern out as col_ptr / row_ind of an m x n matrix"""
    m, n = shape
    return (m, n) + (stored((n, m), t) if csc else stored(shape, t))


@functools.lru_cache(maxsize=None)
def syrk_ref(shape, csc, t, op):
    m, n, ptr, ind, val = arrays(shape, csc, t)
    return restated_syrk(op, csc, m, n, 0, ptr, ind, val)


def dense_of(shape, csc, t):
    """the caller's m x n matrix, one precision up"""
    m, n, ptr, ind, val = arrays(shape, csc, t)
    sm, sn = (n, m) if csc else (m, n)
    D = np.zeros((sm, sn), WIDER[np.dtype(DT[t])])
    np.add.at(D, (np.repeat(np.arange(sm), np.diff(ptr)), ind), val)
    return D.T if csc else D


def legal_ops(t):
    return (N, H) if t in "cz" else (N, T, H)


def ref_op(t, op):
    """on real types op = H is op = T: one restatement serves both"""
    return T if op == H and t in "sd" else op


def same_structure(x, ref, base):
    mc, _, ptr, ind, _ = ref
    assert (x["m"], x["n"], x["base"], x["nnz"]) == (mc, mc, base, len(ind))
    assert np.array_equal(x["row_ptr"], ptr + base) and np.array_equal(x["col_ind"], ind + base)


@pytest.mark.parametrize("csc", [False, True], ids=["csr", "csc"])
@pytest.mark.parametrize("t,dt", TYPES, ids=[t for t, _ in TYPES])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_syrk_equals_the_restatement(shape, t, dt, csc):
    m, n, ptr, ind, val = arrays(shape, csc, t)
    # which path the calls below take (syrk.hpp:221): the branch condition itself is asserted
    assert takes_dense_row_path(False, N, 45, 70, len(stored((45, 70), t)[1]))
    assert 20 < 60 and len(stored((20, 60), t)[1]) > 10 * 20 and not takes_dense_row_path(False, N, 20, 60, len(stored((20, 60), t)[1]))
    assert not takes_dense_row_path(False, N, 70, 45, len(stored((70, 45), t)[1]))
    A = dense_of(shape, csc, t)
    for base in (0, 1):
        Hd = Handle(base, m, n, ptr + base, ind + base, val, csc=csc)
        for op in legal_ops(t):
            st, r = syrk(op, Hd.h)
            assert st == "success", (base, op, st)
            x = export(r.h, t)
            ref = syrk_ref(shape, csc, WIDE[t], ref_op(t, op))
            same_structure(x, ref, base)
            if t == "d":
                assert np.array_equal(x["val"], ref[4]), (base, op)
            left = A if op == N else A.conj().T
            chain = np.count_nonzero(left, axis=1).max()
            check_against_dense((x["m"], base, x["row_ptr"], x["col_ind"], x["val"]), left @ left.conj().T,
                                (np.abs(left) @ np.abs(left).T).astype(np.float64), chain, dt)
    if t in "cz":
        st, r = syrk(T, Hd.h)
        assert st == "not_implemented" and not r.h


def star(k, t):
    """k rows {0, r + 1} on k + 1 columns"""
    ptr = np.arange(0, 2 * k + 1, 2, dtype=np.int32)
    ind = np.stack([np.zeros(k, np.int32), np.arange(1, k + 1, dtype=np.int32)], axis=1).ravel()
    return ptr, ind, values(2 * k, DT[t], k)


@pytest.mark.parametrize("t", ["d", "c"])
@pytest.mark.parametrize("k", [300, 2100, 8200])
def test_star_matrix_covers_every_bin(k, t):
    """A^H A of the star: row 0 of C holds all k + 1 columns in the order 0, k, k - 1, ..., 1 (the walk visits the rows that hold
    column 0 from the last one pushed), every other row holds its diagonal only.  The bins of spgemm_hash_kernel (list capacity 32 /
    256 / 2,048 in LDS, 8,192 in the count pass only, a global slab above):
      k = 300:   row 0, 301 entries: the 2,048 bin in both passes;
      k = 2100:  row 0, 2,101 entries: the 8,192 bin of the count pass, the global slab of the fill pass (above the largest LDS
                 capacity of a fill, 2,048);
      k = 8200:  row 0, 8,201 entries: the global slab in both passes;
      every k:   rows 1 .. k: one entry, the 32 bin.
    The 256 bin is taken by the 70 x 45 pattern (column 5 sits in 67 rows: rows of C hold up to 38 columns).  Handles: CSR with
    op = T / H, and the same arrays as the CSC arrays of the transpose with op = none."""
    ptr, ind, val = star(k, t)
    cplx = t == "c"
    ref = restated_syrk(H, False, k, k + 1, 0, ptr, ind, val.astype(DT[WIDE[t]]))
    assert ref[3][:k + 1].tolist() == [0] + list(range(k, 0, -1)) and ref[2][1] == k + 1 and (np.diff(ref[2][1:]) == 1).all()
    W = WIDER[np.dtype(DT[t])]
    col0, rest = val[0::2].astype(W), val[1::2].astype(W)
    for csc, op in ((False, H if cplx else T), (True, N)):
        Hd = Handle(0, k + 1 if csc else k, k if csc else k + 1, ptr, ind, val, csc=csc)
        st, r = syrk(op, Hd.h)
        assert st == "success"
        x = export(r.h, t)
        # CSR, op = H: A^H A; the same arrays as CSC arrays, op = none: A' A'^H with A' = A^T, i.e. A^T conj(A), its conjugate
        refc = ref if not csc else restated_syrk(N, True, k + 1, k, 0, ptr, ind, val.astype(DT[WIDE[t]]))
        same_structure(x, refc, 0)
        if t == "d":
            assert np.array_equal(x["val"], refc[4])
        # exact: C(0,0) = sum |a_r0|^2, C(0,j) = conj(a_{j-1,0}) a_{j-1,j}, C(j,j) = |a_{j-1,j}|^2 (conjugated for the CSC call)
        u = float(np.finfo(DT[t]).eps) * (2 if cplx else 1)
        got = x["val"].astype(W)
        first = (col0.conj()[::-1] * rest[::-1])
        diag = np.abs(rest) ** 2
        if csc:
            first = first.conj()
        assert abs(got[0] - np.sum(np.abs(col0) ** 2)) <= (k + 4) * u * float(np.sum(np.abs(col0) ** 2))
        assert (np.abs(got[1:k + 1] - first) <= 5 * u * np.abs(first)).all()
        assert (np.abs(got[k + 1:] - diag) <= 5 * u * diag).all()


def test_a_cancelled_sum_is_kept_by_the_walk_and_dropped_by_the_dense_rows():
    """rows 0 and 1 share two columns whose products are +1 and -1"""
    ptr, ind, val = np.array([0, 2, 4, 5], np.int32), np.array([0, 1, 0, 1, 2], np.int32), np.array([1.0, 1.0, 1.0, -1.0, 1.0])
    wide, tall = Handle(0, 3, 4, ptr, ind, val), Handle(0, 3, 3, ptr, ind, val)
    assert takes_dense_row_path(False, N, 3, 4, 5) and not takes_dense_row_path(False, N, 3, 3, 5)
    st, r = syrk(N, wide.h)
    x = export(r.h, "d")
    assert st == "success" and x["row_ptr"].tolist() == [0, 1, 2, 3] and x["col_ind"].tolist() == [0, 1, 2]
    assert x["val"].tolist() == [2.0, 2.0, 1.0]
    st, r = syrk(N, tall.h)
    x = export(r.h, "d")
    assert st == "success" and x["row_ptr"].tolist() == [0, 2, 3, 4] and x["col_ind"].tolist() == [0, 1, 1, 2]
    assert x["val"].tolist() == [2.0, 0.0, 2.0, 1.0]


# ---- sypr ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def b_input(k, t, lower):
    """k x k, fully sorted, entries in both triangles, no entry on three diagonals; the triangle that must not be read holds NaN"""
    ptr, ind, val = symmetric_input(k, k, 0, DT[t], missing=(1, 4, k - 2))
    rows = np.repeat(np.arange(k), np.diff(ptr))
    unread = ind > rows if lower else ind < rows
    poisoned = val.copy()
    poisoned[unread] = np.nan
    return ptr, ind, val, poisoned


@functools.lru_cache(maxsize=None)
def sypr_ref(shape, csc, t, op, lower):
    m, n, ptr, ind, val = arrays(shape, csc, t)
    k = n if op == N else m
    bptr, bind, _, bval = b_input(k, t, lower)
    ref, Tm = restated_sypr(op, (csc, m, n, 0, ptr, ind, val), (k, 0, bptr, bind, bval), lower)
    assert not np.isnan(ref[4].real).any() and not np.isnan(ref[4].imag).any()
    return ref


@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("csc", [False, True], ids=["csr", "csc"])
@pytest.mark.parametrize("t,dt", TYPES, ids=[t for t, _ in TYPES])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=IDS[:2])
def test_sypr_equals_the_restatement(shape, t, dt, csc, lower):
    m, n, ptr, ind, val = arrays(shape, csc, t)
    A = dense_of(shape, csc, t)
    fill = P.FILL_LOWER if lower else P.FILL_UPPER
    for base in (0, 1):
        Hd = Handle(base, m, n, ptr + base, ind + base, val, csc=csc)
        for op in legal_ops(t):
            k = n if op == N else m
            bptr, bind, bclean, bval = b_input(k, t, lower)
            bbase = 1 - base
            Bh = Handle(bbase, k, k, bptr + bbase, bind + bbase, bval)
            d = sym_descr(t, bbase, fill)
            ref = sypr_ref(shape, csc, WIDE[t], ref_op(t, op), lower)
            # the three request sequences give the same C: full; count then finalize; finalize again on that C
            st, full = sypr(op, Hd.h, Bh.h, d.h, FULL)
            assert st == "success", (base, op, st)
            x = export(full.h, t)
            same_structure(x, ref, 0)
            st, two = sypr(op, Hd.h, Bh.h, d.h, COUNT)
            assert st == "success" and two.h
            c = export(two.h, t)
            assert (c["m"], c["n"], c["nnz"], c["base"]) == (x["m"], x["n"], x["nnz"], 0) and np.array_equal(c["row_ptr"], x["row_ptr"])
            for _ in range(2):
                st, same = sypr(op, Hd.h, Bh.h, d.h, FINAL, two)
                assert st == "success" and same is two
                y = export(two.h, t)
                assert np.array_equal(y["row_ptr"], x["row_ptr"]) and np.array_equal(y["col_ind"], x["col_ind"])
                assert np.array_equal(y["val"].view(np.uint8), x["val"].view(np.uint8))
            if t == "d":
                assert np.array_equal(x["val"], ref[4]), (base, op)
            W = WIDER[np.dtype(dt)]
            Bd = np.zeros((k, k), W)
            np.add.at(Bd, (np.repeat(np.arange(k), np.diff(bptr)), bind), bclean)
            Bs = herm(Bd, lower)
            left = A if op == N else A.conj().T
            chain = np.count_nonzero(left, axis=1).max() + np.count_nonzero(Bs, axis=1).max() + 1
            check_against_dense((x["m"], 0, x["row_ptr"], x["col_ind"], x["val"]), left @ Bs @ left.conj().T,
                                (np.abs(left) @ np.abs(Bs) @ np.abs(left).T).astype(np.float64), chain, dt)
    if t in "cz":
        st, r = sypr(T, Hd.h, Bh.h, d.h, FULL)
        assert st == "not_implemented" and not r.h


def test_rows_that_repeat_a_column_give_the_complete_product():
    """the 3 x 4 case of tests/test_sy_dense_gpu.py: rows 0 and 2 repeat a column.  Outside the parity contract: the complete
    product, within (9 + 4) u S (nine stored entries bound every chain of syrk; sypr adds the four of B's longest row)"""
    rng = np.random.default_rng(9)
    dptr = np.array([0, 4, 6, 9], np.int32)
    dind = np.array([0, 1, 1, 3, 1, 2, 0, 3, 3], np.int32)
    dval = rng.uniform(-1, 1, 9)
    R = Handle(0, 3, 4, dptr, dind, dval)
    D = np.zeros((3, 4), np.longdouble)
    np.add.at(D, (np.repeat(np.arange(3), np.diff(dptr)), dind), dval)
    for op, k in ((N, 3), (T, 4)):
        left = D if op == N else D.T
        st, r = syrk(op, R.h)
        assert st == "success"
        x = export(r.h, "d")
        check_against_dense((k, 0, x["row_ptr"], x["col_ind"], x["val"]), left @ left.T, (np.abs(left) @ np.abs(left).T).astype(np.float64),
                            9, np.float64)
        kb = 4 if op == N else 3
        bptr, bind, bval = symmetric_input(kb, kb, 0, np.float64, missing=(1,))
        Bd = np.zeros((kb, kb), np.longdouble)
        np.add.at(Bd, (np.repeat(np.arange(kb), np.diff(bptr)), bind), bval)
        Bs = herm(Bd, True)
        Bh = Handle(0, kb, kb, bptr, bind, bval)
        st, r = sypr(op, R.h, Bh.h, sym_descr("d").h, FULL)
        assert st == "success"
        x = export(r.h, "d")
        check_against_dense((k, 0, x["row_ptr"], x["col_ind"], x["val"]), left @ Bs @ left.T,
                            (np.abs(left) @ np.abs(Bs) @ np.abs(left).T).astype(np.float64), 9 + 4, np.float64)


def test_the_reference_examples_data_through_the_library():
    k = next(c for c in KATS["syrk"] if c["name"] == "sample_dsyrk")
    Hd, _ = kat_handle("d", k)
    st, r = syrk(OPS[k["op"]], Hd.h)
    x, e = export(r.h, "d"), k["expect"]
    assert st == "success" and x["row_ptr"].tolist() == e["row_ptr"] and x["col_ind"].tolist() == e["col_ind"]
    assert np.abs(x["val"] - np.array(e["val"])).max() <= e["tol"]
    k = next(c for c in KATS["sypr"] if c["name"] == "sample_zsypr")
    Ak, _ = kat_handle("z", k["A"])
    Bk, _ = kat_handle("z", dict(k["B"], csc=False))
    st, r = sypr(OPS[k["op"]], Ak.h, Bk.h, sym_descr("z").h, FULL)
    x, e = export(r.h, "z"), k["expect"]
    assert st == "success" and x["row_ptr"].tolist() == e["row_ptr"] and x["col_ind"].tolist() == e["col_ind"]
    d = x["val"] - values_of("z", e["val"])
    assert max(np.abs(d.real).max(), np.abs(d.imag).max()) <= e["tol"]


def test_reference_samples_built_and_pass():
    d = os.path.join(ROOT, "oracle", "_ref", "samples")
    if not glob.glob(os.path.join(d, "sample_*")):
        return  # no reference on the build machine: nothing was built (test_reference_samples_run_unchanged says the same)
    for name in ("sample_dsyrk", "sample_zsypr"):
        exe = os.path.join(d, name)
        assert os.path.exists(exe), name
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.stdout[-400:], r.stderr[-400:])
