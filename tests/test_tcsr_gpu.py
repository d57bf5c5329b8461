"""TCSR handles on the GPU: the general product bit for bit in the order of the reference's aoclsparse_dtcsrmv_avx2
(level2/aoclsparse_tcsrmv.cpp:61-145), the one-triangle products within the CSR path's bound, the solves bit for bit on the
triangle's arrays, stale state after a value change, and the reference's three TCSR samples."""
import ctypes
import glob
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import oracle
from util import EPS32, EPS64, ROOT, kt_lanes, laplace5, pkg, triangular_system, trsv_schedule

pytestmark = pytest.mark.gpu
P = pkg()
L = P.lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fma(a, b, c):
    """correctly rounded a * b + c (exact rational arithmetic, one rounding)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def split(rp, ci, v, base):
    """sorted CSR with a full diagonal -> (ptr_L, col_L, val_L, ptr_U, col_U, val_U): the diagonal ends L's rows and starts U's"""
    m = len(rp) - 1
    rows = np.repeat(np.arange(m), np.diff(rp))
    lo, up = (ci - base) <= rows, (ci - base) >= rows
    pl = np.concatenate([[0], np.cumsum(np.bincount(rows[lo], minlength=m))]) + base
    pu = np.concatenate([[0], np.cumsum(np.bincount(rows[up], minlength=m))]) + base
    return pl.astype(np.int32), ci[lo].copy(), v[lo].copy(), pu.astype(np.int32), ci[up].copy(), v[up].copy()


# ---- the general product --------------------------------------------------------------------------------------------------
NL = (1, 2, 3, 4, 5, 8, 9)  # entries of L's row, diagonal included
NU = (0, 1, 3, 4, 5, 7, 8)  # entries of U's row behind the diagonal


def tcsr_rows(m, base, seed):
    """row i wants (NL, NU)[i mod 49] entries, cut to what fits left and right of the diagonal; columns random, sorted"""
    rng = np.random.default_rng(seed)
    pl, pu, cl, cu, want = [0], [0], [], [], []
    for i in range(m):
        nl, nu = min(NL[i % 7], i + 1), min(NU[(i // 7) % 7], m - 1 - i)
        cl += sorted(rng.choice(i, nl - 1, replace=False).tolist()) + [i]
        cu += [i] + sorted((i + 1 + rng.choice(m - 1 - i, nu, replace=False)).tolist())
        pl.append(len(cl)), pu.append(len(cu)), want.append((nl, nu))
    vl, vu = rng.uniform(-1, 1, len(cl)), rng.uniform(-1, 1, len(cu))
    return (np.array(pl, np.int32) + base, np.array(cl, np.int32) + base, vl, np.array(pu, np.int32) + base,
            np.array(cu, np.int32) + base, vu, want)


def expected_rows(m, base, pl, cl, vl, pu, cu, vu, x):
    """the row sums before alpha and beta, in the order stated in tcsr_kernels.hip / the issue"""
    out = np.zeros(m)
    for i in range(m):
        lanes, r = [0.0] * 4, 0.0
        s, e = pl[i] - base, pl[i + 1] - base
        full_l = (e - s) // 4 * 4
        for j in range(s, s + full_l):
            lanes[(j - s) % 4] = fma(vl[j], x[cl[j] - base], lanes[(j - s) % 4])
        for j in range(s + full_l, e):
            r = fma(vl[j], x[cl[j] - base], r)
        s, e = pu[i] - base + 1, pu[i + 1] - base
        full_u = (e - s) // 4 * 4
        for j in range(s, s + full_u):
            lanes[(j - s) % 4] = fma(vu[j], x[cu[j] - base], lanes[(j - s) % 4])
        if full_l or full_u:
            r = r + ((lanes[0] + lanes[1]) + (lanes[2] + lanes[3]))
        for j in range(s + full_u, e):
            r = fma(vu[j], x[cu[j] - base], r)
        out[i] = r
    return out


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("m", [1, 3, 15, 16, 17, 64, 65, 1000])
def test_general_product_bit_exact(m, base):
    pl, cl, vl, pu, cu, vu, want = tcsr_rows(m, base, 7 * m + base)
    if m == 1000:
        assert {w[0] for w in want} >= set(NL) and {w[1] for w in want} >= set(NU)  # (rows near a corner are cut shorter)
        assert any(w[0] < 4 and w[1] < 4 for w in want) and any(w[0] < 4 <= w[1] for w in want)  # no reduction / only U has a group
    rng = np.random.default_rng(m)
    x, y0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)
    rows = expected_rows(m, base, pl, cl, vl, pu, cu, vu, x)
    A = P.TcsrMatrix(base, m, pl, cl, vl, pu, cu, vu)
    assert A.status == 0
    d = P.Descr(base=base)
    for alpha, beta in ((1.0, 0.0), (-1.5, 0.25), (1.0, 1.0)):
        yin = np.full(m, np.nan) if beta == 0.0 else y0
        ar = alpha * rows
        yref = ar if beta == 0.0 else np.array([fma(beta, yin[i], ar[i]) for i in range(m)])
        y = yin.copy()
        assert P.dmv(P.OP_NONE, alpha, A, d, x, beta, y) == 0
        assert np.array_equal(y, yref), (alpha, beta, "host", int(np.sum(y != yref)))
        xd, yd = dev(x), dev(yin)
        assert P.dmv(P.OP_NONE, alpha, A, d, xd, beta, yd) == 0
        torch.cuda.synchronize()
        assert np.array_equal(yd.cpu().numpy(), yref), (alpha, beta, "device")
    info = A.spmv_info()
    assert info.kernel == 5 and info.device_resident == 1
    if m == 1000:
        # the test can tell the orders apart: the plain chain and the four-lane order over the merged row give other bits
        keep = np.ones(len(cu), bool)
        keep[pu[:-1] - base] = False
        lens = np.diff(pl) + np.diff(pu) - 1
        rp = (np.concatenate([[0], np.cumsum(lens)]) + base).astype(np.int32)
        ci, v = np.empty(rp[-1] - base, np.int32), np.empty(rp[-1] - base)
        cuk, vuk, puk = cu[keep], vu[keep], np.concatenate([[0], np.cumsum(np.diff(pu) - 1)])
        for i in range(m):
            a, nl = rp[i] - base, pl[i + 1] - pl[i]
            ci[a:a + nl], v[a:a + nl] = cl[pl[i] - base:pl[i + 1] - base], vl[pl[i] - base:pl[i + 1] - base]
            ci[a + nl:rp[i + 1] - base], v[a + nl:rp[i + 1] - base] = cuk[puk[i]:puk[i + 1]], vuk[puk[i]:puk[i + 1]]
        long_rows = lens >= 5
        for kid in (-1, 1):
            so, yo = oracle.dcsrmv(kid, base, 1.0, m, len(v), v, ci, rp, x, 0.0, np.zeros(m))
            assert so == 0
            assert np.sum((yo != rows)[long_rows]) >= 0.1 * np.sum(long_rows), kid


def test_general_product_follows_the_runtime_stream_and_the_hint():
    m = 65
    pl, cl, vl, pu, cu, vu, _ = tcsr_rows(m, 0, 3)
    A = P.TcsrMatrix(0, m, pl, cl, vl, pu, cu, vu)
    d = P.Descr()
    assert L.aoclsparse_set_mv_hint(A.h, P.OP_NONE, d.h, 100) == 0 and L.aoclsparse_optimize(A.h) == 0
    assert A.spmv_info().device_resident == 1  # the hint put both triangles in HBM
    x = np.random.default_rng(1).uniform(-1, 1, m)
    rows = expected_rows(m, 0, pl, cl, vl, pu, cu, vu, x)
    yd, dd = dev(np.zeros(m)), np.zeros(1)
    assert L.aoclsparse_ddotmv(P.OP_NONE, 1.0, A.h, d.h, P._ptr(dev(x)), 0.0, P._ptr(yd), P._ptr(dd)) == 0  # dotmv.hpp:47: mv, then a dot
    torch.cuda.synchronize()
    assert np.array_equal(yd.cpu().numpy(), rows)


# ---- symmetric / triangular products on one triangle --------------------------------------------------------------------------
def lap_tcsr(g, base, dtype=np.float64):
    m, rp, ci, v = laplace5(g, base)
    rng = np.random.default_rng(g)
    v = v * rng.uniform(0.9, 1.1, len(v))
    if dtype == np.complex128:
        v = v + 1j * rng.uniform(-0.3, 0.3, len(v))
    return (m,) + split(rp, ci, v.astype(dtype), base)


def tri_args(fill, pl, pu):
    """(ptr, idiag, iurow) of the triangle a fill mode names (level2/aoclsparse_tcsr.hpp:79-94)"""
    if fill == P.FILL_LOWER:
        return pl, pl[1:] - 1, pl[1:]
    return pu, pu[:-1], pu[:-1] + 1


def dense_of(m, base, ptr, col, val):
    D = np.zeros((m, m), val.dtype)
    D[np.repeat(np.arange(m), np.diff(ptr)), col - base] = val
    return D


@pytest.mark.parametrize("fill", [P.FILL_LOWER, P.FILL_UPPER])
@pytest.mark.parametrize("diag", [P.DIAG_NON_UNIT, P.DIAG_UNIT])
def test_symmetric_and_triangular_products_double(fill, diag):
    base = fill  # both bases over the four cases
    m, pl, cl, vl, pu, cu, vu = lap_tcsr(30, base)
    A = P.TcsrMatrix(base, m, pl, cl, vl, pu, cu, vu)
    ptr, idiag, iurow = tri_args(fill, pl, pu)
    col, val = (cl, vl) if fill == P.FILL_LOWER else (cu, vu)
    D = dense_of(m, base, ptr, col, val)
    strict = np.tril(D, -1) if fill == P.FILL_LOWER else np.triu(D, 1)
    dg = np.diag(np.diag(D)) if diag == P.DIAG_NON_UNIT else np.eye(m)
    rng = np.random.default_rng(2)
    x, y0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)
    alpha, beta = 1.7, -0.4
    for mtype in (P.TYPE_SYMMETRIC, P.TYPE_TRIANGULAR):
        d = P.Descr(base=base, mtype=mtype, fill=fill, diag=diag)
        for op in (P.OP_NONE, P.OP_TRANSPOSE):
            yd = dev(y0)
            assert P.dmv(op, alpha, A, d, dev(x), beta, yd) == 0
            torch.cuda.synchronize()
            y = yd.cpu().numpy()
            if mtype == P.TYPE_SYMMETRIC:
                M, kind = strict + strict.T + dg, "symm"
            else:
                M, kind = (strict + dg if op == P.OP_NONE else (strict + dg).T), ("tri" if op == P.OP_NONE else "tri_t")
            so, yo = oracle.dcsrmv_special(kind, base, alpha, m, m, diag, fill, val, col, ptr, idiag, iurow, x, beta, y0)
            assert so == 0
            lens = (M != 0).sum(axis=1)
            bound = (lens + 6) * EPS64 * (abs(alpha) * (np.abs(M) @ np.abs(x)) + np.abs(beta * y0)) + 1e-300
            print("dmv", fill, diag, mtype, op, "max err / bound", np.max(np.abs(y - yo) / bound))
            assert np.all(np.abs(y - yo) <= bound), (mtype, op, np.max(np.abs(y - yo) / bound))


@pytest.mark.parametrize("fill", [P.FILL_LOWER, P.FILL_UPPER])
def test_symmetric_and_triangular_products_complex(fill):
    base = 1 - fill
    m, pl, cl, vl, pu, cu, vu = lap_tcsr(30, base, np.complex128)
    AG = P.TcsrMatrix(base, m, pl, cl, vl, pu, cu, vu)
    # for the Hermitian descriptor: the same triangles with a real diagonal (a Hermitian matrix has one)
    vlh, vuh = vl.copy(), vu.copy()
    vlh[pl[1:] - 1 - base], vuh[pu[:-1] - base] = vlh[pl[1:] - 1 - base].real, vuh[pu[:-1] - base].real
    AH = P.TcsrMatrix(base, m, pl, cl, vlh, pu, cu, vuh)
    assert AG.status == 0 and AH.status == 0
    ptr = pl if fill == P.FILL_LOWER else pu
    col, valg, valh = (cl, vl, vlh) if fill == P.FILL_LOWER else (cu, vu, vuh)
    rng = np.random.default_rng(4)
    x = rng.uniform(-1, 1, m) + 1j * rng.uniform(-1, 1, m)
    y0 = rng.uniform(-1, 1, m) + 1j * rng.uniform(-1, 1, m)
    alpha, beta = 1.7 - 0.3j, -0.4 + 0.2j
    a, b = np.array([alpha]), np.array([beta])
    lens = np.diff(ptr)
    for diag, dname in ((P.DIAG_NON_UNIT, "non_unit"), (P.DIAG_UNIT, "unit")):
        # (Hermitian descriptors and the conjugate-transposed symmetric product run on the triangle as on a CSR handle)
        for mtype, tname, ops in ((P.TYPE_SYMMETRIC, "symmetric", "nth"), (P.TYPE_TRIANGULAR, "triangular", "nt"),
                                  (P.TYPE_HERMITIAN, "hermitian", "nth")):
            d = P.Descr(base=base, mtype=mtype, fill=fill, diag=diag)
            A, val = (AH, valh) if mtype == P.TYPE_HERMITIAN else (AG, valg)
            for op in ops:
                yd = dev(y0)
                st = L.aoclsparse_zmv({"n": P.OP_NONE, "t": P.OP_TRANSPOSE, "h": P.OP_CONJ_TRANSPOSE}[op], P._ptr(a), A.h, d.h, P._ptr(dev(x)), P._ptr(b), P._ptr(yd))
                assert st == 0, P.STATUS[st]
                torch.cuda.synchronize()
                yo, scale = oracle.zmv(op, tname, "lower" if fill == P.FILL_LOWER else "upper", dname, base, alpha, m, m, ptr, col, val, x, beta, y0)
                rowlen = 2 * lens if mtype != P.TYPE_TRIANGULAR else (lens if op == "n" else np.bincount(col - base, minlength=m))
                bound = (rowlen + 6) * EPS64 * scale + 1e-300
                err = np.abs(yd.cpu().numpy() - yo)
                print("zmv", fill, dname, tname, op, "max err / bound", np.max(err / bound))
                assert np.all(err <= bound), (tname, op, np.max(err / bound))


# ---- solves ---------------------------------------------------------------------------------------------------------------------
KIND = {(P.FILL_LOWER, P.OP_NONE): "l", (P.FILL_LOWER, P.OP_TRANSPOSE): "lt", (P.FILL_UPPER, P.OP_NONE): "u", (P.FILL_UPPER, P.OP_TRANSPOSE): "ut"}


def oracle_solve(T, fill, op, unit, alpha, b, kid=None, dtype=np.float64, **kw):
    """the reference's chain on the triangle's arrays (level2/aoclsparse_trsv.cpp:158-176)"""
    m, base, pl, cl, vl, pu, cu, vu = T
    if fill == P.FILL_LOWER:
        a, icol, ilrow, ilend = vl, cl, pl, pl[1:] - 1
    else:
        a, icol, ilrow, ilend = vu, cu, pu, pu[:-1] + 1
    lanes = kt_lanes(kid, dtype)
    if lanes:
        st, x = oracle.trsv_kt(KIND[(fill, op)], lanes, alpha, m, base, a, icol, ilrow, ilend, b, unit, dtype=dtype, **kw)
    else:
        st, x = (oracle.dtrsv if dtype == np.float64 else oracle.strsv)(KIND[(fill, op)], alpha, m, base, a, icol, ilrow, ilend, b, unit, **kw)
    assert st == 0
    return x


@pytest.fixture(scope="module")
def system():
    """a banded system with rows of up to 12 entries as L and U, both bases; built once, never written"""
    out = {}
    for base in (0, 1):
        m = 3000
        rp, ci, v = triangular_system(51, m, 6, base=base, band=100)
        out[base] = (m, base) + split(rp, ci, v, base)
    return out


@pytest.mark.parametrize("kid", [None, -1, 0, 1, 3])  # None: the plain ?trsv entry point; -1 .. 3: ?trsv_kid
@pytest.mark.parametrize("fill", [P.FILL_LOWER, P.FILL_UPPER])
def test_trsv_double_bit_exact(system, fill, kid):
    for base in (0, 1):
        T = system[base]
        m = T[0]
        A = P.TcsrMatrix(base, m, *T[2:])
        b = np.random.default_rng(5).uniform(-1, 1, m)
        for op in (P.OP_NONE, P.OP_TRANSPOSE):
            for unit in (False, True):
                d = P.Descr(base=base, mtype=P.TYPE_TRIANGULAR if base == 0 else P.TYPE_SYMMETRIC, fill=fill,
                            diag=P.DIAG_UNIT if unit else P.DIAG_NON_UNIT)
                xr = oracle_solve(T, fill, op, unit, 1.3, b, kid=kid)
                xd = dev(np.zeros(m))
                assert P.dtrsv(op, 1.3, A, d, dev(b), xd, kid=kid) == 0
                torch.cuda.synchronize()
                assert np.array_equal(xd.cpu().numpy(), xr), (base, op, unit)
        x = np.zeros(m)  # host operands
        d = P.Descr(base=base, mtype=P.TYPE_TRIANGULAR, fill=fill)
        assert P.dtrsv(P.OP_NONE, 1.3, A, d, b, x, kid=kid) == 0
        assert np.array_equal(x, oracle_solve(T, fill, P.OP_NONE, False, 1.3, b, kid=kid))


def test_trsv_strided_and_trsm(system):
    T = system[0]
    m = T[0]
    A = P.TcsrMatrix(0, m, *T[2:])
    rng = np.random.default_rng(6)
    for fill in (P.FILL_LOWER, P.FILL_UPPER):
        d = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=fill)
        b = rng.uniform(-1, 1, m)
        bs, xs = np.zeros(3 * m), np.full(2 * m, 7.0)
        bs[::3] = b
        assert P.dtrsv(P.OP_TRANSPOSE, 0.75, A, d, bs, xs, incb=3, incx=2) == 0
        assert np.array_equal(xs[::2], oracle_solve(T, fill, P.OP_TRANSPOSE, False, 0.75, b)) and np.all(xs[1::2] == 7.0)
        n = 3
        Bm = rng.uniform(-1, 1, (m, n))
        cols = [oracle_solve(T, fill, P.OP_NONE, False, 0.5, np.ascontiguousarray(Bm[:, j])) for j in range(n)]
        for order in (P.ORDER_ROW, P.ORDER_COLUMN):
            Bb = np.ascontiguousarray(Bm if order == P.ORDER_ROW else Bm.T)
            Xd = dev(np.zeros_like(Bb))
            ld = n if order == P.ORDER_ROW else m
            assert L.aoclsparse_dtrsm(P.OP_NONE, 0.5, A.h, d.h, order, P._ptr(dev(Bb)), n, ld, P._ptr(Xd), ld) == 0
            torch.cuda.synchronize()
            X = Xd.cpu().numpy()
            for j in range(n):
                assert np.array_equal(X[:, j] if order == P.ORDER_ROW else X[j], cols[j]), (fill, order, j)


def test_trsv_every_schedule_and_the_plan_report():
    """the 'five' node mesh of test_two_level_trsv_bit_exact_every_triangle (the smallest factor on which the existing tests run the
    two-level schedule, with the chunk plan forced as there; schedules 2-4 run on it too): every triangle, every schedule 2-5 forced,
    the bits of the serial chain, and the schedule that ran is the one that was forced"""
    from test_gpu_trsv_blocks import VARIANTS, fixed, node_mesh

    nodes = 12000
    m, rp, ci, v = node_mesh(904, nodes, 37, fixed(5)(np.random.default_rng(1), nodes), far=0)
    o = oracle.dcsr_optimize(m, m, len(v), 0, rp, ci, v)
    T = (m, 0) + split(o["ptr"], o["ind"], o["val"], 0)
    b = np.random.default_rng(5).uniform(-1, 1, m)
    assert L.aoclsparse_mi355_set_option(P.OPTION_TRSV_CHUNKS, 1) == 0
    try:
        A = P.TcsrMatrix(0, m, *T[2:])
        assert A.status == 0
        for kind, fill, op in VARIANTS:
            fill, op = getattr(P, fill), getattr(P, op)
            d = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=fill)
            assert L.aoclsparse_set_sv_hint(A.h, op, d.h, 3) == 0 and L.aoclsparse_optimize(A.h) == 0
            assert 1 < A.trsv_levels(fill, op) < m and A.trsv_info(fill, op).levels == A.trsv_levels(fill, op)
            xr = oracle_solve(T, fill, op, False, 1.3, b)
            bd, xd = dev(b), dev(np.zeros(m))
            for sched in (2, 3, 4, 5):
                with trsv_schedule(P, sched):
                    xd.fill_(7.0)
                    assert P.dtrsv(op, 1.3, A, d, bd, xd) == 0
                    torch.cuda.synchronize()
                    info = A.trsv_info(fill, op)
                assert np.array_equal(xd.cpu().numpy(), xr), (kind, sched)
                assert info.schedule == sched, (kind, sched, info.schedule)
            assert L.aoclsparse_mi355_trsv_status(A.h) == 0
    finally:
        assert L.aoclsparse_mi355_set_option(P.OPTION_TRSV_CHUNKS, -1) == 0


def test_trsv_float_and_complex(system):
    m, base, pl, cl, vl, pu, cu, vu = system[1]
    # float: the chain of oracle.strsv, bit for bit (the standard of tests/test_gpu_float_stack.py)
    F = (m, base, pl, cl, vl.astype(np.float32), pu, cu, vu.astype(np.float32))
    A = P.TcsrMatrix(base, m, *F[2:])
    b = np.random.default_rng(8).uniform(-1, 1, m).astype(np.float32)
    for fill in (P.FILL_LOWER, P.FILL_UPPER):
        for op in (P.OP_NONE, P.OP_TRANSPOSE):
            d = P.Descr(base=base, mtype=P.TYPE_TRIANGULAR, fill=fill)
            xd = dev(np.zeros(m, np.float32))
            assert P.strsv(op, 0.75, A, d, dev(b), xd) == 0
            torch.cuda.synchronize()
            assert np.array_equal(xd.cpu().numpy(), oracle_solve(F, fill, op, False, 0.75, b, dtype=np.float32)), (fill, op)
    # complex: normwise against a dense solve, 64 eps |x| (the standard of test_complex_trsv_trsm)
    rng = np.random.default_rng(9)
    n = 500
    rp, ci, v = triangular_system(31, n, 4, base=base, band=40)
    vz = v + 1j * rng.uniform(-0.3, 0.3, len(v))
    zl = split(rp, ci, vz, base)
    Z = P.TcsrMatrix(base, n, *zl)
    assert Z.status == 0
    bz = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    alpha = 0.8 - 0.6j
    for fill in (P.FILL_LOWER, P.FILL_UPPER):
        D = dense_of(n, base, *(zl[0:3] if fill == P.FILL_LOWER else zl[3:6]))
        for unit in (False, True):
            M0 = D.copy()
            if unit:
                M0[np.arange(n), np.arange(n)] = 1.0
            d = P.Descr(base=base, mtype=P.TYPE_TRIANGULAR, fill=fill, diag=P.DIAG_UNIT if unit else P.DIAG_NON_UNIT)
            for op, M in ((P.OP_NONE, M0), (P.OP_TRANSPOSE, M0.T), (P.OP_CONJ_TRANSPOSE, M0.conj().T)):
                xr = np.linalg.solve(M, alpha * bz)
                x = np.full(n, np.nan + 0j)
                assert L.aoclsparse_ztrsv(op, P.CDouble(alpha.real, alpha.imag), Z.h, d.h, P._ptr(bz), P._ptr(x)) == 0
                assert np.max(np.abs(x - xr)) <= 64 * EPS64 * np.max(np.abs(xr)), (fill, unit, op)


# ---- stale state ---------------------------------------------------------------------------------------------------------------
def test_value_change_in_place_then_invalidate(system):
    m, base, pl, cl, vl, pu, cu, vu = system[0]
    vl, vu = vl.copy(), vu.copy()  # this test writes them
    A = P.TcsrMatrix(base, m, pl, cl, vl, pu, cu, vu)
    g, t = P.Descr(), P.Descr(mtype=P.TYPE_TRIANGULAR, fill=P.FILL_UPPER)
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, m)
    xd, yd, sd = dev(x), dev(np.zeros(m)), dev(np.zeros(m))
    assert L.aoclsparse_set_mv_hint(A.h, P.OP_NONE, g.h, 10) == 0 and L.aoclsparse_set_sv_hint(A.h, P.OP_NONE, t.h, 10) == 0
    assert L.aoclsparse_optimize(A.h) == 0
    assert P.dmv(P.OP_NONE, 1.0, A, g, xd, 0.0, yd) == 0 and P.dtrsv(P.OP_NONE, 1.0, A, t, xd, sd) == 0
    torch.cuda.synchronize()
    old = yd.cpu().numpy().copy()
    A.val_l *= 1.25
    A.val_u *= -0.75
    A.val_l[pl[1:] - 1 - base] = A.val_u[pu[:-1] - base]  # one diagonal in both triangles
    assert L.aoclsparse_mi355_invalidate(A.h) == 0
    assert P.dmv(P.OP_NONE, 1.0, A, g, xd, 0.0, yd) == 0 and P.dtrsv(P.OP_NONE, 1.0, A, t, xd, sd) == 0
    torch.cuda.synchronize()
    rows = expected_rows(m, base, pl, cl, A.val_l, pu, cu, A.val_u, x)
    assert np.array_equal(yd.cpu().numpy(), rows) and not np.array_equal(rows, old)
    T = (m, base, pl, cl, A.val_l, pu, cu, A.val_u)
    assert np.array_equal(sd.cpu().numpy(), oracle_solve(T, P.FILL_UPPER, P.OP_NONE, False, 1.0, x))


# ---- the reference's own TCSR samples ----------------------------------------------------------------------------------------------
def test_reference_tcsr_samples_built_and_pass():
    d = os.path.join(ROOT, "oracle", "_ref", "samples")
    if not glob.glob(os.path.join(d, "sample_*")):
        return  # no reference on the build machine: nothing was built (test_reference_samples_run_unchanged says the same)
    for name in ("sample_tcsr_dspmv", "sample_tcsr_dtrsv", "sample_tcsr_ztrsv"):
        exe = os.path.join(d, name)
        assert os.path.exists(exe), name
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.stdout[-400:], r.stderr[-400:])
