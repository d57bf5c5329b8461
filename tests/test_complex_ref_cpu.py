"""The bounds of tests/complex_ref.py tell a correct result from a subtly wrong one -- shown without a GPU.

For each kind of bound (products, triangular solve, dot product) the operation is computed in the type under test with plain
numpy arithmetic: that result must sit within the bound at ratio <= 0.5 (the bound is not too tight for correct arithmetic),
and each mutation of the computation -- an entry left out, an entry conjugated, a dependency read as zero, a column of B read
one column to the left, the last element of the dot product left out -- must exceed it by more than 100 x (the bound is not
vacuous).  The level-designed generator is checked against the plain level function for both fills."""
import functools

import numpy as np
import pytest

import complex_ref as cr

pytestmark = pytest.mark.parametrize("prec", ["z", "c"])
DTYPE = {"z": np.complex128, "c": np.complex64}
HONEST, BROKEN = 0.5, 100.0


@pytest.mark.parametrize("op", ["n", "h"])
@pytest.mark.parametrize("ncol", [1, 17])  # 1: ?mv, 17: ?csrmm
def test_product_bound_discriminates(prec, op, ncol):
    dtype = DTYPE[prec]
    m, n = 131, 90
    rp, ci, v = cr.product_matrix(dtype, m, n)
    r, c, a, shape = cr.op_coo(*cr.coo(rp, ci, v, 0), (m, n), op)
    rng = np.random.default_rng(3)
    B, C0 = cr.crand(rng, (shape[1], ncol), dtype), cr.crand(rng, (shape[0], ncol), dtype)
    alpha, beta = dtype(0.7 - 0.2j), dtype(-0.4 + 0.3j)
    ref = cr.product(r, c, a, shape, alpha, B, beta, C0, cr.ext_type(dtype))
    scale, p = cr.product_scale(r, c, a, shape, alpha, B, beta, C0)
    bound = cr.product_bound(p, 0, scale, dtype)

    def run(a_=a, r_=r, c_=c, B_=B):
        got = cr.product(r_, c_, a_, shape, alpha, B_, beta, C0, dtype)
        assert got.dtype == dtype
        return cr.ratio(np.abs(got.astype(cr.ext_type(dtype)) - ref), bound)

    honest = run()
    print("product", prec, op, ncol, "honest ratio", honest)
    assert honest <= HONEST
    for e in np.linspace(0, len(a) - 1, 7).astype(int):  # seven stored entries spread over the matrix
        keep = np.arange(len(a)) != e
        left_out = run(a[keep], r[keep], c[keep])
        conj = a.copy()
        conj[e] = np.conj(conj[e])
        conjugated = run(conj)
        stale = B.copy()
        stale[c[e]] = 0  # what row r[e] (and whoever else reads it) depends on is read as zero
        read_zero = run(B_=stale)
        print("  entry", e, "left out", left_out, "conjugated", conjugated, "read as zero", read_zero)
        assert min(left_out, conjugated, read_zero) > BROKEN
    if ncol > 1:
        for j in (1, ncol - 1):
            shifted = B.copy()
            shifted[:, j] = B[:, j - 1]
            col_minus_1 = run(B_=shifted)
            print("  column", j, "of B read at column - 1:", col_minus_1)
            assert col_minus_1 > BROKEN


@functools.lru_cache(maxsize=None)
def designed(prec):
    return cr.level_triangle(cr.DESIGN_WIDTHS, 41, DTYPE[prec], 0)


@pytest.mark.parametrize("fill", ["lower", "upper"])
def test_generator_delivers_the_requested_levels(prec, fill):
    for base in (0, 1):
        rp, ci, v = cr.level_triangle(cr.DESIGN_WIDTHS, 41, DTYPE[prec], base) if base else designed(prec)
        n = len(rp) - 1
        assert n == sum(cr.DESIGN_WIDTHS) == 5225 and v.dtype == DTYPE[prec]
        assert cr.level_widths(rp, ci, base, fill, "n") == list(cr.DESIGN_WIDTHS)
        r, c, a = cr.coo(rp, ci, v, base)
        assert np.all((np.diff(c) > 0) | (np.diff(r) > 0))  # sorted rows, no duplicates
        dg = r == c
        assert dg.sum() == n and np.all((np.abs(a[dg]) > 2.999) & (np.abs(a[dg]) < 4.001))
        assert np.all(np.abs(a[~dg].real) <= 0.5) and np.all(np.abs(a[~dg].imag) <= 0.5)
        tri = r > c if fill == "lower" else r < c
        assert np.bincount(r[tri], minlength=n).max() == 12  # the seed and up to 11 further entries
        # rowmap far from the identity: the rows of one level are spread over the whole index range
        t = cr.TriOp(rp, ci, v, base, fill, "n", False)
        rows7 = np.flatnonzero(t.levels() == 7)
        assert rows7.max() - rows7.min() > n // 2


@pytest.mark.parametrize("fill", ["lower", "upper"])
def test_solve_bound_discriminates(prec, fill):
    dtype = DTYPE[prec]
    rp, ci, v = designed(prec)
    n = len(rp) - 1
    t = cr.TriOp(rp, ci, v, 0, fill, "n", False)
    level = t.levels()
    b = cr.crand(np.random.default_rng(5), (n, 1), dtype)
    alpha = dtype(0.8 - 0.6j)
    ref = t.solve(alpha, b, cr.ext_type(dtype))

    def run(mutate=None):
        tm = cr.TriOp(rp, ci, v, 0, fill, "n", False)
        if mutate:
            mutate(tm)
        got = tm.solve(alpha, b, dtype)
        assert got.dtype == dtype
        return cr.ratio(np.abs(got.astype(cr.ext_type(dtype)) - ref), t.bound(got, dtype))  # the bound of the TRUE operator

    honest = run()
    print("solve", prec, fill, "honest ratio", honest)
    assert honest <= HONEST
    last = np.flatnonzero((level == len(cr.DESIGN_WIDTHS) - 1) & (t.p >= 2))
    for i in last[[0, len(last) // 2, -1]]:  # three rows of the LAST level
        e = t.ptr[i] + 1  # their second stored entry

        def leave_out(tm):
            tm.val = tm.val.copy()
            tm.val[e] = 0  # (a stored entry that contributes nothing: the row is one entry short)

        def conjugate(tm):
            tm.val = tm.val.copy()
            tm.val[e] = np.conj(tm.val[e])

        def stale(tm):  # xp[j] never written: every row that reads x_j reads zero
            tm.val = tm.val.copy()
            tm.val[tm.ind == t.ind[e]] = 0

        res = [run(f) for f in (leave_out, conjugate, stale)]
        print("  row", i, "left out", res[0], "conjugated", res[1], "read as zero", res[2])
        assert min(res) > BROKEN


def tree_sum(a):
    """pairwise tree in the type of `a` (the depth of the kernels' two-stage reduction, not its exact shape)"""
    a = np.concatenate([a, np.zeros((1 << int(np.ceil(np.log2(len(a))))) - len(a), a.dtype)])
    while len(a) > 1:
        a = a[0::2] + a[1::2]
    return a[0]


def test_dot_bound_discriminates(prec):
    dtype = DTYPE[prec]
    n = cr.DOT_N
    rp, ci, v = cr.bidiagonal(n, 7, dtype, 0)
    x = cr.tail_weighted(n, 8, dtype)
    r, c, a = cr.coo(rp, ci, v, 0)
    y = cr.product(r, c, a, (n, n), dtype(1), x[:, None], dtype(0), np.zeros((n, 1), dtype), dtype)[:, 0]
    ref, bound = cr.cdot(x, y, cr.ext_type(dtype)), cr.cdot_bound(x, y, dtype)

    def run(k=n):
        # chains of ceil(n / 262144) products per "thread", then a tree: 2 + 18 levels of the 2 + 4 + 16 the bound counts
        prod = np.conj(x[:k]) * y[:k]
        prod = np.concatenate([prod, np.zeros(2 * 262144 - k, dtype)]).reshape(2, 262144)
        got = tree_sum(prod[0] + prod[1])
        assert got.dtype == dtype
        return float(abs(cr.ext_type(dtype)(got) - ref) / bound)

    honest, last_left_out, tail_left_out = run(), run(n - 1), run(262144)
    print("dot", prec, "honest ratio", honest, "last element left out", last_left_out, "second turn left out", tail_left_out)
    assert honest <= HONEST
    assert last_left_out > BROKEN and tail_left_out > BROKEN
