"""SELL-64 copies whose cells hold one-byte indices into a table of the matrix's distinct value bit patterns
(aoclsparse_mi355_option_sell_values, aoclsparse_mi355_get_sell_values).

The table holds the values' exact bits, so every product must be bit-identical to the same handle built with the option at 0
(values in the cells) -- and equal to the oracle where the path is the reference's order."""
import contextlib
import ctypes

import numpy as np
import pytest

import oracle
from util import EPS64, laplace5, pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
P = pkg()
L = P.lib()


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    yield


@contextlib.contextmanager
def sell_values(mode):
    assert L.aoclsparse_mi355_set_option(P.OPTION_SELL_VALUES, mode) == 0
    try:
        yield
    finally:
        assert L.aoclsparse_mi355_set_option(P.OPTION_SELL_VALUES, -1) == 0


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(got, ref, what):
    assert np.array_equal(bits(got), bits(ref)), (what, int(np.sum(bits(got) != bits(ref))))


def handle(rp, ci, v, mode, op=P.OP_NONE, kid=None, mtype=P.TYPE_GENERAL, n=None, optimize=True):
    """a handle with an mv hint (kid pinned if given), optimized with sell_values = mode"""
    m = len(rp) - 1
    A = P.Matrix(0, m, m if n is None else n, rp, ci, v)
    assert A.status == 0
    d = P.Descr(mtype=mtype)
    if optimize:
        if kid is None:
            assert L.aoclsparse_set_mv_hint(A.h, op, d.h, 100) == 0
        else:
            assert L.aoclsparse_set_mv_hint_kid(A.h, op, d.h, 100, kid) == 0
        with sell_values(mode):
            assert L.aoclsparse_optimize(A.h) == 0
    return A, d


def product(A, d, x, y0, alpha=1.0, beta=0.0, op=P.OP_NONE):
    dbl = A.val.dtype == np.float64
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    yd = torch.from_numpy(np.ascontiguousarray(y0).copy()).cuda()
    st = (P.dmv if dbl else P.smv)(op, alpha, A, d, xd, beta, yd)
    assert st == 0, P.STATUS[st]
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def pair(rp, ci, v, x, y0, alpha=1.0, beta=0.0, op=P.OP_NONE, kid=None, mtype=P.TYPE_GENERAL, n=None):
    """(y with the table, y with the values in the cells, table entries of the first handle)"""
    A1, d1 = handle(rp, ci, v, -1, op, kid, mtype, n)
    A0, d0 = handle(rp, ci, v, 0, op, kid, mtype, n)
    assert A0.sell_values(op) == 0
    # (a derived operator -- symmetric descriptor -- gets its SELL-64 copy at its first product: the option holds there too)
    y1 = product(A1, d1, x, y0, alpha, beta, op)
    with sell_values(0):
        y0r = product(A0, d0, x, y0, alpha, beta, op)
    info1, info0 = A1.spmv_info(op), A0.spmv_info(op)
    assert info1.kernel == info0.kernel and info1.order == info0.order
    return y1, y0r, A1.sell_values(op), info1


def uniform_rows(seed, m, lo, hi, ncol=None):
    rng = np.random.default_rng(seed)
    n = m if ncol is None else ncol
    lens = rng.integers(lo, hi + 1, m)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in lens]).astype(np.int32)
    return rp, ci


def drawn_values(seed, nnz, k, dtype=np.float64):
    rng = np.random.default_rng(seed)
    pool = rng.uniform(-2, 2, k).astype(dtype)
    v = pool[rng.integers(0, k, nnz)]
    v[:k] = pool  # every pattern occurs
    return np.ascontiguousarray(v)


def laplace7(n):
    r = np.arange(n ** 3, dtype=np.int64)
    i, j, k = r // (n * n), (r // n) % n, r % n
    off = [(-n * n, i > 0), (-n, j > 0), (-1, k > 0), (0, np.ones_like(r, bool)), (1, k < n - 1), (n, j < n - 1), (n * n, i < n - 1)]
    cols = np.stack([r + o for o, _ in off], axis=1)
    ok = np.stack([c for _, c in off], axis=1)
    vals = np.broadcast_to(np.array([-1.0, -1.0, -1.0, 6.0, -1.0, -1.0, -1.0]), cols.shape)
    rp = np.zeros(n ** 3 + 1, np.int64)
    rp[1:] = np.cumsum(ok.sum(axis=1))
    return n ** 3, rp.astype(np.int32), cols[ok].astype(np.int32), np.ascontiguousarray(vals[ok])


@pytest.mark.parametrize("g", [200, 1000, 4096])
def test_laplacian_table_is_bit_identical(g):
    m, rp, ci, v = laplace5(g)
    rng = np.random.default_rng(g)
    x, y0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)
    y1, y0r, ntab, info = pair(rp, ci, v, x, y0)
    assert ntab == 2 and info.kernel in (3, 4)
    same_bits(y1, y0r, "option 0")
    st, yo = oracle.dcsrmv(-1, 0, 1.0, m, len(v), v, ci, rp, x, 0.0, y0)
    assert st == 0
    same_bits(y1, yo, "oracle")


def test_laplacian_7_point_alpha_beta():
    m, rp, ci, v = laplace7(64)
    rng = np.random.default_rng(5)
    x, y0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)
    y1, y0r, ntab, _ = pair(rp, ci, v, x, y0, 1.7, -0.3)
    assert ntab == 2
    same_bits(y1, y0r, "option 0")
    same_bits(y1, oracle.dcsrmv(-1, 0, 1.7, m, len(v), v, ci, rp, x, -0.3, y0)[1], "oracle")


@pytest.mark.parametrize("k", [1, 2, 255, 256, 257])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_random_values_from_k_patterns(k, dtype):
    m = 20000
    rp, ci = uniform_rows(k, m, 6, 9)
    v = drawn_values(k, len(ci), k, dtype)
    rng = np.random.default_rng(3)
    x, y0 = rng.uniform(-1, 1, m).astype(dtype), rng.uniform(-1, 1, m).astype(dtype)
    y1, y0r, ntab, info = pair(rp, ci, v, x, y0, 1.25, 0.5)
    assert info.kernel in (3, 4)
    assert ntab == (k if k <= 256 else 0)
    same_bits(y1, y0r, "option 0")
    if dtype == np.float64:
        ref = oracle.dcsrmv(-1, 0, 1.25, m, len(v), v, ci, rp, x, 0.5, y0)[1]
    else:
        ref = oracle.scsrmv("lane8", 0, 1.25, m, v, ci, rp, x, 0.5, y0)[1]
    same_bits(y1, ref, "oracle")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_special_bit_patterns(dtype):
    """-0.0 and +0.0 are two entries, +-Inf, a NaN with a payload, subnormals: the products keep their bits"""
    m = 30000
    rp, ci = uniform_rows(11, m, 6, 8)
    it = np.uint64 if dtype == np.float64 else np.uint32
    nan = (np.array([0x7FF0000000000ABC], np.uint64) if dtype == np.float64 else np.array([0x7FC00ABC], np.uint32)).view(dtype)[0]
    tiny = np.finfo(dtype).tiny
    special = np.array([-0.0, 0.0, np.inf, -np.inf, nan, tiny / 4, -tiny / 8, 1.0, -1.0, 3.0], dtype)
    rng = np.random.default_rng(12)
    v = special[rng.integers(0, len(special), len(ci))]
    v[: len(special)] = special
    # the infinite and NaN entries only in the first rows: most of y stays finite and informative
    late = np.arange(len(v)) > 200
    v[late & ~np.isfinite(v)] = 2.0
    v[:len(special)] = special
    x, y0 = rng.uniform(-1, 1, m).astype(dtype), rng.uniform(-1, 1, m).astype(dtype)
    x[::7] = 0.0
    y1, y0r, ntab, _ = pair(rp, ci, v, x, y0)
    assert ntab == len(np.unique(v.view(it)))
    same_bits(y1, y0r, "option 0")
    if dtype == np.float64:
        ref = oracle.dcsrmv(-1, 0, 1.0, m, len(v), v, ci, rp, x, 0.0, y0)[1]
    else:
        ref = oracle.scsrmv("lane8", 0, 1.0, m, v, ci, rp, x, 0.0, y0)[1]
    fin = np.isfinite(ref)
    same_bits(y1[fin], ref[fin], "oracle (finite rows)")
    assert np.array_equal(np.isnan(y1), np.isnan(ref)) and np.array_equal(y1[np.isinf(ref)], ref[np.isinf(ref)])


@pytest.mark.parametrize("kid", [0, 1, 2, 3])
@pytest.mark.parametrize("rows", [(12, 14), (18, 21)])  # PACK 1 (< 16 entries per row), PACK 4 (>= 16)
def test_every_kid_and_pack(kid, rows):
    m = 12000
    rp, ci = uniform_rows(kid + rows[0], m, *rows)
    v = drawn_values(kid, len(ci), 37)
    rng = np.random.default_rng(kid)
    x, y0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)
    y1, y0r, ntab, info = pair(rp, ci, v, x, y0, -0.75, 1.5, kid=kid)
    assert ntab == 37 and info.kernel in (3, 4)
    same_bits(y1, y0r, "option 0")
    assert info.stored_cells % (256 if rows[0] >= 16 else 64) == 0
    same_bits(y1, oracle.dcsrmv(kid, 0, -0.75, m, len(v), v, ci, rp, x, 1.5, y0)[1], "oracle")


def test_transposed_plan():
    m, rp, ci, v = laplace5(300)
    n = m
    v = drawn_values(21, len(ci), 5)
    rng = np.random.default_rng(22)
    x, y0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, n)
    y1, y0r, ntab, info = pair(rp, ci, v, x, y0, 5.1, 3.2, op=P.OP_TRANSPOSE, n=n)
    assert ntab == 5 and info.kernel in (3, 4)
    same_bits(y1, y0r, "option 0")
    st, yo = oracle.dcsrmvt(0, 5.1, m, n, v, ci, rp, x, 3.2, y0)
    absx = np.zeros(n)
    np.add.at(absx, ci, np.abs(v) * np.abs(np.repeat(x, np.diff(rp))))
    cnt = np.bincount(ci, minlength=n)
    assert np.all(np.abs(y1 - yo) <= (cnt + 4) * EPS64 * 5.1 * absx + 2 * EPS64 * np.abs(3.2 * y0) + 1e-300)


def test_symmetric_hint_goes_through_the_derived_operator():
    """derived.cpp builds its own SELL-64 copy (the query does not reach it): bits against option 0"""
    m, rp, ci, v = laplace5(400)
    rng = np.random.default_rng(31)
    x, y0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)
    y1, y0r, _, _ = pair(rp, ci, v, x, y0, 1.3, -0.4, mtype=P.TYPE_SYMMETRIC)
    same_bits(y1, y0r, "option 0")


def test_unhinted_handle_promoted_at_the_eighth_product():
    m, rp, ci, v = laplace5(300)
    rng = np.random.default_rng(41)
    x, y0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)
    A, d = handle(rp, ci, v, -1, optimize=False)
    ys = [product(A, d, x, y0, 2.0, 0.5) for _ in range(9)]
    assert A.spmv_info().kernel in (3, 4) and A.sell_values() == 2
    ref = oracle.dcsrmv(-1, 0, 2.0, m, len(v), v, ci, rp, x, 0.5, y0)[1]
    for y in ys:
        same_bits(y, ref, "oracle")


def test_complex_handle_keeps_full_values():
    m, rp, ci, v = laplace5(300)
    vc = np.ascontiguousarray(v.astype(np.complex128))
    h = ctypes.c_void_p()
    assert L.aoclsparse_create_zcsr(ctypes.byref(h), 0, m, m, len(vc), P._ptr(rp), P._ptr(ci), P._ptr(vc)) == 0
    d = P.Descr()
    try:
        assert L.aoclsparse_set_mv_hint(h, P.OP_NONE, d.h, 100) == 0 and L.aoclsparse_optimize(h) == 0
        rng = np.random.default_rng(51)
        x = np.ascontiguousarray(rng.uniform(-1, 1, m) + 1j * rng.uniform(-1, 1, m))
        y = np.zeros(m, np.complex128)
        one, zero = P.CDouble(1.0, 0.0), P.CDouble(0.0, 0.0)
        assert L.aoclsparse_zmv(P.OP_NONE, ctypes.byref(one), h, d.h, P._ptr(x), ctypes.byref(zero), P._ptr(y)) == 0
        n = P._I(-1)
        assert L.aoclsparse_mi355_get_sell_values(h, P.OP_NONE, ctypes.byref(n)) == 0 and n.value == 0
        ref = np.zeros(m, np.complex128)
        np.add.at(ref, np.repeat(np.arange(m), np.diff(rp)), vc * x[ci])
        assert np.allclose(y, ref, rtol=1e-14, atol=1e-14)
    finally:
        L.aoclsparse_destroy(ctypes.byref(h))


def test_value_updates_follow_the_table():
    """2 -> 1,000 distinct values -> 2, then a third value by ?set_value: the table count follows and y is the oracle's on the
    NEW values after each change"""
    m, rp, ci, v = laplace5(400)
    v2 = v.copy()  # (the handle aliases v: ?update_values writes into it)
    A, d = handle(rp, ci, v, -1)
    rng = np.random.default_rng(61)
    x, y0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)

    def check(ntab):
        y = product(A, d, x, y0, 1.1, 0.9)
        assert A.sell_values() == ntab and A.spmv_info().kernel in (3, 4)
        same_bits(y, oracle.dcsrmv(-1, 0, 1.1, m, len(A.val), A.val, A.col_ind, A.row_ptr, x, 0.9, y0)[1], "oracle")

    check(2)
    many = np.ascontiguousarray(np.random.default_rng(62).uniform(-1, 1, 1000)[np.arange(len(v)) % 1000])
    assert L.aoclsparse_dupdate_values(A.h, len(many), P._ptr(many)) == 0
    check(0)
    assert L.aoclsparse_dupdate_values(A.h, len(v2), P._ptr(v2)) == 0
    check(2)
    r = m // 2
    p = int(A.row_ptr[r])
    assert L.aoclsparse_dset_value(A.h, r, int(A.col_ind[p]), 0.125) == 0
    check(3)
