"""The short-row SELL-64 kernel with packed slice records and several slices per wavefront: what its branch-free control flow can
get wrong.  Every product is compared bit for bit with the CPU oracle (scalar order) through the C ABI.

The matrices have whole slices of width 0 (runs of empty rows at the start, inside and at the end of a group of slices, and an
empty partial last slice: those read the padding cells behind the arrays), groups that mix slices whose rows follow lead[]
(mode 0, at the grid edges of a stencil) with single-list slices (shift = lane in the interior, no shift where 64 rows share one
list), and slice counts that are odd (no multiple of 4 waves x 1 / 2 / 4 slices: the last workgroup reads the padding records).
Sizes reach the short kernel's gate (>= 4,096 slices) and the gate of the several-slices-per-wavefront variants (>= 100,000).
Every handle runs four products -- two (alpha, beta) pairs, each in both sweep directions."""
import contextlib
import ctypes

import numpy as np
import pytest

import oracle
from util import pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
P = pkg()
L = P.lib()

SMALL = 4102 * 64 + 17  # 4,103 slices, the last one partial
BIG = 100002 * 64 + 5  # 100,003 slices


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


def empty_rows(m):
    """runs of empty rows: slices 0-2 (the start of the first group), 21 (inside one), 40-43 and 44-47 (whole groups), a run that
    covers parts of slices 50 and 52 and all of 51, and everything from the slice before the last on (the end)"""
    e = np.zeros(m, bool)
    for a, b in ((0, 3 * 64), (21 * 64, 22 * 64), (40 * 64, 48 * 64), (50 * 64 + 10, 52 * 64 + 30), ((m // 64 - 1) * 64, m)):
        e[a:b] = True
    return e


def stencil_pattern(m, g=1000):
    """5-point stencil on rows of g points (lists shifted by one in the interior, broken at the edges), rows [200 g, 200 g + 64 x 300)
    with ONE list per 64 rows (four entries), and the empty runs of empty_rows()"""
    r = np.arange(m, dtype=np.int64)
    j = r % g
    cols = np.stack([r - g, r - 1, r, r + 1, r + g], axis=1)
    ok = (cols >= 0) & (cols < m)
    ok[:, 1] &= j > 0
    ok[:, 3] &= j < g - 1
    a = (200 * g) // 64 * 64
    same = slice(a, a + 64 * 300)
    cols[same] = (r[same] // 64 * 64)[:, None] + np.array([0, 3, 7, 11, 0])
    ok[same] = np.array([True, True, True, True, False])
    ok[empty_rows(m)] = False
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum(ok.sum(axis=1))
    return rp.astype(np.int32), cols[ok].astype(np.int32)


def scattered_pattern(m, seed):
    """5-7 ascending columns per row with random gaps, one row in 50 empty (no two rows share a list: the column lists are not
    shared; padding below the SELL-64 budget), and the empty runs"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(5, 8, m)
    lens[rng.random(m) < 0.02] = 0
    lens[empty_rows(m)] = 0
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    nnz = int(rp[-1])
    row = np.repeat(np.arange(m), lens)
    step = np.cumsum(rng.integers(1, 40, nnz))
    first = step[np.minimum(rp[:-1], nnz - 1)]  # (the running sum at every row's first entry)
    ci = rng.integers(0, m, m)[row] + step - first[row]
    return rp.astype(np.int32), ci.astype(np.int32), m + 40 * 8


def values(nnz, k, dtype, seed=5):
    """nnz values with exactly k distinct bit patterns (k = 0: all different)"""
    rng = np.random.default_rng(seed)
    if k == 0:
        return np.ascontiguousarray(rng.uniform(-2, 2, nnz).astype(dtype))
    pool = np.unique(rng.uniform(-2, 2, 4 * k).astype(dtype))[:k]
    assert len(pool) == k
    v = pool[rng.integers(0, k, nnz)]
    v[:k] = pool
    return np.ascontiguousarray(v)


def check_products(rp, ci, v, n, ntab, shared, min_slices):
    """optimize, assert the path, then four products against the oracle"""
    m, dtype = len(rp) - 1, v.dtype
    A = P.Matrix(0, m, n, rp, ci, v)
    assert A.status == 0
    d = P.Descr()
    assert L.aoclsparse_set_mv_hint(A.h, P.OP_NONE, d.h, 100) == 0
    with sell_values(-1 if ntab else 0):
        assert L.aoclsparse_optimize(A.h) == 0
    info = A.spmv_info()
    # the short-row kernel: a SELL-64 copy (4 = shared column lists), scalar order, the slice gate, no slice wider than 8
    assert info.kernel == (4 if shared else 3) and info.order == 0
    assert info.sell_slices == (m + 63) // 64 and info.sell_slices >= min_slices and info.sell_slices % 2 == 1
    assert int(np.diff(rp).max()) <= 7 and info.stored_cells <= 7 * 64 * info.sell_slices
    assert A.sell_values() == ntab
    rng = np.random.default_rng(m % 1000 + ntab)
    x, y0 = rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, m).astype(dtype)
    xd = torch.from_numpy(x).cuda()
    for alpha, beta in ((1.0, 0.0), (1.0, 0.0), (1.7, -0.3), (1.7, -0.3)):  # (consecutive products alternate the sweep direction)
        if dtype == np.float64:
            st, ref = oracle.dcsrmv(-1, 0, alpha, m, len(v), v, ci, rp, x, beta, y0)
        else:  # (rows shorter than 8: the float kernel's scalar tail only)
            st, ref = oracle.scsrmv("lane8", 0, alpha, m, v, ci, rp, x, beta, y0)
        assert st == 0
        yd = torch.from_numpy(y0.copy()).cuda()
        st = (P.dmv if dtype == np.float64 else P.smv)(P.OP_NONE, alpha, A, d, xd, beta, yd)
        assert st == 0, P.STATUS[st]
        torch.cuda.synchronize()
        got = yd.cpu().numpy()
        bad = int(np.sum(bits(got) != bits(ref)))
        assert bad == 0, (alpha, beta, bad, np.flatnonzero(bits(got) != bits(ref))[:8])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("ntab", [1, 2, 3, 256, 0])
def test_stencil_with_empty_slices(ntab, dtype):
    rp, ci = stencil_pattern(SMALL)
    check_products(rp, ci, values(len(ci), ntab, dtype), SMALL, ntab, True, 4096)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("ntab", [2, 256, 0])
def test_own_column_lists_with_empty_slices(ntab, dtype):
    rp, ci, n = scattered_pattern(SMALL, 9)
    check_products(rp, ci, values(len(ci), ntab, dtype), n, ntab, False, 4096)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("ntab", [2, 256, 0])
def test_large_launch_with_empty_slices(ntab, dtype):
    """>= 100,000 slices: the launches that put several slices on a wavefront"""
    rp, ci = stencil_pattern(BIG)
    check_products(rp, ci, values(len(ci), ntab, dtype), BIG, ntab, True, 100000)


def test_complex_handle_shares_the_kernel():
    """zmv on real-valued complex cells, alpha = 1, beta = 0: the real and the imaginary part of y are the oracle's products with
    the real and the imaginary part of x (the terms with the zero imaginary part of a value add an exact zero)"""
    m = SMALL
    rp, ci = stencil_pattern(m)
    v = values(len(ci), 0, np.float64)
    vc = np.ascontiguousarray(v.astype(np.complex128))
    h = ctypes.c_void_p()
    assert L.aoclsparse_create_zcsr(ctypes.byref(h), 0, m, m, len(vc), P._ptr(rp), P._ptr(ci), P._ptr(vc)) == 0
    d = P.Descr()
    try:
        assert L.aoclsparse_set_mv_hint(h, P.OP_NONE, d.h, 100) == 0 and L.aoclsparse_optimize(h) == 0
        rng = np.random.default_rng(51)
        xr, xi = rng.uniform(0.1, 1, m), rng.uniform(0.1, 1, m)
        x = np.ascontiguousarray(xr + 1j * xi)
        one, zero = P.CDouble(1.0, 0.0), P.CDouble(0.0, 0.0)
        zeros = np.zeros(m)
        ref_re = oracle.dcsrmv(-1, 0, 1.0, m, len(v), v, ci, rp, xr, 0.0, zeros)[1]
        ref_im = oracle.dcsrmv(-1, 0, 1.0, m, len(v), v, ci, rp, xi, 0.0, zeros)[1]
        for _ in range(2):  # (both sweep directions)
            y = np.full(m, np.nan + 0j)
            assert L.aoclsparse_zmv(P.OP_NONE, ctypes.byref(one), h, d.h, P._ptr(x), ctypes.byref(zero), P._ptr(y)) == 0
            assert np.array_equal(bits(y.real.copy()), bits(ref_re)) and np.array_equal(bits(y.imag.copy()), bits(ref_im))
        info = P.SpmvInfo()  # (a complex handle gets its SELL-64 copy at its first product)
        assert L.aoclsparse_mi355_get_spmv_info(h, P.OP_NONE, ctypes.byref(info)) == 0
        assert info.kernel == 4 and info.sell_slices >= 4096
    finally:
        L.aoclsparse_destroy(ctypes.byref(h))
