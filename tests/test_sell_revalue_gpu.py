"""GPU tier: the SELL-64 copy of a handle keeps its STRUCTURE through aoclsparse_mi355_?revalue_device (keep_value_maps set) and
the next product runs the values stage alone (include/aoclsparse_mi355.h: ?revalue_device (4), get_sell_keep_info).

Every case follows the twin protocol of tests/test_revalue_device_gpu.py: a handle with the flag, an mv hint and optimize; products
on the old values; ?revalue_device; then a FRESH handle over the new values built under the same options.  Compared: two
consecutive products (both sweep directions) for the three (alpha, beta) of S.AB, bit for bit (double also against
oracle.dcsrmv), and every SELL getter -- spmv_info, sell_values, sell_packing, sell_records, sell_period, sell_march.  Every case
asserts structure_builds unchanged and value_fills + 1 across revalue + product, and the last_route it was constructed for
(2: values stage with the search, or with nothing to search; 3: the periodic range carried over), so that no case passes by
missing its path.  The controls show the counter moving on every other route.  The uniform lists themselves have no getter: they
are covered through sell_period / sell_march (functions of the records and lists) and through the products."""
import contextlib
import functools

import numpy as np
import pytest

import complex_ref as cr
import test_gpu_sell_march as MR
import test_gpu_sell_packed as S
import test_gpu_sell_period as T
import test_gpu_sell_records as R
from util import pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
P = pkg()
L = P.lib()

AB = S.AB
DTYPES = S.DTYPES
GX, M = 512, 512 * 512  # 4,096 slices: the smallest copy with slice records
NONE = (0, 0, 0, 0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    yield
    assert L.aoclsparse_mi355_set_option(P.OPTION_SELL, -1) == 0
    assert L.aoclsparse_mi355_set_option(P.OPTION_SELL_VALUES, -1) == 0


@contextlib.contextmanager
def option_sell(mode):
    assert L.aoclsparse_mi355_set_option(P.OPTION_SELL, mode) == 0
    try:
        yield
    finally:
        assert L.aoclsparse_mi355_set_option(P.OPTION_SELL, -1) == 0


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def prod(A, d, x, y0, alpha, beta, mode=-1):
    """one real ?mv of the handle's type (host-created and device-created handles alike) under option sell_values = mode"""
    xd, yd = dev(x), dev(y0.copy())
    with S.sell_values(mode):  # (a values stage reads the option again)
        st = (P.dmv if x.dtype == np.float64 else P.smv)(P.OP_NONE, alpha, A, d, xd, beta, yd)
    assert st == 0, P.STATUS[st]
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def getters(A):
    i = A.spmv_info()
    return (tuple(getattr(i, k) for k, _ in P.SpmvInfo._fields_), A.sell_values(), A.sell_packing(), A.sell_records(), A.sell_period(),
            A.sell_march())


def keep(A):
    i = A.sell_keep_info()
    return {k: getattr(i, k) for k, _ in P.SellKeepInfo._fields_}


class Case:
    """one handle under test and what its twins are made from"""

    def __init__(self, rp, ci, v, n=None, mode=-1, seed=1, flag=True, hint=True):
        self.rp, self.ci, self.mode = rp, ci, mode
        self.m = len(rp) - 1
        self.n = self.m if n is None else n
        self.x, self.y0 = R.operands(self.n, self.m, v.dtype, seed)
        if hint:
            self.A, self.d = S.handle(rp, ci, v.copy(), mode, n=self.n)
        else:
            self.A, self.d = P.Matrix(0, self.m, self.n, rp, ci, v.copy()), P.Descr()
            assert self.A.status == 0
        if flag:
            assert self.A.keep_value_maps() == 0

    def twin(self, v, mode=None):
        return S.handle(self.rp, self.ci, v.copy(), self.mode if mode is None else mode, n=self.n)

    def check(self, v, twin=None, mode=None, oracle_too=True):
        """the handle against a fresh twin over v (made here unless given): products, then every getter"""
        mode = self.mode if mode is None else mode
        Tw, dT = twin if twin is not None else self.twin(v, mode)
        for alpha, beta in AB:
            for lap in range(2):
                ya = prod(self.A, self.d, self.x, self.y0, alpha, beta, mode)
                S.same_bits(ya, prod(Tw, dT, self.x, self.y0, alpha, beta, mode), ("twin", alpha, beta, lap))
                if lap == 0 and oracle_too and v.dtype == np.float64:
                    S.same_bits(ya, S.cpu_chain(v, self.ci, self.rp, self.x, self.y0, alpha, beta), ("oracle", alpha, beta))
        assert getters(self.A) == getters(Tw), (getters(self.A), getters(Tw))
        return Tw, dT

    def stale(self, v2):
        """?revalue_device alone: the structure is kept, the copy serves no product, no stage has run"""
        k0 = keep(self.A)
        assert self.A.revalue_device(dev(v2)) == 0
        k1 = keep(self.A)
        assert k1["kept"] == 1 and k1["valid"] == 0, k1
        for k in ("structure_builds", "value_fills", "searches_skipped", "last_route"):
            assert k1[k] == k0[k], (k, k0, k1)
        return k0

    def revalue(self, v2, route, twin=None, mode=None, oracle_too=True):
        k0 = self.stale(v2)
        tw = self.check(v2, twin, mode, oracle_too)
        k2 = keep(self.A)
        assert k2["kept"] == 1 and k2["valid"] == 1, k2
        assert k2["structure_builds"] == k0["structure_builds"], ("the structure was built again", k0, k2)
        assert k2["value_fills"] == k0["value_fills"] + 1, (k0, k2)
        assert k2["last_route"] == route, (route, k2)
        assert k2["searches_skipped"] == k0["searches_skipped"] + (route == 3), (k0, k2)
        assert k2["kept_bytes"] >= 0
        return tw


@functools.lru_cache(maxsize=None)
def laplace(dtype):
    rp, ci, v = T.grid(GX, M)
    return rp, ci, np.ascontiguousarray(v, dtype=dtype)


def flipped(rp, v, row, cell=1):
    """v with the two table values swapped in one cell of one row"""
    v2 = v.copy()
    e = rp[row] + cell
    lo, hi = v.min(), v.max()
    v2[e] = hi if v2[e] == lo else lo
    return v2


# ---- 4,096 slices -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_scaled_values_carry_the_range_over(dtype):
    """2 x the values: the order of the bit patterns, hence every index, word, flag and list, is unchanged -- no search"""
    rp, ci, v = laplace(dtype)
    c = Case(rp, ci, v)
    c.check(v)
    assert keep(c.A)["last_route"] == 1 and c.A.sell_period() != NONE and c.A.sell_packing()[:2] == (1, 1)
    rng = c.A.sell_period()
    Tw, _ = c.revalue((2 * v).astype(dtype), 3)
    assert c.A.sell_period() == rng == Tw.sell_period()
    assert keep(c.A)["kept_bytes"] > 0
    c.revalue(v, 3)  # ... and back, through the set that was the spare one


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_exception_slice_loses_its_flags(dtype):
    """slice 8 is the first slice of grid line 1 (its first row has no west neighbour): an exception slice.  One other value in
    one of its rows: the slice keeps neither flag; the old values bring both back.  The search runs both times."""
    rp, ci, v = laplace(dtype)
    c = Case(rp, ci, v, seed=2)
    c.check(v)
    u0, e0 = c.A.sell_records()
    assert e0 > 0
    c.revalue(flipped(rp, v, 64 * 8 + 5), 2)
    assert c.A.sell_records() == (u0 - 1, e0 - 1)
    c.revalue(v, 2)
    assert c.A.sell_records() == (u0, e0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_interior_slice_loses_its_word(dtype):
    rp, ci, v = laplace(dtype)
    c = Case(rp, ci, v, seed=3)
    c.check(v)
    u0, e0 = c.A.sell_records()
    rng = c.A.sell_period()
    c.revalue(flipped(rp, v, 64 * 11 + 5), 2)
    assert c.A.sell_records() == (u0 - 1, e0) and c.A.sell_period() != rng


# ---- encoding classes ---------------------------------------------------------------------------------------------------------------
def classes(dtype, steps):
    rp, ci, _ = laplace(dtype)
    c = Case(rp, ci, S.table_values(rp, steps[0], dtype), seed=4)
    c.check(S.table_values(rp, steps[0], dtype))
    for ntab in steps[1:]:
        v2 = S.table_values(rp, ntab, dtype)
        assert len(np.unique(S.bits(v2))) == ntab
        c.revalue(v2, 2)
        assert c.A.sell_values() == (ntab if ntab <= 256 else 0)
        want = S.expected_packing(rp, ntab) if ntab <= 256 else (0, 0)
        assert c.A.sell_packing()[:2] == want, (ntab, c.A.sell_packing())
        if want == (0, 0):
            assert c.A.sell_packing()[2] == 0  # no uniform lists without packed words
        else:
            assert c.A.sell_packing()[2] > 0


def test_encoding_classes_double():
    """packed words of 1, 2 and 4 bytes, one byte per cell, values, and back: buffers change with the class, the structure stays"""
    rp = laplace(np.float64)[0]
    assert [S.expected_packing(rp, k) for k in (2, 3, 5, 17)] == [(1, 1), (2, 2), (4, 4), (0, 0)]
    classes(np.float64, (2, 3, 5, 17, 300, 2))


def test_encoding_classes_float():
    classes(np.float32, (2, 300, 2))


@pytest.mark.parametrize("dtype", DTYPES)
def test_bit_patterns(dtype):
    """+0.0 and -0.0, two NaN payloads and the all-ones pattern (the table pass's own "empty" key) are seven table entries with
    1.5 and -0.75; products compared as bits"""
    rp, ci, v = laplace(dtype)
    U = np.uint64 if dtype == np.float64 else np.uint32
    nan = 0x7ff8000000000000 if dtype == np.float64 else 0x7fc00000
    pats = np.array([0, 1 << (63 if dtype == np.float64 else 31), nan | 1, nan | 0xff, np.iinfo(U).max], dtype=U)
    tab = np.concatenate([pats.view(dtype), np.array([1.5, -0.75], dtype)])
    lens = np.diff(rp.astype(np.int64))
    i = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    k = np.arange(len(i), dtype=np.int64) - np.repeat(rp[:-1].astype(np.int64), lens)
    v2 = np.ascontiguousarray(tab[(5 * i + 3 * k) % 7])
    assert len(np.unique(S.bits(v2))) == 7
    c = Case(rp, ci, v, seed=5)
    c.check(v)
    c.revalue(v2, 2, oracle_too=False)
    assert c.A.sell_values() == 7 and c.A.sell_packing()[:2] == (4, 4)
    c.revalue(v, 2)


# ---- 61,440 slices: the stacked periods -----------------------------------------------------------------------------------------------
def test_stacked_periods_double():
    """the boundary-free 5-offset stencil of tests/test_gpu_sell_march.py: stacked, still stacked after 2 x the values without a
    search, not stacked after that test's two-cell change, stacked again with the old values"""
    rp, ci, v, n = MR.free(tuple(MR.OFF5))
    v = np.ascontiguousarray(v, dtype=np.float64)
    whole = (0, MR.NS, MR.G, MR.MAP5)
    c = Case(rp, ci, v, n=n, mode=1, seed=9)
    old = c.check(v)
    assert c.A.sell_march() == whole
    c.revalue(2 * v, 3)
    assert c.A.sell_march() == whole
    v2 = v.copy()
    for s in (20001, 41003):
        e = rp[64 * s + 5] + 1
        v2[e] = 1.5 if v2[e] == -0.75 else -0.75
    c.revalue(v2, 2)
    assert c.A.sell_march() == NONE and c.A.sell_values() == 2
    c.revalue(v, 2, twin=old)
    assert c.A.sell_march() == whole


# ---- ragged, empty, small, PACK 4 -------------------------------------------------------------------------------------------------------
def without_rows(rp, ci, v, rows):
    lens = np.diff(rp.astype(np.int64))
    gone = np.zeros(len(lens), bool)
    gone[rows] = True
    keep_e = ~np.repeat(gone, lens)
    rp2 = np.zeros(len(lens) + 1, np.int64)
    rp2[1:] = np.cumsum(np.where(gone, 0, lens))
    return rp2.astype(np.int32), np.ascontiguousarray(ci[keep_e]), np.ascontiguousarray(v[keep_e])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_ragged_last_slice_and_empty_rows(dtype):
    m = M - 27
    rp, ci, v = T.grid(GX, m)
    rows = np.concatenate([[3, 700, 70001, m - 1], np.arange(64 * 77, 64 * 78)])
    rp, ci, v = without_rows(rp, ci, np.ascontiguousarray(v, dtype=dtype), rows)
    assert (len(rp) - 1) % 64 != 0 and np.diff(rp)[64 * 77:64 * 78].max() == 0
    c = Case(rp, ci, v, seed=6)
    c.check(v)
    assert c.A.sell_packing()[:2] == (1, 1)
    c.revalue((2 * v).astype(dtype), 3)
    from test_gpu_sell_wide import two_values
    c.revalue(two_values(rp, dtype), 2)  # every row its own index bits


@pytest.mark.parametrize("dtype", DTYPES)
def test_below_the_gates(dtype):
    """1,000 rows of 5: no shared lists, no table, no records -- the refill alone runs"""
    rp, ci, _ = S.banded(1000, -2, 2)
    rng = np.random.default_rng(7)
    v, v2 = rng.uniform(-1, 1, len(ci)).astype(dtype), rng.uniform(-1, 1, len(ci)).astype(dtype)
    c = Case(rp, ci, v, seed=7)
    c.check(v)
    assert c.A.spmv_info().kernel == 3 and c.A.sell_values() == 0 and c.A.sell_packing() == (0, 0, 0)
    c.revalue(v2, 2)
    assert c.A.spmv_info().kernel == 3 and c.A.sell_values() == 0 and keep(c.A)["searches_skipped"] == 0


def long_rows(m, rows_per_list, seed):
    """16 - 20 ascending columns per row; `rows_per_list` consecutive rows repeat one list (4: the dofs of a node, 1: scattered)"""
    rng = np.random.default_rng(seed)
    nn = m // rows_per_list
    start = rng.integers(0, m - 2100, nn)
    cols = start[:, None] + np.cumsum(rng.integers(1, 100, (nn, 20)), axis=1)
    lens = rng.integers(16, 21, nn)
    cols, lens = np.repeat(cols, rows_per_list, axis=0), np.repeat(lens, rows_per_list)
    keep_e = np.arange(20)[None, :] < lens[:, None]
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    return rp.astype(np.int32), cols[keep_e].astype(np.int32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows_per_list, kernel", [(4, 4), (1, 3)])
def test_pack_4(rows_per_list, kernel, dtype):
    """8,192 rows of 16 - 20: four cells of a row adjacent; as 4-dof nodes (shared lists) and scattered (own lists).  No table ->
    a table of two (one byte per cell: no records at 128 slices) -> no table"""
    rp, ci = long_rows(8192, rows_per_list, 8)
    assert len(ci) >= 1 << 17 and len(ci) >= 16 * 8192
    rng = np.random.default_rng(9)
    v = rng.uniform(-1, 1, len(ci)).astype(dtype)
    v2 = np.where(rng.integers(0, 2, len(ci)) == 1, 1.5, -2.0).astype(dtype)
    assert len(np.unique(S.bits(v))) > 256 and len(np.unique(S.bits(v2))) == 2  # table absent, then present
    c = Case(rp, ci, v, seed=8)
    c.check(v)
    assert c.A.spmv_info().kernel == kernel and c.A.sell_values() == 0
    c.revalue(v2, 2)
    assert c.A.spmv_info().kernel == kernel and c.A.sell_values() == 2 and c.A.sell_packing() == (0, 0, 0)
    c.revalue(v, 2)
    assert c.A.sell_values() == 0
    c.revalue((2 * v).astype(dtype), 2)  # (no records: nothing to carry over, the refill alone)


# ---- complex ----------------------------------------------------------------------------------------------------------------------------
def cprod(A, d, x, y0, alpha, beta):
    fn = L.aoclsparse_zmv if x.dtype == np.complex128 else L.aoclsparse_cmv
    y = y0.copy()
    a, b = np.array([alpha], x.dtype), np.array([beta], x.dtype)
    assert fn(P.OP_NONE, P._ptr(a), A.h, d.h, P._ptr(x), P._ptr(b), P._ptr(y)) == 0
    return y


def chandle(rp, ci, v, n):
    A = P.Matrix.from_device(0, len(rp) - 1, n, len(v), dev(rp), dev(ci), dev(v))  # (the host constructor takes real types only)
    assert A.status == 0
    d = P.Descr()
    assert L.aoclsparse_set_mv_hint(A.h, P.OP_NONE, d.h, 100) == 0 and L.aoclsparse_optimize(A.h) == 0
    return A, d


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("shape", ["below 2^17 entries", "2^17 entries, node lists"])
def test_complex(shape, dtype):
    if shape.startswith("below"):
        rp, ci, _ = S.banded(20000, -2, 2)
        kernel = 3
    else:  # 4-row nodes of 8 columns: 16,384 x 8 = 2^17 entries, one list per four rows
        rng = np.random.default_rng(10)
        cols = np.sort(rng.integers(0, 16000, (4096, 1)) + np.cumsum(rng.integers(1, 40, (4096, 8)), axis=1), axis=1)
        rp, ci = (8 * np.arange(16385)).astype(np.int32), np.repeat(cols, 4, axis=0).reshape(-1).astype(np.int32)
        assert len(ci) == 1 << 17
        kernel = 4
    m = len(rp) - 1
    n = int(ci.max()) + 1
    rng = np.random.default_rng(11)
    v, v2 = cr.crand(rng, len(ci), dtype), cr.crand(rng, len(ci), dtype)
    x, y0 = cr.crand(rng, n, dtype), cr.crand(rng, m, dtype)
    A, d = chandle(rp, ci, v, n)
    assert A.keep_value_maps() == 0
    r, cc, _ = cr.coo(rp, ci, v, 0)

    def against(vals, Tw, dT):
        for alpha, beta in ((1.0, 0.0), (1.7 - 0.4j, -0.3 + 0.2j), (-0.75j, 1.5)):
            ref = cr.product(r, cc, vals, (m, n), alpha, x[:, None], beta, y0[:, None], cr.ext_type(dtype))
            scale, p = cr.product_scale(r, cc, vals, (m, n), alpha, x[:, None], beta, y0[:, None])
            bound = cr.product_bound(p, 6, scale, dtype)
            for lap in range(2):
                ya = cprod(A, d, x, y0, alpha, beta)
                assert np.array_equal(ya.view(cr.real_type(dtype)), cprod(Tw, dT, x, y0, alpha, beta).view(cr.real_type(dtype)))
                assert cr.ratio(np.abs(ya[:, None].astype(cr.ext_type(dtype)) - ref), bound) < 1
        assert getters(A) == getters(Tw)

    against(v, *chandle(rp, ci, v, n))
    k0 = keep(A)
    assert k0["last_route"] == 1 and k0["valid"] == 1 and A.spmv_info().kernel == kernel
    assert A.revalue_device(dev(v2)) == 0
    k1 = keep(A)
    assert k1["kept"] == 1 and k1["valid"] == 0
    against(v2, *chandle(rp, ci, v2, n))
    k2 = keep(A)
    assert (k2["structure_builds"], k2["value_fills"], k2["last_route"], k2["valid"]) == (k0["structure_builds"], k0["value_fills"] + 1, 2, 1)
    assert A.spmv_info().kernel == kernel


# ---- promotion, sequences -----------------------------------------------------------------------------------------------------------------
def test_a_promoted_handle_keeps_its_structure():
    """no hint, no optimize: the eighth product builds the copy; revalued afterwards, the structure is kept"""
    rp, ci, v = laplace(np.float64)
    c = Case(rp, ci, v, seed=12, hint=False)
    assert keep(c.A)["kept"] == 0
    for _ in range(8):
        prod(c.A, c.d, c.x, c.y0, 1.0, 0.0)
    k = keep(c.A)
    assert (k["kept"], k["valid"], k["structure_builds"], k["last_route"]) == (1, 1, 1, 1) and c.A.spmv_info().kernel == 4
    c.check(v)
    c.revalue(2 * v, 3)


def test_two_revalues_without_a_product():
    rp, ci, v = laplace(np.float64)
    c = Case(rp, ci, v, seed=13)
    c.check(v)
    k0 = c.stale(3 * v)
    k1 = keep(c.A)
    c.stale(2 * v)
    assert keep(c.A) == k1
    c.check(2 * v)
    k2 = keep(c.A)
    assert (k2["structure_builds"], k2["value_fills"], k2["last_route"]) == (k0["structure_builds"], k0["value_fills"] + 1, 3)


def test_optimize_is_the_first_caller():
    """a new mv hint and aoclsparse_optimize after the revalue: the values stage has run before any product"""
    rp, ci, v = laplace(np.float64)
    c = Case(rp, ci, v, seed=14)
    c.check(v)
    k0 = c.stale(2 * v)
    assert L.aoclsparse_set_mv_hint(c.A.h, P.OP_NONE, c.d.h, 50) == 0 and L.aoclsparse_optimize(c.A.h) == 0
    k1 = keep(c.A)
    assert (k1["valid"], k1["structure_builds"], k1["value_fills"], k1["last_route"]) == (1, k0["structure_builds"], k0["value_fills"] + 1, 3)
    c.check(2 * v)
    assert keep(c.A) == k1


def test_sell_values_0_between_revalue_and_product():
    """the values stage reads option sell_values: the table is gone, the structure is not"""
    rp, ci, v = laplace(np.float64)
    c = Case(rp, ci, v, seed=15)
    c.check(v)
    assert c.A.sell_values() == 2
    c.revalue(2 * v, 2, mode=0)
    assert c.A.sell_values() == 0 and c.A.sell_packing() == (0, 0, 0) and c.A.sell_period() == NONE


def test_option_sell_0_between_revalue_and_product():
    """the structure was built under another option value: as a fresh handle decides under 0, there is no copy"""
    rp, ci, v = laplace(np.float64)
    c = Case(rp, ci, v, seed=16)
    c.check(v)
    c.stale(2 * v)
    with option_sell(0):
        Tw, dT = c.check(2 * v)
        assert Tw.spmv_info().kernel == c.A.spmv_info().kernel == 1
    k = keep(c.A)
    assert (k["kept"], k["valid"]) == (0, 0)


# ---- controls: every other route rebuilds --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["flag never set", "dupdate_values_device", "dupdate_values", "dset_value"])
def test_other_routes_build_the_structure_again(how):
    rp, ci, v = laplace(np.float64)
    c = Case(rp, ci, v, seed=17, flag=how != "flag never set")
    c.check(v)
    k0 = keep(c.A)
    v2 = 2 * v
    if how == "flag never set":
        assert c.A.revalue_device(dev(v2)) == 0
    elif how == "dupdate_values_device":
        assert c.A.update_values_device(dev(v2)) == 0
    elif how == "dupdate_values":
        assert L.aoclsparse_dupdate_values(c.A.h, len(v2), P._ptr(v2)) == 0
    else:
        v2 = v.copy()
        v2[rp[700] + 2] = -1.0  # the diagonal of row 700
        assert ci[rp[700] + 2] == 700 and L.aoclsparse_dset_value(c.A.h, 700, 700, -1.0) == 0
    k1 = keep(c.A)
    assert (k1["kept"], k1["valid"]) == (0, 0)
    c.check(v2)
    k2 = keep(c.A)
    assert k2["structure_builds"] == k0["structure_builds"] + 1 and k2["last_route"] == 1 and k2["value_fills"] == k0["value_fills"] + 1


def test_a_triplet_refresh_builds_the_structure_again():
    rp, ci, v = laplace(np.float64)
    row = np.repeat(np.arange(M, dtype=np.int32), np.diff(rp))
    A = P.Matrix.from_coo_device(0, M, M, len(v), dev(row), dev(ci), dev(v), duplicates=P.COO_KEEP, refreshable=True)
    assert A.status == 0 and A.keep_value_maps() == 0
    d = P.Descr()
    assert L.aoclsparse_set_mv_hint(A.h, P.OP_NONE, d.h, 100) == 0 and L.aoclsparse_optimize(A.h) == 0
    x, y0 = R.operands(M, M, np.float64, 18)
    Tw, dT = S.handle(rp, ci, v.copy(), -1)
    S.same_bits(prod(A, d, x, y0, 1.7, -0.3), prod(Tw, dT, x, y0, 1.7, -0.3), "old values")
    k0 = keep(A)
    assert (k0["kept"], k0["valid"]) == (1, 1)
    assert A.refresh_from_coo_device(dev(2 * v)) == 0
    assert (keep(A)["kept"], keep(A)["valid"]) == (0, 0)
    Tw, dT = S.handle(rp, ci, 2 * v, -1)
    for alpha, beta in AB:
        S.same_bits(prod(A, d, x, y0, alpha, beta), prod(Tw, dT, x, y0, alpha, beta), ("twin", alpha, beta))
    assert getters(A)[1:] == getters(Tw)[1:]
    k2 = keep(A)
    assert k2["structure_builds"] == k0["structure_builds"] + 1 and k2["last_route"] == 1


@pytest.mark.parametrize("how", ["order_mat_device", "aoclsparse_mi355_invalidate"])
def test_what_releases_the_structure(how):
    rp, ci, v = laplace(np.float64)
    c = Case(rp, ci, v, seed=19)
    c.check(v)
    c.stale(2 * v)  # (a kept, stale structure is released as well as a valid copy's)
    k0 = keep(c.A)
    assert (c.A.order_device() if how == "order_mat_device" else L.aoclsparse_mi355_invalidate(c.A.h)) == 0
    k1 = keep(c.A)
    assert (k1["kept"], k1["valid"], k1["kept_bytes"]) == (0, 0, 0)
    c.check(2 * v)
    k2 = keep(c.A)
    assert k2["structure_builds"] == k0["structure_builds"] + 1 and (k2["kept"], k2["valid"], k2["last_route"]) == (1, 1, 1)


# ---- with the kept clean CSR and TRSV plans ---------------------------------------------------------------------------------------------------
def test_with_kept_trsv_plans():
    """one handle, one revalue: the lower solve runs on its kept plan, the product on its kept structure, nothing is analysed"""
    from test_revalue_device_gpu import solve
    g = 96
    rp, ci, v = T.grid(g, g * g)
    v = np.ascontiguousarray(v, dtype=np.float64)
    m = g * g
    b = np.random.default_rng(20).uniform(-1, 1, m)
    A = P.Matrix(0, m, m, rp, ci, v.copy())
    assert A.status == 0 and A.keep_value_maps() == 0
    d = P.Descr()
    assert L.aoclsparse_set_mv_hint(A.h, P.OP_NONE, d.h, 100) == 0 and L.aoclsparse_optimize(A.h) == 0
    x, y0 = R.operands(m, m, np.float64, 21)
    v2 = v * np.random.default_rng(22).uniform(1.0, 2.0, len(v))
    Hold, Hnew = S.handle(rp, ci, v.copy(), -1), S.handle(rp, ci, v2.copy(), -1)
    x0 = solve(A, P.FILL_LOWER, P.OP_NONE, False, b)
    assert np.array_equal(x0, solve(Hold[0], P.FILL_LOWER, P.OP_NONE, False, b))
    S.same_bits(prod(A, d, x, y0, 1.7, -0.3), prod(*Hold, x, y0, 1.7, -0.3), "old values")
    i0, k0 = A.value_map_info(), keep(A)
    assert i0.plans_mapped == 1 and (k0["kept"], k0["valid"]) == (1, 1)
    assert A.revalue_device(dev(v2)) == 0
    x1 = solve(A, P.FILL_LOWER, P.OP_NONE, False, b)
    assert np.array_equal(x1, solve(Hnew[0], P.FILL_LOWER, P.OP_NONE, False, b)) and not np.array_equal(x1, x0)
    for alpha, beta in AB:
        for lap in range(2):
            ya = prod(A, d, x, y0, alpha, beta)
            S.same_bits(ya, prod(*Hnew, x, y0, alpha, beta), ("twin", alpha, beta, lap))
        S.same_bits(ya, S.cpu_chain(v2, ci, rp, x, y0, alpha, beta), ("oracle", alpha, beta))
    i1, k1 = A.value_map_info(), keep(A)
    assert (i1.plan_builds, i1.clean_builds) == (i0.plan_builds, i0.clean_builds) and i1.last_kept_plans == 1
    assert (k1["structure_builds"], k1["value_fills"], k1["valid"]) == (k0["structure_builds"], k0["value_fills"] + 1, 1)
    assert getters(A)[1:] == getters(Hnew[0])[1:]
