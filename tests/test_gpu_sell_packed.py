"""SELL-64 copies of short rows with packed table indices (one word per row) and uniform column lists (one scalar list per
slice): aoclsparse_mi355_get_sell_packing says which of the two a copy has, and every product is bit-identical to the same
matrix built with sell_values = 0 (values in the cells and no uniform lists: the established path) and to the CPU oracle in the
handle's order.

Every case runs double and float, (alpha, beta) = (1, 0), (1.7, -0.3), (-0.75, 1.5), and two consecutive products per handle
(consecutive products sweep the slices in opposite directions)."""
import contextlib

import numpy as np
import pytest

import oracle
from util import EPS64, pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
P = pkg()
L = P.lib()

AB = ((1.0, 0.0), (1.7, -0.3), (-0.75, 1.5))
DTYPES = [np.float64, np.float32]
WMAX = 8  # SELL_SHORT_WMAX
MIN_SLICES = 4096  # SELL_SHORT_MIN_SLICES


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


# ---- matrices ------------------------------------------------------------------------------------------------------------
def stencil(m, offsets, ok):
    """rows r with columns r + offsets[k] where ok[k][r]; values: 1 + k (replaced by the callers)"""
    r = np.arange(m, dtype=np.int64)
    cols = np.stack([r + o for o in offsets], axis=1)
    keep = np.stack(ok, axis=1)
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum(keep.sum(axis=1))
    k = np.broadcast_to(np.arange(len(offsets)), cols.shape)[keep]
    return rp.astype(np.int32), cols[keep].astype(np.int32), k


def laplace5_grid(gx, gy):
    """5-point Laplacian on gy lines of gx points: 4 on the diagonal, -1 off"""
    m = gx * gy
    r = np.arange(m, dtype=np.int64)
    i, j = r // gx, r % gx
    rp, ci, k = stencil(m, [-gx, -1, 0, 1, gx], [i > 0, j > 0, np.ones(m, bool), j < gx - 1, i < gy - 1])
    return rp, ci, np.where(k == 2, 4.0, -1.0)


def banded(m, lo, hi):
    """columns r + lo .. r + hi, clipped to the matrix: hi - lo + 1 cells per interior row"""
    r = np.arange(m, dtype=np.int64)
    offs = list(range(lo, hi + 1))
    rp, ci, k = stencil(m, offs, [(r + o >= 0) & (r + o < m) for o in offs])
    return rp, ci, np.where(np.array(offs)[k] == 0, float(2 * len(offs)), -1.0)


def laplace7(n):
    m = n ** 3
    r = np.arange(m, dtype=np.int64)
    i, j, k = r // (n * n), (r // n) % n, r % n
    rp, ci, q = stencil(m, [-n * n, -n, -1, 0, 1, n, n * n],
                        [i > 0, j > 0, k > 0, np.ones(m, bool), k < n - 1, j < n - 1, i < n - 1])
    return rp, ci, np.where(q == 3, 6.0, -1.0)


def same_list_blocks(m):
    """rows 64 k .. 64 k + 63 all carry the list 64 k + {0, 5, 17, 40}: one list per slice, no shift (mode 2)"""
    r = np.arange(m, dtype=np.int64)
    cols = ((r // 64) * 64)[:, None] + np.array([0, 5, 17, 40])
    rp = (4 * np.arange(m + 1)).astype(np.int32)
    return rp, cols.reshape(-1).astype(np.int32), np.where(np.arange(4 * m) % 4 == 1, 3.0, -0.5)


def scattered(m, seed):
    """3 to 5 ascending random columns per row: no two rows share a list (mode 3 everywhere, no uniform lists)"""
    rng = np.random.default_rng(seed)
    start = rng.integers(0, m - 5000, m)
    cols = start[:, None] + np.concatenate([np.zeros((m, 1), np.int64), np.cumsum(rng.integers(1, 1000, (m, 4)), axis=1)], axis=1)
    lens = rng.integers(3, 6, m)
    keep = np.arange(5)[None, :] < lens[:, None]
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    return rp.astype(np.int32), cols[keep].astype(np.int32), np.where(rng.integers(0, 2, int(lens.sum())) == 1, 1.5, -2.0)


def table_values(rp, ntab, dtype):
    """values tab[(7 i + 3 k) % ntab] for cell k of row i; the table holds +0.0 and -0.0"""
    k = np.arange(max(ntab - 2, 0))
    tab = np.concatenate([[0.0, -0.0], (0.375 + 0.125 * k) * (-1.0) ** k])[:ntab].astype(dtype)
    assert len(np.unique(bits(tab))) == ntab
    lens = np.diff(rp)
    i = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    k = np.arange(len(i), dtype=np.int64) - np.repeat(rp[:-1].astype(np.int64), lens)
    return np.ascontiguousarray(tab[(7 * i + 3 * k) % ntab])


# ---- what the plan must report ---------------------------------------------------------------------------------------------
def expected_packing(rp, ntab):
    """(index bits, word bytes) by the documented rule: fields of 1 / 2 / 4 / 8 bits, the smallest word that holds the widest row"""
    w = int(np.diff(rp).max())
    b = next(b for b in (1, 2, 4, 8) if (1 << b) >= ntab)
    if w * b > 32:
        return 0, 0
    return b, next(n for n in (1, 2, 4) if 8 * n >= w * b)


def expected_uniform(rp, ci):
    """full slices whose 64 rows have one length and repeat one column list, as it is or shifted by one per row"""
    m = len(rp) - 1
    lens = np.diff(rp)
    n = 0
    for s in range(m // 64):
        ls = lens[64 * s:64 * s + 64]
        if ls.min() != ls.max():
            continue
        if ls[0] == 0:
            n += 1
            continue
        d = np.diff(ci[rp[64 * s]:rp[64 * s + 64]].reshape(64, int(ls[0])).astype(np.int64), axis=0)
        n += bool(np.all(d == 1) or np.all(d == 0))
    return n


# ---- handles and products --------------------------------------------------------------------------------------------------
def handle(rp, ci, v, mode, op=P.OP_NONE, kid=None, n=None):
    m = len(rp) - 1
    A = P.Matrix(0, m, m if n is None else n, rp, ci, v)
    assert A.status == 0
    d = P.Descr()
    if kid is None:
        assert L.aoclsparse_set_mv_hint(A.h, op, d.h, 100) == 0
    else:
        assert L.aoclsparse_set_mv_hint_kid(A.h, op, d.h, 100, kid) == 0
    with sell_values(mode):
        assert L.aoclsparse_optimize(A.h) == 0
    return A, d


def product(A, d, x, y0, alpha, beta, op=P.OP_NONE, mode=-1):
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    yd = torch.from_numpy(np.ascontiguousarray(y0).copy()).cuda()
    with sell_values(mode):  # (a lazy rebuild after a value change reads the option again)
        st = (P.dmv if A.val.dtype == np.float64 else P.smv)(op, alpha, A, d, xd, beta, yd)
    assert st == 0, P.STATUS[st]
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def cpu_chain(v, ci, rp, x, y0, alpha, beta, kid=None, order=0):
    """the oracle in the pinned order: double by the reference's dispatch rule for the kid (-1: automatic), float by the kernel of
    the order the handle reports (0: the scalar chain, 2: eight lanes)"""
    m = len(rp) - 1
    if v.dtype == np.float32:
        st, y = oracle.scsrmv({0: "ref", 2: "lane8"}[order], 0, alpha, m, v, ci, rp, x, beta, y0)
    else:
        st, y = oracle.dcsrmv(-1 if kid is None else kid, 0, alpha, m, len(v), v, ci, rp, x, beta, y0)
    assert st == 0
    return y


def run_case(rp, ci, v, dtype, ntab, uniform=None, kid=None, seed=1):
    """the forced-table handle against the sell_values = 0 handle and the oracle; -> the packed handle's (bits, bytes, uniform)"""
    v = np.ascontiguousarray(v, dtype=dtype)
    m = len(rp) - 1
    assert (m + 63) // 64 >= MIN_SLICES and np.diff(rp).max() <= WMAX
    rng = np.random.default_rng(seed)
    x, y0 = rng.uniform(-1, 1, m).astype(dtype), rng.uniform(-1, 1, m).astype(dtype)
    A1, d1 = handle(rp, ci, v, 1, kid=kid)
    A0, d0 = handle(rp, ci, v, 0, kid=kid)
    assert A1.sell_values() == ntab and A0.sell_values() == 0
    assert A1.spmv_info().kernel in (3, 4) and A0.spmv_info().kernel == A1.spmv_info().kernel
    pb, pw, pu = A1.sell_packing()
    assert (pb, pw) == expected_packing(rp, ntab), (pb, pw)
    assert A0.sell_packing()[:2] == (0, 0)
    if uniform is None:
        uniform = expected_uniform(rp, ci)
    # (uniform lists are built next to packed words only: the sell_values = 0 handle runs the kernels it always had)
    assert pu == (uniform if pb else 0) and A0.sell_packing()[2] == 0, (pu, uniform)
    for alpha, beta in AB:
        ref = cpu_chain(v, ci, rp, x, y0, alpha, beta, kid, A1.spmv_info().order)
        for lap in range(2):
            y1 = product(A1, d1, x, y0, alpha, beta, mode=1)
            same_bits(y1, product(A0, d0, x, y0, alpha, beta, mode=0), ("option 0", alpha, beta, lap))
            same_bits(y1, ref, ("oracle", alpha, beta, lap))
    return pb, pw, pu


# ---- the cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("gx,gy", [(512, 512), (2048, 1920), (515, 509)])
def test_laplacians(gx, gy, dtype):
    """512 x 512: 4096 slices, one slice per wavefront, six slices in eight uniform; 2048 x 1920: 61,440 slices, several slices
    per wavefront; 515 x 509: m is no multiple of 64, the ends of the grid lines fall anywhere inside a slice (about one slice in
    eight reads its columns from the lists, and so does its whole group), a partial last slice"""
    rp, ci, v = laplace5_grid(gx, gy)
    pb, pw, pu = run_case(rp, ci, v, dtype, 2, seed=gx)
    nslices = (gx * gy + 63) // 64
    assert (pb, pw) == (1, 1)
    if gx % 64 == 0:
        assert pu == nslices * (gx // 64 - 2) // (gx // 64)
    else:  # (run_case has checked pu against the count from the CSR arrays: both kinds of group run)
        assert 0 < pu < nslices - nslices // 16


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["diagonal", "tridiagonal", "laplace7", "band8"])
def test_widths_1_to_8(name, dtype):
    m = 64 ** 3
    rp, ci, v = {"diagonal": lambda: banded(m, 0, 0), "tridiagonal": lambda: banded(m, -1, 1), "laplace7": lambda: laplace7(64),
                 "band8": lambda: banded(m, -4, 3)}[name]()
    assert int(np.diff(rp).max()) == {"diagonal": 1, "tridiagonal": 3, "laplace7": 7, "band8": 8}[name]
    ntab = 1 if name == "diagonal" else 2
    pb, pw, pu = run_case(rp, ci, v, dtype, ntab, seed=3)
    # (64^3: a slice is one grid line, whose first and last rows are shorter -- no slice of the 7-point stencil is uniform, all
    # its groups read the lists in col with packed words; the banded ones are uniform but for the first and the last slice)
    assert (pb, pw) == (1, 1) and (pu == 0 if name == "laplace7" else pu >= MIN_SLICES - 2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_list_per_slice_without_shift(dtype):
    """mode 2: every slice is uniform"""
    m = 64 * MIN_SLICES
    rp, ci, v = same_list_blocks(m)
    assert run_case(rp, ci, v, dtype, 2, uniform=MIN_SLICES, seed=4) == (1, 1, MIN_SLICES)


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_shared_lists_still_packs(dtype):
    """mode 3: no uniform lists, the columns come from the cells' own lists; the indices are packed all the same"""
    rp, ci, v = scattered(64 * MIN_SLICES, 5)
    assert run_case(rp, ci, v, dtype, 2, uniform=0, seed=5) == (1, 1, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ntab,name", [(2, "tridiagonal"), (3, "tridiagonal"), (4, "tridiagonal"), (5, "tridiagonal"),
                                       (16, "tridiagonal"), (17, "tridiagonal"), (256, "tridiagonal"), (3, "laplace7"),
                                       (16, "band8"), (5, "laplace5"), (17, "laplace5"), (256, "laplace5")])
def test_table_sizes(ntab, name, dtype):
    """fields of 1, 2, 4 and 8 bits in words of 1, 2 and 4 bytes; width 5 with 17 or 256 entries (40 bits) does not fit and keeps
    one byte per cell (index_bits 0) -- and still matches"""
    m = 64 * MIN_SLICES
    rp, ci, _ = {"tridiagonal": lambda: banded(m, -1, 1), "laplace7": lambda: laplace7(64), "band8": lambda: banded(m, -4, 3),
                 "laplace5": lambda: laplace5_grid(512, 512)}[name]()
    v = table_values(rp, ntab, dtype)
    pb, pw, pu = run_case(rp, ci, v, dtype, ntab, seed=ntab)
    w = int(np.diff(rp).max())
    if name == "laplace5" and ntab > 16:
        assert (pb, pw, pu) == (0, 0, 0)
    else:
        assert pb == {2: 1, 3: 2, 4: 2, 5: 4, 16: 4, 17: 8, 256: 8}[ntab] and 8 * pw >= w * pb > 4 * pw * (pw > 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kid", [1, 2, 3])
def test_pinned_kids_read_the_packed_words(kid, dtype):
    """kids 1 - 3 run the general kernel on the packed plan: the oracle in the pinned order (float has one kernel, eight lanes, which on
    rows of five cells is the scalar chain: the order the handle reports)"""
    rp, ci, _ = laplace5_grid(512, 512)
    v = table_values(rp, 5, dtype)
    m = len(rp) - 1
    rng = np.random.default_rng(kid)
    x, y0 = rng.uniform(-1, 1, m).astype(dtype), rng.uniform(-1, 1, m).astype(dtype)
    A1, d1 = handle(rp, ci, v, 1, kid=kid)
    A0, d0 = handle(rp, ci, v, 0, kid=kid)
    assert A1.sell_values() == 5 and A1.sell_packing()[:2] == (4, 4) and A0.sell_packing()[:2] == (0, 0)
    for alpha, beta in AB:
        for lap in range(2):
            y1 = product(A1, d1, x, y0, alpha, beta, mode=1)
            same_bits(y1, product(A0, d0, x, y0, alpha, beta, mode=0), ("option 0", alpha, beta, lap))
            same_bits(y1, cpu_chain(v, ci, rp, x, y0, alpha, beta, kid, A1.spmv_info().order), ("oracle", alpha, beta, lap))


@pytest.mark.parametrize("dtype", DTYPES)
def test_transposed_product_reads_the_packed_words(dtype):
    """the transposed plan is a SELL-64 copy of A^T: bits against option 0; the oracle's transposed product sums in another order
    (tolerance of tests/test_gpu_sell_values.py: test_transposed_plan)"""
    rp, ci, _ = laplace5_grid(512, 512)
    v = table_values(rp, 3, dtype)
    m = len(rp) - 1
    rng = np.random.default_rng(7)
    x, y0 = rng.uniform(-1, 1, m).astype(dtype), rng.uniform(-1, 1, m).astype(dtype)
    A1, d1 = handle(rp, ci, v, 1, op=P.OP_TRANSPOSE)
    A0, d0 = handle(rp, ci, v, 0, op=P.OP_TRANSPOSE)
    assert A1.sell_values(P.OP_TRANSPOSE) == 3 and A1.sell_packing(P.OP_TRANSPOSE)[:2] == (2, 2)
    for alpha, beta in AB:
        for lap in range(2):
            y1 = product(A1, d1, x, y0, alpha, beta, op=P.OP_TRANSPOSE, mode=1)
            same_bits(y1, product(A0, d0, x, y0, alpha, beta, op=P.OP_TRANSPOSE, mode=0), ("option 0", alpha, beta, lap))
        if dtype == np.float64:
            st, yo = oracle.dcsrmvt(0, alpha, m, m, v, ci, rp, x, beta, y0)
            absx = np.zeros(m)
            np.add.at(absx, ci, np.abs(v) * np.abs(np.repeat(x, np.diff(rp))))
            cnt = np.bincount(ci, minlength=m)
            assert st == 0 and np.all(np.abs(y1 - yo) <= (cnt + 4) * EPS64 * abs(alpha) * absx + 2 * EPS64 * np.abs(beta * y0) + 1e-300)


@pytest.mark.parametrize("dtype", DTYPES)
def test_value_changes_repack_and_fall_back(dtype):
    """2 -> 3 table entries by ?set_value: the fields grow from 1 to 2 bits; then > 256 distinct values: the plan holds values again
    (uniform lists go with the packed words).  The sell_values = 0 handle is given the same changes."""
    rp, ci, v = laplace5_grid(512, 512)
    m = len(rp) - 1
    dbl = dtype == np.float64
    # (a handle aliases its value array: ?update_values writes into it, so each handle gets its own)
    A1, d1 = handle(rp, ci, np.ascontiguousarray(v, dtype=dtype), 1)
    A0, d0 = handle(rp, ci, np.ascontiguousarray(v, dtype=dtype), 0)
    rng = np.random.default_rng(61)
    x, y0 = rng.uniform(-1, 1, m).astype(dtype), rng.uniform(-1, 1, m).astype(dtype)
    uniform = expected_uniform(rp, ci)

    def check(ntab, packing):
        for alpha, beta in AB:
            ref = None
            for lap in range(2):
                y1 = product(A1, d1, x, y0, alpha, beta, mode=1)
                if ref is None:  # (after the product: the rebuilt plan reports its order)
                    ref = cpu_chain(A1.val, A1.col_ind, A1.row_ptr, x, y0, alpha, beta, order=A1.spmv_info().order)
                same_bits(y1, product(A0, d0, x, y0, alpha, beta, mode=0), ("option 0", ntab, alpha, beta, lap))
                same_bits(y1, ref, ("oracle", ntab, alpha, beta, lap))
        assert A1.sell_values() == ntab and A1.sell_packing() == packing + (uniform if packing[0] else 0,)
        assert A0.sell_values() == 0 and A0.sell_packing() == (0, 0, 0)

    check(2, (1, 1))
    r = m // 2
    for A in (A1, A0):
        assert (L.aoclsparse_dset_value if dbl else L.aoclsparse_sset_value)(A.h, r, int(A.col_ind[int(A.row_ptr[r])]), 0.125) == 0
    check(3, (2, 2))
    many = np.ascontiguousarray(np.random.default_rng(62).uniform(-1, 1, 1000).astype(dtype)[np.arange(len(v)) % 1000])
    assert len(np.unique(bits(many))) > 256
    for A in (A1, A0):
        assert (L.aoclsparse_dupdate_values if dbl else L.aoclsparse_supdate_values)(A.h, len(many), P._ptr(many)) == 0
    check(0, (0, 0))
