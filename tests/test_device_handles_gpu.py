"""Matrix handles from, to and updated by CSR arrays in HBM: aoclsparse_mi355_create_?csr_device, ?update_values_device,
export_csr_device (device_handle_api.cpp, matcheck_kernels.hip) and their Python layer.

The yardstick everywhere is the HOST route of the same library on the same arrays (aoclsparse_create_?csr on numpy arrays): equal
statuses, equal sort class and full-diagonal flag, and products with the same bits -- plus the oracle for ?mv, so that "equal"
cannot mean "equally wrong".

The handle has no public getter for the sort class and the full-diagonal flag.  They are read through the two entry points that
refuse on them before anything else happens (probe()): aoclsparse_silu_smoother on a double handle answers unsorted_input for
class 3, numerical_error without a full diagonal and wrong_type otherwise; aoclsparse_dsyrkd with op = T and ldc = 0 answers
unsorted_input for class 2 / 3 and invalid_value for class 1.  After aoclsparse_optimize with a trsv hint, aoclsparse_export_dcsr
(clean copy or not) and aoclsparse_mi355_export_diag are compared as well."""
import ctypes
from ctypes import byref, c_void_p

import numpy as np
import pytest

import oracle
from util import laplace5, pkg, random_csr, triangular_system

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
P = pkg()
L = P.lib()

SUCCESS, NOT_IMPLEMENTED, INVALID_POINTER, INVALID_VALUE, INVALID_INDEX, WRONG_TYPE, NUMERICAL, UNSORTED = 0, 1, 2, 5, 6, 9, 11, 13


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    yield
    L.aoclsparse_mi355_set_pointer_mode(P.PTR_AUTO)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_arr(a):
    """device copy of an index / value array; an empty one becomes one element (an empty tensor has no address)"""
    a = np.ascontiguousarray(a)
    return dev(a if len(a) else np.zeros(1, a.dtype))


class HostMatrix(P.Matrix):
    """aoclsparse_create_?csr with an explicit nnz (P.Matrix derives it from row_ptr) and any of the four value types"""

    def __init__(self, base, m, n, nnz, rp, ci, v):
        self.row_ptr = np.ascontiguousarray(rp, dtype=np.int32)
        self.col_ind = np.ascontiguousarray(ci if len(ci) else np.zeros(1), dtype=np.int32)
        self.val = np.ascontiguousarray(v if len(v) else np.zeros(1, np.asarray(v).dtype))
        self.letter = P.Matrix._LETTER[str(self.val.dtype)]
        self.double = self.val.dtype == np.float64
        self.m, self.n, self.nnz, self.base = m, n, nnz, base
        self.h = c_void_p()
        fn = getattr(L, "aoclsparse_create_%scsr" % self.letter)
        self.status = fn(byref(self.h), base, m, n, nnz, P._ptr(self.row_ptr), P._ptr(self.col_ind), P._ptr(self.val))


def device_matrix(base, m, n, nnz, rp, ci, v):
    t = dev_arr(np.asarray(rp, np.int32)), dev_arr(np.asarray(ci, np.int32)), dev_arr(v)
    torch.cuda.synchronize()
    return P.Matrix.from_device(base, m, n, nnz, *t), t


def both(base, m, n, rp, ci, v, nnz=None):
    nnz = len(v) if nnz is None else nnz
    H = HostMatrix(base, m, n, nnz, rp, ci, v)
    D, _ = device_matrix(base, m, n, nnz, rp, ci, v)
    return H, D


_dummy = np.zeros(8, np.float32)


def probe(A):
    """(class 3 / no full diagonal / neither, class 1 or not) as the statuses of two calls that refuse before they compute"""
    pre = c_void_p()
    d = P.Descr(base=A.base)
    a = L.aoclsparse_silu_smoother(P.OP_NONE, A.h, d.h, byref(pre), None, P._ptr(_dummy), P._ptr(_dummy))
    b = L.aoclsparse_dsyrkd(P.OP_TRANSPOSE, A.h, 1.0, 0.0, P._ptr(_dummy), P.ORDER_ROW, 0)
    return a, b


CLASS1_FULL, CLASS1_NODIAG, CLASS2_FULL, CLASS3 = (WRONG_TYPE, INVALID_VALUE), (NUMERICAL, INVALID_VALUE), (WRONG_TYPE, UNSORTED), (UNSORTED, UNSORTED)


def same_analysis(H, D, want=None):
    """equal status; on success equal sort class and full-diagonal flag, and equal clean CSR after optimize with a trsv hint"""
    assert D.status == H.status, ("device %s, host %s" % (P.STATUS.get(D.status), P.STATUS.get(H.status)))
    if H.status != 0:
        assert not D.h.value
        return
    ph, pd = probe(H), probe(D)
    assert pd == ph, ("sort class / full diagonal differ: device %s, host %s" % (pd, ph))
    if want is not None:
        assert ph == want, (ph, want)  # (the probe tells the classes apart on this input)
    if H.m != H.n:
        return
    outs = []
    for A in (H, D):
        d = P.Descr(base=A.base, mtype=P.TYPE_TRIANGULAR, fill=P.FILL_LOWER)
        assert L.aoclsparse_set_sv_hint(A.h, P.OP_NONE, d.h, 1) == 0
        outs.append((L.aoclsparse_optimize(A.h), A.export(), A.export_diag()))
    (sh, eh, dh), (sd, ed, dd) = outs
    assert sd == sh
    if sh != 0:
        return
    assert ed["status"] == 0 and dd["status"] == dh["status"] == 0
    assert dd["is_internal"] == dh["is_internal"]  # clean copy made or not
    assert eh["aliased"] == (not dh["is_internal"])
    for k in ("base", "m", "n", "nnz"):
        assert ed[k] == eh[k], k
    for k in ("row_ptr", "col_ind", "val"):
        assert np.array_equal(ed[k], eh[k]), k
    assert np.array_equal(dd["idiag"], dh["idiag"]) and np.array_equal(dd["iurow"], dh["iurow"])


# --------------------------------------------------------------------------------------------------
# the check kernel against mat_check
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("m,n", [(1, 40), (63, 63), (64, 64), (65, 65), (257, 257), (6000, 6000), (300, 200), (200, 300)])
def test_random_matrices(m, n, sort, base):
    """sorted and shuffled rows (some empty), one block and many, tall and wide, both bases"""
    rp, ci, v = random_csr(m + 7 * n, m, n, lambda r, i: r.integers(0, 12), base=base, sort=sort)
    assert np.any(np.diff(rp) == 0) or m == 1
    H, D = both(base, m, n, rp, ci, v)
    assert H.status == 0
    same_analysis(H, D)


def test_no_entries_and_no_rows():
    for base in (0, 1):
        rp = np.full(6, base, np.int32)
        same_analysis(*both(base, 5, 5, rp, np.zeros(0, np.int32), np.zeros(0)), want=CLASS1_NODIAG)
        same_analysis(*both(base, 5, 0, rp, np.zeros(0, np.int32), np.zeros(0)), want=(WRONG_TYPE, SUCCESS))  # no row i < n
        H, D = both(base, 0, 5, rp[:1], np.zeros(0, np.int32), np.zeros(0))
        assert H.status == 0
        same_analysis(H, D)


ROW, M_SP, N_SP = 7, 20, 6000


def special(length, base=0, edit=None, other=None):
    """20 x 6000 (or square 6000 x 6000 when other == "square"), sorted rows with their diagonal; row 7 has `length` sorted entries
    with its diagonal at position 4 (columns 1 3 5 6 | 7 | upper ones).  edit(cols) -> the row's new column list (0-based);
    other(rows) may change the other rows (a dict row -> column list)."""
    rng = np.random.default_rng(length)
    m = N_SP if other == "square" else M_SP
    rows = {}
    for i in range(m):
        c = np.unique(np.concatenate([rng.integers(0, N_SP, size=5), [i]]))
        rows[i] = c
    up = np.sort(rng.choice(np.arange(ROW + 1, N_SP), size=length - 5, replace=False))
    cols = np.concatenate([[1, 3, 5, 6, ROW], up])
    rows[ROW] = np.asarray(edit(cols.copy()) if edit else cols)
    if callable(other):
        other(rows)
    lens = np.array([len(rows[i]) for i in range(m)])
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32) + base
    ci = (np.concatenate([rows[i] for i in range(m)]) + base).astype(np.int32)
    v = rng.uniform(-1, 1, len(ci))
    return base, m, N_SP, rp, ci, v


def swap(a, b):
    def f(c):
        c[a], c[b] = c[b], c[a]
        return c
    return f


def move_to_end(a):
    return lambda c: np.concatenate([np.delete(c, a), [c[a]]])


def diag_first(c):
    return np.concatenate([[ROW], c[:4], c[5:]])


@pytest.mark.parametrize("length", [12, 64, 65, 5000])
def test_row_lengths_around_the_wavefront_threshold(length):
    """a sorted row of 64 entries (a lane), 65 (its wavefront) and 5,000 (79 passes of it)"""
    for base in (0, 1):
        same_analysis(*both(*special(length, base)), want=CLASS1_FULL)
    same_analysis(*both(*special(length, 0, other="square")), want=CLASS1_FULL)


@pytest.mark.parametrize("length", [12, 65, 5000])
def test_sort_classes(length):
    far = length - 2
    # class 2: the groups L | D | U are kept, the order inside one is broken
    same_analysis(*both(*special(length, 0, swap(0, 2))), want=CLASS2_FULL)  # inside L
    same_analysis(*both(*special(length, 1, swap(far, far + 1))), want=CLASS2_FULL)  # inside U, adjacent entries
    same_analysis(*both(*special(length, 0, swap(5, far))), want=CLASS2_FULL)  # inside U, far apart
    if length > 200:  # neighbours held by two lanes / by the last lane of one pass and the first of the next
        same_analysis(*both(*special(length, 0, swap(100, 101))), want=CLASS2_FULL)
        same_analysis(*both(*special(length, 0, swap(127, 128))), want=CLASS2_FULL)
    # class 3: an entry <= i behind an upper one (a lower entry / the diagonal moved to the row's end) ...
    same_analysis(*both(*special(length, 0, move_to_end(2))), want=CLASS3)
    same_analysis(*both(*special(length, 1, move_to_end(4))), want=CLASS3)
    same_analysis(*both(*special(length, 0, swap(4, 5))), want=CLASS3)  # the diagonal right behind the first upper entry
    # ... or an entry < i behind the diagonal (no upper entry in front of it)
    same_analysis(*both(*special(length, 0, diag_first)), want=CLASS3)
    same_analysis(*both(*special(length, 1, swap(3, 4))), want=CLASS3)
    # unsorted in one row only of a large square matrix: the clean copy is made
    same_analysis(*both(*special(length, 0, move_to_end(1), other="square")), want=CLASS3)


@pytest.mark.parametrize("length", [12, 65, 5000])
def test_missing_diagonals(length):
    same_analysis(*both(*special(length, 0, lambda c: np.delete(c, 4))), want=CLASS1_NODIAG)
    same_analysis(*both(*special(length, 1, lambda c: np.delete(c, 4), other="square")), want=CLASS1_NODIAG)
    # an upper entry in front of the lower ones AND no diagonal
    same_analysis(*both(*special(length, 0, lambda c: move_to_end(0)(np.delete(c, 4)))), want=(UNSORTED, UNSORTED))


def test_tall_matrix_misses_diagonals_only_in_rows_beyond_n():
    m, n = 90, 70
    rows = [np.unique(np.concatenate([[min(i, n - 1)], [i % 13, (5 * i) % n]])) for i in range(m)]
    for i in range(n, m):  # rows >= n cannot hold a diagonal entry
        assert i not in rows[i]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    v = np.random.default_rng(1).uniform(-1, 1, len(ci))
    same_analysis(*both(0, m, n, rp, ci, v), want=CLASS1_FULL)
    # ... and one row < n without it
    keep = np.ones(len(ci), bool)
    keep[rp[5] + int(np.nonzero(ci[rp[5]:rp[6]] == 5)[0][0])] = False
    rp2 = np.concatenate([[0], np.cumsum(np.add.reduceat(keep.astype(int), rp[:-1]))]).astype(np.int32)
    same_analysis(*both(0, m, n, rp2, ci[keep], v[keep]), want=CLASS1_NODIAG)


def set_at(pos, col):
    def f(c):
        c[pos] = col
        return c
    return f


def chain(*fs):
    def f(c):
        for g in fs:
            c = g(c)
        return c
    return f


@pytest.mark.parametrize("length", [12, 65, 5000])
def test_invalid_entries(length):
    far, mid = length - 3, length // 2
    for base in (0, 1):
        for pos in (0, mid, far):
            H, D = both(*special(length, base, set_at(pos, N_SP)))  # a column == n (0-based)
            assert H.status == INVALID_INDEX
            same_analysis(H, D)
            H, D = both(*special(length, base, set_at(pos, -1)))  # a column < base
            assert H.status == INVALID_INDEX
            same_analysis(H, D)
    for pos in (5, mid, far):  # a second diagonal entry
        H, D = both(*special(length, 0, set_at(pos, ROW)))
        assert H.status == INVALID_VALUE
        same_analysis(H, D)
    # both in one row: whichever comes first decides
    pairs = [(5, far), (mid, far), (5, 6)] + ([(64 + 5, 128 + 5), (100, 4000)] if length > 200 else [])
    for a, b in pairs:
        H, D = both(*special(length, 0, chain(set_at(a, N_SP), set_at(b, ROW))))
        assert H.status == INVALID_INDEX
        same_analysis(H, D)
        H, D = both(*special(length, 1, chain(set_at(a, ROW), set_at(b, -1))))
        assert H.status == INVALID_VALUE
        same_analysis(H, D)
    # a bad index in FRONT of the diagonal's first occurrence and a second diagonal behind it
    H, D = both(*special(length, 0, chain(set_at(2, N_SP + 3), set_at(far, ROW))))
    assert H.status == INVALID_INDEX
    same_analysis(H, D)


def test_the_earlier_row_decides():
    def dup_in_row_10(rows):
        rows[10] = np.concatenate([rows[10], [10]])
        rows[3] = np.concatenate([rows[3], [N_SP]])
    H, D = both(*special(12, 0, other=dup_in_row_10))
    assert H.status == INVALID_INDEX
    same_analysis(H, D)

    def bad_in_row_10(rows):
        rows[10] = np.concatenate([rows[10], [N_SP]])
        rows[3] = np.concatenate([rows[3], [3]])
    H, D = both(*special(5000, 0, set_at(4000, N_SP), other=bad_in_row_10))  # rows 3 (dup), 7 (bad, long), 10 (bad)
    assert H.status == INVALID_VALUE
    same_analysis(H, D)


def test_bad_row_pointers_are_refused_before_the_columns_are_read():
    base, m, n, rp, ci, v = special(12)
    nnz = len(v)
    for b in (0, 1):
        r = rp + b
        r1 = r.copy()
        r1[0] += 1  # row_ptr[0] != base
        H, D = both(b, m, n, r1, ci + b, v)
        assert H.status == INVALID_VALUE
        same_analysis(H, D)
        H, D = both(b, m, n, r, ci + b, v, nnz=nnz - 1)  # row_ptr[m] - base != nnz
        assert H.status == INVALID_VALUE
        same_analysis(H, D)
        H, D = both(b, m, n, r, ci + b, v, nnz=nnz + 1)
        assert H.status == INVALID_VALUE
        same_analysis(H, D)
        # decreasing, with entries far beyond nnz: first and last entry are right, so only the monotonicity test can refuse it --
        # and it must, before any column is read with such bounds
        r2 = r.copy()
        r2[4], r2[5], r2[11] = 1_000_000_000, 3, 2_000_000_000
        H, D = both(b, m, n, r2, ci + b, v)
        assert H.status == INVALID_VALUE
        assert D.status == INVALID_VALUE
        same_analysis(H, D)


def test_arrays_that_are_not_device_memory():
    base, m, n, rp, ci, v = special(12)
    t = [dev_arr(rp), dev_arr(ci), dev_arr(v)]
    torch.cuda.synchronize()
    for k, host in enumerate((rp, ci, v)):
        args = list(t)
        args[k] = host
        torch.cuda.synchronize()
        A = P.Matrix.from_device(base, m, n, len(v), *args)
        assert A.status == INVALID_POINTER and not A.h.value


def test_a_base_outside_0_1_answers_as_the_host_call():
    """aoclsparse_create_dcsr does not refuse the base as such: the arrays are checked against it"""
    _, m, n, rp, ci, v = special(12)
    statuses = []
    for arrays_base in (0, 2):
        H, D = both(2, m, n, rp + arrays_base, ci + arrays_base, v)
        assert D.status == H.status
        statuses.append(H.status)
    assert statuses[0] == INVALID_VALUE  # row_ptr[0] != 2


# --------------------------------------------------------------------------------------------------
# the handle does not depend on the caller's arrays
# --------------------------------------------------------------------------------------------------
def run_dmv(A, x, y0, alpha=1.3, beta=-0.4, op=P.OP_NONE, d=None):
    yd = dev(y0)
    assert P.dmv(op, alpha, A, d or P.Descr(base=A.base), dev(x), beta, yd) == 0
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def test_independent_of_the_callers_arrays_and_resident_at_once():
    m = 3000
    rp, ci, v = random_csr(17, m, m, lambda r, i: r.integers(1, 20))
    D, t = device_matrix(0, m, m, len(v), rp, ci, v)
    assert D.status == 0
    assert D.spmv_info().device_resident == 1  # before any product
    for a in t:
        a.zero_()
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    x, y0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)
    so, yr = oracle.dcsrmv(-1, 0, 1.3, m, len(v), v, ci, rp, x, -0.4, y0)
    assert so == 0
    assert np.array_equal(run_dmv(D, x, y0), yr)
    e = D.export()  # the owned host view
    assert np.array_equal(e["row_ptr"], rp) and np.array_equal(e["col_ind"], ci) and np.array_equal(e["val"], v)


# --------------------------------------------------------------------------------------------------
# the same bits as a host-created handle
# --------------------------------------------------------------------------------------------------
def _matrix(name):
    if name == "random6000":
        m = 6000
        return (m,) + random_csr(23, m, m, lambda r, i: r.integers(1, 24))
    m, rp, ci, v = laplace5(64)
    return m, rp, ci, v * np.random.default_rng(8).uniform(0.5, 1.5, len(v))


@pytest.fixture
def forced_sell():
    assert L.aoclsparse_mi355_set_option(P.OPTION_SELL, 1) == 0
    yield
    assert L.aoclsparse_mi355_set_option(P.OPTION_SELL, -1) == 0


@pytest.mark.parametrize("name", ["random6000", "laplace64"])
def test_dmv_same_bits(name, forced_sell):
    m, rp, ci, v = _matrix(name)
    rng = np.random.default_rng(5)
    x, y0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)
    so, yr = oracle.dcsrmv(-1, 0, 1.3, m, len(v), v, ci, rp, x, -0.4, y0)
    assert so == 0
    for optimize in (False, True):
        H, D = both(0, m, m, rp, ci, v)
        assert H.status == 0 and D.status == 0
        d = P.Descr()
        if optimize:  # an mv hint + optimize: the SELL-64 copy (forced, so that the small input reaches it)
            for A in (H, D):
                assert L.aoclsparse_set_mv_hint(A.h, P.OP_NONE, d.h, 100) == 0 and L.aoclsparse_optimize(A.h) == 0
        yh, yd = run_dmv(H, x, y0, d=d), run_dmv(D, x, y0, d=d)
        assert np.array_equal(yd, yh)
        assert np.array_equal(yd, yr), "differs from the oracle"
        ih, idv = H.spmv_info(), D.spmv_info()
        assert (idv.kernel, idv.order, idv.sell_slices) == (ih.kernel, ih.order, ih.sell_slices)
        if optimize:
            assert idv.kernel in (3, 4), idv.kernel
        assert np.array_equal(run_dmv(D, y0, x, op=P.OP_TRANSPOSE, d=d), run_dmv(H, y0, x, op=P.OP_TRANSPOSE, d=d))


@pytest.mark.parametrize("name", ["random6000", "laplace64"])
def test_csrmm_copy_and_sp2m_same_bits(name):
    m, rp, ci, v = _matrix(name)
    H, D = both(0, m, m, rp, ci, v)
    d = P.Descr()
    n = 8
    rng = np.random.default_rng(6)
    B, C0 = rng.uniform(-1, 1, m * n), rng.uniform(-1, 1, m * n)
    for order, ld in ((P.ORDER_ROW, n), (P.ORDER_COLUMN, m)):
        out = []
        for A in (H, D):
            Cd = dev(C0)
            assert P.dcsrmm(P.OP_NONE, 1.25, A, d, order, dev(B), n, ld, -0.5, Cd, ld) == 0
            torch.cuda.synchronize()
            out.append(Cd.cpu().numpy())
        assert np.array_equal(out[1], out[0]), order
    # aoclsparse_copy, then dmv on the copy
    x, y0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)
    ys = []
    for A in (H, D):
        c = c_void_p()
        assert L.aoclsparse_copy(A.h, d.h, byref(c)) == 0
        C = P.Matrix.from_handle(c)
        ys.append(run_dmv(C, x, y0))
    assert np.array_equal(ys[1], ys[0])
    # sp2m of the handle with itself
    es = []
    for A in (H, D):
        c = c_void_p()
        assert L.aoclsparse_sp2m(P.OP_NONE, d.h, A.h, P.OP_NONE, d.h, A.h, P.STAGE_FULL, byref(c)) == 0
        es.append(P.Matrix.from_handle(c).export())
    for k in ("row_ptr", "col_ind", "val"):
        assert np.array_equal(es[1][k], es[0][k]), k


def test_dtrsv_same_bits():
    m = 3000
    rp, ci, v = triangular_system(31, m, 4, band=60)
    b = np.random.default_rng(2).uniform(-1, 1, m)
    H, D = both(0, m, m, rp, ci, v)
    for fill in (P.FILL_LOWER, P.FILL_UPPER):
        d = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=fill)
        xs = []
        for A in (H, D):
            xd = torch.full((m,), 7.0, dtype=torch.float64, device="cuda")
            assert P.dtrsv(P.OP_NONE, 0.75, A, d, dev(b), xd) == 0
            torch.cuda.synchronize()
            xs.append(xd.cpu().numpy())
        assert np.array_equal(xs[1], xs[0]), fill
        assert np.all(np.isfinite(xs[1]))


@pytest.mark.parametrize("name", ["random6000", "laplace64"])
def test_float_and_complex_handles_same_bits(name):
    m, rp, ci, v = _matrix(name)
    rng = np.random.default_rng(9)
    # smv
    vf = v.astype(np.float32)
    H, D = both(0, m, m, rp, ci, vf)
    assert H.status == 0 and D.status == 0 and D.letter == "s"
    x, y0 = rng.uniform(-1, 1, m).astype(np.float32), rng.uniform(-1, 1, m).astype(np.float32)
    d = P.Descr()
    ys = []
    for A in (H, D):
        yd = dev(y0)
        assert P.smv(P.OP_NONE, 1.5, A, d, dev(x), 0.25, yd) == 0
        torch.cuda.synchronize()
        ys.append(yd.cpu().numpy())
    assert np.array_equal(ys[1], ys[0])
    # zmv (and cmv)
    for dt, fn, ct in ((np.complex128, L.aoclsparse_zmv, P.CDouble), (np.complex64, L.aoclsparse_cmv, P.CFloat)):
        vz = (v + 1j * rng.uniform(-1, 1, len(v))).astype(dt)
        H, D = both(0, m, m, rp, ci, vz)
        assert H.status == 0 and D.status == 0
        xz = (rng.uniform(-1, 1, m) + 1j * rng.uniform(-1, 1, m)).astype(dt)
        yz = (rng.uniform(-1, 1, m) + 1j * rng.uniform(-1, 1, m)).astype(dt)
        a, b = ct(1.25, -0.5), ct(0.5, 0.25)
        ys = []
        for A in (H, D):
            yd = dev(yz)
            assert fn(P.OP_NONE, byref(a), A.h, d.h, P._ptr(dev(xz)), byref(b), P._ptr(yd)) == 0
            torch.cuda.synchronize()
            ys.append(yd.cpu().numpy())
        assert np.array_equal(ys[1], ys[0]), dt
        ref = (1.25 - 0.5j) * _dense_mv(m, rp, ci, vz.astype(np.complex128), xz.astype(np.complex128)) + (0.5 + 0.25j) * yz
        eps = np.finfo(np.float64 if dt == np.complex128 else np.float32).eps
        # (24 entries per row at most, complex products: a generous componentwise forward bound, to pin "equal" to "right")
        scale = 2.0 * (_dense_mv(m, rp, ci, np.abs(vz).astype(np.float64), np.abs(xz).astype(np.float64)) + np.abs(yz))
        assert np.all(np.abs(ys[1] - ref) <= 64 * eps * scale + 1e-300)


def _dense_mv(m, rp, ci, v, x):
    prod = v * x[ci]
    out = np.zeros(m, prod.dtype)
    nz = np.diff(rp) > 0
    out[nz] = np.add.reduceat(prod, rp[:-1][nz])
    return out


# --------------------------------------------------------------------------------------------------
# update_values_device
# --------------------------------------------------------------------------------------------------
def _three_products(A, dg, dt, x, B, C0, n):
    m = A.m
    y = run_dmv(A, x, x[::-1].copy(), d=dg)
    Cd = dev(C0)
    assert P.dcsrmm(P.OP_NONE, 1.25, A, dg, P.ORDER_ROW, dev(B), n, n, -0.5, Cd, n) == 0
    xd = torch.full((m,), 7.0, dtype=torch.float64, device="cuda")
    assert P.dtrsv(P.OP_NONE, 1.0, A, dt, dev(x), xd) == 0
    torch.cuda.synchronize()
    return y, Cd.cpu().numpy(), xd.cpu().numpy()


@pytest.mark.parametrize("created", ["device", "host"])
def test_update_values_device(created, forced_sell):
    m = 4000
    rp, ci, v = triangular_system(41, m, 5, band=80)
    v2 = np.ascontiguousarray(v * np.random.default_rng(12).uniform(0.5, 1.5, len(v)))
    dg, dt = P.Descr(), P.Descr(mtype=P.TYPE_TRIANGULAR, fill=P.FILL_LOWER)
    n = 8
    rng = np.random.default_rng(13)
    x, B, C0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m * n), rng.uniform(-1, 1, m * n)

    def hinted(A):
        assert A.status == 0
        assert L.aoclsparse_set_mv_hint(A.h, P.OP_NONE, dg.h, 100) == 0 and L.aoclsparse_optimize(A.h) == 0
        return A

    if created == "device":
        A = hinted(device_matrix(0, m, m, len(v), rp, ci, v)[0])
    else:
        A = hinted(HostMatrix(0, m, m, len(v), rp, ci, v.copy()))
    old = _three_products(A, dg, dt, x, B, C0, n)
    assert A.spmv_info().kernel in (3, 4) and A.spmv_info().device_resident == 1
    t2 = dev(v2)
    torch.cuda.synchronize()
    assert A.update_values_device(t2) == 0
    assert A.spmv_info().device_resident == 1  # straight after the update: the next product uploads nothing
    t2.zero_()  # (the values were copied)
    torch.cuda.synchronize()
    assert np.array_equal(A.export()["val"], v2)
    if created == "host":
        assert np.array_equal(A.val, v2)  # the host view of a host-created handle is the caller's array, as with ?update_values
    new = _three_products(A, dg, dt, x, B, C0, n)
    assert A.spmv_info().kernel in (3, 4)
    fresh = _three_products(hinted(HostMatrix(0, m, m, len(v), rp, ci, v2.copy())), dg, dt, x, B, C0, n)
    for got, want, before, what in zip(new, fresh, old, ("dmv", "dcsrmm", "dtrsv")):
        assert np.array_equal(got, want), what
        assert not np.array_equal(got, before), what
    so, yr = oracle.dcsrmv(-1, 0, 1.3, m, len(v2), v2, ci, rp, x, -0.4, x[::-1].copy())
    assert so == 0 and np.array_equal(new[0], yr)
    # a second update, onto the resident copy the first one left: back to the old values
    t3 = dev(v)
    torch.cuda.synchronize()
    assert A.update_values_device(t3) == 0
    again = _three_products(A, dg, dt, x, B, C0, n)
    for got, want, what in zip(again, old, ("dmv", "dcsrmm", "dtrsv")):
        assert np.array_equal(got, want), what
    # a wrong length and a host array are refused, and leave the handle as it is
    assert A.update_values_device(dev(v2[:-1])) == 3
    assert L.aoclsparse_mi355_dupdate_values_device(A.h, len(v2), P._ptr(v2)) == INVALID_POINTER
    assert np.array_equal(run_dmv(A, x, x[::-1].copy(), d=dg), old[0])


def test_update_values_device_is_refused_by_csc_and_tcsr_handles():
    m, rp, ci, v = laplace5(20)
    v = v * np.random.default_rng(1).uniform(0.5, 1.5, len(v))
    x = np.random.default_rng(2).uniform(-1, 1, m)
    new = dev(np.ones(len(v)))
    torch.cuda.synchronize()
    # created from CSC arrays
    st, cp, ri, cv = oracle.dcsr2csc(m, m, len(v), 0, 0, rp, ci, v)
    assert st == 0
    cp, ri, cv = cp.astype(np.int32), ri.astype(np.int32), np.ascontiguousarray(cv)
    C = P.Matrix.__new__(P.Matrix)
    C.row_ptr = C.col_ind = C.val = None
    C.double, C.m, C.n, C.nnz, C.base, C.h = True, m, m, len(v), 0, c_void_p()
    assert L.aoclsparse_create_dcsc(byref(C.h), 0, m, m, len(v), P._ptr(cp), P._ptr(ri), P._ptr(cv)) == 0
    y0 = run_dmv(C, x, x)
    assert L.aoclsparse_mi355_dupdate_values_device(C.h, len(v), P._ptr(new)) == NOT_IMPLEMENTED
    assert np.array_equal(run_dmv(C, x, x), y0)
    # TCSR
    rid = np.repeat(np.arange(m), np.diff(rp))

    def tri(keep):
        p = np.concatenate([[0], np.cumsum(np.add.reduceat(keep.astype(int), rp[:-1]))]).astype(np.int32)
        return p, ci[keep].copy(), v[keep].copy()

    T = P.TcsrMatrix(0, m, *tri(ci <= rid), *tri(ci >= rid))
    assert T.status == 0
    y0 = run_dmv(T, x, x)
    assert L.aoclsparse_mi355_dupdate_values_device(T.h, T.nnz, P._ptr(new)) == NOT_IMPLEMENTED
    assert np.array_equal(run_dmv(T, x, x), y0)


# --------------------------------------------------------------------------------------------------
# export_csr_device
# --------------------------------------------------------------------------------------------------
def fetch(addr, count, dtype):
    """count elements at a device address -> numpy (hipMemcpy through torch's runtime would need a tensor: the library's own
    device-to-host path is a dmv away, so a plain ctypes hipMemcpy it is)"""
    out = np.zeros(max(count, 1), dtype)
    hip = ctypes.CDLL(P.hip_runtime_path()[1])
    hip.hipMemcpy.argtypes = [c_void_p, c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip.hipMemcpy(P._ptr(out), c_void_p(addr), count * out.itemsize, 2) == 0  # hipMemcpyDeviceToHost
    return out[:count]


def exported(A, dtype=np.float64):
    e = A.export_device()
    assert e["status"] == 0, P.STATUS.get(e["status"])
    return e, fetch(e["row_ptr"], e["m"] + 1, np.int32), fetch(e["col_ind"], e["nnz"], np.int32), fetch(e["val"], e["nnz"], dtype)


def test_export_csr_device():
    m, n = 700, 900
    rp, ci, v = random_csr(51, m, n, lambda r, i: r.integers(0, 15), base=1)
    # a host-created handle (not resident yet: uploaded by the export)
    H = HostMatrix(1, m, n, len(v), rp, ci, v)
    assert H.spmv_info().device_resident == 0
    e, erp, eci, ev = exported(H)
    assert (e["base"], e["m"], e["n"], e["nnz"]) == (1, m, n, len(v))
    assert np.array_equal(erp, rp) and np.array_equal(eci, ci) and np.array_equal(ev, v)
    assert H.spmv_info().device_resident == 1
    # an sp2m result
    d = P.Descr(base=1)
    c = c_void_p()
    assert L.aoclsparse_sp2m(P.OP_NONE, d.h, H.h, P.OP_TRANSPOSE, d.h, H.h, P.STAGE_FULL, byref(c)) == 0
    C = P.Matrix.from_handle(c)
    ec = C.export()
    e, erp, eci, ev = exported(C)
    assert (e["base"], e["m"], e["n"], e["nnz"]) == (ec["base"], m, m, ec["nnz"])
    assert np.array_equal(erp, ec["row_ptr"]) and np.array_equal(eci, ec["col_ind"]) and np.array_equal(ev, ec["val"])
    # a device-created handle: its exported pointers make a second handle with the same product
    D, _ = device_matrix(1, m, n, len(v), rp, ci, v)
    e = D.export_device()
    assert e["status"] == 0
    torch.cuda.synchronize()
    D2 = P.Matrix.from_device(e["base"], e["m"], e["n"], e["nnz"], e["row_ptr"], e["col_ind"], e["val"], dtype="float64")
    assert D2.status == 0
    rng = np.random.default_rng(4)
    x, y0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, m)
    y1, y2 = run_dmv(D, x, y0), run_dmv(D2, x, y0)
    assert np.array_equal(y2, y1)
    so, yr = oracle.dcsrmv(-1, 1, 1.3, m, len(v), v, ci, rp, x, -0.4, y0)
    assert so == 0 and np.array_equal(y1, yr)
    # a float handle: val points to floats
    F, _ = device_matrix(1, m, n, len(v), rp, ci, v.astype(np.float32))
    assert np.array_equal(exported(F, np.float32)[3], v.astype(np.float32))


# --------------------------------------------------------------------------------------------------
# Python layer
# --------------------------------------------------------------------------------------------------
def test_from_torch_csr():
    m, n = 500, 400
    rp, ci, v = random_csr(61, m, n, lambda r, i: r.integers(0, 9))
    t = torch.sparse_csr_tensor(torch.from_numpy(rp.astype(np.int64)), torch.from_numpy(ci.astype(np.int64)), torch.from_numpy(v),
                                size=(m, n)).cuda()
    A = P.Matrix.from_torch_csr(t)
    assert A.status == 0 and (A.m, A.n, A.nnz) == (m, n, len(v)) and A.double
    assert A.spmv_info().device_resident == 1
    rng = np.random.default_rng(5)
    x, y0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, m)
    so, yr = oracle.dcsrmv(-1, 0, 1.3, m, len(v), v, ci, rp, x, -0.4, y0)
    assert so == 0
    assert np.array_equal(run_dmv(A, x, y0), yr)
    # one-based, and float32 values
    A1 = P.Matrix.from_torch_csr(t, base=1)
    assert A1.status == 0 and A1.base == 1
    assert np.array_equal(run_dmv(A1, x, y0), yr)
    tf = torch.sparse_csr_tensor(t.crow_indices(), t.col_indices(), t.values().to(torch.float32), size=(m, n))
    Af = P.Matrix.from_torch_csr(tf)
    assert Af.status == 0 and Af.letter == "s"
    # new values from a tensor
    v2 = dev(2.0 * v)
    torch.cuda.synchronize()
    assert A.update_values_device(v2) == 0
    so, yr2 = oracle.dcsrmv(-1, 0, 1.3, m, len(v), 2.0 * v, ci, rp, x, -0.4, y0)
    assert np.array_equal(run_dmv(A, x, y0), yr2)
