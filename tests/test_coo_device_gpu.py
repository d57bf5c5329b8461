"""CSR handles from unordered (row, col, value) triplets in HBM: aoclsparse_mi355_create_?csr_from_coo_device
(device_handle_api.cpp, coo_sort_kernels.hip) and Matrix.from_coo_device / Matrix.from_torch_coo.

`keep` mode: the yardstick is the library's own HOST route on the same numpy triplets -- aoclsparse_create_?coo, then
aoclsparse_convert_csr (the reference's stable counting sort by row), aoclsparse_export_?csr, and aoclsparse_create_?csr on those
arrays for the status, the sort class and the full-diagonal flag.  Integers must be equal, values bitwise equal; one dmv goes
against the oracle so that "equal" cannot mean "equally wrong".

`sum` mode: the yardstick is restated here (sum_reference): np.lexsort((col, row)), which is stable, then an explicit loop that
adds every run of equal coordinates from left to right in the value's dtype.  Bitwise equal again: the chain order is part of the
interface.

T = P.COO_SORT_TILE is what a workgroup of the sort takes per pass (AOCLSPARSE_MI355_COO_SORT_TILE in the header); the sizes
around it, around the wavefront (64) and around the digit boundaries of M (2^8, 2^16, 2^24) are where the sort can go wrong."""
import ctypes
from ctypes import byref, c_int, c_int32, c_void_p

import numpy as np
import pytest

import oracle
from util import EPS64, abs_row_sums, pkg, random_csr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
P = pkg()
L = P.lib()
T = P.COO_SORT_TILE

SUCCESS, INVALID_POINTER, INVALID_VALUE, INVALID_INDEX, WRONG_TYPE, NUMERICAL, UNSORTED = 0, 2, 5, 6, 9, 11, 13
KEEP, SUM = P.COO_KEEP, P.COO_SUM
LETTER = {np.dtype(np.float32): "s", np.dtype(np.float64): "d", np.dtype(np.complex64): "c", np.dtype(np.complex128): "z"}


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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


_dummy = np.zeros(8, np.float32)


def probe(A):
    """(class 3 / no full diagonal / neither, class 1 or not) as the statuses of two calls that refuse before they compute
    (tests/test_device_handles_gpu.py explains them)"""
    pre = c_void_p()
    d = P.Descr(base=A.base)
    a = L.aoclsparse_silu_smoother(P.OP_NONE, A.h, d.h, byref(pre), None, P._ptr(_dummy), P._ptr(_dummy))
    b = L.aoclsparse_dsyrkd(P.OP_TRANSPOSE, A.h, 1.0, 0.0, P._ptr(_dummy), P.ORDER_ROW, 0)
    return a, b


def export_host(h, dtype):
    """aoclsparse_export_?csr of a raw handle -> (status, base, m, n, nnz, row_ptr, col_ind, val) as copies"""
    base, m, n, nnz = c_int(), c_int32(), c_int32(), c_int32()
    rp, ci, v = c_void_p(), c_void_p(), c_void_p()
    fn = getattr(L, "aoclsparse_export_%scsr" % LETTER[np.dtype(dtype)])
    st = fn(h, byref(base), byref(m), byref(n), byref(nnz), byref(rp), byref(ci), byref(v))
    if st != 0:
        return (st,)

    def arr(p, count, dt):
        return np.frombuffer(ctypes.string_at(p.value, count * np.dtype(dt).itemsize), dt).copy() if count else np.zeros(0, dt)

    return (0, base.value, m.value, n.value, nnz.value, arr(rp, m.value + 1, np.int32), arr(ci, nnz.value, np.int32),
            arr(v, nnz.value, dtype))


class HostMatrix(P.Matrix):
    """aoclsparse_create_?csr with an explicit nnz and any of the four value types"""

    def __init__(self, base, m, n, nnz, rp, ci, v):
        self.row_ptr = np.ascontiguousarray(rp, dtype=np.int32)
        self.col_ind = np.ascontiguousarray(ci if len(ci) else np.zeros(1), dtype=np.int32)
        self.val = np.ascontiguousarray(v if len(v) else np.zeros(1, np.asarray(v).dtype))
        self.letter = LETTER[self.val.dtype]
        self.double = self.val.dtype == np.float64
        self.m, self.n, self.nnz, self.base = m, n, nnz, base
        self.h = c_void_p()
        fn = getattr(L, "aoclsparse_create_%scsr" % self.letter)
        self.status = fn(byref(self.h), base, m, n, nnz, P._ptr(self.row_ptr), P._ptr(self.col_ind), P._ptr(self.val))


def host_route(base, m, n, row, col, val):
    """create_?coo -> convert_csr -> export_?csr -> create_?csr: (status, row_ptr, col_ind, val, HostMatrix or None)"""
    nnz = len(val)
    row, col, val = (np.ascontiguousarray(a if len(a) else np.zeros(1, a.dtype)) for a in (row, col, val))
    t = LETTER[val.dtype]
    h, c = c_void_p(), c_void_p()
    st = getattr(L, "aoclsparse_create_%scoo" % t)(byref(h), base, m, n, nnz, P._ptr(row), P._ptr(col), P._ptr(val))
    if st != 0:
        return st, None, None, None, None
    try:
        assert L.aoclsparse_convert_csr(h, P.OP_NONE, byref(c)) == 0
        e = export_host(c, val.dtype)
        assert e[0] == 0 and e[1:5] == (base, m, n, nnz)
    finally:
        L.aoclsparse_destroy(byref(c))
        L.aoclsparse_destroy(byref(h))
    H = HostMatrix(base, m, n, nnz, e[5], e[6], e[7])
    return H.status, e[5], e[6], e[7], (H if H.status == 0 else None)


def fetch(addr, count, dtype):
    """count elements at a device address -> numpy, by a plain ctypes hipMemcpy"""
    out = np.zeros(max(count, 1), dtype)
    hip = ctypes.CDLL(P.hip_runtime_path()[1])
    hip.hipMemcpy.argtypes = [c_void_p, c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip.hipMemcpy(P._ptr(out), c_void_p(addr), count * out.itemsize, 2) == 0  # hipMemcpyDeviceToHost
    return out[:count]


def device_route(base, m, n, row, col, val, dup, nnz=None):
    nnz = len(val) if nnz is None else nnz
    t = dev_arr(np.asarray(row, np.int32)), dev_arr(np.asarray(col, np.int32)), dev_arr(val)
    torch.cuda.synchronize()
    D = P.Matrix.from_coo_device(base, m, n, nnz, *t, duplicates=dup)
    for a in t:  # the arrays were copied
        a.zero_()
    torch.cuda.synchronize()
    return D


def handle_arrays(D, dtype):
    """the handle's CSR twice: aoclsparse_export_?csr (the host view) and export_csr_device copied back; both must agree"""
    e = export_host(D.h, dtype)
    assert e[0] == 0
    ed = D.export_device()
    assert ed["status"] == 0
    assert (ed["base"], ed["m"], ed["n"], ed["nnz"]) == e[1:5]
    drp, dci = fetch(ed["row_ptr"], ed["m"] + 1, np.int32), fetch(ed["col_ind"], ed["nnz"], np.int32)
    dv = fetch(ed["val"], ed["nnz"], dtype)
    assert np.array_equal(drp, e[5]) and np.array_equal(dci, e[6]) and same_bits(dv, e[7])
    return e[4], e[5], e[6], e[7]


def check_keep(base, m, n, row, col, val, want_status=None):
    """device route == host route: status, class and diagonal flag, host view, resident arrays -> the device handle"""
    row, col, val = np.asarray(row, np.int32), np.asarray(col, np.int32), np.asarray(val)
    hs, rp, ci, v, H = host_route(base, m, n, row, col, val)
    D = device_route(base, m, n, row, col, val, KEEP)
    assert D.status == hs, ("device %s, host %s" % (P.STATUS.get(D.status), P.STATUS.get(hs)))
    if want_status is not None:
        assert hs == want_status, P.STATUS.get(hs)
    if hs != 0:
        assert not D.h.value
        return None
    assert D.spmv_info().device_resident == 1  # before any product
    assert probe(D) == probe(H), "sort class / full diagonal differ"
    nnz, drp, dci, dv = handle_arrays(D, val.dtype)
    assert nnz == len(val) == D.nnz
    assert np.array_equal(drp, rp) and np.array_equal(dci, ci) and same_bits(dv, v)
    return D


def sum_reference(base, m, row, col, val):
    """stable (row, column) order, every run of equal coordinates added left to right in val's dtype -> row_ptr, col_ind, val"""
    order = np.lexsort((col, row))  # stable: equal coordinates keep their triplet order
    r, c, v = row[order], col[order], val[order]
    orow, ocol, oval = [], [], []
    i = 0
    while i < len(v):
        acc = v[i]
        j = i + 1
        while j < len(v) and r[j] == r[i] and c[j] == c[i]:
            acc = acc + v[j]  # numpy scalars of val's dtype: one rounding per addition (per component for complex values)
            j += 1
        assert acc.dtype == val.dtype
        orow.append(r[i]), ocol.append(c[i]), oval.append(acc)
        i = j
    cnt = np.bincount(np.asarray(orow, np.int64) - base, minlength=m)[:m] if orow else np.zeros(m, np.int64)
    rp = (np.concatenate([[0], np.cumsum(cnt)]) + base).astype(np.int32)
    return rp, np.asarray(ocol, np.int32), np.asarray(oval, val.dtype)


def check_sum(base, m, n, row, col, val):
    row, col, val = np.asarray(row, np.int32), np.asarray(col, np.int32), np.asarray(val)
    rp, ci, v = sum_reference(base, m, row, col, val)
    D = device_route(base, m, n, row, col, val, SUM)
    assert D.status == 0, P.STATUS.get(D.status)
    assert D.spmv_info().device_resident == 1
    nnz, drp, dci, dv = handle_arrays(D, val.dtype)
    distinct = len(set(zip(row.tolist(), col.tolist())))
    assert nnz == distinct == len(v) == D.nnz
    assert np.array_equal(drp, rp) and np.array_equal(dci, ci)
    assert same_bits(dv, v), "a run was not added left to right in triplet order"
    # fully sorted rows: class 1, and what create_?csr decides on the same arrays
    H = HostMatrix(base, m, n, nnz, rp, ci, v)
    assert H.status == 0 and probe(D) == probe(H)
    if val.dtype == np.float64:
        assert probe(D)[1] == INVALID_VALUE  # ?syrkd's answer for class 1
    return D


def shuffled(seed, m, n, rowlen, base=0, dtype=np.float64):
    """random_csr's triplets under a seeded permutation"""
    rp, ci, v = random_csr(seed, m, n, rowlen, base=base)
    row = (np.repeat(np.arange(m), np.diff(rp)) + base).astype(np.int32)
    p = np.random.default_rng(seed + 1000).permutation(len(v))
    v = v.astype(dtype) if np.dtype(dtype).kind != "c" else (v + 1j * np.random.default_rng(seed + 2000).uniform(-1, 1, len(v))).astype(dtype)
    return row[p], ci[p], v[p]


def random_triplets(seed, m, n, nnz, base=0, dtype=np.float64, diag_free=True):
    """nnz triplets with repeats; no diagonal entries, so that `keep` mode cannot meet a second one"""
    rng = np.random.default_rng(seed)
    row, col = rng.integers(0, m, nnz), rng.integers(0, n, nnz)
    if diag_free and n > 1:
        col = np.where(col == row, (col + 1) % n, col)
    return (row + base).astype(np.int32), (col + base).astype(np.int32), rng.uniform(-1, 1, nnz).astype(dtype)


def run_dmv(A, x, y0, alpha=1.3, beta=-0.4):
    yd = dev(y0)
    assert P.dmv(P.OP_NONE, alpha, A, P.Descr(base=A.base), dev(x), beta, yd) == 0
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def dmv_bound(base, rp, ci, v, x, y0, alpha=1.3, beta=-0.4):
    """componentwise forward bound of alpha * A x + beta * y0 summed in any order: (k + 3) eps (|alpha| sum |a x| + |beta y0|),
    k the longest row"""
    k = int(np.max(np.diff(rp))) if len(rp) > 1 else 0
    return (k + 3) * EPS64 * (abs(alpha) * abs_row_sums(rp, ci, v, x, base) + abs(beta) * np.abs(y0)) + 1e-300


# --------------------------------------------------------------------------------------------------
# keep mode
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nnz", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17])
def test_keep_entry_counts_around_the_wavefront_and_the_tile(nnz):
    m, n = 300, 280
    row, col, val = random_triplets(nnz, m, n, nnz)
    check_keep(0, m, n, row, col, val, want_status=0)
    check_sum(1, m, n, row + 1, col + 1, val)


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("m", [1, 255, 256, 257, 65535, 65537])
def test_keep_row_counts_around_the_digit_boundaries(m, base):
    """one, two and three row passes; M = 1 sorts nothing"""
    n = 50
    row, col, val = random_triplets(m, m, n, 2 * T + 100, base=base)
    # the first and the last row are there, and so is the first row of the highest digit
    row[:3] = np.array([0, m - 1, (m - 1) & ~0xFF]) + base
    col[:3] = np.array([n - 1, n - 2, n - 3]) + base
    check_keep(base, m, n, row, col, val, want_status=0)


def test_keep_fourth_row_pass():
    m, n, nnz = 2 ** 24 + 3, 40, 1000
    rng = np.random.default_rng(24)
    row = rng.choice(np.array([0, 2 ** 24 - 1, 2 ** 24, m - 1]), nnz).astype(np.int32)
    col, val = rng.integers(0, n, nnz).astype(np.int32), rng.uniform(-1, 1, nnz)
    col = np.where(col == row, col + 1, col).astype(np.int32)
    check_keep(0, m, n, row, col, val, want_status=0)
    D = check_sum(0, m, n, row, col, val)
    assert D.nnz <= 4 * n


@pytest.mark.parametrize("base", [0, 1])
def test_one_row_and_one_column_holding_5000_of_6000_entries(base):
    """what the device transpose declines: a segment far beyond 2,048 entries"""
    big, rng = 7000, np.random.default_rng(50)
    long_ = rng.choice(big, 5000, replace=False)
    other_r, other_c = rng.integers(0, 300, 1000), rng.integers(0, big, 1000)
    other_r = np.where(other_r == 3, 4, other_r)
    other_c = np.where(other_c == other_r, other_c + 1, other_c)  # (no diagonal entry among them: `keep` refuses a second one)
    val = rng.uniform(-1, 1, 6000)
    p = rng.permutation(6000)
    # a 300 x 7000 matrix whose row 3 holds 5,000 distinct columns ...
    row = (np.concatenate([np.full(5000, 3), other_r])[p] + base).astype(np.int32)
    col = (np.concatenate([long_, other_c])[p] + base).astype(np.int32)
    check_keep(base, 300, big, row, col, val, want_status=0)
    check_sum(base, 300, big, row, col, val)
    # ... and its transpose: column 3 holds 5,000 distinct rows
    check_keep(base, big, 300, col, row, val, want_status=0)
    check_sum(base, big, 300, col, row, val)


def test_keep_a_wavefront_of_equal_digits_and_one_of_different_digits():
    m, n = 500, 90
    row, col, val = random_triplets(7, m, n, T + 200)
    row[128:192] = 77  # 64 consecutive triplets of one row, aligned with a wavefront's round ...
    col[128:192] = np.arange(64)
    row[200:264] = 78  # ... and not aligned
    col[200:264] = np.arange(64)
    row[320:384] = np.arange(100, 164)  # 64 consecutive triplets of 64 different rows
    col[320:384] = 5
    check_keep(0, m, n, row, col, val, want_status=0)
    check_sum(0, m, n, row, col, val)


def test_keep_descending_rows_and_every_second_row_empty():
    m, n = 3000, 3100
    rng = np.random.default_rng(9)
    row = np.repeat(np.arange(m - 1, -1, -1), 3).astype(np.int32)  # rows in descending order, three entries each
    col = rng.integers(0, n - 1, len(row)).astype(np.int32)
    col = np.where(col == row, n - 1, col).astype(np.int32)
    val = rng.uniform(-1, 1, len(row))
    check_keep(0, m, n, row, col, val, want_status=0)
    keep = row % 2 == 0  # every second row empty
    D = check_keep(1, m, n, row[keep] + 1, col[keep] + 1, val[keep], want_status=0)
    rp = handle_arrays(D, np.float64)[1]
    assert np.all(np.diff(rp)[1::2] == 0) and np.all(np.diff(rp)[0::2] == 3)


@pytest.mark.parametrize("m,n", [(700, 90), (90, 700)])
def test_tall_and_wide(m, n):
    row, col, val = random_triplets(m, m, n, T + 31, base=1)
    check_keep(1, m, n, row, col, val, want_status=0)
    check_sum(1, m, n, row, col, val)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
def test_all_four_value_types(dtype):
    m, n = 2500, 2300
    row, col, val = shuffled(61, m, n, lambda r, i: r.integers(0, 9), dtype=dtype)
    assert len(val) > 2 * T
    D = check_keep(0, m, n, row, col, val, want_status=0)
    assert D.letter == LETTER[np.dtype(dtype)]
    # distinct coordinates: `sum` mode changes no value, only the order inside a row
    check_sum(0, m, n, row, col, val)
    # ... and with repeats
    row, col, val = random_triplets(62, 60, 50, T + 9, dtype=np.float64)
    val = val.astype(dtype) if np.dtype(dtype).kind != "c" else (val + 1j * val[::-1]).astype(dtype)
    check_sum(0, 60, 50, row, col, val)


def test_keep_dmv_against_the_oracle():
    m, n = 4000, 3900
    row, col, val = shuffled(71, m, n, lambda r, i: r.integers(0, 14))
    D = check_keep(0, m, n, row, col, val, want_status=0)
    _, rp, ci, v, H = host_route(0, m, n, row, col, val)
    rng = np.random.default_rng(5)
    x, y0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, m)
    so, yr = oracle.dcsrmv(-1, 0, 1.3, m, len(v), v, ci, rp, x, -0.4, y0)
    assert so == 0
    yd, yh = run_dmv(D, x, y0), run_dmv(H, x, y0)
    assert np.array_equal(yd, yh)  # the same arrays in the same library
    assert np.all(np.abs(yd - yr) <= dmv_bound(0, rp, ci, v, x, y0)), "differs from the oracle"
    assert np.linalg.norm(yr) > 1.0


def test_keep_off_diagonal_duplicates_stay_in_triplet_order():
    m, n = 40, 40
    row = np.array([5, 2, 5, 5, 2, 5, 0], np.int32)
    col = np.array([7, 3, 7, 1, 3, 7, 9], np.int32)
    val = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0])
    D = check_keep(0, m, n, row, col, val, want_status=0)
    _, rp, ci, v = handle_arrays(D, np.float64)
    assert ci.tolist() == [9, 3, 3, 7, 7, 1, 7] and v.tolist() == [7.0, 2.0, 5.0, 1.0, 3.0, 4.0, 6.0]
    S = check_sum(0, m, n, row, col, val)
    _, rp, ci, v = handle_arrays(S, np.float64)
    assert ci.tolist() == [9, 3, 1, 7] and v.tolist() == [7.0, 7.0, 4.0, 10.0]


def test_a_duplicated_diagonal_entry_is_refused_by_both_routes_in_keep_mode():
    row, col, val = random_triplets(3, 200, 200, 900)
    row[[10, 500]] = 17
    col[[10, 500]] = 17
    assert check_keep(0, 200, 200, row, col, val, want_status=INVALID_VALUE) is None
    check_sum(0, 200, 200, row, col, val)  # `sum` mode adds them


@pytest.mark.parametrize("dup", [KEEP, SUM])
def test_indices_out_of_range(dup):
    m, n = 120, 90
    row, col, val = random_triplets(4, m, n, T + 50)
    for base, where, r, c in ((0, 0, m, 0), (0, T + 49, 0, n), (0, 70, -1, 3), (1, 64, 0, 5), (1, 4000, 5, 0), (1, 9, m + 1, 5),
                              (1, T, 5, n + 1)):
        rr, cc = row + base, col + base
        rr[where], cc[where] = r, c
        D = device_route(base, m, n, rr, cc, val, dup)
        assert D.status == INVALID_INDEX and not D.h.value, (base, where)
        if dup == KEEP:
            assert host_route(base, m, n, rr, cc, val)[0] == INVALID_INDEX
    # M == 0 with entries: every row is out of range
    D = device_route(0, 0, n, row[:5], col[:5], val[:5], dup)
    assert D.status == INVALID_INDEX and not D.h.value


@pytest.mark.parametrize("dup", [KEEP, SUM])
def test_no_entries_and_no_rows(dup):
    one = np.zeros(1, np.int32)
    for base in (0, 1):
        for m, n in ((5, 5), (5, 0), (0, 5)):
            D = device_route(base, m, n, one, one, np.zeros(1), dup, nnz=0)
            assert D.status == 0 and D.spmv_info().device_resident == 1
            nnz, rp, ci, v = handle_arrays(D, np.float64)
            assert nnz == 0 and np.array_equal(rp, np.full(m + 1, base, np.int32))
            H = HostMatrix(base, m, n, 0, rp, np.zeros(0, np.int32), np.zeros(0))
            assert H.status == 0 and probe(D) == probe(H)


def test_a_host_array_is_refused_in_automatic_pointer_mode():
    row, col, val = random_triplets(5, 50, 50, 300)
    t = [dev_arr(row), dev_arr(col), dev_arr(val)]
    torch.cuda.synchronize()
    for k, host in enumerate((row, col, val)):
        args = list(t)
        args[k] = host
        for dup in (KEEP, SUM):
            A = P.Matrix.from_coo_device(0, 50, 50, len(val), *args, duplicates=dup, dtype="float64")
            assert A.status == INVALID_POINTER and not A.h.value


@pytest.mark.parametrize("dup", [KEEP, SUM])
def test_the_same_call_twice_gives_identical_arrays(dup):
    m, n = 900, 800
    row, col, val = random_triplets(6, m, n, 3 * T + 17)
    out = []
    for _ in range(2):
        D = device_route(0, m, n, row, col, val, dup)
        assert D.status == 0
        out.append(handle_arrays(D, np.float64))
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        assert same_bits(a, b)


# --------------------------------------------------------------------------------------------------
# sum mode
# --------------------------------------------------------------------------------------------------
def _chain(dtype):
    """a run whose left-to-right sum differs from the sum in any sorted order"""
    big = 1e16 if np.dtype(dtype) in (np.dtype(np.float64), np.dtype(np.complex128)) else 1e8
    run = np.array([big, 1.0, -big, 1.0])
    if np.dtype(dtype).kind == "c":
        run = run + 1j * run
    return run.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
def test_sum_the_chain_order_matters(dtype):
    run = _chain(dtype)
    # the restated chain differs from sorted summation on this input: the case cannot silently go soft
    chain = run[0]
    for x in run[1:]:
        chain = chain + x
    srt = np.sort(run)
    sorted_sum = srt[0]
    for x in srt[1:]:
        sorted_sum = sorted_sum + x
    assert chain != sorted_sum and chain != np.sum(srt) and chain == np.asarray(1.0 + (1.0j if run.dtype.kind == "c" else 0)).astype(dtype)
    m, n = 70, 60
    row, col, val = random_triplets(8, m, n, T + 300, dtype=np.float64)
    val = val.astype(dtype) if run.dtype.kind != "c" else (val + 1j * val[::-1]).astype(dtype)
    # the run's members far apart in the triplets (two tiles), and a second run back to back across a wavefront's round
    for k, p in enumerate((5, 700, T - 1, T + 250)):
        row[p], col[p], val[p] = 33, 44, run[k]
    for k, p in enumerate((62, 63, 64, 65)):
        row[p], col[p], val[p] = 34, 2, run[k]
    clash = ((row == 33) & (col == 44)) | ((row == 34) & (col == 2))
    clash[[5, 700, T - 1, T + 250, 62, 63, 64, 65]] = False
    col[clash] += 1  # nothing else lands on the two coordinates
    D = check_sum(0, m, n, row, col, val)
    _, rp, ci, v = handle_arrays(D, dtype)
    for r, c in ((33, 44), (34, 2)):
        seg = slice(rp[r], rp[r + 1])
        assert v[seg][ci[seg] == c][0] == chain


def test_sum_run_lengths_and_runs_across_tile_boundaries():
    """runs of 1, 2, 63, 64, 65 and 300 equal coordinates; with 1,600 coordinates for 3T + 17 entries the sorted runs lie across
    every tile boundary, and their members are spread over all tiles of the input"""
    m, n = 40, 40
    rng = np.random.default_rng(11)
    row, col = rng.integers(0, m - 8, 3 * T + 17), rng.integers(0, n, 3 * T + 17)
    extra_r, extra_c = [], []
    for k, length in enumerate((1, 2, 63, 64, 65, 300)):  # rows 32 .. 37 hold exactly one run each
        extra_r += [m - 8 + k] * length
        extra_c += [3 * k] * length
    row, col = np.concatenate([row, extra_r]), np.concatenate([col, extra_c])
    p = rng.permutation(len(row))
    row, col = row[p].astype(np.int32), col[p].astype(np.int32)
    val = rng.uniform(-1, 1, len(row)) * 10.0 ** rng.integers(-8, 8, len(row))  # magnitudes that make the order visible
    D = check_sum(0, m, n, row, col, val)
    _, rp, ci, v = handle_arrays(D, np.float64)
    assert np.diff(rp)[m - 8:m - 2].tolist() == [1] * 6
    # sorted order: the runs straddle the tile boundaries of the sorted sequence
    order = np.lexsort((col, row))
    assert any((row[order][b - 1], col[order][b - 1]) == (row[order][b], col[order][b]) for b in (T, 2 * T, 3 * T))
    check_sum(0, m, n, row, col, val.astype(np.float32))


def test_sum_a_run_that_adds_up_to_zero_stays_an_entry():
    row = np.array([3, 1, 3, 2, 3], np.int32)
    col = np.array([4, 1, 4, 0, 9], np.int32)
    val = np.array([1.5, 2.0, -1.5, 3.0, 4.0])
    D = check_sum(0, 6, 12, row, col, val)
    nnz, rp, ci, v = handle_arrays(D, np.float64)
    assert nnz == 4 and ci.tolist() == [1, 0, 4, 9] and v.tolist() == [2.0, 3.0, 0.0, 4.0]


def test_sum_update_values_device_then_dmv():
    m, n = 1500, 1400
    row, col, val = random_triplets(12, m, n, 2 * T + 5, diag_free=False)
    row[1::10], col[1::10] = row[0::10][:len(row[1::10])], col[0::10][:len(col[1::10])]  # every tenth one repeated
    D = check_sum(0, m, n, row, col, val)
    nnz, rp, ci, v = handle_arrays(D, np.float64)
    assert nnz < len(val)
    rng = np.random.default_rng(13)
    x, y0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, m)
    so, yr = oracle.dcsrmv(-1, 0, 1.3, m, nnz, v, ci, rp, x, -0.4, y0)
    assert so == 0 and np.all(np.abs(run_dmv(D, x, y0) - yr) <= dmv_bound(0, rp, ci, v, x, y0))
    v2 = rng.uniform(-1, 1, nnz)
    t2 = dev(v2)
    torch.cuda.synchronize()
    assert D.update_values_device(t2) == 0
    assert D.spmv_info().device_resident == 1
    so, yr2 = oracle.dcsrmv(-1, 0, 1.3, m, nnz, v2, ci, rp, x, -0.4, y0)
    y2 = run_dmv(D, x, y0)
    assert so == 0 and np.all(np.abs(y2 - yr2) <= dmv_bound(0, rp, ci, v2, x, y0))
    assert not np.array_equal(y2, yr)
    assert D.update_values_device(dev(np.ones(len(val)))) == 3  # the triplets' count is not the handle's nnz


# --------------------------------------------------------------------------------------------------
# Python layer
# --------------------------------------------------------------------------------------------------
def test_from_torch_coo():
    m, n = 300, 260
    row, col, val = random_triplets(14, m, n, T + 77, diag_free=False)
    idx = torch.from_numpy(np.stack([row, col]).astype(np.int64))
    t = torch.sparse_coo_tensor(idx, torch.from_numpy(val), size=(m, n)).cuda()
    assert not t.is_coalesced()
    A = P.Matrix.from_torch_coo(t)
    B = device_route(0, m, n, row, col, val, SUM)
    assert A.status == 0 and B.status == 0 and (A.m, A.n) == (m, n) and A.double
    assert A.nnz == B.nnz < len(val) and A.spmv_info().device_resident == 1
    for a, b in zip(handle_arrays(A, np.float64), handle_arrays(B, np.float64)):
        assert same_bits(np.asarray(a), np.asarray(b))
    # one-based, float32
    tf = torch.sparse_coo_tensor(idx, torch.from_numpy(val.astype(np.float32)), size=(m, n)).cuda()
    A1 = P.Matrix.from_torch_coo(tf, base=1, duplicates=SUM)
    B1 = device_route(1, m, n, row + 1, col + 1, val.astype(np.float32), SUM)
    assert A1.status == 0 and A1.base == 1 and A1.letter == "s"
    for a, b in zip(handle_arrays(A1, np.float32), handle_arrays(B1, np.float32)):
        assert same_bits(np.asarray(a), np.asarray(b))
    # an empty tensor
    te = torch.sparse_coo_tensor(torch.zeros((2, 0), dtype=torch.int64), torch.zeros(0, dtype=torch.float64), size=(m, n)).cuda()
    E = P.Matrix.from_torch_coo(te)
    assert E.status == 0 and E.nnz == 0
