"""What tests/test_clean_device_cpu.py and tests/test_clean_device_gpu.py share: the handles aoclsparse_mi355_clean_csr_device answers
before it touches the device, a numpy restatement of the clean CSR csr_optimize builds (clean_reference), the edge matrices, and the
twin -- a host-created handle over copies of the arrays, put through aoclsparse_optimize, exported and checked against the restatement.

The three cases (include/aoclsparse_mi355.h: clean_csr_device).  `sorted`: in every row nothing left of the diagonal follows the
diagonal or something right of it, and the diagonal follows nothing right of it (L | D | U group order).  `fulldiag`: every row
i < min(m, n) holds column i.
  1. sorted and fulldiag: the arrays as they are, idiag / iurow in their base, is_internal = 0.
  2. sorted, a diagonal missing: 0-based, the rows' entries in their given order, an explicit zero in front of the first entry with
     column >= i (at the row's end when there is none) in every row i < min(m, n) without one.
  3. not sorted: every row into ascending column order first, stably; then as 2."""
import ctypes
from ctypes import byref, c_int, c_int32, c_void_p

import numpy as np

from order_cases import Raw
from util import pkg

P = pkg()
L = P.lib()

SUCCESS, NOT_IMPLEMENTED, INVALID_POINTER, INVALID_OPERATION = 0, 1, 2, 12
assert P.STATUS[INVALID_OPERATION] == "invalid_operation"
LETTER = {np.dtype(np.float32): "s", np.dtype(np.float64): "d", np.dtype(np.complex64): "c", np.dtype(np.complex128): "z"}
DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
RW = P.CLEAN_ROW_WAVE  # rows of up to this many entries are searched by one lane, longer ones by their wavefront


def early_cases():
    """[(name, handle object or None, status)]: csr_optimize's answers that need no device"""
    i32 = lambda *a: np.array(a, np.int32)  # noqa: E731
    v = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    cases = [("null", None, INVALID_POINTER)]
    cases.append(("tcsr", P.TcsrMatrix(0, 3, i32(0, 1, 2, 4), i32(0, 1, 0, 2), np.array([1.0, 2.0, 5.0, 4.0]),
                                       i32(0, 2, 3, 4), i32(0, 1, 1, 2), np.array([1.0, 3.0, 2.0, 4.0])), NOT_IMPLEMENTED))
    cases.append(("bsr", P.BsrMatrix(0, P.ORDER_ROW, 2, 2, 2, i32(0, 2, 3), i32(1, 0, 1), np.arange(12.0)), NOT_IMPLEMENTED))
    cases.append(("coo", Raw("aoclsparse_create_dcoo", 0, 3, 3, 5, i32(0, 0, 1, 2, 2), i32(1, 0, 1, 2, 0), v.copy()), INVALID_POINTER))
    for name, A, _ in cases:
        assert A is None or A.status == 0, (name, P.STATUS.get(A.status, A.status))
    return cases


class HostMatrix(P.Matrix):
    """aoclsparse_create_?csr over copies of the arrays, any of the four value types"""

    def __init__(self, base, m, n, rp, ci, v):
        self.row_ptr = np.array(rp, dtype=np.int32)
        self.col_ind = np.array(ci, dtype=np.int32) if len(ci) else np.zeros(1, np.int32)  # (the call wants non-null arrays)
        self.val = np.array(v) if len(v) else np.zeros(1, np.asarray(v).dtype)
        self.letter = LETTER[self.val.dtype]
        self.double = self.val.dtype == np.float64
        self.m, self.n, self.nnz, self.base = m, n, len(v), base
        self.h = c_void_p()
        fn = getattr(L, "aoclsparse_create_%scsr" % self.letter)
        self.status = fn(byref(self.h), base, m, n, self.nnz, P._ptr(self.row_ptr), P._ptr(self.col_ind), P._ptr(self.val))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


# --------------------------------------------------------------------------------------------------
# the restatement
# --------------------------------------------------------------------------------------------------
def _first_at_or_right(m, ptr, col):
    """(first, isdiag) per row of 0-based arrays: the first position whose column is >= the row (the row end when there is none),
    and whether that entry is the diagonal -- csr_indices' idiag, and iurow - idiag"""
    rows = np.repeat(np.arange(m), np.diff(ptr))
    first = ptr[1:].astype(np.int64).copy()
    ge = col >= rows
    np.minimum.at(first, rows[ge], np.flatnonzero(ge))
    isdiag = np.zeros(m, bool)
    inside = first < ptr[1:]
    isdiag[inside] = col[first[inside]] == np.flatnonzero(inside)
    return first, isdiag


def clean_reference(base, m, n, rp, ci, v):
    """-> (ptr, ind, val, idiag, iurow, internal): what csr_optimize leaves for aoclsparse_export_?csr and export_diag"""
    ptr, col, val = np.asarray(rp, np.int64) - base, np.asarray(ci, np.int64) - base, np.asarray(v)
    rows = np.repeat(np.arange(m), np.diff(ptr))
    side = np.sign(col - rows)  # L | D | U group order: the side of the diagonal never steps back inside a row
    ordered = not np.any((np.diff(side) < 0) & (rows[1:] == rows[:-1]))
    has = np.zeros(m, bool)
    has[rows[col == rows]] = True
    fulldiag = bool(np.all(has[: min(m, n)]))
    if ordered and fulldiag:  # case 1
        first, isdiag = _first_at_or_right(m, ptr, col)
        return (np.asarray(rp, np.int32), np.asarray(ci, np.int32), val, (first + base).astype(np.int32),
                (first + isdiag + base).astype(np.int32), False)
    if not ordered:  # case 3
        perm = np.lexsort((np.arange(len(col)), col, rows))
        col, val = col[perm], val[perm]
    first, isdiag = _first_at_or_right(m, ptr, col)
    miss = np.flatnonzero(~isdiag[: min(m, n)])
    col, val = np.insert(col, first[miss], miss), np.insert(val, first[miss], 0)
    add = np.zeros(m + 1, np.int64)
    add[miss + 1] = 1
    ptr = ptr + np.cumsum(add)
    first, isdiag = _first_at_or_right(m, ptr, col)
    return ptr.astype(np.int32), col.astype(np.int32), val, first.astype(np.int32), (first + isdiag).astype(np.int32), True


# --------------------------------------------------------------------------------------------------
# what a handle shows of its clean CSR, and the twin
# --------------------------------------------------------------------------------------------------
def export_clean(A, dtype):
    """aoclsparse_export_?csr + aoclsparse_mi355_export_diag -> (base, ptr, ind, val, idiag, iurow, internal), copies"""
    base, m, n, nnz = c_int(), c_int32(), c_int32(), c_int32()
    rp, ci, v = c_void_p(), c_void_p(), c_void_p()
    fn = getattr(L, "aoclsparse_export_%scsr" % LETTER[np.dtype(dtype)])
    st = fn(A.h, byref(base), byref(m), byref(n), byref(nnz), byref(rp), byref(ci), byref(v))
    assert st == 0, P.STATUS.get(st, st)

    def arr(p, count, dt):
        return np.frombuffer(ctypes.string_at(p.value, count * np.dtype(dt).itemsize), dt).copy() if count else np.zeros(0, dt)

    d = A.export_diag()
    assert d["status"] == 0, P.STATUS.get(d["status"], d["status"])
    return (base.value, arr(rp, m.value + 1, np.int32), arr(ci, nnz.value, np.int32), arr(v, nnz.value, dtype), d["idiag"], d["iurow"],
            d["is_internal"])


def assert_same_clean(got, want, what=""):
    """two export_clean results: integers equal, values bitwise equal, is_internal equal"""
    names = ("base", "row_ptr", "col_ind", "val", "idiag", "iurow", "is_internal")
    assert got[0] == want[0] and got[6] == want[6], (what, got[0], want[0], got[6], want[6])
    for k in (1, 2, 4, 5):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, names[k])
    assert same_bits(got[3], want[3]), (what, "val")


def twin(base, m, n, rp, ci, v):
    """the yardstick: (handle, its export_clean) of a host handle over copies, after aoclsparse_optimize, which is csr_optimize
    here; checked against clean_reference first.  aoclsparse_optimize returns at once without a pending hint (as the reference's
    does), so the handle gets the one hint that asks for the clean CSR and for nothing else, on the device or off it: a forward
    SOR sweep."""
    v = np.asarray(v)
    H = HostMatrix(base, m, n, rp, ci, v)
    assert H.status == 0, P.STATUS.get(H.status, H.status)
    assert H.export_diag()["status"] == INVALID_OPERATION  # no clean CSR yet
    d = P.Descr(base=base)
    assert L.aoclsparse_set_sorv_hint(H.h, d.h, 0, 1) == 0  # aoclsparse_sor_forward
    st = L.aoclsparse_optimize(H.h)
    assert st == 0, P.STATUS.get(st, st)
    got = export_clean(H, v.dtype)
    ptr, ind, val, idiag, iurow, internal = clean_reference(base, m, n, rp, ci, v)
    assert_same_clean(got, (0 if internal else base, ptr, ind, val.astype(v.dtype), idiag, iurow, internal), "host route vs numpy")
    return H, got


# --------------------------------------------------------------------------------------------------
# the edge matrices: 0-based structures, built once
# --------------------------------------------------------------------------------------------------
KINDS = ("present", "front", "middle", "end")  # the diagonal: there | missing, and the zero goes in front | in the middle | at the end
EDGE_LENGTHS = sorted({0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, RW - 1, RW, RW + 1})
EDGE_LONG = 5000  # one row: the radix path of the sort, the wavefront path of the mark kernel
EDGE_SHAPES = {"tall": (6100, 6000), "wide": (6000, 6100)}  # m > n: the last rows can never get a diagonal
_cache = {}


def _edge_row(rng, i, k, kind, n):
    """k distinct columns of row i < n of the given kind, shuffled (a kind the row has no room for becomes 'anything but i')"""
    if i >= n:
        return rng.permutation(rng.choice(n, size=min(k, n), replace=False))
    lo, hi = np.arange(0, i), np.arange(i + 1, n)
    if kind == "present" and k >= 1:
        c = np.concatenate([[i], rng.choice(np.concatenate([lo, hi]), size=k - 1, replace=False)])
    elif kind == "front" and len(hi) >= k:
        c = rng.choice(hi, size=k, replace=False)
    elif kind == "end" and len(lo) >= k:
        c = rng.choice(lo, size=k, replace=False)
    elif kind == "middle" and k >= 2 and len(lo) and len(hi):
        a, b = rng.choice(lo), rng.choice(hi)
        rest = np.concatenate([lo[lo != a], hi[hi != b]])
        c = np.concatenate([[a, b], rng.choice(rest, size=k - 2, replace=False)])
    else:
        c = rng.choice(np.concatenate([lo, hi]), size=k, replace=False)
    return rng.permutation(c)


def edge_structure(shape):
    """(m, n, row_ptr, col_ind): every length of EDGE_LENGTHS in every kind of KINDS, one row of EDGE_LONG entries with the zero
    going in the middle, short rows of all kinds around them; a column held twice, off the diagonal, in every 50th short row"""
    if shape in _cache:
        return _cache[shape]
    m, n = EDGE_SHAPES[shape]
    rng = np.random.default_rng(2424)
    special = {2060 + 30 * j: lk for j, lk in enumerate((k, kind) for k in EDGE_LENGTHS for kind in KINDS)}
    assert max(special) + max(EDGE_LENGTHS) < min(m, n) and min(special) >= max(EDGE_LENGTHS)  # room on either side of the diagonal
    special[3007] = (EDGE_LONG, "middle")
    rows, twice = [], 0
    for i in range(m):
        k, kind = special.get(i, (int(rng.integers(0, 9)), KINDS[i % 4]))
        c = _edge_row(rng, i, k, kind, n)
        if i not in special and i % 50 == 1 and len(c) >= 3:
            off = np.flatnonzero(c != i)
            c[off[0]] = c[off[1]]
            twice += 1
        rows.append(c)
    for i, (k, kind) in special.items():  # the rows are what their kind says
        c = rows[i]
        assert len(c) == k and ((i in c) == (kind == "present" and k > 0))
        if kind == "front":
            assert np.all(c > i)
        if kind == "end":
            assert np.all(c < i)
        if kind == "middle" and k >= 2:
            assert np.any(c < i) and np.any(c > i)
    assert twice > 50
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int32)
    _cache[shape] = m, n, rp, np.concatenate(rows).astype(np.int32)
    return _cache[shape]


def scan_edge_structure(m):
    """(m, m, row_ptr, col_ind): (i, i - 1), (i, i), fully sorted; no diagonal in row 0, rows 1,023 and 1,024, the last row and
    every 7th row.  Class 1, case 2: the scan's blocks of 1,024 rows."""
    gone = {0, 1023, 1024, m - 1} | set(range(0, m, 7))
    rows = [[c for c in (i - 1, i) if c >= 0 and not (c == i and i in gone)] for i in range(m)]
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int32)
    return m, m, rp, np.array([c for r in rows for c in r], np.int32)


def class2_structure(full):
    """(m, n, row_ptr, col_ind), 300 x 300: rows in L | D | U group order but DESCENDING inside the groups; row 200 holds 150
    entries left and 90 right of the diagonal (the wavefront's path).  full: every diagonal present; else every 5th is missing."""
    m = 300
    rows = []
    for i in range(m):
        left = [c for c in (i - 1, i - 3, i - 4) if c >= 0]
        right = [c for c in (i + 9, i + 5, i + 2) if c < m]
        if i == 200:
            left, right = list(range(199, 49, -1)), list(range(295, 205, -1))
        rows.append(left + ([i] if full or i % 5 else []) + right)
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int32)
    return m, m, rp, np.array([c for r in rows for c in r], np.int32)


def tridiagonal_structure(m=500):
    """class 1, full diagonal: case 1"""
    rows = [[c for c in (i - 1, i, i + 1) if 0 <= c < m] for i in range(m)]
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int32)
    return m, m, rp, np.array([c for r in rows for c in r], np.int32)


def one_row_structure():
    """3 x 6,000: row 1 holds 5,500 shuffled entries, column 0 among them and column 1 not; rows 0 and 2 are empty"""
    rng = np.random.default_rng(55)
    c = rng.permutation(np.concatenate([[0], rng.permutation(np.arange(2, 6000))[:5499]]))
    return 3, 6000, np.array([0, 0, 5500, 5500], np.int32), c.astype(np.int32)


def empty_structures():
    """[(name, m, n, row_ptr, col_ind)]: no rows; five empty rows, which get five zeros; no columns"""
    none = np.zeros(0, np.int32)
    return [("m = 0", 0, 4, np.zeros(1, np.int32), none), ("nnz = 0", 5, 5, np.zeros(6, np.int32), none),
            ("n = 0", 4, 0, np.zeros(5, np.int32), none)]


def small_structures():
    """[(name, m, n, row_ptr, col_ind)]: every edge matrix but the two large ones"""
    out = [("scan %d" % m,) + scan_edge_structure(m) for m in (1023, 1024, 1025, 2049)]
    out += [("class 2, diagonals missing",) + class2_structure(False), ("class 2, full diagonal",) + class2_structure(True),
            ("class 1, full diagonal",) + tridiagonal_structure(), ("one row holds everything",) + one_row_structure()]
    return out + empty_structures()


def edge_values(dtype, nnz, seed=77):
    """nnz distinct values (exact in every type: integers below 2^24 over 1024, signs mixed), so that the entries of a repeated
    column can be told apart; among them -0.0, +-inf, a NaN with a payload and subnormals, which only a move leaves as they are"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    v = (rng.permutation(nnz) + 1) / 1024.0 * np.where(rng.integers(0, 2, nnz) == 0, 1.0, -1.0)
    if dtype.kind == "c":
        v = v + 1j * rng.uniform(-1, 1, nnz)
    v = v.astype(dtype)
    real = np.float32 if dtype in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64
    r = v.view(real)
    tiny = np.finfo(real).smallest_subnormal
    nan = np.array([0x7FC12345], np.uint32).view(np.float32)[0] if real is np.float32 else \
        np.array([0x7FF8000000012345], np.uint64).view(np.float64)[0]
    special = [-0.0, np.inf, -np.inf, nan, tiny, -3 * tiny]
    for k, x in enumerate(special * 3):  # (three of each, spread over the array; a complex value gets one in either part)
        if len(r):
            r[(k * 7919 + 3) % len(r)] = x
    return v
