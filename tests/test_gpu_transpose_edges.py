"""The device transpose (aocl-sparse_amd/csrc/transpose_kernels.hip) where it changes its path: rows of more than TR_ROW_WAVE = 128
entries, which tr_count_kernel / tr_scatter_kernel walk with the whole wavefront (several per wavefront, 128 and 129 side by side,
one in the last, partial wavefront of the grid), column segments of exactly 32 / 33 (insertion sort / wavefront rank sort) and
2,048 / 2,049 entries (accepted / declined: the host loop), and the 16-byte gather of complex values.  The sort only goes to the
device from 2^20 entries, so the matrix has that many.  Reference: the oracle's stable counting sort (aoclsparse_csr2csc_template),
bit for bit; ?mv with op = T / H within the bound of the restated product."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from test_sy_sparse_cpu import Handle, export
from util import EPS32, EPS64, pkg, random_csr

pytestmark = pytest.mark.gpu
P = pkg()
L = P.lib()

M_ROWS, N_COLS = 10596, 60000
CYCLE = (0, 127, 128, 129, 256, 1, 129, 129)
SEGMENTS = (31, 32, 33, 2047, 2048)  # entries of columns 0 .. 4; "declined" adds column 5 with 2,049
TR_ROW_WAVE, TR_INSERTION_MAX, TR_WAVE_CAP = 128, 32, 2048  # transpose_kernels.hip


@functools.lru_cache(maxsize=None)
def long_row_csr(kind):
    """-> (m, n, row_ptr, col_ind, val), zero-based, read only.  Row lengths cycle through CYCLE: five of every eight rows are
    long, so a wavefront of 64 rows holds 40 of them, 128 next to 129; m % 256 = 100, so the last workgroup's second wavefront is
    partial (36 rows) and the very last row has 129 entries.  Columns: random ascending steps from a random start; every 7th long
    row is shuffled, every 11th repeats a column; columns 0 .. 5 are kept free and then given exactly SEGMENTS entries, one per
    row (the row's first entry is replaced)."""
    assert kind in ("accepted", "declined")
    rng = np.random.default_rng(23)
    m, n = M_ROWS, N_COLS
    assert m % 256 >= 64 and m % 64 != 0
    lens = np.array(CYCLE, np.int64)[np.arange(m) % len(CYCLE)]
    assert lens[-1] == 129 and (lens[m - m % 64:] > TR_ROW_WAVE).sum() > 1  # long rows in the last, partial wavefront
    ptr = np.zeros(m + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    nnz = int(ptr[m])
    assert nnz >= 1 << 20
    rows = np.repeat(np.arange(m), lens)
    run = np.cumsum(rng.integers(1, 200, nnz))
    ind = rng.integers(6, n - 256 * 200, m)[rows] + (run - run[ptr[rows]])  # distinct, ascending inside a row, >= 6
    assert ind.min() >= 6 and ind.max() < n
    for j, i in enumerate(np.flatnonzero(lens > TR_ROW_WAVE)):
        s, e = ptr[i], ptr[i + 1]
        if j % 7 == 3:
            ind[s:e] = rng.permutation(ind[s:e])
        if j % 11 == 5:
            p = s + 1 + int(rng.integers(0, e - s - 2))
            if ind[p] == i:  # (a handle refuses a diagonal stored twice)
                p = p + 1 if p + 2 < e else p - 1
            ind[p + 1] = ind[p]
    want = SEGMENTS + ((TR_WAVE_CAP + 1,) if kind == "declined" else ())
    hosts = rng.permutation(np.flatnonzero(lens > 0))
    assert sum(want) <= len(hosts)
    at = 0
    for c, k in enumerate(want):
        ind[ptr[hosts[at:at + k]]] = c
        at += k
    seg = np.bincount(ind, minlength=n)
    assert tuple(seg[:len(want)]) == want and (kind == "declined" or (seg[5] == 0 and seg.max() <= TR_WAVE_CAP))
    assert (seg > TR_INSERTION_MAX).sum() > 1000 and (seg <= TR_INSERTION_MAX).sum() > 1000  # both sorts have plenty to do
    out = ptr.astype(np.int32), ind.astype(np.int32), rng.uniform(-1, 1, nnz)
    for a in out:
        a.setflags(write=False)
    return (m, n) + out


@functools.lru_cache(maxsize=None)
def csc_ref(kind, base_in, base_out):
    m, n, rp, ci, v = long_row_csr(kind)
    st, cp, ri, cv = oracle.dcsr2csc(m, n, len(v), base_in, base_out, rp + base_in, ci + base_in, v)
    assert st == 0
    return cp, ri, cv


def csr2csc(fn, kind, base_in, base_out, dt):
    m, n, rp, ci, v = long_row_csr(kind)
    nnz = len(v)
    rpb, cib, vt = rp + base_in, ci + base_in, v.astype(dt)
    d = P.Descr(base=base_in)
    op, oi, ov = np.zeros(n + 1, np.int32), np.zeros(nnz, np.int32), np.zeros(nnz, dt)
    assert fn(m, n, nnz, d.h, base_out, P._ptr(rpb), P._ptr(cib), P._ptr(vt), P._ptr(oi), P._ptr(op), P._ptr(ov)) == 0
    return op, oi, ov


@pytest.mark.parametrize("bases", [(0, 1), (1, 0)], ids=["0to1", "1to0"])
@pytest.mark.parametrize("kind", ["accepted", "declined"])
def test_csr2csc_long_rows_and_segment_edges(kind, bases):
    """aoclsparse_dcsr2csc / scsr2csc: col_ptr, row_ind and val bit for bit the oracle's.  accepted: the long-row loops of
    tr_count_kernel (transpose_kernels.hip:54-68) and tr_scatter_kernel (:87-100), segments of 31 / 32 in tr_sort_short_kernel
    (:111), of 33 / 2,047 / 2,048 in tr_sort_wave_kernel (:135).  declined: a column of 2,049 (hist[3] > 0, :203) -- the count
    kernel's long-row loop still runs, the host loop gives the same bits."""
    cp, ri, cv = csc_ref(kind, *bases)
    op, oi, ov = csr2csc(L.aoclsparse_dcsr2csc, kind, bases[0], bases[1], np.float64)
    assert np.array_equal(op, cp) and np.array_equal(oi, ri) and np.array_equal(ov, cv)
    op, oi, ov = csr2csc(L.aoclsparse_scsr2csc, kind, bases[0], bases[1], np.float32)
    assert np.array_equal(op, cp) and np.array_equal(oi, ri) and np.array_equal(ov, cv.astype(np.float32))


def release():
    freed = ctypes.c_size_t(0)
    assert L.aoclsparse_mi355_release_staging(ctypes.byref(freed)) == 0
    return freed.value


def test_the_device_sort_is_told_from_the_host_loop_by_its_staging():
    """The library has no flag that says where a conversion ran; the staging slots do.  device_transpose_run takes slot 40 (n
    ints: the column counts) and slot 41 (256 bytes) before it decides (:187-188), and only an accepted matrix goes on to slot 42
    (n ints: cursors, :209), slot 43 (nnz ints: the positions, :210), the scan scratch and slot 45 (n ints: the column order, :228).
    The operands travel in buffers of their own (formats_api.cpp:64-69), so after a release the bytes a conversion leaves behind
    are exactly these: accepted - declined >= 4 nnz + 4 n, and a declined one holds less than one nnz-sized slot."""
    m, n, _, _, v = long_row_csr("accepted")
    nnz = len(v)
    release()
    csr2csc(L.aoclsparse_dcsr2csc, "accepted", 0, 1, np.float64)
    accepted = release()
    csr2csc(L.aoclsparse_dcsr2csc, "declined", 0, 1, np.float64)
    declined = release()
    assert 4 * n <= declined < 4 * nnz, declined
    assert accepted - declined >= 4 * nnz + 4 * n, (accepted, declined)
    assert release() == 0


def test_handle_transpose_long_rows_every_value_size():
    """The same matrix as a handle: the transposes kept for op = T / H come from the same device sort, with 8-, 4- and 16-byte
    values (tr_gather_kernel<double> / <float> / <double2>, transpose_kernels.hip:234-242).  dmv / smv with op = T and zmv with
    op = T / H within (2 colmax + 16) eps scale (doubled for the complex multiply) of scipy's product; sp2m(A^T, B) with a thin
    B bit for bit the oracle's csr2csc + csr2m, which pins the order inside the columns."""
    import scipy.sparse as sp
    m, n, rp, ci, v = long_row_csr("accepted")
    colmax = int(np.bincount(ci, minlength=n).max())
    assert colmax == TR_WAVE_CAP
    rng = np.random.default_rng(2)
    d = P.Descr()
    for dt, mv, eps in ((np.float64, P.dmv, EPS64), (np.float32, P.smv, EPS32)):
        vt = v.astype(dt)
        A = P.Matrix(0, m, n, rp, ci, vt)
        assert A.status == 0
        x, y0 = rng.uniform(-1, 1, m).astype(dt), rng.uniform(-1, 1, n).astype(dt)
        y = y0.copy()
        assert mv(P.OP_TRANSPOSE, 1.5, A, d, x, -0.5, y) == 0
        A64 = sp.csr_matrix((vt.astype(np.float64), ci.copy(), rp.copy()), shape=(m, n))  # (copies: scipy may sort shared arrays)
        x64, y64 = x.astype(np.float64), y0.astype(np.float64)
        ref = 1.5 * (A64.T @ x64) - 0.5 * y64
        scale = 1.5 * (abs(A64).T @ np.abs(x64)) + 0.5 * np.abs(y64)
        assert np.all(np.abs(y - ref) <= (2 * colmax + 16) * eps * (scale + 1e-300)), dt
        if dt is np.float64:
            # A^T (n x m) times a thin B (m x 64 columns)
            pb, ib, vb = random_csr(9, m, 64, lambda r, i: r.integers(0, 3))
            B = P.Matrix(0, m, 64, pb, ib, vb)
            st, cp, ri, cv = oracle.dcsr2csc(m, n, len(v), 0, 0, rp, ci, v)
            so, pc, ic, vc = oracle.dcsr2m(n, 64, 0, cp, ri.astype(np.int32), cv, 0, pb, ib, vb)
            assert st == 0 and so == 0
            C = ctypes.c_void_p()
            assert L.aoclsparse_sp2m(P.OP_TRANSPOSE, d.h, A.h, P.OP_NONE, d.h, B.h, P.STAGE_FULL, ctypes.byref(C)) == 0
            x_ = export(C, "d")
            assert x_["nnz"] == len(ic)
            assert np.array_equal(x_["row_ptr"], pc) and np.array_equal(x_["col_ind"], ic) and np.array_equal(x_["val"], vc)
            assert L.aoclsparse_destroy(ctypes.byref(C)) == 0
    vz = (v + 1j * rng.uniform(-1, 1, len(v))).astype(np.complex128)
    Z = Handle(0, m, n, rp, ci, vz)
    Z64 = sp.csr_matrix((vz.copy(), ci.copy(), rp.copy()), shape=(m, n))  # (the handle aliases vz: scipy must not sort it)
    alpha, beta = np.array([0.7 - 0.4j]), np.array([-0.3 + 0.2j])
    x = rng.uniform(-1, 1, m) + 1j * rng.uniform(-1, 1, m)
    y0 = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    scale = abs(alpha[0]) * (abs(Z64).T @ np.abs(x)) + abs(beta[0]) * np.abs(y0)
    for op, left in ((P.OP_TRANSPOSE, Z64.T), (P.OP_CONJ_TRANSPOSE, Z64.conj().T)):
        y = y0.copy()
        assert L.aoclsparse_zmv(op, P._ptr(alpha), Z.h, d.h, P._ptr(x), P._ptr(beta), P._ptr(y)) == 0
        ref = alpha[0] * (left @ x) + beta[0] * y0
        assert np.all(np.abs(y - ref) <= 2 * (2 * colmax + 16) * EPS64 * (scale + 1e-300)), op
