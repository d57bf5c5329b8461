"""aoclsparse_mi355_order_mat_device (device_handle_api.cpp, order_kernels.hip) and Matrix.order_device: the rows of a CSR handle
put into ascending column order in HBM, the handle resident afterwards.

The yardstick is the library's own HOST route: a twin handle over copies of the same arrays, put through aoclsparse_order_mat and
exported with aoclsparse_export_?csr.  A few lines of numpy restate it (stable_order: np.lexsort((position, column, row))), so that
"equal" cannot mean "equally wrong".  Integers must be equal, values bitwise equal.

S = P.ORDER_SHORT_MAX (a lane per row up to it), W = P.ORDER_LDS_MAX (a workgroup in LDS up to it, the radix sort above) and
T = P.COO_SORT_TILE (what a workgroup of the radix sort takes per pass) are the header's macros; the row lengths around them, around
the wavefront (64) and around the one-wavefront / four-wavefront split of the LDS kernel (256) are where the sort can go wrong."""
import ctypes
from ctypes import byref, c_int, c_int32, c_void_p

import numpy as np
import pytest

from order_cases import early_cases
from util import laplace5, pkg, random_csr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
P = pkg()
L = P.lib()
S, W, T = P.ORDER_SHORT_MAX, P.ORDER_LDS_MAX, P.COO_SORT_TILE

SUCCESS, INVALID_VALUE = 0, 5
LETTER = {np.dtype(np.float32): "s", np.dtype(np.float64): "d", np.dtype(np.complex64): "c", np.dtype(np.complex128): "z"}
DTYPES = [np.float32, np.float64, np.complex64, np.complex128]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    yield
    L.aoclsparse_mi355_set_pointer_mode(P.PTR_AUTO)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def fetch(addr, count, dtype):
    """count elements at a device address -> numpy, by a plain ctypes hipMemcpy"""
    out = np.zeros(max(count, 1), dtype)
    hip = ctypes.CDLL(P.hip_runtime_path()[1])
    hip.hipMemcpy.argtypes = [c_void_p, c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip.hipMemcpy(P._ptr(out), c_void_p(addr), count * out.itemsize, 2) == 0  # hipMemcpyDeviceToHost
    return out[:count]


def export_host(h, dtype):
    """aoclsparse_export_?csr of a raw handle -> (row_ptr, col_ind, val) as copies"""
    base, m, n, nnz = c_int(), c_int32(), c_int32(), c_int32()
    rp, ci, v = c_void_p(), c_void_p(), c_void_p()
    fn = getattr(L, "aoclsparse_export_%scsr" % LETTER[np.dtype(dtype)])
    assert fn(h, byref(base), byref(m), byref(n), byref(nnz), byref(rp), byref(ci), byref(v)) == 0

    def arr(p, count, dt):
        return np.frombuffer(ctypes.string_at(p.value, count * np.dtype(dt).itemsize), dt).copy() if count else np.zeros(0, dt)

    return arr(rp, m.value + 1, np.int32), arr(ci, nnz.value, np.int32), arr(v, nnz.value, dtype)


def export_dev(A, dtype):
    """aoclsparse_mi355_export_csr_device, read back -> (row_ptr, col_ind, val)"""
    e = A.export_device()
    assert e["status"] == 0, P.STATUS.get(e["status"], e["status"])
    return (fetch(e["row_ptr"], e["m"] + 1, np.int32), fetch(e["col_ind"], e["nnz"], np.int32), fetch(e["val"], e["nnz"], dtype))


class HostMatrix(P.Matrix):
    """aoclsparse_create_?csr over copies of the arrays, any of the four value types"""

    def __init__(self, base, m, n, rp, ci, v):
        self.row_ptr = np.array(rp, dtype=np.int32)
        self.col_ind = np.array(ci, dtype=np.int32)
        self.val = np.array(v)
        self.letter = LETTER[self.val.dtype]
        self.double = self.val.dtype == np.float64
        self.m, self.n, self.nnz, self.base = m, n, len(self.val), base
        self.h = c_void_p()
        fn = getattr(L, "aoclsparse_create_%scsr" % self.letter)
        self.status = fn(byref(self.h), base, m, n, self.nnz, P._ptr(self.row_ptr), P._ptr(self.col_ind), P._ptr(self.val))


def device_matrix(base, m, n, rp, ci, v):
    t = dev(np.asarray(rp, np.int32)), dev(np.asarray(ci, np.int32)), dev(v)
    torch.cuda.synchronize()
    D = P.Matrix.from_device(base, m, n, len(v), *t)
    for a in t:  # the arrays were copied
        a.zero_()
    torch.cuda.synchronize()
    return D


def stable_order(rp, ci, base):
    """the permutation aoclsparse_order_mat applies, restated: by (row, column, position)"""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    return np.lexsort((np.arange(len(ci)), ci, rows))


def twin(base, m, n, rp, ci, v):
    """the yardstick: (handle, col_ind, val) of a host handle over copies, after aoclsparse_order_mat; checked against numpy"""
    H = HostMatrix(base, m, n, rp, ci, v)
    assert H.status == 0, P.STATUS.get(H.status, H.status)
    assert L.aoclsparse_order_mat(H.h) == 0
    hp, hc, hv = export_host(H.h, v.dtype)
    perm = stable_order(rp, ci, base)
    assert np.array_equal(hp, rp) and np.array_equal(hc, ci[perm]) and same_bits(hv, v[perm])
    return H, hc, hv


_dummy = np.zeros(8, np.float32)


def probe(A):
    """(class 3 / no full diagonal / neither, class 1 or not) as the statuses of two calls that refuse before they compute
    (tests/test_device_handles_gpu.py explains them)"""
    pre = c_void_p()
    d = P.Descr(base=A.base)
    a = L.aoclsparse_silu_smoother(P.OP_NONE, A.h, d.h, byref(pre), None, P._ptr(_dummy), P._ptr(_dummy))
    b = L.aoclsparse_dsyrkd(P.OP_TRANSPOSE, A.h, 1.0, 0.0, P._ptr(_dummy), P.ORDER_ROW, 0)
    return a, b


def mv(A, dtype, op, x, y0):
    """y = 1.3 op(A) x - 0.4 y0 in the handle's value type (host vectors) -> y"""
    dtype = np.dtype(dtype)
    alpha, beta, y = np.array([1.3], dtype), np.array([-0.4], dtype), y0.copy()
    fn = getattr(L, "aoclsparse_%smv" % LETTER[dtype])
    assert fn(op, P._ptr(alpha), A.h, P.Descr(base=A.base).h, P._ptr(x), P._ptr(beta), P._ptr(y)) == 0
    return y


def vectors(dtype, m, n, seed):
    rng = np.random.default_rng(seed)

    def vec(k):
        r = rng.uniform(-1, 1, k)
        return (r + 1j * rng.uniform(-1, 1, k) if np.dtype(dtype).kind == "c" else r).astype(dtype)

    return vec(n), vec(m), vec(m), vec(n)  # x, y0 for op = none; x, y0 for op = transpose


def same_products(A, B, dtype, m, n, seed=3):
    xn, yn, xt, yt = vectors(dtype, m, n, seed)
    assert same_bits(mv(A, dtype, P.OP_NONE, xn, yn), mv(B, dtype, P.OP_NONE, xn, yn))
    assert same_bits(mv(A, dtype, P.OP_TRANSPOSE, xt, yt), mv(B, dtype, P.OP_TRANSPOSE, xt, yt))


# --------------------------------------------------------------------------------------------------
# 1. the edge matrix
# --------------------------------------------------------------------------------------------------
EDGE_M, EDGE_N = 3 * 256 + 100, 20000
EDGE_CYCLE = [0, 1, 2, S - 1, S, S + 1, 63, 64, 65, 255, 256, 257]
# one row each; 3T + 17 at row 0, T + 1 in the last, partial wavefront of the last, partial workgroup (rows 832 .. 867)
EDGE_SPECIAL = {0: 3 * T + 17, 100: W - 1, 400: W + 1, 500: W, EDGE_M - 8: T + 1}
_edge = {}


def edge_structure():
    """(row_ptr, col_ind) 0-based, built once: lengths cycle through EDGE_CYCLE, the kind of order cycles so that every length
    meets every kind: 0 ascending already, 1 descending, 2 a random permutation, 3 a permutation with one column held twice and
    (from five entries on) another one three times -- never the diagonal, which a handle refuses twice"""
    if "s" in _edge:
        return _edge["s"]
    rng = np.random.default_rng(2323)
    rows, kinds = [], []
    for i in range(EDGE_M):
        k = EDGE_SPECIAL.get(i, EDGE_CYCLE[i % len(EDGE_CYCLE)])
        kind = (i + i // len(EDGE_CYCLE)) % 4
        if i in EDGE_SPECIAL:
            kind = {0: 2, 100: 1, 400: 3, 500: 2, EDGE_M - 8: 3}[i]
        extra = (1 if k >= 2 else 0) + (2 if k >= 5 else 0) if kind == 3 else 0
        c = np.sort(rng.choice(EDGE_N, size=k - extra, replace=False))
        if kind == 1:
            c = c[::-1]
        elif kind == 2:
            c = rng.permutation(c)
        elif kind == 3 and k >= 2:
            cand = c[c != i]
            twice = cand[rng.integers(len(cand))]
            c = np.concatenate([c, [twice]])
            if k >= 5:
                thrice = rng.choice(cand[cand != twice])
                c = np.concatenate([c, [thrice, thrice]])
            c = rng.permutation(c)
        assert len(c) == k
        rows.append(c)
        kinds.append(kind)
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    assert 80000 < len(ci) < 120000
    for i in (0, EDGE_M - 8):  # a long row at row 0 and one in the last partial wavefront
        assert rp[i + 1] - rp[i] > W and not np.all(np.diff(ci[rp[i]:rp[i + 1]]) >= 0)
    assert EDGE_M - 8 >= 3 * 256 + 64
    _edge["s"] = rp, ci
    return _edge["s"]


def edge_values(dtype):
    """distinct values (exact in every type: integers below 2^24 over 1024, signs mixed), so that the entries of a repeated column
    can be told apart: that pins stability"""
    rp, ci = edge_structure()
    rng = np.random.default_rng(77)
    v = (rng.permutation(len(ci)) + 1) / 1024.0 * np.where(rng.integers(0, 2, len(ci)) == 0, 1.0, -1.0)
    if np.dtype(dtype).kind == "c":
        v = v + 1j * rng.uniform(-1, 1, len(ci))
    v = v.astype(dtype)
    assert len(np.unique(np.abs(v.real))) == len(v)
    return v


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_matrix(dtype, base):
    rp, ci = edge_structure()
    rp, ci, v = rp + base, ci + base, edge_values(dtype)
    H, hc, hv = twin(base, EDGE_M, EDGE_N, rp, ci, v)
    D = device_matrix(base, EDGE_M, EDGE_N, rp, ci, v)
    assert D.status == 0
    assert D.order_device() == SUCCESS
    assert D.spmv_info().device_resident == 1  # before any product
    dp, dc, dv = export_dev(D, dtype)
    assert np.array_equal(dp, rp) and np.array_equal(dc, hc) and same_bits(dv, hv)
    ep, ec, ev = export_host(D.h, dtype)
    assert np.array_equal(ep, rp) and np.array_equal(ec, hc) and same_bits(ev, hv)
    assert probe(D) == probe(H)
    same_products(D, H, dtype, EDGE_M, EDGE_N)
    assert D.spmv_info().device_resident == 1


# --------------------------------------------------------------------------------------------------
# 2. - 6. the kinds of handle
# --------------------------------------------------------------------------------------------------
def test_host_created_handle_is_sorted_in_place_and_resident():
    rp, ci = edge_structure()
    v = edge_values(np.float64)
    _, hc, hv = twin(0, EDGE_M, EDGE_N, rp, ci, v)
    A = HostMatrix(0, EDGE_M, EDGE_N, rp, ci, v)
    assert A.status == 0 and A.spmv_info().device_resident == 0
    assert A.order_device() == SUCCESS
    assert np.array_equal(A.row_ptr, rp) and np.array_equal(A.col_ind, hc) and same_bits(A.val, hv)  # the caller's own arrays
    assert A.spmv_info().device_resident == 1
    dp, dc, dv = export_dev(A, np.float64)
    assert np.array_equal(dp, rp) and np.array_equal(dc, hc) and same_bits(dv, hv)


def test_derived_state_is_dropped_and_the_mirror_current():
    """a SELL-64 copy and a kept transpose of the UNSORTED arrays exist when the handle is ordered; the products afterwards are
    those of the host-ordered twin, which went through the same calls"""
    m = 6000
    rp, ci, v = random_csr(41, m, m, lambda r, i: r.integers(1, 24), sort=False)
    assert L.aoclsparse_mi355_set_option(P.OPTION_SELL, 1) == 0
    try:
        A, B = device_matrix(0, m, m, rp, ci, v), HostMatrix(0, m, m, rp, ci, v)
        xn, yn, xt, yt = vectors(np.float64, m, m, 9)
        for X in (A, B):
            assert X.status == 0
            d = P.Descr()
            assert L.aoclsparse_set_mv_hint(X.h, P.OP_NONE, d.h, 100) == 0 and L.aoclsparse_optimize(X.h) == 0
            mv(X, np.float64, P.OP_NONE, xn, yn)
            mv(X, np.float64, P.OP_TRANSPOSE, xt, yt)
        assert A.spmv_info().kernel in (3, 4)  # the SELL-64 copy is what the product ran on
        assert A.order_device() == SUCCESS and L.aoclsparse_order_mat(B.h) == 0
        assert A.spmv_info().device_resident == 1
        same_products(A, B, np.float64, m, m, seed=9)
        # ... and they are the products of a fresh handle over the sorted arrays, not of a copy that outlived the call
        perm = stable_order(rp, ci, 0)
        same_products(A, HostMatrix(0, m, m, rp, ci[perm], v[perm]), np.float64, m, m, seed=10)
    finally:
        assert L.aoclsparse_mi355_set_option(P.OPTION_SELL, -1) == 0


def sp2m(A, B):
    d, C = P.Descr(), c_void_p()
    assert L.aoclsparse_sp2m(P.OP_NONE, d.h, A.h, P.OP_NONE, d.h, B.h, P.STAGE_FULL, byref(C)) == 0
    return P.Matrix.from_handle(C, True)


def _lap():
    m, rp, ci, v = laplace5(40)
    return m, m, (rp, ci, v * np.random.default_rng(8).uniform(0.5, 1.5, len(v))), None


def _pair():
    m, k, n = 700, 500, 900
    return m, n, random_csr(5, m, k, lambda r, i: r.integers(0, 9)), random_csr(6, k, n, lambda r, i: r.integers(0, 40))


@pytest.mark.parametrize("make", [_lap, _pair], ids=["laplacian squared", "random pair"])
def test_sp2m_result(make):
    m, n, a, b = make()
    A = HostMatrix(0, m, len(a[0]) - 1 if b is None else len(b[0]) - 1, *a)
    B = A if b is None else HostMatrix(0, len(b[0]) - 1, n, *b)
    C = sp2m(A, B)
    e = C.export()
    rp, ci, v = e["row_ptr"], e["col_ind"], e["val"]
    unsorted = sum(bool(np.any(np.diff(ci[rp[i]:rp[i + 1]]) < 0)) for i in range(m))
    assert unsorted > m // 4, "the result's rows are in first-touch order: the input is not vacuous"
    H, hc, hv = twin(0, m, n, rp, ci, v)
    assert C.order_device() == SUCCESS
    assert C.spmv_info().device_resident == 1
    dp, dc, dv = export_dev(C, np.float64)
    assert np.array_equal(dp, rp) and np.array_equal(dc, hc) and same_bits(dv, hv)
    e = C.export()
    assert np.array_equal(e["col_ind"], hc) and same_bits(e["val"], hv)
    # as an operand of a second product
    Bt = HostMatrix(0, n, m, *random_csr(7, n, m, lambda r, i: r.integers(0, 6)))
    e1, e2 = sp2m(C, Bt).export(), sp2m(H, Bt).export()
    assert e1["nnz"] == e2["nnz"] > 0
    for k in ("row_ptr", "col_ind"):
        assert np.array_equal(e1[k], e2[k]), k
    assert same_bits(e1["val"], e2["val"])


def test_triplet_created_handle_loses_its_map():
    m, n = 900, 700
    rng = np.random.default_rng(12)
    nnz = 30000
    flat = rng.choice(m * n, size=nnz, replace=False)  # distinct coordinates, any order: the rows come out unsorted
    row, col, v = (flat // n).astype(np.int32), (flat % n).astype(np.int32), rng.uniform(-1, 1, nnz)
    t = dev(row), dev(col), dev(v)
    torch.cuda.synchronize()
    A = P.Matrix.from_coo_device(0, m, n, nnz, *t, duplicates=P.COO_KEEP, refreshable=True)
    assert A.status == 0 and A.coo_map_info().kept == 1
    rp, ci, cv = export_dev(A, np.float64)
    _, hc, hv = twin(0, m, n, rp, ci, cv)
    assert not np.array_equal(ci, hc)
    assert A.order_device() == SUCCESS
    assert A.coo_map_info().kept == 0
    assert A.refresh_from_coo_device(t[2]) == INVALID_VALUE
    dp, dc, dv = export_dev(A, np.float64)
    assert np.array_equal(dp, rp) and np.array_equal(dc, hc) and same_bits(dv, hv)


def test_fully_sorted_handle_is_left_alone():
    m, n = 5000, 7000
    rp, ci, v = random_csr(19, m, n, lambda r, i: r.integers(0, 90), base=1)
    A = device_matrix(1, m, n, rp, ci, v)
    assert A.status == 0
    before = probe(A)
    assert A.order_device() == SUCCESS
    assert A.spmv_info().device_resident == 1
    dp, dc, dv = export_dev(A, np.float64)
    assert np.array_equal(dp, rp) and np.array_equal(dc, ci) and same_bits(dv, v)
    ep, ec, ev = export_host(A.h, np.float64)
    assert np.array_equal(ep, rp) and np.array_equal(ec, ci) and same_bits(ev, v)
    assert probe(A) == before


# --------------------------------------------------------------------------------------------------
# 7. statuses
# --------------------------------------------------------------------------------------------------
def test_statuses():
    for name, A, want in early_cases():
        got = L.aoclsparse_mi355_order_mat_device(A.h if A is not None else None)
        assert got == want, (name, P.STATUS.get(got, got), P.STATUS.get(want, want))
