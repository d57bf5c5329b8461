"""aoclsparse_mi355_clean_csr_device (device_handle_api.cpp, clean_csr_kernels.hip) and Matrix.clean_device: the clean CSR of a
handle -- rows in group order, a full diagonal, idiag / iurow -- built in HBM.

The yardstick is always a twin (clean_cases.twin): a host-created handle over copies of the same arrays, put through the library's
own HOST route (aoclsparse_optimize -> csr_optimize), exported, and first checked against a numpy restatement, so that "equal" cannot
mean "equally wrong".  The handle under test then calls clean_device() and must export the same row_ptr, col_ind, values (bitwise),
idiag, iurow and is_internal.

RW = P.CLEAN_ROW_WAVE is the header's macro: rows of up to RW entries are searched by one lane, longer ones by their wavefront; the
scan works in blocks of 1,024 rows, the copy in workgroups of 1,024 entries whatever rows they belong to."""
import ctypes
from ctypes import byref, c_void_p

import numpy as np
import pytest

from clean_cases import (DTYPES, EDGE_LONG, EDGE_SHAPES, INVALID_OPERATION, LETTER, SUCCESS, HostMatrix, assert_same_clean, class2_structure,
                         early_cases, edge_structure, edge_values, empty_structures, export_clean, one_row_structure, same_bits,
                         scan_edge_structure, tridiagonal_structure, twin)
from order_cases import Raw
from util import laplace5, pkg, random_csr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
P = pkg()
L = P.lib()

INVALID_VALUE = 5


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    yield
    L.aoclsparse_mi355_set_pointer_mode(P.PTR_AUTO)


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if len(a) else np.zeros(1, a.dtype)).cuda()  # (the library wants allocations, as the host call does)


def fetch(addr, count, dtype):
    """count elements at a device address -> numpy, by a plain ctypes hipMemcpy"""
    out = np.zeros(max(count, 1), dtype)
    hip = ctypes.CDLL(P.hip_runtime_path()[1])
    hip.hipMemcpy.argtypes = [c_void_p, c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip.hipMemcpy(P._ptr(out), c_void_p(addr), count * out.itemsize, 2) == 0  # hipMemcpyDeviceToHost
    return out[:count]


def export_dev(A, dtype):
    """aoclsparse_mi355_export_csr_device, read back -> (row_ptr, col_ind, val)"""
    e = A.export_device()
    assert e["status"] == 0, P.STATUS.get(e["status"], e["status"])
    return (fetch(e["row_ptr"], e["m"] + 1, np.int32), fetch(e["col_ind"], e["nnz"], np.int32), fetch(e["val"], e["nnz"], dtype))


def device_matrix(base, m, n, rp, ci, v):
    t = dev(np.asarray(rp, np.int32)), dev(np.asarray(ci, np.int32)), dev(v)
    torch.cuda.synchronize()
    D = P.Matrix.from_device(base, m, n, len(v), *t)
    for a in t:  # the arrays were copied
        a.zero_()
    torch.cuda.synchronize()
    assert D.status == 0, P.STATUS.get(D.status, D.status)
    return D


def check(base, m, n, rp, ci, v, what=""):
    """device-created handle + clean_device() against the twin -> (handle, twin handle, the common export)"""
    v = np.asarray(v)
    H, want = twin(base, m, n, rp, ci, v)
    D = device_matrix(base, m, n, rp, ci, v)
    assert D.export_diag()["status"] == INVALID_OPERATION
    st = D.clean_device()
    assert st == SUCCESS, (what, P.STATUS.get(st, st))
    assert_same_clean(export_clean(D, v.dtype), want, what)
    return D, H, want


# --------------------------------------------------------------------------------------------------
# 1. the edge matrix: class 3, every row length in every kind of row, all four value types
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(EDGE_SHAPES))
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_matrix(dtype, base, shape):
    m, n, rp, ci = edge_structure(shape)
    v = edge_values(dtype, len(ci))
    D, _, want = check(base, m, n, rp + base, ci + base, v, shape)
    cbase, cptr, cind, cval, idiag, iurow, internal = want
    assert internal and cbase == 0
    # every inserted entry is all-zero bits: the clean copy minus the original entries, row by row, is zeros on the diagonal
    inserted = len(cind) - len(ci)
    assert inserted > 1000 and inserted == np.count_nonzero(np.diff(cptr) - np.diff(rp))
    rows = np.repeat(np.arange(m), np.diff(cptr))
    zero = np.all(cval.reshape(len(cval), -1).view(np.uint8) == 0, axis=1)
    assert np.count_nonzero(zero & (cind == rows)) >= inserted
    assert np.max(np.diff(rp)) == EDGE_LONG


# --------------------------------------------------------------------------------------------------
# 2. case 2: the scan's block edges (class 1), the given order inside a row (class 2)
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1023, 1024, 1025, 2049])
def test_scan_edges(m):
    _, n, rp, ci = scan_edge_structure(m)
    for base, dtype in ((0, np.float64), (1, np.complex64)):
        _, _, want = check(base, m, n, rp + base, ci + base, edge_values(dtype, len(ci)), "scan %d" % m)
        assert want[6] and np.array_equal(want[2][want[4]], np.arange(m))  # a diagonal entry in every row, where idiag says


@pytest.mark.parametrize("base", [0, 1])
def test_class_2_rows_keep_their_given_order(base):
    m, n, rp, ci = class2_structure(False)
    v = edge_values(np.float64, len(ci))
    _, _, want = check(base, m, n, rp + base, ci + base, v)
    cptr, cind, cval = want[1:4]
    assert want[6] and len(cind) == len(ci) + m // 5
    zero = np.all(cval.reshape(len(cval), -1).view(np.uint8) == 0, axis=1)  # (all-zero bits: -0.0 is a value of the input)
    keep = ~((cind == np.repeat(np.arange(m), np.diff(cptr))) & zero)  # without the inserted entries: the arrays as given
    assert np.array_equal(cind[keep], ci) and same_bits(cval[keep], v)
    assert np.any(np.diff(cind[cptr[200]:cptr[201]]) < 0)  # descending runs survive


# --------------------------------------------------------------------------------------------------
# 3. case 1: nothing is copied
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("make", [tridiagonal_structure, lambda: class2_structure(True)], ids=["class 1", "class 2"])
def test_clean_arrays_are_used_as_they_are(make, base):
    m, n, rp, ci = make()
    for dtype in (np.float64, np.complex128):
        v = edge_values(dtype, len(ci))
        D, _, want = check(base, m, n, rp + base, ci + base, v)
        cbase, cptr, cind, cval, idiag, iurow, internal = want
        assert not internal and cbase == base
        assert np.array_equal(cptr, rp + base) and np.array_equal(cind, ci + base) and same_bits(cval, v)  # the handle's own arrays
        assert np.array_equal(cind[idiag - base], np.arange(m) + base) and np.array_equal(iurow, idiag + 1)  # positions keep the base
        dp, dc, dv = export_dev(D, dtype)
        assert np.array_equal(dp, rp + base) and np.array_equal(dc, ci + base) and same_bits(dv, v)


# --------------------------------------------------------------------------------------------------
# 4. one row holds every entry; empty shapes
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_row_holds_everything(dtype):
    m, n, rp, ci = one_row_structure()
    _, _, want = check(0, m, n, rp, ci, edge_values(dtype, len(ci)))
    assert np.array_equal(want[1], [0, 1, 5502, 5503]) and np.array_equal(want[4], [0, 2, 5502])  # (0, 0) | 0, (1, 1), 2 .. | (2, 2)


def test_empty_shapes():
    for name, m, n, rp, ci in empty_structures():
        for base in (0, 1):
            _, _, want = check(base, m, n, rp + base, ci + base, np.zeros(0, np.float64), name)
            assert len(want[2]) == (5 if name == "nnz = 0" else 0) and want[6] == (name == "nnz = 0"), name


# --------------------------------------------------------------------------------------------------
# 5. lifecycle
# --------------------------------------------------------------------------------------------------
def _tall(dtype=np.float64):
    m, n, rp, ci = edge_structure("tall")
    return m, n, rp, ci, edge_values(dtype, len(ci))


def test_second_call_resident_handle_and_untouched_mirror():
    m, n, rp, ci, v = _tall()
    D, _, want = check(0, m, n, rp, ci, v)
    assert D.spmv_info().device_resident == 1
    assert D.clean_device() == SUCCESS
    assert_same_clean(export_clean(D, v.dtype), want)
    dp, dc, dv = export_dev(D, v.dtype)  # the original, unsorted arrays
    assert np.array_equal(dp, rp) and np.array_equal(dc, ci) and same_bits(dv, v)


def test_host_created_handle_before_any_product():
    m, n, rp, ci, v = _tall()
    _, want = twin(0, m, n, rp, ci, v)
    A = HostMatrix(0, m, n, rp, ci, v)
    assert A.status == 0 and A.spmv_info().device_resident == 0
    assert A.clean_device() == SUCCESS
    assert A.spmv_info().device_resident == 1
    assert_same_clean(export_clean(A, v.dtype), want)
    assert np.array_equal(A.row_ptr, rp) and np.array_equal(A.col_ind, ci) and same_bits(A.val, v)  # the caller's arrays


def test_value_update_drops_the_copy_and_a_new_one_has_the_new_values():
    m, n, rp, ci, v = _tall()
    D, _, _ = check(0, m, n, rp, ci, v)
    v2 = edge_values(np.float64, len(ci), seed=78)
    assert not same_bits(v, v2)
    t = dev(v2)
    torch.cuda.synchronize()
    assert D.update_values_device(t) == SUCCESS
    assert D.export_diag()["status"] == INVALID_OPERATION
    assert D.clean_device() == SUCCESS
    _, want = twin(0, m, n, rp, ci, v2)
    assert_same_clean(export_clean(D, np.float64), want)


def test_sp2m_result():
    m, rp, ci, v = laplace5(60)
    A = HostMatrix(0, m, m, rp, ci, v * np.random.default_rng(8).uniform(0.5, 1.5, len(v)))
    d, C = P.Descr(), c_void_p()
    assert L.aoclsparse_sp2m(P.OP_NONE, d.h, A.h, P.OP_NONE, d.h, A.h, P.STAGE_FULL, byref(C)) == 0
    C = P.Matrix.from_handle(C, True)
    e = C.export()
    crp, cci, cv = e["row_ptr"], e["col_ind"], e["val"]
    assert sum(bool(np.any(np.diff(cci[crp[i]:crp[i + 1]]) < 0)) for i in range(m)) > m // 4, "rows in first-touch order"
    _, want = twin(0, m, m, crp, cci, cv)
    assert C.spmv_info().device_resident == 1
    assert C.clean_device() == SUCCESS
    assert_same_clean(export_clean(C, np.float64), want)


def test_csc_created_handle():
    """a handle created from CSC arrays holds a CSR of its own, which is what csr_optimize cleans"""
    m, n = 400, 300
    cp, ri, v = random_csr(21, n, m, lambda r, i: r.integers(0, 12))  # the CSR arrays of the transpose are the CSC arrays
    raw = Raw("aoclsparse_create_dcsc", 0, m, n, len(v), cp, ri, v)
    assert raw.status == 0
    A = P.Matrix.from_handle(raw.h, True)
    raw.h = None  # (A destroys it)
    e = A.export()
    assert e["status"] == 0 and (e["m"], e["n"], e["nnz"]) == (m, n, len(v))
    _, want = twin(e["base"], m, n, e["row_ptr"], e["col_ind"], e["val"])
    assert want[6] and len(want[2]) > len(v)  # diagonals were missing
    assert A.clean_device() == SUCCESS
    assert_same_clean(export_clean(A, np.float64), want)


def test_triplet_created_handle_keeps_its_map():
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
    _, want = twin(0, m, n, rp, ci, cv)
    assert A.clean_device() == SUCCESS
    assert_same_clean(export_clean(A, np.float64), want)
    assert A.coo_map_info().kept == 1
    assert A.refresh_from_coo_device(t[2]) == SUCCESS


# --------------------------------------------------------------------------------------------------
# 6. the consumers: triangular solves read the clean CSR and the diagonal's values this call left in HBM
# --------------------------------------------------------------------------------------------------
SOLVE_M = 3000


def solve_system(dtype, drop):
    """3,000 x 3,000, diagonally dominant, every row shuffled (class 3); drop: no diagonal entry in every 11th row"""
    rng = np.random.default_rng(31)
    rows, vals = [], []
    for i in range(SOLVE_M):
        c = rng.choice(SOLVE_M - 1, size=8, replace=False)
        c = c + (c >= i)  # anything but i
        x = rng.uniform(-0.05, 0.05, 8)
        if not (drop and i % 11 == 3):
            c, x = np.concatenate([c, [i]]), np.concatenate([x, [rng.uniform(2.0, 4.0)]])
        p = rng.permutation(len(c))
        rows.append(c[p])
        vals.append(x[p])
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int32)
    v = np.concatenate(vals)
    if np.dtype(dtype).kind == "c":
        v = v * np.exp(0.3j * rng.uniform(-1, 1, len(v)))
    return rp, np.concatenate(rows).astype(np.int32), v.astype(dtype)


def trsv(A, dtype, fill, diag, op, b):
    x = np.zeros_like(b)
    d = P.Descr(base=A.base, mtype=P.TYPE_TRIANGULAR, fill=fill, diag=diag)
    if np.dtype(dtype).kind == "c":
        st = L.aoclsparse_ztrsv(op, P.CDouble(0.5, 0.25), A.h, d.h, P._ptr(b), P._ptr(x))
    else:
        st = L.aoclsparse_dtrsv(op, 0.75, A.h, d.h, P._ptr(b), P._ptr(x))
    return st, x


@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_triangular_solves_and_the_product(dtype):
    rng = np.random.default_rng(5)
    b = rng.uniform(-1, 1, SOLVE_M).astype(dtype)
    if np.dtype(dtype).kind == "c":
        b = b + 1j * rng.uniform(-1, 1, SOLVE_M).astype(dtype)
    rp, ci, v = solve_system(dtype, drop=False)
    D, H, want = check(0, SOLVE_M, SOLVE_M, rp, ci, v)
    assert want[6] and len(want[2]) == len(ci)  # sorted copy, nothing inserted
    for fill in (P.FILL_LOWER, P.FILL_UPPER):
        for diag in (P.DIAG_NON_UNIT, P.DIAG_UNIT):
            for op in (P.OP_NONE, P.OP_TRANSPOSE):
                (sd, xd), (sh, xh) = trsv(D, dtype, fill, diag, op, b), trsv(H, dtype, fill, diag, op, b)
                assert sd == sh == SUCCESS and same_bits(xd, xh), (fill, diag, op)
                assert np.all(np.isfinite(xd)) and np.any(xd != 0)
    # diagonals missing: the non-unit solve refuses on the flag of the ORIGINAL arrays, the unit solve never reads the diagonal
    rp, ci, v = solve_system(dtype, drop=True)
    D2, H2, want = check(0, SOLVE_M, SOLVE_M, rp, ci, v)
    assert len(want[2]) > len(ci)
    for fill in (P.FILL_LOWER, P.FILL_UPPER):
        (sd, _), (sh, _) = trsv(D2, dtype, fill, P.DIAG_NON_UNIT, P.OP_NONE, b), trsv(H2, dtype, fill, P.DIAG_NON_UNIT, P.OP_NONE, b)
        assert sd == sh == INVALID_VALUE, (fill, P.STATUS.get(sd, sd), P.STATUS.get(sh, sh))
        (sd, xd), (sh, xh) = trsv(D2, dtype, fill, P.DIAG_UNIT, P.OP_NONE, b), trsv(H2, dtype, fill, P.DIAG_UNIT, P.OP_NONE, b)
        assert sd == sh == SUCCESS and same_bits(xd, xh), fill
    # the product path is undisturbed
    ys = []
    for X in (D, H):
        alpha, beta, y = np.array([1.3], dtype), np.array([-0.4], dtype), b.copy()
        d = P.Descr()
        fn = getattr(L, "aoclsparse_%smv" % LETTER[np.dtype(dtype)])
        assert fn(P.OP_NONE, P._ptr(alpha), X.h, d.h, P._ptr(b), P._ptr(beta), P._ptr(y)) == 0
        ys.append(y)
    assert same_bits(ys[0], ys[1]) and not same_bits(ys[0], b)


# --------------------------------------------------------------------------------------------------
# 7. statuses
# --------------------------------------------------------------------------------------------------
def test_statuses():
    for name, A, want in early_cases():
        got = L.aoclsparse_mi355_clean_csr_device(A.h if A is not None else None)
        assert got == want, (name, P.STATUS.get(got, got), P.STATUS.get(want, want))
