"""CPU tier of the device-array handle entry points (aoclsparse_mi355_create_?csr_device, ?update_values_device,
export_csr_device): everything they decide BEFORE the device is touched, and that the twelve names are declared, bound and exported.
What they do with arrays in HBM is tests/test_device_handles_gpu.py."""
import subprocess
from ctypes import byref, c_int, c_int32, c_void_p

import numpy as np
import pytest

from util import laplace5, pkg, random_csr

P = pkg()
L = P.lib()

INVALID_POINTER, INVALID_SIZE, WRONG_TYPE, NOT_IMPLEMENTED, INVALID_VALUE = 2, 3, 9, 1, 5
LETTERS = "sdcz"
DTYPE = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}


def _csr(dtype=np.float64):
    rp, ci, v = random_csr(5, 12, 9, lambda r, i: r.integers(0, 5))
    return rp, ci, v.astype(dtype)


def test_the_twelve_names_are_bound_and_exported():
    names = ["aoclsparse_mi355_create_%scsr_device" % t for t in LETTERS]
    names += ["aoclsparse_mi355_%supdate_values_device" % t for t in LETTERS]
    names += ["aoclsparse_mi355_export_csr_device"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", P.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for n in names:
        assert n in P.SIGNATURES, n
        assert n in exported, n
        assert getattr(L, n).argtypes == P.SIGNATURES[n][1]
    for t in LETTERS:  # the argument lists of the host entry points they mirror
        assert P.SIGNATURES["aoclsparse_mi355_create_%scsr_device" % t] == P.SIGNATURES["aoclsparse_create_%scsr" % t]
        assert P.SIGNATURES["aoclsparse_mi355_%supdate_values_device" % t] == P.SIGNATURES["aoclsparse_%supdate_values" % t]


@pytest.mark.parametrize("t", LETTERS)
def test_create_null_pointers(t):
    rp, ci, v = _csr(DTYPE[t])
    fn = getattr(L, "aoclsparse_mi355_create_%scsr_device" % t)
    nnz = len(v)
    assert fn(None, 0, 12, 9, nnz, P._ptr(rp), P._ptr(ci), P._ptr(v)) == INVALID_POINTER
    for k in range(3):
        h = c_void_p(1)
        args = [P._ptr(rp), P._ptr(ci), P._ptr(v)]
        args[k] = None
        assert fn(byref(h), 0, 12, 9, nnz, *args) == INVALID_POINTER
        assert not h.value, "*mat is cleared, as aoclsparse_create_?csr does"
    # a null array comes before a negative size, as in mat_check
    h = c_void_p()
    assert fn(byref(h), 0, -1, 9, nnz, None, P._ptr(ci), P._ptr(v)) == INVALID_POINTER


@pytest.mark.parametrize("M,N,nnz", [(-1, 9, 3), (12, -1, 3), (12, 9, -1), (-1, -1, -1)])
def test_create_negative_sizes_answer_as_the_host_call(M, N, nnz):
    rp, ci, v = _csr()
    h0, h1 = c_void_p(), c_void_p()
    host = L.aoclsparse_create_dcsr(byref(h0), 0, M, N, nnz, P._ptr(rp), P._ptr(ci), P._ptr(v))
    dev = L.aoclsparse_mi355_create_dcsr_device(byref(h1), 0, M, N, nnz, P._ptr(rp), P._ptr(ci), P._ptr(v))
    assert host != 0 and dev == host, (P.STATUS.get(dev), P.STATUS.get(host))
    assert dev == INVALID_SIZE
    assert not h1.value


def test_update_values_device_statuses_in_the_order_of_the_host_call():
    rp, ci, v = _csr()
    A = P.Matrix(0, 12, 9, rp, ci, v)
    assert A.status == 0
    nnz = len(v)
    new = np.ones(nnz)
    for dev_fn, host_fn in ((L.aoclsparse_mi355_dupdate_values_device, L.aoclsparse_dupdate_values),
                            (L.aoclsparse_mi355_supdate_values_device, L.aoclsparse_supdate_values)):
        wrong_type = dev_fn is L.aoclsparse_mi355_supdate_values_device
        cases = [(None, nnz, P._ptr(new)),  # null handle
                 (A.h, nnz, None),  # null values
                 (A.h, nnz + 1, None),  # null values before the wrong length
                 (A.h, nnz + 1, P._ptr(new))]  # wrong length (before the wrong type)
        if wrong_type:
            cases.append((A.h, nnz, P._ptr(new)))
        for args in cases:
            want = host_fn(*args)
            assert want != 0
            assert dev_fn(*args) == want, (args[1], P.STATUS.get(want))
    assert L.aoclsparse_mi355_supdate_values_device(A.h, nnz + 1, P._ptr(new)) == INVALID_SIZE
    assert L.aoclsparse_mi355_supdate_values_device(A.h, nnz, P._ptr(new)) == WRONG_TYPE
    assert L.aoclsparse_mi355_dupdate_values_device(A.h, nnz, None) == INVALID_POINTER
    assert np.array_equal(A.val, v), "a refused update leaves the values alone"


def test_update_values_device_on_handles_without_a_csr_of_their_own():
    """TCSR / BSR: not_implemented, as ?update_values; COO and CSC-created handles: not_implemented (their values follow host arrays)"""
    m, rp, ci, v = laplace5(4)
    new = np.ones(len(v))
    # COO
    rows = np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))
    h = c_void_p()
    assert L.aoclsparse_create_dcoo(byref(h), 0, m, m, len(v), P._ptr(rows), P._ptr(ci), P._ptr(v)) == 0
    assert L.aoclsparse_mi355_dupdate_values_device(h, len(v), P._ptr(new)) == NOT_IMPLEMENTED
    assert L.aoclsparse_mi355_dupdate_values_device(h, len(v) + 1, P._ptr(new)) == INVALID_SIZE
    base, M, N, nnz, a, b, c = c_int(), c_int32(), c_int32(), c_int32(), c_void_p(), c_void_p(), c_void_p()
    assert L.aoclsparse_mi355_export_csr_device(h, byref(base), byref(M), byref(N), byref(nnz), byref(a), byref(b), byref(c)) == INVALID_VALUE
    L.aoclsparse_destroy(byref(h))
    # CSC (the Laplacian is symmetric: its CSR arrays are its CSC arrays)
    h = c_void_p()
    assert L.aoclsparse_create_dcsc(byref(h), 0, m, m, len(v), P._ptr(rp), P._ptr(ci), P._ptr(v)) == 0
    assert L.aoclsparse_mi355_dupdate_values_device(h, len(v), P._ptr(new)) == NOT_IMPLEMENTED
    L.aoclsparse_destroy(byref(h))
    # TCSR
    keep_l, keep_u = ci <= np.repeat(np.arange(m), np.diff(rp)), ci >= np.repeat(np.arange(m), np.diff(rp))

    def tri(keep):
        p = np.concatenate([[0], np.cumsum(np.add.reduceat(keep.astype(int), rp[:-1]))]).astype(np.int32)
        return p, ci[keep].copy(), v[keep].copy()

    T = P.TcsrMatrix(0, m, *tri(keep_l), *tri(keep_u))
    assert T.status == 0
    assert L.aoclsparse_mi355_dupdate_values_device(T.h, T.nnz, P._ptr(new)) == NOT_IMPLEMENTED
    assert L.aoclsparse_mi355_export_csr_device(T.h, byref(base), byref(M), byref(N), byref(nnz), byref(a), byref(b), byref(c)) == INVALID_VALUE


def test_export_csr_device_null_arguments():
    rp, ci, v = _csr()
    A = P.Matrix(0, 12, 9, rp, ci, v)
    base, M, N, nnz, a, b, c = c_int(), c_int32(), c_int32(), c_int32(), c_void_p(), c_void_p(), c_void_p()
    outs = [byref(base), byref(M), byref(N), byref(nnz), byref(a), byref(b), byref(c)]
    assert L.aoclsparse_mi355_export_csr_device(None, *outs) == INVALID_POINTER
    for k in range(len(outs)):
        args = list(outs)
        args[k] = None
        assert L.aoclsparse_mi355_export_csr_device(A.h, *args) == INVALID_POINTER, k
