"""CPU tier of aoclsparse_mi355_create_?csr_from_coo_device (CSR handles from unordered triplets in HBM): that the four names are
declared, bound and exported, and everything they decide BEFORE the device is touched -- in the order of aoclsparse_create_?coo,
where sizes come before arrays.  What they do with triplets in HBM is tests/test_coo_device_gpu.py."""
import os
import re
import subprocess
from ctypes import POINTER, byref, c_int32, c_void_p

import numpy as np
import pytest

from util import ROOT, pkg

P = pkg()
L = P.lib()

INVALID_POINTER, INVALID_SIZE, INVALID_VALUE = 2, 3, 5
LETTERS = "sdcz"
DTYPE = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}
M, N = 12, 9


def _coo(dtype=np.float64):
    rng = np.random.default_rng(3)
    nnz = 30
    return rng.integers(0, M, nnz).astype(np.int32), rng.integers(0, N, nnz).astype(np.int32), rng.uniform(-1, 1, nnz).astype(dtype)


def _fn(t):
    return getattr(L, "aoclsparse_mi355_create_%scsr_from_coo_device" % t)


def test_the_four_names_are_declared_bound_and_exported():
    names = ["aoclsparse_mi355_create_%scsr_from_coo_device" % t for t in LETTERS]
    header = open(os.path.join(ROOT, "include", "aoclsparse_mi355.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", P.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for n in names:
        assert re.search(r"DLL_PUBLIC\s+aoclsparse_status\s+%s\s*\(" % n, header), n
        assert n in P.SIGNATURES, n
        assert n in exported, n
        assert getattr(L, n).argtypes == P.SIGNATURES[n][1]
    for t in LETTERS:  # the argument list of aoclsparse_create_?coo plus one integer
        res, args = P.SIGNATURES["aoclsparse_mi355_create_%scsr_from_coo_device" % t]
        hres, hargs = P.SIGNATURES["aoclsparse_create_%scoo" % t]
        assert res == hres and args == hargs + [c_int32]
    assert (P.COO_KEEP, P.COO_SUM) == (0, 1)
    m = re.search(r"#define\s+AOCLSPARSE_MI355_COO_SORT_TILE\s+(\d+)", header)
    assert m and int(m.group(1)) == P.COO_SORT_TILE


def test_python_constructors_exist():
    assert callable(P.Matrix.from_coo_device) and callable(P.Matrix.from_torch_coo)


@pytest.mark.parametrize("t", LETTERS)
def test_null_pointers(t):
    r, c, v = _coo(DTYPE[t])
    fn, nnz = _fn(t), len(v)
    assert fn(None, 0, M, N, nnz, P._ptr(r), P._ptr(c), P._ptr(v), 0) == INVALID_POINTER
    for k in range(3):
        h = c_void_p(1)
        args = [P._ptr(r), P._ptr(c), P._ptr(v)]
        args[k] = None
        assert fn(byref(h), 0, M, N, nnz, *args, 0) == INVALID_POINTER
        assert not h.value, "*mat is cleared"
        if t == "d":  # the host counterpart answers the same
            h0 = c_void_p(1)
            assert L.aoclsparse_create_dcoo(byref(h0), 0, M, N, nnz, *args) == INVALID_POINTER
            assert not h0.value
    assert L.aoclsparse_create_dcoo(None, 0, M, N, nnz, P._ptr(r), P._ptr(c), P._ptr(v)) == INVALID_POINTER


@pytest.mark.parametrize("m,n,nnz", [(-1, N, 3), (M, -1, 3), (M, N, -1), (-1, -1, -1)])
@pytest.mark.parametrize("null", [None, 0, 1, 2])
def test_negative_sizes_come_before_null_arrays_as_in_create_coo(m, n, nnz, null):
    r, c, v = _coo()
    args = [P._ptr(r), P._ptr(c), P._ptr(v)]
    if null is not None:
        args[null] = None
    h0, h1 = c_void_p(1), c_void_p(1)
    host = L.aoclsparse_create_dcoo(byref(h0), 0, m, n, nnz, *args)
    dev = L.aoclsparse_mi355_create_dcsr_from_coo_device(byref(h1), 0, m, n, nnz, *args, 0)
    assert host == INVALID_SIZE and dev == host, (P.STATUS.get(dev), P.STATUS.get(host))
    assert not h1.value


@pytest.mark.parametrize("t", LETTERS)
@pytest.mark.parametrize("dup", [2, -1, 7])
def test_duplicates_other_than_0_and_1(t, dup):
    r, c, v = _coo(DTYPE[t])
    h = c_void_p(1)
    assert _fn(t)(byref(h), 0, M, N, len(v), P._ptr(r), P._ptr(c), P._ptr(v), dup) == INVALID_VALUE
    assert not h.value
    # ... behind the sizes and the null arrays
    h = c_void_p(1)
    assert _fn(t)(byref(h), 0, -1, N, len(v), P._ptr(r), P._ptr(c), P._ptr(v), dup) == INVALID_SIZE
    assert not h.value
    h = c_void_p(1)
    assert _fn(t)(byref(h), 0, M, N, len(v), P._ptr(r), None, P._ptr(v), dup) == INVALID_POINTER
    assert not h.value
