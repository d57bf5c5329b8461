"""CPU tier of aoclsparse_mi355_?ilu0_refactor_device / aoclsparse_mi355_get_ilu_info: the symbols, and every status that is
decided before the device is touched, in the smoother's order (no device needed)."""
import ctypes
import os
import re
import subprocess
from ctypes import byref, c_void_p

import numpy as np

from util import ROOT, laplace5, pkg, random_csr

P = pkg()
L = P.lib()
NOT_IMPLEMENTED, INVALID_POINTER, INVALID_SIZE, INVALID_VALUE, WRONG_TYPE, NUMERICAL_ERROR, UNSORTED = 1, 2, 3, 5, 9, 11, 13
NAMES = ["aoclsparse_mi355_%silu0_refactor_device" % t for t in "sdcz"] + ["aoclsparse_mi355_get_ilu_info"]


def _with_diagonal(rp, ci, m, n, shuffle_seed=None):
    """every row i < min(m, n) holds its diagonal; rows sorted, or (shuffle_seed) in random order"""
    rp, ci = rp.copy(), ci.copy()
    rng = np.random.default_rng(shuffle_seed)
    for i in range(m):
        row = ci[rp[i]:rp[i + 1]]
        if i < n and i not in row:
            row[0] = i
        row[:] = np.sort(row) if shuffle_seed is None else rng.permutation(row)
    return rp, ci


def test_symbols_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "aoclsparse_mi355.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", P.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NAMES:
        assert re.search(r"DLL_PUBLIC\s+aoclsparse_status\s+%s\s*\(" % name, src), name
        assert name in exported, name
        assert name in P.SIGNATURES and getattr(L, name).argtypes is not None, name
    assert re.search(r"aoclsparse_mi355_option_ilu_search\s*=\s*%d\b" % P.OPTION_ILU_SEARCH, src)
    assert re.search(r"#define\s+AOCLSPARSE_MI355_ILU_SEARCH_MIN\s+%d\b" % P.ILU_SEARCH_MIN, src)


def test_ilu_search_option_is_validated():
    for bad in (-2, 2, 7):
        assert L.aoclsparse_mi355_set_option(P.OPTION_ILU_SEARCH, bad) == INVALID_VALUE
    for good in (0, 1, -1):  # (-1, the default, last)
        assert L.aoclsparse_mi355_set_option(P.OPTION_ILU_SEARCH, good) == 0
    assert L.aoclsparse_mi355_set_option(P.OPTION_ILU_SEARCH + 1, 0) == INVALID_VALUE


def test_early_statuses_in_the_smoothers_order():
    """Each handle provokes one status and every status that comes AFTER it in the order, so the order itself is pinned:
    null A, the format, the sort class, the full diagonal, the value type, the shape, and m == 0."""
    f = c_void_p(12345)
    refactor = {t: getattr(L, "aoclsparse_mi355_%silu0_refactor_device" % t) for t in "sdcz"}
    for fn in refactor.values():
        assert fn(None, byref(f)) == INVALID_POINTER
        assert fn(None, None) == INVALID_POINTER
    m, rp, ci, v = laplace5(4)
    # formats without a CSR of their own: TCSR and BSR are refused as not implemented, whatever else is wrong (here: the type)
    rid = np.repeat(np.arange(m), np.diff(rp))
    keep_l, keep_u = ci <= rid, ci >= rid

    def tri(keep):
        p = np.concatenate([[0], np.cumsum(np.add.reduceat(keep.astype(int), rp[:-1]))]).astype(np.int32)
        return p, ci[keep].copy(), v[keep].copy()

    T = P.TcsrMatrix(0, m, *tri(keep_l), *tri(keep_u))
    assert T.status == 0
    B = P.BsrMatrix(0, 0, m, m, 1, rp, ci, v)
    assert B.status == 0
    for H in (T, B):
        for fn in refactor.values():
            assert fn(H.h, byref(f)) == NOT_IMPLEMENTED
    # ... and a COO handle holds no CSR arrays at all: the smoother's answer, invalid_pointer
    h = c_void_p()
    assert L.aoclsparse_create_dcoo(byref(h), 0, m, m, len(v), P._ptr(rid.astype(np.int32)), P._ptr(ci), P._ptr(v)) == 0
    assert refactor["d"](h, byref(f)) == INVALID_POINTER
    L.aoclsparse_destroy(byref(h))
    # 12 x 9, float64, called through the float entry point: wrong type AND not square, from here on
    M, N = 12, 9
    rp0, ci0, v0 = random_csr(5, M, N, lambda r, i: 4)
    # rows in random order (with their diagonal): unsorted_input comes first
    rpu, ciu = _with_diagonal(rp0, ci0, M, N, shuffle_seed=3)
    U = P.Matrix(0, M, N, rpu, ciu, v0)
    assert U.status == 0
    assert refactor["s"](U.h, byref(f)) == UNSORTED and refactor["d"](U.h, byref(f)) == UNSORTED
    # sorted rows, row 2 without its diagonal: numerical_error comes before the type and the shape
    rps, cis = _with_diagonal(rp0, ci0, M, N)
    r2 = cis[rps[2]:rps[3]]
    r2[r2 == 2] = max(c for c in range(N) if c not in r2)
    r2[:] = np.sort(r2)
    assert len(np.unique(r2)) == len(r2) and 2 not in r2
    D = P.Matrix(0, M, N, rps, cis, v0)
    assert D.status == 0
    assert refactor["s"](D.h, byref(f)) == NUMERICAL_ERROR and refactor["d"](D.h, byref(f)) == NUMERICAL_ERROR
    # sorted, full diagonal: the wrong type before the shape, then the shape
    rps, cis = _with_diagonal(rp0, ci0, M, N)
    W = P.Matrix(0, M, N, rps, cis, v0)
    assert W.status == 0
    for t in "scz":
        assert refactor[t](W.h, byref(f)) == WRONG_TYPE, t
    assert refactor["d"](W.h, byref(f)) == INVALID_SIZE
    assert refactor["d"](W.h, None) == INVALID_SIZE
    # m == 0: success at once, nothing touched (no device is needed for it)
    Z = P.Matrix(0, 0, 0, np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1))
    assert Z.status == 0
    assert refactor["d"](Z.h, byref(f)) == 0 and refactor["d"](Z.h, None) == 0
    assert refactor["s"](Z.h, byref(f)) == WRONG_TYPE
    assert f.value == 12345, "a refused call (and the empty matrix) leaves *precond_csr_val alone"
    for H in (U, D, W, Z):
        i = H.ilu_info()
        assert (i.factorized, i.levels, i.analyses, i.factorizations, i.schedule_bytes) == (0, 0, 0, 0, 0)


def test_get_ilu_info_checks_its_arguments_and_honours_a_short_struct_size():
    m, rp, ci, v = laplace5(3)
    A = P.Matrix(0, m, m, rp, ci, v)
    info = P.IluInfo(struct_size=ctypes.sizeof(P.IluInfo))
    assert L.aoclsparse_mi355_get_ilu_info(None, byref(info)) == INVALID_POINTER
    assert L.aoclsparse_mi355_get_ilu_info(A.h, None) == INVALID_POINTER
    info.struct_size = ctypes.sizeof(ctypes.c_size_t) - 1
    assert L.aoclsparse_mi355_get_ilu_info(A.h, byref(info)) == INVALID_SIZE
    # a caller that knows the struct up to `search` only: nothing behind it is written
    short = P.IluInfo.plans_kept_last.offset
    raw = (ctypes.c_ubyte * ctypes.sizeof(P.IluInfo))(*([0xAB] * ctypes.sizeof(P.IluInfo)))
    info = P.IluInfo.from_buffer(raw)
    info.struct_size = short
    assert L.aoclsparse_mi355_get_ilu_info(A.h, byref(info)) == 0
    assert info.struct_size == short
    assert (info.factorized, info.levels, info.max_row, info.syncfree, info.search) == (0, 0, 0, 0, 0)
    assert all(b == 0xAB for b in bytes(raw)[short:])
    full = A.ilu_info()
    assert full.struct_size == ctypes.sizeof(P.IluInfo) and full.factor_plan_builds == 0 and full.plans_kept_last == 0
