"""CPU tier of aoclsparse_mi355_sp2m_numeric_device / aoclsparse_mi355_get_sp2m_plan_info: the symbols, every status that is
decided before the device is touched, in the documented order, and the observer's argument checks (no device needed)."""
import ctypes
import os
import re
import subprocess
from ctypes import byref, c_void_p

import numpy as np

from test_sy_dense_cpu import Handle, bsr, tcsr
from util import ROOT, pkg

P = pkg()
L = P.lib()
NOT_IMPLEMENTED, INVALID_POINTER, INVALID_SIZE, INVALID_VALUE, WRONG_TYPE = 1, 2, 3, 5, 9
assert [P.STATUS[k] for k in (1, 2, 3, 5, 9)] == ["not_implemented", "invalid_pointer", "invalid_size", "invalid_value", "wrong_type"]
N, T, H = P.OP_NONE, P.OP_TRANSPOSE, P.OP_CONJ_TRANSPOSE
NAMES = ["aoclsparse_mi355_sp2m_numeric_device", "aoclsparse_mi355_get_sp2m_plan_info"]
numeric = L.aoclsparse_mi355_sp2m_numeric_device


def dense_handle(m, n, dt=np.float64, base=0):
    """every entry stored, rows ascending"""
    ptr = np.arange(m + 1, dtype=np.int32) * n + base
    ind = np.tile(np.arange(n, dtype=np.int32), m) + base
    return Handle(base, m, n, ptr, ind, (1.0 + np.arange(m * n)).astype(dt))


def plan_info(h):
    info = P.Sp2mPlanInfo(struct_size=ctypes.sizeof(P.Sp2mPlanInfo))
    assert L.aoclsparse_mi355_get_sp2m_plan_info(h, byref(info)) == 0
    return info


def test_symbols_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "aoclsparse_mi355.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", P.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NAMES:
        assert re.search(r"DLL_PUBLIC\s+aoclsparse_status\s+%s\s*\(" % name, src), name
        assert name in exported, name
        assert name in P.SIGNATURES and getattr(L, name).argtypes is not None, name
    assert "(round 29)" in src and "aoclsparse_mi355_sp2m_plan_info;" in src
    assert callable(P.Matrix.sp2m_plan_info)


def test_early_statuses_in_the_documented_order():
    """Each call provokes one status together with every status that comes AFTER it in the order, so the order itself is pinned:
    the checks of a finalize call (each with a null C on top), the null C, both operations transposing, the format of C, its value
    type, its dimensions, C among the operands."""
    d0, d1 = P.Descr(base=0), P.Descr(base=1)
    A, B = dense_handle(3, 4), dense_handle(4, 2)  # the product is 3 x 2
    Az = dense_handle(3, 4, np.complex128)
    C = dense_handle(3, 2)
    # 1. what sp2m_checks returns for stage_finalize, in its order; C is null throughout, which must not be noticed yet
    assert numeric(N, None, A.h, N, d0.h, B.h, None) == INVALID_POINTER
    assert numeric(N, d0.h, None, N, d0.h, B.h, None) == INVALID_POINTER
    coo = c_void_p()
    rid = np.repeat(np.arange(3, dtype=np.int32), 4)
    assert L.aoclsparse_create_dcoo(byref(coo), 0, 3, 4, 12, P._ptr(rid), P._ptr(A.ind), P._ptr(A.val)) == 0
    assert numeric(N, d0.h, coo, N, d0.h, B.h, None) == NOT_IMPLEMENTED  # the operand's format before its type
    assert numeric(N, d0.h, A.h, N, d0.h, Az.h, None) == WRONG_TYPE  # B's type is not A's
    assert numeric(N, d1.h, A.h, N, d0.h, B.h, None) == INVALID_VALUE  # the descriptor's base is not the handle's
    sym = P.Descr(base=0, mtype=P.TYPE_SYMMETRIC)
    assert numeric(N, sym.h, A.h, N, d0.h, B.h, None) == NOT_IMPLEMENTED
    assert numeric(7, d0.h, A.h, N, d0.h, B.h, None) == INVALID_VALUE  # no operation
    assert numeric(T, d0.h, A.h, T, d0.h, B.h, None) == INVALID_SIZE  # A^T B^T: 4 x 3 times 2 x 4 -- before "both transpose"
    # ... and its empty-product quick return succeeds and does nothing, whatever C is
    E = Handle(0, 3, 4, np.zeros(4, np.int32), np.zeros(1, np.int32), np.zeros(1))
    before = C.val.copy()
    assert numeric(N, d0.h, E.h, N, d0.h, B.h, C.h) == 0 and numeric(N, d0.h, E.h, N, d0.h, B.h, None) == 0
    assert numeric(N, d0.h, E.h, N, d0.h, B.h, A.h) == 0  # (not even its dimensions are looked at)
    assert np.array_equal(C.val, before)
    # 2. a null C, with everything that follows wrong as well
    S, R = dense_handle(4, 4), dense_handle(4, 4)
    assert numeric(T, d0.h, S.h, T, d0.h, R.h, None) == INVALID_POINTER
    # 3. both operations transpose: before the format, the type, the dimensions and the identity of C
    for opa, opb in ((T, T), (T, H), (H, H)):
        assert numeric(opa, d0.h, S.h, opb, d0.h, R.h, coo) == NOT_IMPLEMENTED
        assert numeric(opa, d0.h, S.h, opb, d0.h, R.h, S.h) == NOT_IMPLEMENTED
    # 4. a C that is no plain CSR handle, of the wrong type and the wrong dimensions
    Cz43 = dense_handle(4, 3, np.complex128)
    csc = Handle(0, 4, 3, np.arange(4, dtype=np.int32) * 4, np.tile(np.arange(4, dtype=np.int32), 3), Cz43.val, csc=True)
    TC, BS = tcsr(np.complex128), bsr(np.complex128)
    ccoo = c_void_p()
    assert L.aoclsparse_create_zcoo(byref(ccoo), 0, 3, 4, 12, P._ptr(rid), P._ptr(A.ind), P._ptr(Az.val)) == 0
    for bad in (ccoo, csc.h, TC.h, BS.h):
        assert numeric(N, d0.h, A.h, N, d0.h, B.h, bad) == NOT_IMPLEMENTED
    # 5. a CSR handle of another value type, and of other dimensions
    assert numeric(N, d0.h, A.h, N, d0.h, B.h, Cz43.h) == WRONG_TYPE
    Bz = dense_handle(4, 2, np.complex128)
    assert numeric(N, d0.h, Az.h, N, d0.h, Bz.h, C.h) == WRONG_TYPE
    # 6. the dimensions, for every way an operation changes them; C among the operands on top
    C23, C24, C42 = dense_handle(2, 3), dense_handle(2, 4), dense_handle(4, 2)
    assert numeric(N, d0.h, A.h, N, d0.h, B.h, C23.h) == INVALID_SIZE
    assert numeric(N, d0.h, A.h, N, d0.h, B.h, A.h) == INVALID_SIZE
    assert numeric(T, d0.h, S.h, N, d0.h, C42.h, C24.h) == INVALID_SIZE  # 4 x 2, not 2 x 4
    assert numeric(N, d0.h, C24.h, T, d0.h, S.h, C42.h) == INVALID_SIZE  # 2 x 4, not 4 x 2
    # 7. C is A or B (square operands: the dimensions are right)
    assert numeric(N, d0.h, S.h, N, d0.h, R.h, S.h) == INVALID_VALUE
    assert numeric(N, d0.h, S.h, N, d0.h, R.h, R.h) == INVALID_VALUE
    assert numeric(T, d0.h, S.h, N, d0.h, S.h, S.h) == INVALID_VALUE
    # nothing above counted as a run or a refusal, and no plan was built
    for h in (C.h, S.h, R.h, A.h):
        i = plan_info(h)
        assert (i.kept, i.heavy_rows, list(i.rows_in_bin), i.plan_builds, i.numeric_runs, i.refused, i.plan_bytes) == (
            0, 0, [0] * 5, 0, 0, 0, 0)
    L.aoclsparse_destroy(byref(coo))
    L.aoclsparse_destroy(byref(ccoo))


def test_get_sp2m_plan_info_checks_its_arguments_and_honours_a_short_struct_size():
    A = dense_handle(3, 3)
    info = P.Sp2mPlanInfo(struct_size=ctypes.sizeof(P.Sp2mPlanInfo))
    assert L.aoclsparse_mi355_get_sp2m_plan_info(None, byref(info)) == INVALID_POINTER
    assert L.aoclsparse_mi355_get_sp2m_plan_info(A.h, None) == INVALID_POINTER
    info.struct_size = ctypes.sizeof(ctypes.c_size_t) - 1
    assert L.aoclsparse_mi355_get_sp2m_plan_info(A.h, byref(info)) == INVALID_SIZE
    # a caller that knows the struct up to `rows_in_bin` only: nothing behind it is written
    short = P.Sp2mPlanInfo.plan_builds.offset
    raw = (ctypes.c_ubyte * ctypes.sizeof(P.Sp2mPlanInfo))(*([0xAB] * ctypes.sizeof(P.Sp2mPlanInfo)))
    info = P.Sp2mPlanInfo.from_buffer(raw)
    info.struct_size = short
    assert L.aoclsparse_mi355_get_sp2m_plan_info(A.h, byref(info)) == 0
    assert info.struct_size == short
    assert (info.kept, info.heavy_rows, list(info.rows_in_bin)) == (0, 0, [0] * 5)
    assert all(b == 0xAB for b in bytes(raw)[short:])
    # a fresh handle reports zeros, through the helper of the Python binding too
    m = 3
    M = P.Matrix(0, m, m, A.ptr, A.ind, A.val)
    full = M.sp2m_plan_info()
    assert full.struct_size == ctypes.sizeof(P.Sp2mPlanInfo)
    assert (full.kept, full.heavy_rows, list(full.rows_in_bin), full.plan_builds, full.numeric_runs, full.refused, full.plan_bytes) == (
        0, 0, [0] * 5, 0, 0, 0, 0)
