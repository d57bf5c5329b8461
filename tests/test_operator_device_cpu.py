"""CPU tier: what aoclsparse_mi355_build_operator_device / get_operator_info / export_operator (include/aoclsparse_mi355.h) decide
before the device is touched -- the statuses in their documented order, on handles that need no device; the info struct's
struct_size rule; export without an operator."""
import ctypes
from ctypes import byref

import numpy as np

from order_cases import Raw
from util import pkg

P = pkg()
L = P.lib()

SUCCESS, NOT_IMPLEMENTED, INVALID_POINTER, INVALID_SIZE, INVALID_VALUE = 0, 1, 2, 3, 5
assert [P.STATUS[k] for k in (1, 2, 3, 5)] == ["not_implemented", "invalid_pointer", "invalid_size", "invalid_value"]

i32 = lambda *a: np.array(a, np.int32)  # noqa: E731
build = L.aoclsparse_mi355_build_operator_device


def square(base=0, dtype=np.float64):
    """3 x 3, sorted rows, full diagonal"""
    A = P.Matrix(base, 3, 3, i32(0, 2, 4, 6) + base, i32(0, 1, 0, 1, 1, 2) + base, np.arange(1.0, 7.0).astype(dtype))
    assert A.status == 0
    return A


def poke_type(d, value):
    """a descriptor whose type no setter accepts: the first int of the struct"""
    ctypes.cast(d.h, ctypes.POINTER(ctypes.c_int))[0] = value


def test_statuses_in_order():
    A, sym, gen = square(), P.Descr(mtype=P.TYPE_SYMMETRIC), P.Descr()
    # 1. null handle or descriptor
    assert build(None, sym.h, P.OP_NONE) == INVALID_POINTER
    assert build(A.h, None, P.OP_NONE) == INVALID_POINTER
    # 2. base, type, operation -- before the descriptor's type is weighed
    assert build(A.h, P.Descr(base=1, mtype=P.TYPE_SYMMETRIC).h, P.OP_NONE) == INVALID_VALUE
    assert build(A.h, P.Descr(base=1).h, P.OP_NONE) == INVALID_VALUE  # (general comes later)
    assert build(A.h, sym.h, 999) == INVALID_VALUE and build(A.h, gen.h, 999) == INVALID_VALUE
    bad = P.Descr(mtype=P.TYPE_SYMMETRIC)
    poke_type(bad, 9)
    assert build(A.h, bad.h, P.OP_NONE) == INVALID_VALUE
    # 3. a general descriptor
    assert build(A.h, gen.h, P.OP_NONE) == NOT_IMPLEMENTED
    # 4. handles that are no plain CSR -- before Hermitian on a real type and before the shape
    w = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    others = [("coo", Raw("aoclsparse_create_dcoo", 0, 3, 3, 5, i32(0, 0, 1, 2, 2), i32(1, 0, 1, 2, 0), w.copy())),
              ("csc", Raw("aoclsparse_create_dcsc", 0, 3, 3, 5, i32(0, 2, 4, 5), i32(2, 0, 1, 0, 2), w.copy())),
              ("tcsr", P.TcsrMatrix(0, 3, i32(0, 1, 2, 4), i32(0, 1, 0, 2), np.array([1.0, 2.0, 5.0, 4.0]),
                                    i32(0, 2, 3, 4), i32(0, 1, 1, 2), np.array([1.0, 3.0, 2.0, 4.0]))),
              ("bsr", P.BsrMatrix(0, P.ORDER_ROW, 2, 2, 2, i32(0, 2, 3), i32(1, 0, 1), np.arange(12.0)))]
    for name, X in others:
        assert X.status == 0, name
        for mtype in (P.TYPE_SYMMETRIC, P.TYPE_HERMITIAN, P.TYPE_TRIANGULAR):
            assert build(X.h, P.Descr(mtype=mtype).h, P.OP_NONE) == NOT_IMPLEMENTED, (name, mtype)
        assert build(X.h, P.Descr(base=1, mtype=P.TYPE_SYMMETRIC).h, P.OP_NONE) == INVALID_VALUE, name
    # 5. Hermitian on a real value type -- before the shape
    rect = P.Matrix(0, 2, 3, i32(0, 1, 2), i32(0, 1), np.array([1.0, 2.0]))
    assert rect.status == 0
    for X in (A, square(dtype=np.float32), rect):
        assert build(X.h, P.Descr(mtype=P.TYPE_HERMITIAN).h, P.OP_NONE) == NOT_IMPLEMENTED
    # 6. symmetric on a matrix that is not square
    assert build(rect.h, sym.h, P.OP_NONE) == INVALID_SIZE
    # an empty matrix succeeds and builds nothing
    for m, n, rp in ((0, 0, i32(0)), (4, 4, i32(0, 0, 0, 0, 0)), (0, 3, i32(0))):
        E = P.Matrix(0, m, n, rp, i32(0), np.zeros(1))
        assert E.status == 0
        for d in (sym, P.Descr(mtype=P.TYPE_TRIANGULAR, fill=P.FILL_UPPER)):
            if d is sym and m != n:
                continue
            assert build(E.h, d.h, P.OP_TRANSPOSE) == SUCCESS
            assert E.operator_info(d, P.OP_TRANSPOSE).present == 0 and E.operator_info(d).device_builds == 0


def test_operator_info_struct_size():
    A, sym = square(), P.Descr(mtype=P.TYPE_SYMMETRIC)
    info = P.OperatorInfo(struct_size=ctypes.sizeof(P.OperatorInfo))
    get = L.aoclsparse_mi355_get_operator_info
    assert get(None, sym.h, P.OP_NONE, byref(info)) == INVALID_POINTER
    assert get(A.h, None, P.OP_NONE, byref(info)) == INVALID_POINTER
    assert get(A.h, sym.h, P.OP_NONE, None) == INVALID_POINTER
    assert get(A.h, P.Descr(base=1, mtype=P.TYPE_SYMMETRIC).h, P.OP_NONE, byref(info)) == INVALID_VALUE
    assert get(A.h, sym.h, 7, byref(info)) == INVALID_VALUE
    assert get(A.h, sym.h, P.OP_NONE, byref(info)) == SUCCESS
    assert (info.present, info.built_on_device, info.mapped, info.rows, info.cols, info.nnz) == (0, 0, 0, 0, 0, 0)
    assert (info.device_builds, info.host_builds, info.followed, info.dropped_by_value_change, info.map_bytes) == (0, 0, 0, 0, 0)
    # short: no more than struct_size bytes are written
    small = P.OperatorInfo(struct_size=ctypes.sizeof(ctypes.c_size_t) + 4, present=-3, built_on_device=-7, host_builds=-9)
    assert get(A.h, sym.h, P.OP_NONE, byref(small)) == SUCCESS
    assert (small.present, small.built_on_device, small.host_builds) == (0, -7, -9)
    small.struct_size = 2
    assert get(A.h, sym.h, P.OP_NONE, byref(small)) == INVALID_SIZE

    # long: a caller that knows a larger struct gets this library's part and nothing behind it
    class Longer(ctypes.Structure):
        _fields_ = [("info", P.OperatorInfo), ("tail", ctypes.c_longlong * 4)]

    big = Longer()
    big.info.struct_size = ctypes.sizeof(Longer)
    for k in range(4):
        big.tail[k] = -5
    assert get(A.h, sym.h, P.OP_NONE, byref(big)) == SUCCESS
    assert big.info.struct_size == ctypes.sizeof(Longer) and big.info.present == 0 and list(big.tail) == [-5] * 4


def test_export_without_an_operator():
    A, sym = square(), P.Descr(mtype=P.TYPE_SYMMETRIC)
    assert A.export_operator(sym)["status"] == INVALID_VALUE
    assert A.export_operator(P.Descr(mtype=P.TYPE_TRIANGULAR), P.OP_TRANSPOSE)["status"] == INVALID_VALUE
    r, c, k = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    p, q, v = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    ex = L.aoclsparse_mi355_export_operator
    assert ex(None, sym.h, P.OP_NONE, byref(r), byref(c), byref(k), byref(p), byref(q), byref(v)) == INVALID_POINTER
    assert ex(A.h, None, P.OP_NONE, byref(r), byref(c), byref(k), byref(p), byref(q), byref(v)) == INVALID_POINTER
    assert ex(A.h, sym.h, P.OP_NONE, None, byref(c), byref(k), byref(p), byref(q), byref(v)) == INVALID_POINTER
    assert ex(A.h, sym.h, 5, byref(r), byref(c), byref(k), byref(p), byref(q), byref(v)) == INVALID_VALUE
