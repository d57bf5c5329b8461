"""CPU tier of aoclsparse_mi355_get_sell_keep_info (what a handle's SELL-64 copy keeps through aoclsparse_mi355_?revalue_device):
that the name is declared, bound and exported, the struct, the statuses, the struct_size protocol, and the zeros of handles that
hold no copy.  What the kept structure does on the device is tests/test_sell_revalue_gpu.py."""
import ctypes
import os
import re
import subprocess
from ctypes import byref

import numpy as np
import pytest

from util import ROOT, pkg

P = pkg()
L = P.lib()

SUCCESS, INVALID_POINTER, INVALID_SIZE = 0, 2, 3
assert [P.STATUS[k] for k in (2, 3)] == ["invalid_pointer", "invalid_size"]
NAME = "aoclsparse_mi355_get_sell_keep_info"
FIELDS = ["struct_size", "kept", "valid", "last_route", "reserved", "structure_builds", "value_fills", "searches_skipped", "kept_bytes"]
OPS = (P.OP_NONE, P.OP_TRANSPOSE, P.OP_CONJ_TRANSPOSE)


def _host_handle():
    rp = np.array([0, 2, 3, 5], np.int32)
    ci = np.array([0, 2, 1, 0, 2], np.int32)
    A = P.Matrix(0, 3, 3, rp, ci, np.arange(1.0, 6.0))
    assert A.status == 0
    return A


def _zeros(info):
    return all(getattr(info, f) == 0 for f in FIELDS[1:])


def test_the_name_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "aoclsparse_mi355.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", P.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert re.search(r"DLL_PUBLIC\s+aoclsparse_status\s+%s\s*\(" % NAME, header)
    assert NAME in P.SIGNATURES and NAME in exported
    assert getattr(L, NAME).argtypes == P.SIGNATURES[NAME][1]
    assert callable(P.Matrix.sell_keep_info)


def test_the_info_struct_matches_the_header():
    header = open(os.path.join(ROOT, "include", "aoclsparse_mi355.h")).read()
    body = re.search(r"typedef struct\s*\{([^}]*)\}\s*aoclsparse_mi355_sell_keep_info;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip().split()[-1] for f in body.split(";") if f.strip()]
    assert fields == [f[0] for f in P.SellKeepInfo._fields_] == FIELDS
    assert ctypes.sizeof(P.SellKeepInfo) == 56 and P.SellKeepInfo.structure_builds.offset == 24
    assert P.SellKeepInfo.kept_bytes.offset == 48


def test_statuses():
    A = _host_handle()
    info = P.SellKeepInfo(struct_size=ctypes.sizeof(P.SellKeepInfo))
    assert L.aoclsparse_mi355_get_sell_keep_info(None, P.OP_NONE, byref(info)) == INVALID_POINTER
    assert L.aoclsparse_mi355_get_sell_keep_info(A.h, P.OP_NONE, None) == INVALID_POINTER
    assert L.aoclsparse_mi355_get_sell_keep_info(None, P.OP_NONE, None) == INVALID_POINTER
    for size in (0, 4, 7):
        small = P.SellKeepInfo(struct_size=size)
        assert L.aoclsparse_mi355_get_sell_keep_info(A.h, P.OP_NONE, byref(small)) == INVALID_SIZE
    # (a null handle is reported before a struct that is too small)
    assert L.aoclsparse_mi355_get_sell_keep_info(None, P.OP_NONE, byref(P.SellKeepInfo(struct_size=2))) == INVALID_POINTER


@pytest.mark.parametrize("op", OPS)
def test_zeros_on_a_fresh_handle(op):
    """also after aoclsparse_optimize with an mv hint: without a GPU no copy is built, and with one a 3 x 3 handle gets a copy
    only for op = none (everything else reports zeros by definition)"""
    A = _host_handle()
    info = A.sell_keep_info(op)
    assert _zeros(info) and info.struct_size == ctypes.sizeof(P.SellKeepInfo)
    if op != P.OP_NONE:
        d = P.Descr()
        assert L.aoclsparse_set_mv_hint(A.h, op, d.h, 10) == 0 and L.aoclsparse_optimize(A.h) == 0
        assert _zeros(A.sell_keep_info(op))


def test_zeros_on_tcsr_and_bsr_handles():
    i32 = lambda *a: np.array(a, np.int32)  # noqa: E731
    T = P.TcsrMatrix(0, 3, i32(0, 1, 2, 4), i32(0, 1, 0, 2), np.array([1.0, 2.0, 5.0, 4.0]),
                     i32(0, 2, 3, 4), i32(0, 1, 1, 2), np.array([1.0, 3.0, 2.0, 4.0]))
    B = P.BsrMatrix(0, P.ORDER_ROW, 2, 2, 2, i32(0, 2, 3), i32(1, 0, 1), np.arange(12.0))
    for X in (T, B):
        assert X.status == 0
        for op in OPS:
            info = P.SellKeepInfo(struct_size=ctypes.sizeof(P.SellKeepInfo))
            assert L.aoclsparse_mi355_get_sell_keep_info(X.h, op, byref(info)) == SUCCESS
            assert _zeros(info)


@pytest.mark.parametrize("size", [8, 12, 16, 24, 32, 40, 56, 64, 96])
def test_no_more_than_struct_size_is_written(size):
    """the struct and a canary behind it, all bytes 0xA5: what lies past struct_size stays as it was"""
    full = ctypes.sizeof(P.SellKeepInfo)
    buf = (ctypes.c_ubyte * (full + 48))(*([0xA5] * (full + 48)))
    info = P.SellKeepInfo.from_buffer(buf)
    info.struct_size = size
    A = _host_handle()
    assert L.aoclsparse_mi355_get_sell_keep_info(A.h, P.OP_NONE, byref(info)) == SUCCESS
    raw = bytes(buf)
    written = min(size, full)
    assert raw[written:] == b"\xa5" * (full + 48 - written), "written past struct_size"
    assert info.struct_size == size
    assert raw[8:written] == b"\x00" * (written - 8)  # zeros, as far as the caller's struct goes


def test_a_short_struct_keeps_the_fields_behind_its_size():
    A = _host_handle()
    small = P.SellKeepInfo(struct_size=ctypes.sizeof(ctypes.c_size_t) + 8, kept=-3, valid=-4, last_route=-5, structure_builds=-6,
                           kept_bytes=-7)
    assert L.aoclsparse_mi355_get_sell_keep_info(A.h, P.OP_NONE, byref(small)) == SUCCESS
    assert (small.kept, small.valid) == (0, 0)
    assert (small.last_route, small.structure_builds, small.kept_bytes) == (-5, -6, -7)
