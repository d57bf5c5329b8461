"""CPU tier of aoclsparse_mi355_?refresh_values_from_coo_device and aoclsparse_mi355_get_coo_map_info (new values for a CSR handle
that kept the map of its triplet sort): that the five names are declared, bound and exported, the flag's value, and everything
decided BEFORE the device is touched.  What a refresh does with values in HBM is tests/test_coo_refresh_gpu.py."""
import ctypes
import os
import re
import subprocess
from ctypes import byref, c_void_p

import numpy as np
import pytest

from util import ROOT, pkg

P = pkg()
L = P.lib()

SUCCESS, INVALID_POINTER, INVALID_SIZE, INVALID_VALUE = 0, 2, 3, 5
LETTERS = "sdcz"
DTYPE = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}
M, N = 12, 9
NAMES = ["aoclsparse_mi355_%srefresh_values_from_coo_device" % t for t in LETTERS] + ["aoclsparse_mi355_get_coo_map_info"]


def _coo(dtype=np.float64):
    rng = np.random.default_rng(3)
    nnz = 30
    return rng.integers(0, M, nnz).astype(np.int32), rng.integers(0, N, nnz).astype(np.int32), rng.uniform(-1, 1, nnz).astype(dtype)


def _host_handle():
    """a small aoclsparse_create_dcsr handle: it never held a triplet map"""
    rp = np.array([0, 2, 3, 5], np.int32)
    ci = np.array([0, 2, 1, 0, 2], np.int32)
    v = np.arange(1.0, 6.0)
    A = P.Matrix(0, 3, 3, rp, ci, v)
    assert A.status == 0
    return A


def test_the_five_names_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "aoclsparse_mi355.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", P.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for n in NAMES:
        assert re.search(r"DLL_PUBLIC\s+aoclsparse_status\s+%s\s*\(" % n, header), n
        assert n in P.SIGNATURES, n
        assert n in exported, n
        assert getattr(L, n).argtypes == P.SIGNATURES[n][1]
    for t in LETTERS:  # the argument list of ?update_values_device
        assert P.SIGNATURES["aoclsparse_mi355_%srefresh_values_from_coo_device" % t] == P.SIGNATURES["aoclsparse_mi355_%supdate_values_device" % t]
    assert callable(P.Matrix.refresh_from_coo_device) and callable(P.Matrix.coo_map_info)


def test_the_flag_is_16_here_and_in_the_header():
    assert P.COO_KEEP_MAP == 16 and (P.COO_KEEP, P.COO_SUM) == (0, 1)
    header = open(os.path.join(ROOT, "include", "aoclsparse_mi355.h")).read()
    m = re.search(r"aoclsparse_mi355_coo_keep_map\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == 16


def test_the_info_struct_matches_the_header():
    header = open(os.path.join(ROOT, "include", "aoclsparse_mi355.h")).read()
    body = re.search(r"typedef struct\s*\{([^}]*)\}\s*aoclsparse_mi355_coo_map_info;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip().split()[-1] for f in body.split(";") if f.strip()]
    assert fields == [f[0] for f in P.CooMapInfo._fields_] == ["struct_size", "kept", "mode", "triplets", "entries", "map_bytes"]
    assert ctypes.sizeof(P.CooMapInfo) == 32 and P.CooMapInfo.map_bytes.offset == 24


@pytest.mark.parametrize("t", LETTERS)
@pytest.mark.parametrize("dup", [15, 18, 32, 2, -1, 7])
def test_duplicates_other_than_0_1_16_17(t, dup):
    r, c, v = _coo(DTYPE[t])
    fn = getattr(L, "aoclsparse_mi355_create_%scsr_from_coo_device" % t)
    h = c_void_p(1)
    assert fn(byref(h), 0, M, N, len(v), P._ptr(r), P._ptr(c), P._ptr(v), dup) == INVALID_VALUE
    assert not h.value, "*mat is cleared"
    # ... behind the sizes and the null arrays, as before
    h = c_void_p(1)
    assert fn(byref(h), 0, -1, N, len(v), P._ptr(r), P._ptr(c), P._ptr(v), dup) == INVALID_SIZE
    assert not h.value
    h = c_void_p(1)
    assert fn(byref(h), 0, M, N, len(v), P._ptr(r), None, P._ptr(v), dup) == INVALID_POINTER
    assert not h.value


@pytest.mark.parametrize("t", LETTERS)
def test_refresh_null_pointers(t):
    fn = getattr(L, "aoclsparse_mi355_%srefresh_values_from_coo_device" % t)
    v = np.ones(5, DTYPE[t])
    A = _host_handle()
    assert fn(None, 5, P._ptr(v)) == INVALID_POINTER
    assert fn(A.h, 5, None) == INVALID_POINTER
    assert fn(None, 5, None) == INVALID_POINTER


@pytest.mark.parametrize("t", LETTERS)
@pytest.mark.parametrize("length", [5, 4, 0, -1])
def test_refresh_of_a_handle_without_a_map_is_invalid_value_before_size_and_type(t, length):
    """a double handle of 5 entries: neither a wrong len nor a wrong value type gets its say"""
    fn = getattr(L, "aoclsparse_mi355_%srefresh_values_from_coo_device" % t)
    v = np.ones(5, DTYPE[t])
    A = _host_handle()
    assert fn(A.h, length, P._ptr(v)) == INVALID_VALUE
    assert A.export()["val"].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]


def test_map_info_of_a_handle_without_a_map():
    A = _host_handle()
    info = A.coo_map_info()
    assert (info.kept, info.mode, info.triplets, info.entries, info.map_bytes) == (0, 0, 0, 0, 0)
    assert info.struct_size == ctypes.sizeof(P.CooMapInfo)
    assert L.aoclsparse_mi355_get_coo_map_info(None, byref(info)) == INVALID_POINTER
    assert L.aoclsparse_mi355_get_coo_map_info(A.h, None) == INVALID_POINTER


@pytest.mark.parametrize("size", [8, 12, 16, 24, 32, 64])
def test_map_info_writes_no_more_than_struct_size(size):
    """the struct and a canary behind it, all bytes 0xA5: what lies past struct_size stays as it was"""
    full = ctypes.sizeof(P.CooMapInfo)
    buf = (ctypes.c_ubyte * (full + 32))(*([0xA5] * (full + 32)))
    info = P.CooMapInfo.from_buffer(buf)
    info.struct_size = size
    A = _host_handle()
    assert L.aoclsparse_mi355_get_coo_map_info(A.h, byref(info)) == SUCCESS
    raw = bytes(buf)
    written = min(size, full)
    assert raw[written:] == b"\xa5" * (full + 32 - written), "written past struct_size"
    assert info.struct_size == size
    assert raw[8:written] == b"\x00" * (written - 8)  # kept = 0 and zeros, as far as the caller's struct goes


def test_map_info_struct_size_too_small_for_itself():
    info = P.CooMapInfo(struct_size=4)
    assert L.aoclsparse_mi355_get_coo_map_info(_host_handle().h, byref(info)) == INVALID_SIZE
