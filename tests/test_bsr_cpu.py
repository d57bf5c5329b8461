"""BSR handles without a GPU: creator statuses (create/aoclsparse_create.cpp:116-190 of the reference), aoclsparse_convert_bsr against
the oracle's csr2bsr (conversion/aoclsparse_convert.cpp:1218-1476), what every other entry point answers for such a handle, the
product statuses that are decided before the device is touched, the aliasing contract and the reference's known answers."""
import json
import os
import subprocess
from ctypes import byref, c_int, c_int32, c_void_p

import numpy as np
import pytest

import oracle
from util import ROOT, pkg, random_csr

P = pkg()
L = P.lib()
ST = {v: k for k, v in P.STATUS.items()}
TYPES = (("s", np.float32), ("d", np.float64), ("c", np.complex64), ("z", np.complex128))


def bsr_arrays(base=0, dtype=np.float64, dim=2):
    """2 x 2 blocks of dim x dim: block row 0 holds block columns {0, 1}, block row 1 holds {1}"""
    rp = np.array([0, 2, 3], np.int32) + base
    ci = np.array([0, 1, 1], np.int32) + base
    v = (np.arange(3 * dim * dim) + 1.0).astype(dtype)
    return 2, 2, dim, rp, ci, v


def create(t, base, order, bm, bn, dim, rp, ci, v, mat=True, fast=False):
    h = c_void_p(0xdead)
    st = getattr(L, "aoclsparse_create_%sbsr" % t)(byref(h) if mat else None, base, order, bm, bn, dim, P._ptr(rp), P._ptr(ci), P._ptr(v), fast)
    if st == 0:
        L.aoclsparse_destroy(byref(h))
    else:
        assert not mat or rp is None or not h.value, "*mat is NULL after every failure (create.cpp:131)"
    return P.STATUS[st]


@pytest.mark.parametrize("t,dt", TYPES, ids=[t for t, _ in TYPES])
@pytest.mark.parametrize("base", [0, 1])
def test_creator_statuses_in_the_reference_order(t, dt, base):
    bm, bn, dim, rp, ci, v = bsr_arrays(base, dt)
    ok = dict(t=t, base=base, order=P.ORDER_COLUMN, bm=bm, bn=bn, dim=dim, rp=rp, ci=ci, v=v)
    assert create(**ok) == "success"
    assert create(**{**ok, "order": P.ORDER_ROW}) == "success"
    assert create(**{**ok, "order": 7}) == "success"  # the block order is stored unchecked (create.cpp:163-173)
    # 1. mat or row_ptr null, before anything else is looked at (:129-130)
    assert create(**{**ok, "dim": 0, "bm": -1}, mat=False) == "invalid_pointer"
    h = c_void_p(0xdead)
    assert getattr(L, "aoclsparse_create_%sbsr" % t)(byref(h), base, 1, -1, bn, 0, None, P._ptr(ci), P._ptr(v), False) == ST["invalid_pointer"]
    # 2. the block size (:132-133), before the sizes
    assert create(**{**ok, "dim": 0, "bm": -1}) == "invalid_value"
    assert create(**{**ok, "dim": -3}) == "invalid_value"
    # 3. bM (:134-135)
    assert create(**{**ok, "bm": -1}) == "invalid_size"
    # 4. the matrix check on the block pattern (:143-158 -> analysis/aoclsparse_csr_util.cpp:142-260)
    assert create(**{**ok, "ci": None}) == "invalid_pointer"
    assert create(**{**ok, "v": None}) == "invalid_pointer"
    assert create(**{**ok, "bn": -1}) == "invalid_size"
    bad = ci.copy()
    bad[1] = base + bn  # a block column at bN
    assert create(**{**ok, "ci": bad}) == "invalid_index_value"
    bad[1] = base + bn + 5
    assert create(**{**ok, "ci": bad}) == "invalid_index_value"
    bad[1] = base - 1
    assert create(**{**ok, "ci": bad}) == "invalid_index_value"
    dec = np.array([0, 3, 2, 3], np.int32) + base  # decreasing row_ptr, right ends
    assert create(**{**ok, "bm": 3, "rp": dec}) == "invalid_value"
    off = rp.copy()
    off[0] += 1  # row_ptr[0] != base
    assert create(**{**ok, "rp": off}) == "invalid_value"
    neg = rp.copy()
    neg[bm] = base - 1  # bnnz < 0
    assert create(**{**ok, "rp": neg}) == "invalid_size"
    # bM = 0: an empty handle
    assert create(**{**ok, "bm": 0, "rp": np.array([base], np.int32)}) == "success"
    assert create(**{**ok, "bm": 0, "bn": 0, "rp": np.array([base], np.int32)}) == "success"
    # fast_chck: pointers, sizes and the two ends of row_ptr only (csr_util.cpp:142-188)
    assert create(**{**ok, "ci": bad}, fast=True) == "success"
    assert create(**{**ok, "rp": off}, fast=True) == "invalid_value"
    assert create(**{**ok, "ci": None}, fast=True) == "invalid_pointer"


@pytest.mark.parametrize("base", [0, 1])
def test_handle_reports_the_scalar_dimensions_and_the_block_pattern(base):
    bm, bn, dim = 3, 4, 3
    rp = np.array([0, 2, 2, 4], np.int32) + base
    ci = np.array([3, 1, 0, 2], np.int32) + base  # block row 0 unsorted
    v = np.arange(4 * 9, dtype=np.float64)
    A = P.BsrMatrix(base, P.ORDER_ROW, bm, bn, dim, rp, ci, v)
    assert A.status == 0
    e = A.export_bsr()
    assert (e["base"], e["order"], e["bm"], e["bn"], e["block_dim"], e["is_internal"]) == (base, P.ORDER_ROW, bm, bn, dim, 0)
    for got, mine in ((e["row_ptr"], A.row_ptr), (e["col_ind"], A.col_ind), (e["val"], A.val)):
        assert got.ctypes.data == mine.ctypes.data  # aliased, not copied
    # m = bM * block_dim, n = bN * block_dim, nnz = bnnz * block_dim^2 (create.cpp:183-184), seen through the argument checks
    assert L.aoclsparse_dupdate_values(A.h, 4 * 9 + 1, P._ptr(np.ones(40))) == ST["invalid_size"]
    assert L.aoclsparse_dupdate_values(A.h, 4 * 9, P._ptr(np.ones(40))) == ST["not_implemented"]
    assert L.aoclsparse_dset_value(A.h, base + bm * dim, base, 1.0) == ST["invalid_value"]
    assert L.aoclsparse_dset_value(A.h, base, base + bn * dim, 1.0) == ST["invalid_value"]
    assert L.aoclsparse_dset_value(A.h, base + bm * dim - 1, base + bn * dim - 1, 1.0) == ST["not_implemented"]
    info = A.spmv_info()
    assert info.kernel == 0 and info.device_resident == 0  # row-major blocks have no kernel; nothing uploaded
    h = c_void_p()
    assert L.aoclsparse_mi355_export_bsr(P.Matrix(0, 1, 1, [0, 1], [0], [1.0]).h, *[byref(c_int()) for _ in range(2)],
                                         *[byref(c_int32()) for _ in range(3)], byref(h), byref(h), byref(h), None) == ST["invalid_value"]


def test_all_six_names_and_default_visibility():
    vis = subprocess.run(["readelf", "--dyn-syms", "-W", P.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = ["aoclsparse_create_%sbsr" % t for t in "sdcz"] + ["aoclsparse_convert_bsr", "aoclsparse_mi355_export_bsr"]
    for name in names:
        rows = [r for r in vis.splitlines() if r.split() and r.split()[-1].split("@")[0] == name]
        assert rows and all("DEFAULT" in r and "GLOBAL" in r and "FUNC" in r for r in rows), name
    for t, dt in TYPES:
        bm, bn, dim, rp, ci, v = bsr_arrays(0, dt)
        A = P.BsrMatrix(0, P.ORDER_COLUMN, bm, bn, dim, rp, ci, v)
        assert A.status == 0, t
        A.destroy()


def test_create_and_destroy_leave_the_callers_arrays_alone():
    """(under tests/run_san.sh a free or a write of an aliased array is a report)"""
    for base in (0, 1):
        for t, dt in TYPES:
            bm, bn, dim, rp, ci, v = bsr_arrays(base, dt, 3)
            keep = [a.tobytes() for a in (rp, ci, v)]
            A = P.BsrMatrix(base, P.ORDER_COLUMN, bm, bn, dim, rp, ci, v)
            assert A.status == 0
            for a, b in zip((A.row_ptr, A.col_ind, A.val), (rp, ci, v)):
                assert a.ctypes.data == b.ctypes.data
            assert L.aoclsparse_set_mv_hint(A.h, P.OP_NONE, P.Descr(base=base).h, 5) == 0
            assert L.aoclsparse_mi355_invalidate(A.h) == 0
            A.destroy()
            assert not A.h
            for a, k in zip((rp, ci, v), keep):
                assert a.tobytes() == k
                a[:] = a  # still writable memory of ours


# ---- aoclsparse_convert_bsr -------------------------------------------------------------------------------------------------
def _sources():
    out = {}
    out["sorted"] = (12, 12) + random_csr(11, 12, 12, lambda r, i: 1 + i % 4)
    out["unsorted"] = (10, 13) + random_csr(12, 10, 13, lambda r, i: 2 + i % 5, sort=False)
    out["rectangular"] = (7, 11) + random_csr(13, 7, 11, lambda r, i: 1 + (3 * i) % 5)
    out["empty_row"] = (9, 8) + random_csr(14, 9, 8, lambda r, i: 0 if i in (0, 4, 8) else 3)
    out["empty"] = (6, 5, np.zeros(7, np.int32), np.zeros(1, np.int32), np.zeros(1))
    return out


SOURCES = _sources()


def _transpose(m, n, rp, ci, v, conj):
    """CSR of A^T (A^H) built in numpy: 0-based in, 0-based out, rows sorted by the source row"""
    rows = np.repeat(np.arange(m), np.diff(rp))
    order = np.lexsort((rows, ci))
    tp = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=n))]).astype(np.int32)
    tv = v[order]
    return tp, rows[order].astype(np.int32), (np.conj(tv) if conj else tv)


def _oracle_bsr(m, n, base, rp, ci, v, dim, rowmajor):
    """oracle.csr2bsr is a double routine; the fill only moves values, so a complex matrix is its real and its imaginary part"""
    bp, bi, br = oracle.csr2bsr(m, n, base, rp, ci, np.ascontiguousarray(v.real, np.float64), dim, rowmajor)
    if np.iscomplexobj(v):
        bp2, bi2, bim = oracle.csr2bsr(m, n, base, rp, ci, np.ascontiguousarray(v.imag, np.float64), dim, rowmajor)
        assert np.array_equal(bp, bp2) and np.array_equal(bi, bi2)
        br = br + 1j * bim
    return bp, bi, br


@pytest.mark.parametrize("dt", [np.float64, np.float32, np.complex128, np.complex64], ids=["d", "s", "z", "c"])
@pytest.mark.parametrize("src", sorted(SOURCES))
def test_convert_bsr_equals_the_oracle(src, dt):
    m, n, rp0, ci0, v0 = SOURCES[src]
    nnz = int(rp0[m])
    rng = np.random.default_rng(5)
    v0 = v0[:max(nnz, 1)].astype(dt)
    if np.issubdtype(dt, np.complexfloating):
        v0 = (v0 + 1j * rng.uniform(-1, 1, len(v0))).astype(dt)
    create = {np.float64: L.aoclsparse_create_dcsr, np.float32: L.aoclsparse_create_scsr, np.complex128: L.aoclsparse_create_zcsr,
              np.complex64: L.aoclsparse_create_ccsr}[dt]
    for base in (0, 1):
        rp, ci, v = (rp0 + base).astype(np.int32), (ci0 + base).astype(np.int32), v0.copy()
        keep = [a.tobytes() for a in (rp, ci, v)]
        h = c_void_p()
        assert create(byref(h), base, m, n, nnz, P._ptr(rp), P._ptr(ci), P._ptr(v)) == 0
        for op in (P.OP_NONE, P.OP_TRANSPOSE, P.OP_CONJ_TRANSPOSE):
            if op == P.OP_NONE:
                om, on, orp, oci, ov = m, n, rp0[:m + 1], ci0[:nnz], v0[:nnz]
            else:
                orp, oci, ov = _transpose(m, n, rp0[:m + 1], ci0[:nnz], v0[:nnz], op == P.OP_CONJ_TRANSPOSE)
                om, on = n, m
            for dim in (1, 2, 3, 4, 5):
                for order in (P.ORDER_ROW, P.ORDER_COLUMN):
                    what = (src, base, op, dim, order)
                    d = c_void_p(0xdead)
                    assert L.aoclsparse_convert_bsr(h, dim, order, op, byref(d)) == 0, what
                    B = P.BsrMatrix.from_handle(d, dt)
                    e = B.export_bsr(dt)
                    mb, nb = (om + dim - 1) // dim, (on + dim - 1) // dim
                    bp, bi, bv = _oracle_bsr(om, on, base, (orp + base).astype(np.int32), (oci + base).astype(np.int32), ov, dim,
                                             order == P.ORDER_ROW)
                    assert (e["base"], e["order"], e["bm"], e["bn"], e["block_dim"], e["is_internal"]) == (base, order, mb, nb, dim, 1), what
                    assert np.array_equal(e["row_ptr"], bp) and np.array_equal(e["col_ind"], bi), what
                    assert e["val"].dtype == dt and np.array_equal(e["val"], bv.astype(dt)), what
                    # the padded dimensions (convert.cpp:1419-1423), seen through the argument checks of the setter
                    setv = {np.float64: (L.aoclsparse_dset_value, 1.0), np.float32: (L.aoclsparse_sset_value, 1.0)}.get(dt)
                    if setv:
                        assert setv[0](d, base + mb * dim - 1, base + nb * dim - 1, setv[1]) == ST["not_implemented"], what
                        assert setv[0](d, base + mb * dim, base, setv[1]) == ST["invalid_value"], what
                        assert setv[0](d, base, base + nb * dim, setv[1]) == ST["invalid_value"], what
                    B.destroy()
        for a, k in zip((rp, ci, v), keep):
            assert a.tobytes() == k  # the source is left untouched
        L.aoclsparse_destroy(byref(h))


def test_convert_bsr_error_statuses():
    """conversion/aoclsparse_convert.cpp:1431-1454 in their order, then :1227-1232"""
    A = P.Matrix(0, 2, 2, [0, 1, 2], [0, 1], [1.0, 2.0])
    d = c_void_p(0xdead)
    cv = L.aoclsparse_convert_bsr
    assert cv(None, 0, 7, 5, byref(d)) == ST["invalid_pointer"]  # :1437-1438
    assert cv(A.h, 0, 7, 5, None) == ST["invalid_pointer"]
    assert cv(A.h, 0, 7, 5, byref(d)) == ST["invalid_value"]  # :1440-1441 block_dim, before the order
    assert cv(A.h, -2, P.ORDER_ROW, P.OP_NONE, byref(d)) == ST["invalid_value"]
    assert cv(A.h, 2, 7, 5, byref(d)) == ST["invalid_value"]  # :1443-1444 block order, before the operation
    assert cv(A.h, 2, P.ORDER_ROW, 5, byref(d)) == ST["not_implemented"]  # :1446-1448
    assert d.value == 0xdead  # *dest is written only from :1450 on
    # :1453-1454: only a handle created from CSR arrays
    m, pl, cl, vl, pu, cu, vu = 2, *(np.array(a) for a in ([0, 1, 3], [0, 0, 1], [1.0, 2.0, 3.0], [0, 2, 3], [0, 1, 1], [1.0, 4.0, 3.0]))
    T = P.TcsrMatrix(0, m, pl, cl, vl, pu, cu, vu)
    assert T.status == 0
    assert cv(T.h, 2, P.ORDER_ROW, P.OP_NONE, byref(d)) == ST["not_implemented"] and not d.value
    coo = c_void_p()
    r, c, v = np.array([0, 1], np.int32), np.array([0, 1], np.int32), np.array([1.0, 2.0])
    assert L.aoclsparse_create_dcoo(byref(coo), 0, 2, 2, 2, P._ptr(r), P._ptr(c), P._ptr(v)) == 0
    d = c_void_p(0xdead)
    assert cv(coo, 2, P.ORDER_ROW, P.OP_NONE, byref(d)) == ST["not_implemented"] and not d.value
    L.aoclsparse_destroy(byref(coo))
    bm, bn, dim, rp, ci, bv = bsr_arrays()
    B = P.BsrMatrix(0, P.ORDER_COLUMN, bm, bn, dim, rp, ci, bv)
    d = c_void_p(0xdead)
    assert cv(B.h, 2, P.ORDER_ROW, P.OP_NONE, byref(d)) == ST["not_implemented"] and not d.value
    # and the same handle again is fine
    st, C = P.convert_bsr(A, 2, P.ORDER_COLUMN, P.OP_TRANSPOSE)
    assert st == 0 and np.array_equal(C.val, [1.0, 0.0, 0.0, 2.0])


# ---- every other entry point --------------------------------------------------------------------------------------------------
# what the reference answers for a BSR handle (input_format == aoclsparse_bsr_mat, the first matrix an aoclsparse::bsr, which is no
# aoclsparse::csr), with the line that decides it
REFUSALS = [
    ("trsv", "not_implemented", "level2/aoclsparse_trsv.cpp:64-67"),
    ("trsm", "not_implemented", "level3/aoclsparse_trsm.hpp:64-67"),
    ("csrmm", "not_implemented", "level3/aoclsparse_csrmm.hpp:492-494"),
    ("sp2m", "not_implemented", "level3/aoclsparse_csr2m.cpp:619-621"),
    ("csr2m", "not_implemented", "level3/aoclsparse_csr2m.cpp:619-621"),
    ("spmm", "not_implemented", "level3/aoclsparse_csr2m.cpp:619-621"),
    ("sp2md", "not_implemented", "level3/aoclsparse_sp2md.hpp:237-240"),
    ("spmmd", "not_implemented", "level3/aoclsparse_spmmd.cpp:106-109"),
    ("add", "not_implemented", "level3/aoclsparse_csradd.hpp:345-346"),
    ("symgs", "not_implemented", "solvers/aoclsparse_symgs.hpp:299-301"),
    ("symgs_mv", "not_implemented", "solvers/aoclsparse_symgs.hpp:299-301"),
    ("ilu_smoother", "not_implemented", "solvers/aoclsparse_ilu.hpp:63-65"),
    ("sorv", "not_implemented", "solvers/aoclsparse_sorv.hpp:160-162"),
    # aoclsparse_itsol_?_solve: the matrix goes through aoclsparse_csr_csc_optimize, which finds no CSR among a BSR handle's matrices
    ("itsol_d_solve", "not_implemented", "solvers/aoclsparse_itsol_functions.hpp:591 -> analysis/aoclsparse_csr_util.hpp:804-805"),
    ("itsol_s_solve", "not_implemented", "solvers/aoclsparse_itsol_functions.hpp:591 -> analysis/aoclsparse_csr_util.hpp:804-805"),
    ("itsol_c_solve", "not_implemented", "solvers/aoclsparse_itsol_functions.hpp:591 -> analysis/aoclsparse_csr_util.hpp:804-805"),
    ("itsol_z_solve", "not_implemented", "solvers/aoclsparse_itsol_functions.hpp:591 -> analysis/aoclsparse_csr_util.hpp:804-805"),
    ("itsol_d_solve_gmres", "not_implemented", "solvers/aoclsparse_itsol_functions.hpp:591 (before the method is looked at)"),
    ("set_value", "not_implemented", "extra/aoclsparse_auxiliary.hpp:457-458"),
    ("update_values", "not_implemented", "extra/aoclsparse_auxiliary.hpp:255-256"),
    ("export_csr", "invalid_value", "extra/aoclsparse_auxiliary.cpp:1343 (no CSR among the handle's matrices)"),
    ("export_csc", "invalid_value", "extra/aoclsparse_auxiliary.cpp:1402"),
    ("export_coo", "invalid_value", "extra/aoclsparse_auxiliary.hpp:343-344"),
    ("copy", "invalid_value", "extra/aoclsparse_auxiliary.cpp:1234-1235"),
    ("order_mat", "not_implemented", "extra/aoclsparse_auxiliary.cpp:850-851"),
    ("convert_csr", "not_implemented", "conversion/aoclsparse_convert.cpp:1252-1303"),
    ("convert_bsr", "not_implemented", "conversion/aoclsparse_convert.cpp:1453-1454"),
    # the hints are format-blind (analysis/aoclsparse_analysis.cpp:566-624); aoclsparse_optimize then finds that the first matrix
    # is no CSR (analysis.cpp:472-474), after aoclsparse_matrix_transform has passed a non-CSR handle through (csr_util.hpp:521, :755)
    ("set_mv_hint", "success", "analysis/aoclsparse_analysis.cpp:566-624"),
    ("set_mv_hint_kid", "success", "analysis/aoclsparse_analysis.cpp:566-624"),
    ("set_dotmv_hint", "success", "analysis/aoclsparse_analysis.cpp:566-624"),
    ("set_sv_hint", "success", "analysis/aoclsparse_analysis.cpp:566-624"),
    ("set_mm_hint", "success", "analysis/aoclsparse_analysis.cpp:566-624"),
    ("set_2m_hint", "success", "analysis/aoclsparse_analysis.cpp:566-624"),
    ("set_lu_smoother_hint", "success", "analysis/aoclsparse_analysis.cpp:566-624"),
    ("set_symgs_hint", "success", "analysis/aoclsparse_analysis.cpp:566-624"),
    ("set_sm_hint", "success", "analysis/aoclsparse_analysis.cpp:566-624"),
    ("set_memory_hint", "success", "analysis/aoclsparse_analysis.cpp (no format check)"),
    ("set_mv_hint_other_base", "invalid_value", "analysis/aoclsparse_analysis.cpp:585-588"),
    ("optimize", "not_implemented", "analysis/aoclsparse_analysis.cpp:472-474"),
    ("optimize_after_mv_hint", "not_implemented", "analysis/aoclsparse_analysis.cpp:472-474"),
]


def _bsr(t, base):
    dt = dict(TYPES)[t]
    bm, bn, dim, rp, ci, v = bsr_arrays(base, dt)
    A = P.BsrMatrix(base, P.ORDER_COLUMN, bm, bn, dim, rp, ci, v)
    assert A.status == 0
    return A


def _itsol_solve(t, base, d, opts=()):
    """aoclsparse_itsol_<t>_solve on a BSR handle of that value type"""
    dt = dict(TYPES)[t]
    M = _bsr(t, base)
    h = c_void_p()
    assert getattr(L, "aoclsparse_itsol_%s_init" % t)(byref(h)) == 0
    for k, v in opts:
        assert L.aoclsparse_itsol_option_set(h, k.encode(), v.encode()) == 0
    b, x = np.ones(M.m, dt), np.zeros(M.m, dt)
    rinfo = np.zeros(100, np.float32 if t in "sc" else np.float64)
    st = getattr(L, "aoclsparse_itsol_%s_solve" % t)(h, M.m, M.h, d.h, P._ptr(b), P._ptr(x), P._ptr(rinfo), None, None, None)
    L.aoclsparse_itsol_destroy(byref(h))
    return st


def _call(name, A, d):
    if name.startswith("itsol_"):
        return _itsol_solve(name[6], A.base, d, (("iterative method", "GMRES"),) if name.endswith("gmres") else ())
    m = A.m
    x, y, C = np.ones(m), np.zeros(m), np.zeros(m * m)
    h, pv = c_void_p(), c_void_p()
    b, mm, nn, nz = c_int(), c_int32(), c_int32(), c_int32()
    a1, a2, a3 = c_void_p(), c_void_p(), c_void_p()
    ex = (byref(b), byref(mm), byref(nn), byref(nz), byref(a1), byref(a2), byref(a3))
    tri = P.Descr(base=A.base, mtype=P.TYPE_TRIANGULAR)
    other = P.Descr(base=1 - A.base)

    def optimize_after_mv_hint():
        assert L.aoclsparse_set_mv_hint(A.h, P.OP_NONE, d.h, 10) == 0
        return L.aoclsparse_optimize(A.h)

    return {
        "trsv": lambda: P.dtrsv(P.OP_NONE, 1.0, A, tri, x, y),
        "trsm": lambda: L.aoclsparse_dtrsm(P.OP_NONE, 1.0, A.h, tri.h, 0, P._ptr(x), 1, m, P._ptr(y), m),
        "csrmm": lambda: L.aoclsparse_dcsrmm(P.OP_NONE, 1.0, A.h, d.h, 0, P._ptr(C), m, m, 0.0, P._ptr(C), m),
        "sp2m": lambda: L.aoclsparse_sp2m(P.OP_NONE, d.h, A.h, P.OP_NONE, d.h, A.h, 0, byref(h)),
        "csr2m": lambda: L.aoclsparse_dcsr2m(P.OP_NONE, d.h, A.h, P.OP_NONE, d.h, A.h, 0, byref(h)),
        "spmm": lambda: L.aoclsparse_spmm(P.OP_NONE, A.h, A.h, byref(h)),
        "sp2md": lambda: L.aoclsparse_dsp2md(P.OP_NONE, d.h, A.h, P.OP_NONE, d.h, A.h, 1.0, 0.0, P._ptr(C), 0, m),
        "spmmd": lambda: L.aoclsparse_dspmmd(P.OP_NONE, A.h, A.h, 0, P._ptr(C), m),
        "add": lambda: L.aoclsparse_dadd(P.OP_NONE, A.h, 1.0, A.h, byref(h)),
        "symgs": lambda: L.aoclsparse_dsymgs(P.OP_NONE, A.h, d.h, 1.0, P._ptr(x), P._ptr(y)),
        "symgs_mv": lambda: L.aoclsparse_dsymgs_mv(P.OP_NONE, A.h, d.h, 1.0, P._ptr(x), P._ptr(y), P._ptr(C)),
        "ilu_smoother": lambda: L.aoclsparse_dilu_smoother(P.OP_NONE, A.h, d.h, byref(pv), None, P._ptr(y), P._ptr(x)),
        "sorv": lambda: L.aoclsparse_dsorv(0, d.h, A.h, 1.0, 1.0, P._ptr(y), P._ptr(x)),
        "set_value": lambda: L.aoclsparse_dset_value(A.h, A.base, A.base, 2.0),
        "update_values": lambda: L.aoclsparse_dupdate_values(A.h, A.nnz, P._ptr(np.ones(A.nnz))),
        "export_csr": lambda: L.aoclsparse_export_dcsr(A.h, *ex),
        "export_csc": lambda: L.aoclsparse_export_dcsc(A.h, *ex),
        "export_coo": lambda: L.aoclsparse_export_dcoo(A.h, *ex),
        "copy": lambda: L.aoclsparse_copy(A.h, d.h, byref(h)),
        "order_mat": lambda: L.aoclsparse_order_mat(A.h),
        "convert_csr": lambda: L.aoclsparse_convert_csr(A.h, P.OP_NONE, byref(h)),
        "convert_bsr": lambda: L.aoclsparse_convert_bsr(A.h, 2, P.ORDER_COLUMN, P.OP_NONE, byref(h)),
        "set_mv_hint": lambda: L.aoclsparse_set_mv_hint(A.h, P.OP_NONE, d.h, 10),
        "set_mv_hint_kid": lambda: L.aoclsparse_set_mv_hint_kid(A.h, P.OP_NONE, d.h, 10, 1),
        "set_dotmv_hint": lambda: L.aoclsparse_set_dotmv_hint(A.h, P.OP_NONE, d.h, 10),
        "set_sv_hint": lambda: L.aoclsparse_set_sv_hint(A.h, P.OP_TRANSPOSE, tri.h, 10),
        "set_mm_hint": lambda: L.aoclsparse_set_mm_hint(A.h, P.OP_NONE, d.h, 10),
        "set_2m_hint": lambda: L.aoclsparse_set_2m_hint(A.h, P.OP_NONE, d.h, 10),
        "set_lu_smoother_hint": lambda: L.aoclsparse_set_lu_smoother_hint(A.h, P.OP_NONE, d.h, 10),
        "set_symgs_hint": lambda: L.aoclsparse_set_symgs_hint(A.h, P.OP_NONE, d.h, 10),
        "set_sm_hint": lambda: L.aoclsparse_set_sm_hint(A.h, P.OP_NONE, tri.h, 0, 10),
        "set_memory_hint": lambda: L.aoclsparse_set_memory_hint(A.h, 0),
        "set_mv_hint_other_base": lambda: L.aoclsparse_set_mv_hint(A.h, P.OP_NONE, other.h, 10),
        "optimize": lambda: L.aoclsparse_optimize(A.h),
        "optimize_after_mv_hint": optimize_after_mv_hint,
    }[name]()


@pytest.mark.parametrize("name,expected,where", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_other_entry_point_answers_as_the_reference(name, expected, where):
    for base in (1, 0):
        A = _bsr("d", base)
        keep = [a.tobytes() for a in (A.row_ptr, A.col_ind, A.val)]
        assert P.STATUS[_call(name, A, P.Descr(base=base))] == expected, where
        assert [a.tobytes() for a in (A.row_ptr, A.col_ind, A.val)] == keep  # a refused setter has written nothing
        assert A.spmv_info().device_resident == 0  # and nothing has gone to the device


def test_mv_statuses_decided_before_the_device():
    x, y = np.ones(4), np.full(4, 7.0)
    g = P.Descr()
    A = _bsr("d", 0)
    mv = lambda op, d, M=A: P.dmv(op, 1.0, M, d, x, 0.0, y)  # noqa: E731
    # mv.cpp:55-66: null pointers
    one = np.ones(1)
    for k in range(6):
        args = [P._ptr(one), A.h, g.h, P._ptr(x), P._ptr(one), P._ptr(y)]
        args[k] = None
        assert L.aoclsparse_dmv(P.OP_NONE, *args) == ST["invalid_pointer"], k
    assert mv(P.OP_NONE, P.Descr(base=1)) == ST["invalid_value"]  # mv.cpp:71-72: the descriptor's base is the handle's
    assert mv(77, g) == ST["invalid_value"]  # :75-78
    assert P.smv(P.OP_NONE, 1.0, A, g, x, 0.0, y) == ST["wrong_type"]  # :81-82
    R = P.BsrMatrix(0, P.ORDER_COLUMN, 2, 3, 2, [0, 1, 2], [0, 2], np.ones(8))
    assert R.status == 0
    for mt in (P.TYPE_SYMMETRIC, P.TYPE_HERMITIAN):
        assert mv(P.OP_NONE, P.Descr(mtype=mt), R) == ST["invalid_size"]  # :87-90
    assert mv(P.OP_NONE, P.Descr(mtype=P.TYPE_HERMITIAN)) == ST["not_implemented"]  # :105-106 (real types)
    # no matrix of a BSR handle has an effective doid of gn for these (magic_box.hpp:103-107, :260-271): get_best_matrix returns
    # nothing, mtx_t stays uninitialised and the switch of mv.cpp:202 ends in its default, :344-345
    NI = ST["not_implemented"]
    for op in (P.OP_TRANSPOSE, P.OP_CONJ_TRANSPOSE):
        assert mv(op, g) == NI
    for mt in (P.TYPE_SYMMETRIC, P.TYPE_TRIANGULAR):
        for fill in (P.FILL_LOWER, P.FILL_UPPER):
            for op in (P.OP_NONE, P.OP_TRANSPOSE, P.OP_CONJ_TRANSPOSE):
                assert mv(op, P.Descr(mtype=mt, fill=fill)) == NI, (mt, fill, op)
    # row-major blocks: mv.cpp:325-329
    bm, bn, dim, rp, ci, v = bsr_arrays()
    Rm = P.BsrMatrix(0, P.ORDER_ROW, bm, bn, dim, rp, ci, v)
    assert mv(P.OP_NONE, g, Rm) == NI
    assert np.all(y == 7.0)  # nothing was written
    # the complex types: the same table, and a Hermitian descriptor goes the same way (no :105-106 for them)
    for t, fn in (("c", L.aoclsparse_cmv), ("z", L.aoclsparse_zmv)):
        Z = _bsr(t, 1)
        dt = dict(TYPES)[t]
        xz, yz, one = np.ones(4, dt), np.zeros(4, dt), np.ones(1, dt)
        cmv = lambda op, d, M=Z: fn(op, P._ptr(one), M.h, d.h, P._ptr(xz), P._ptr(one), P._ptr(yz))  # noqa: E731
        g1 = P.Descr(base=1)
        assert cmv(P.OP_NONE, g) == ST["invalid_value"]  # the base
        for op in (P.OP_TRANSPOSE, P.OP_CONJ_TRANSPOSE):
            assert cmv(op, g1) == NI
        for mt in (P.TYPE_SYMMETRIC, P.TYPE_HERMITIAN, P.TYPE_TRIANGULAR):
            for fill in (P.FILL_LOWER, P.FILL_UPPER):
                for op in (P.OP_NONE, P.OP_TRANSPOSE, P.OP_CONJ_TRANSPOSE):
                    assert cmv(op, P.Descr(base=1, mtype=mt, fill=fill)) == NI, (t, mt, fill, op)
        bm, bn, dim, rp, ci, v = bsr_arrays(1, dt)
        Zr = P.BsrMatrix(1, P.ORDER_ROW, bm, bn, dim, rp, ci, v)
        assert cmv(P.OP_NONE, g1, Zr) == NI
        wrong = L.aoclsparse_zmv if t == "c" else L.aoclsparse_cmv
        assert wrong(P.OP_NONE, P._ptr(one), Z.h, g1.h, P._ptr(xz), P._ptr(one), P._ptr(yz)) == ST["wrong_type"]
        assert np.all(yz == 0)
    # aoclsparse_?dotmv is mv followed by a dot (level2/aoclsparse_dotmv.hpp:47-59): the same refusals
    dot = np.zeros(1)
    assert L.aoclsparse_ddotmv(P.OP_TRANSPOSE, 1.0, A.h, g.h, P._ptr(x), 0.0, P._ptr(y), P._ptr(dot)) == NI


# ---- the reference's known answers -------------------------------------------------------------------------------------------
with open(os.path.join(ROOT, "tests", "golden", "bsr_kats.json")) as _f:
    KATS = json.load(_f)


@pytest.mark.parametrize("case", KATS["create"], ids=[c["name"] for c in KATS["create"]])
def test_kat_creator(case):
    for t, dt in TYPES:
        for order in (P.ORDER_ROW, P.ORDER_COLUMN):
            rp, ci = np.array(case["row_ptr"], np.int32), np.array(case["col_idx"], np.int32)
            v = np.zeros(max(1, len(ci)) * case["block_dim"] ** 2 + 1, dt)
            assert create(t, case["base"], order, case["bm"], case["bn"], case["block_dim"], rp, ci, v) == case["status"], (t, order)


@pytest.mark.parametrize("exp", KATS["convert"]["expected"], ids=["%d-%s" % (e["block_dim"], e["order"]) for e in KATS["convert"]["expected"]])
@pytest.mark.parametrize("base", [0, 1])
def test_kat_convert(exp, base):
    K = KATS["convert"]
    order = P.ORDER_ROW if exp["order"] == "row" else P.ORDER_COLUMN
    for t, dt in TYPES:
        rp, ci = np.array(K["row_ptr"], np.int32) + base, np.array(K["col_ind"], np.int32) + base
        cplx = t in "cz"
        v = (np.array(K["val"]) + (1j * np.array(K["val_imag"]) if cplx else 0)).astype(dt)
        h = c_void_p()
        assert getattr(L, "aoclsparse_create_%scsr" % t)(byref(h), base, K["m"], K["n"], len(v), P._ptr(rp), P._ptr(ci), P._ptr(v)) == 0
        d = c_void_p()
        assert L.aoclsparse_convert_bsr(h, exp["block_dim"], order, P.OP_NONE, byref(d)) == 0
        B = P.BsrMatrix.from_handle(d, dt)
        want = (np.array(exp["bsr_val"]) + (1j * np.array(exp["bsr_val_imag"]) if cplx else 0)).astype(dt)
        assert np.array_equal(B.row_ptr, np.array(exp["bsr_ptr"]) + base)
        assert np.array_equal(B.col_ind, np.array(exp["bsr_ind"]) + base)
        assert np.array_equal(B.val, want), t
        B.destroy()
        L.aoclsparse_destroy(byref(h))
