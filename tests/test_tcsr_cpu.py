"""TCSR handles without a GPU: creator statuses (extra/aoclsparse_auxiliary.hpp:54-193 of the reference), what every other entry
point answers for such a handle, the product statuses that are decided before the device is touched, and the aliasing contract."""
import ctypes
import subprocess
from ctypes import byref, c_int, c_int32, c_void_p

import numpy as np
import pytest

from util import pkg

P = pkg()
ST = {v: k for k, v in P.STATUS.items()}


def tcsr_arrays(base=0, dtype=np.float64):
    """4 x 4, every entry present: L rows end with the diagonal, U rows start with it"""
    m = 4
    pl = np.cumsum([0] + [i + 1 for i in range(m)])
    cl = np.concatenate([np.arange(i + 1) for i in range(m)])
    pu = np.cumsum([0] + [m - i for i in range(m)])
    cu = np.concatenate([np.arange(i, m) for i in range(m)])
    vl = (np.arange(len(cl)) + 1.0).astype(dtype)
    vu = (np.arange(len(cu)) + 2.0).astype(dtype)
    return m, (pl + base).astype(np.int32), (cl + base).astype(np.int32), vl, (pu + base).astype(np.int32), (cu + base).astype(np.int32), vu


def create(base, m, n, nnz, pl, pu, cl, cu, vl, vu, fn="aoclsparse_create_dtcsr", mat=True):
    h = c_void_p(0xdead)
    st = getattr(P.lib(), fn)(byref(h) if mat else None, base, m, n, nnz, P._ptr(pl), P._ptr(pu), P._ptr(cl), P._ptr(cu), P._ptr(vl), P._ptr(vu))
    if st == 0:
        P.lib().aoclsparse_destroy(byref(h))
    else:
        assert not mat or not h.value, "*mat is set to NULL before anything else (auxiliary.hpp:71)"
    return P.STATUS[st]


@pytest.mark.parametrize("base", [0, 1])
def test_creator_statuses_in_the_reference_order(base):
    m, pl, cl, vl, pu, cu, vu = tcsr_arrays(base)
    nnz = len(vl) + len(vu) - m
    ok = dict(base=base, m=m, n=m, nnz=nnz, pl=pl, pu=pu, cl=cl, cu=cu, vl=vl, vu=vu)
    assert create(**ok) == "success"
    assert create(**ok, mat=False) == "invalid_pointer"  # :69-70
    for k in ("pl", "pu", "cl", "cu", "vl", "vu"):  # :72-77, before the sizes are looked at
        assert create(**{**ok, k: None, "m": -1}) == "invalid_pointer", k
    assert create(**{**ok, "base": 2, "m": -1}) == "invalid_value"  # :80-81, before the sizes
    assert create(**{**ok, "m": -1}) == "invalid_size"  # :84-85
    assert create(**{**ok, "nnz": -1}) == "invalid_size"
    assert create(**{**ok, "n": m + 1}) == "invalid_size"  # :89-90
    assert create(**{**ok, "nnz": nnz + 1}) == "invalid_size"  # :96-97
    # each triangle through the matrix check with its shape (:105-140): an entry on the wrong side of the diagonal
    bad = cl.copy()
    bad[1] = base + 3  # row 1 of L: column 3
    assert create(**{**ok, "cl": bad}) == "invalid_index_value"
    bad = cu.copy()
    bad[len(cu) - 1] = base  # last row of U: column 0
    assert create(**{**ok, "cu": bad}) == "invalid_index_value"
    # unsorted: the diagonal in front of a lower entry (:118-119, :137-138)
    un = cl.copy()
    un[1], un[2] = un[2], un[1]
    assert create(**{**ok, "cl": un}) == "unsorted_input"
    # a missing diagonal (:120-121, :139-140): row 1 of L = {0, 0} is a duplicate, so drop the diagonal of U's row 0 instead
    pu2 = pu.copy()
    pu2[1:] -= 1
    assert create(**{**ok, "pu": pu2, "cu": cu[1:].copy(), "vu": vu[1:].copy(), "nnz": nnz - 1}) == "invalid_value"
    pl2 = pl.copy()
    pl2[1:] -= 1
    assert create(**{**ok, "pl": pl2, "cl": cl[1:].copy(), "vl": vl[1:].copy(), "nnz": nnz - 1}) == "invalid_value"
    # partially sorted triangles are taken (:188-191): the lower entries of L's last row swapped
    ps = cl.copy()
    ps[6], ps[7] = ps[7], ps[6]
    assert create(**{**ok, "cl": ps}) == "success"


def test_all_four_creators_and_default_visibility():
    lib_path = P.LIB_PATH
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    for t, dt in (("s", np.float32), ("d", np.float64), ("c", np.complex64), ("z", np.complex128)):
        name = "aoclsparse_create_%stcsr" % t
        assert any(line.split()[-1] == name and line.split()[-2] == "T" for line in out.splitlines()), name
        m, pl, cl, vl, pu, cu, vu = tcsr_arrays(0, dt)
        A = P.TcsrMatrix(0, m, pl, cl, vl, pu, cu, vu)
        assert A.status == 0, name
        A.destroy()
    vis = subprocess.run(["readelf", "--dyn-syms", "-W", lib_path], capture_output=True, text=True, check=True).stdout
    for t in "sdcz":
        rows = [r for r in vis.splitlines() if r.split() and r.split()[-1].split("@")[0] == "aoclsparse_create_%stcsr" % t]
        assert rows and all("DEFAULT" in r and "GLOBAL" in r for r in rows), t


# what the reference answers for a TCSR handle in every other entry point that takes a handle, with the line that decides it
REFUSALS = [
    ("csrmm", "not_implemented", "level3/aoclsparse_csrmm.hpp:454-456"),
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
    # aoclsparse_itsol_?_solve: the matrix goes through aoclsparse_csr_csc_optimize, which finds no CSR among a TCSR handle's matrices
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
]
# aoclsparse_?csr2dense takes raw arrays, no handle.  aoclsparse_?dotmv is aoclsparse::mv followed by a dense dot
# (level2/aoclsparse_dotmv.hpp:47-59), so it accepts what ?mv accepts: covered by the product statuses below and on the GPU.


def _itsol_solve(t, A, d, opts=()):
    """aoclsparse_itsol_<t>_solve on a handle of that value type over the same pattern as A"""
    L = P.lib()
    dt = {"d": np.float64, "s": np.float32, "c": np.complex64, "z": np.complex128}[t]
    m, pl, cl, vl, pu, cu, vu = tcsr_arrays(A.base, dt)
    M = P.TcsrMatrix(A.base, m, pl, cl, vl, pu, cu, vu)
    assert M.status == 0
    h = c_void_p()
    assert getattr(L, "aoclsparse_itsol_%s_init" % t)(byref(h)) == 0
    for k, v in opts:
        assert L.aoclsparse_itsol_option_set(h, k.encode(), v.encode()) == 0
    b, x = np.ones(m, dt), np.zeros(m, dt)
    rinfo = np.zeros(100, np.float32 if t in "sc" else np.float64)
    st = getattr(L, "aoclsparse_itsol_%s_solve" % t)(h, m, M.h, d.h, P._ptr(b), P._ptr(x), P._ptr(rinfo), None, None, None)
    L.aoclsparse_itsol_destroy(byref(h))
    return st


def _call(name, A, d):
    L = P.lib()
    if name.startswith("itsol_"):
        return _itsol_solve(name[6], A, d, (("iterative method", "GMRES"),) if name.endswith("gmres") else ())
    m = A.m
    x, y, C = np.ones(m), np.zeros(m), np.zeros(m * m)
    h, pv = c_void_p(), c_void_p()
    b, mm, nn, nz = c_int(), c_int32(), c_int32(), c_int32()
    a1, a2, a3 = c_void_p(), c_void_p(), c_void_p()
    ex = (byref(b), byref(mm), byref(nn), byref(nz), byref(a1), byref(a2), byref(a3))
    return {
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
    }[name]()


@pytest.mark.parametrize("name,expected,where", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_other_entry_point_answers_as_the_reference(name, expected, where):
    m, pl, cl, vl, pu, cu, vu = tcsr_arrays(1)
    A = P.TcsrMatrix(1, m, pl, cl, vl, pu, cu, vu)
    assert A.status == 0
    keep = (vl.copy(), vu.copy())
    assert P.STATUS[_call(name, A, P.Descr(base=1))] == expected, where
    assert np.array_equal(A.val_l, keep[0]) and np.array_equal(A.val_u, keep[1])  # a refused setter has written nothing


def test_hints_and_optimize_accept_the_handle():
    L = P.lib()
    m, pl, cl, vl, pu, cu, vu = tcsr_arrays(0)
    A = P.TcsrMatrix(0, m, pl, cl, vl, pu, cu, vu)
    g, t = P.Descr(), P.Descr(mtype=P.TYPE_TRIANGULAR, fill=P.FILL_UPPER)
    assert L.aoclsparse_set_mv_hint(A.h, P.OP_NONE, g.h, 10) == 0
    assert L.aoclsparse_set_mv_hint_kid(A.h, P.OP_NONE, g.h, 10, 1) == 0
    assert L.aoclsparse_set_sv_hint(A.h, P.OP_TRANSPOSE, t.h, 10) == 0
    assert L.aoclsparse_set_sm_hint(A.h, P.OP_NONE, t.h, 0, 10) == 0
    assert L.aoclsparse_set_mv_hint(A.h, P.OP_NONE, P.Descr(base=1).h, 10) == ST["invalid_value"]  # the base must match
    assert L.aoclsparse_optimize(A.h) == 0  # analysis/aoclsparse_analysis.cpp:467-468
    assert L.aoclsparse_optimize(A.h) == 0


def test_product_and_solve_statuses_decided_before_the_device():
    L = P.lib()
    x, y = np.ones(4), np.zeros(4)
    m, pl, cl, vl, pu, cu, vu = tcsr_arrays(0)
    A = P.TcsrMatrix(0, m, pl, cl, vl, pu, cu, vu)
    g = P.Descr()
    # level2/aoclsparse_tcsr.hpp:115-118: no transposed general product
    assert P.dmv(P.OP_TRANSPOSE, 1.0, A, g, x, 0.0, y) == ST["not_implemented"]
    assert P.dmv(P.OP_CONJ_TRANSPOSE, 1.0, A, g, x, 0.0, y) == ST["not_implemented"]
    assert P.dmv(P.OP_NONE, 1.0, A, P.Descr(base=1), x, 0.0, y) == ST["invalid_value"]  # mv.cpp:71-72
    assert P.dmv(P.OP_NONE, 1.0, A, P.Descr(mtype=P.TYPE_HERMITIAN), x, 0.0, y) == ST["not_implemented"]  # mv.cpp:105-106
    assert P.smv(P.OP_NONE, 1.0, A, g, x, 0.0, y) == ST["wrong_type"]  # mv.cpp:81-82
    # :99-114: the general product exists for double only
    m, pl, cl, vl, pu, cu, vu = tcsr_arrays(0, np.float32)
    S = P.TcsrMatrix(0, m, pl, cl, vl, pu, cu, vu)
    xs, ys = np.ones(4, np.float32), np.zeros(4, np.float32)
    assert P.smv(P.OP_NONE, 1.0, S, g, xs, 0.0, ys) == ST["not_implemented"]
    for dt, fn in ((np.complex64, L.aoclsparse_cmv), (np.complex128, L.aoclsparse_zmv)):
        m, pl, cl, vl, pu, cu, vu = tcsr_arrays(0, dt)
        Z = P.TcsrMatrix(0, m, pl, cl, vl, pu, cu, vu)
        xz, yz = np.ones(4, dt), np.zeros(4, dt)
        one = np.ones(1, dt)
        assert fn(P.OP_NONE, P._ptr(one), Z.h, g.h, P._ptr(xz), P._ptr(one), P._ptr(yz)) == ST["not_implemented"]
        # :178-183: the conjugate forms of a triangular product are refused
        for fill in (P.FILL_LOWER, P.FILL_UPPER):
            t = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=fill)
            assert fn(P.OP_CONJ_TRANSPOSE, P._ptr(one), Z.h, t.h, P._ptr(xz), P._ptr(one), P._ptr(yz)) == ST["not_implemented"]
    # solves: level2/aoclsparse_trsv.cpp:59-113 on a TCSR handle
    t = P.Descr(mtype=P.TYPE_TRIANGULAR)
    assert P.dtrsv(P.OP_NONE, 1.0, A, g, x, y) == ST["invalid_value"]  # general descriptor
    assert P.dtrsv(P.OP_NONE, 1.0, A, P.Descr(mtype=P.TYPE_TRIANGULAR, diag=P.DIAG_ZERO), x, y) == ST["invalid_value"]
    assert P.dtrsv(P.OP_NONE, 1.0, A, t, x, y, incb=-1, incx=1) == ST["invalid_value"]
    assert P.strsv(P.OP_NONE, 1.0, A, t, x, y) == ST["wrong_type"]
    assert P.dtrsv(P.OP_NONE, 1.0, A, t, x, y, kid=4) == ST["invalid_kid"]
    assert L.aoclsparse_dtrsm(P.OP_NONE, 1.0, A.h, g.h, 0, P._ptr(x), 1, 1, P._ptr(y), 1) == ST["invalid_value"]


def test_create_and_destroy_leave_the_callers_arrays_alone():
    """(under tests/run_san.sh a free or a write of an aliased array is a report)"""
    for base in (0, 1):
        m, pl, cl, vl, pu, cu, vu = tcsr_arrays(base)
        keep = [a.copy() for a in (pl, cl, vl, pu, cu, vu)]
        A = P.TcsrMatrix(base, m, pl, cl, vl, pu, cu, vu)
        assert A.status == 0
        for a in (A.ptr_l, A.col_l, A.val_l, A.ptr_u, A.col_u, A.val_u):  # aliased, not copied
            assert any(a.ctypes.data == b.ctypes.data for b in (pl, cl, vl, pu, cu, vu))
        assert P.lib().aoclsparse_set_sv_hint(A.h, P.OP_NONE, P.Descr(base=base, mtype=P.TYPE_TRIANGULAR).h, 5) == 0
        assert P.lib().aoclsparse_optimize(A.h) == 0
        assert P.lib().aoclsparse_mi355_invalidate(A.h) == 0
        A.destroy()
        assert not A.h
        for a, k in zip((pl, cl, vl, pu, cu, vu), keep):
            assert np.array_equal(a, k)
            a[:] = a  # still writable memory of ours
