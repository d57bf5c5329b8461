"""GPU tier: the three routes that bring new values in HBM to a CSR handle -- ?refresh_values_from_coo_device, ?revalue_device and
?update_values_device (include/aoclsparse_mi355.h) -- end in one commit step (device_handle_api.cpp: commit_values_device).  The
tests of each route use a handle of their own; here the routes follow one another on ONE handle that holds everything the step
decides about: the triplet map, a clean COPY with its value map, the diagonal and two mapped TRSV plans.

The matrix: the 5-point Laplacian on a 21 x 21 grid, 441 rows and 2,121 entries (one more than the 2,048 a workgroup of the gather
kernel takes), every 7th diagonal entry removed (the clean CSR is a copy with inserted zeros), the triplets shuffled with a fixed
seed (so every row is unsorted).  After every step the handle is compared with the oracle -- dmv within the bound of
tests/test_gpu_value_updates.py, (len + 24) eps sum |a||x| per row; the unit-diagonal solves, the exported CSR and the exported
clean CSR exactly -- and bit for bit with a FRESH handle over the same arrays with the new values."""
import ctypes

import numpy as np
import pytest

import oracle
from clean_cases import DTYPES, export_clean, same_bits
from util import EPS64, abs_row_sums, laplace5, pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from test_gpu_value_updates import _trsv_expect, scaled  # noqa: E402
from test_operator_device_gpu import mv as op_mv  # noqa: E402
from test_order_device_gpu import fetch  # noqa: E402
from test_revalue_device_gpu import dev, oracle_clean_values  # noqa: E402

P = pkg()
L = P.lib()
GRID, M = 21, 441
LOWER_N, UPPER_N = (P.FILL_LOWER, P.OP_NONE), (P.FILL_UPPER, P.OP_NONE)
# spmv_info().device_resident right after each route behind a mirror a host ?set_value has invalidated, as observed on the commit
# before the routes were unified: none of them uploads, the next product does
RESIDENT_BEHIND_INVALID_MIRROR = {"refresh": 0, "revalue": 0, "update": 0}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    yield
    L.aoclsparse_mi355_set_pointer_mode(P.PTR_AUTO)


@pytest.fixture(scope="module")
def case():
    """0-based: the shuffled triplets (row, col, values) and the CSR the stable sort by row makes of them (rp, ci, order: CSR entry
    q is triplet order[q])"""
    _, rp, ci, _ = laplace5(GRID)
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    rows = np.repeat(np.arange(M), np.diff(rp))
    keep = ~((rows == ci) & (rows % 7 == 0))
    rows, cols = rows[keep], ci[keep]
    assert len(ci) == 2121 and len(rows) == 2058  # (still more than the 2,048 entries of one gather tile)
    rng = np.random.default_rng(2727)
    shuffle = rng.permutation(len(rows))
    rows, cols = rows[shuffle], cols[shuffle]
    vals = rng.uniform(0.5, 1.5, len(rows)) * np.where(rows == cols, 4.0, -1.0)
    order = np.argsort(rows, kind="stable")
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=M))]).astype(np.int32)
    ci2 = cols[order].astype(np.int32)
    assert np.any(np.diff(ci2.astype(np.int64))[np.diff(rows[order]) == 0] < 0), "unsorted rows"
    return dict(row=rows.astype(np.int32), col=cols.astype(np.int32), val=vals, rp=rp2, ci=ci2, order=order)


def typed(v, dtype, seed=3):
    dtype = np.dtype(dtype)
    if dtype.kind == "c":
        v = v * np.exp(0.3j * np.random.default_rng(seed).uniform(-1, 1, len(v)))
    return np.ascontiguousarray(v.astype(dtype))


def handle(case, base, trip_vals):
    """the handle under test: from the shuffled triplets, with the triplet map and the keep_value_maps flag"""
    n = len(trip_vals)
    A = P.Matrix.from_coo_device(base, M, M, n, dev(case["row"] + base), dev(case["col"] + base), dev(trip_vals), P.COO_KEEP,
                                 refreshable=True)
    assert A.status == 0, P.STATUS.get(A.status, A.status)
    assert A.keep_value_maps() == 0 and A.coo_map_info().kept == 1
    return A


def fresh(case, base, csr_vals):
    A = P.Matrix.from_device(base, M, M, len(csr_vals), dev(case["rp"] + base), dev(case["ci"] + base), dev(csr_vals))
    assert A.status == 0, P.STATUS.get(A.status, A.status)
    return A


def mv(A, x, y0):
    y = dev(y0)
    assert P.dmv(P.OP_NONE, 1.3, A, P.Descr(base=A.base), dev(x), -0.4, y) == 0
    torch.cuda.synchronize()
    return y.cpu().numpy()


def solve(A, fill, op, b):
    """one unit-diagonal ?trsv of b's type through host pointers -> x"""
    d = P.Descr(base=A.base, mtype=P.TYPE_TRIANGULAR, fill=fill, diag=P.DIAG_UNIT)
    x = np.zeros_like(b)
    letter = P.Matrix._LETTER[str(b.dtype)]
    alpha = {"s": 0.75, "d": 0.75, "c": P.CFloat(0.75, 0.25), "z": P.CDouble(0.75, 0.25)}[letter]
    st = getattr(L, "aoclsparse_%strsv" % letter)(op, alpha, A.h, d.h, P._ptr(b), P._ptr(x))
    assert st == 0, P.STATUS.get(st, st)
    return x


def exported(A, dtype):
    e = A.export_device()
    assert e["status"] == 0 and (e["base"], e["m"], e["n"]) == (A.base, M, M)
    return fetch(e["row_ptr"], M + 1, np.int32), fetch(e["col_ind"], e["nnz"], np.int32), fetch(e["val"], e["nnz"], dtype), e["val"]


def check_double(A, case, base, v, x, y0, b, what):
    """everything the handle shows, against the oracle and against a fresh handle over the same arrays with these values"""
    rp, ci = case["rp"] + base, case["ci"] + base
    F = fresh(case, base, v)
    y = mv(A, x, y0)
    so, yr = oracle.dcsrmv(-1, base, 1.3, M, len(v), v, ci, rp, x, -0.4, y0)
    assert so == 0
    bound = (np.diff(rp) + 24) * EPS64 * abs_row_sums(case["rp"], case["ci"], v, x) + 1e-300
    print(what, "dmv: max |got - oracle| / bound =", float(np.max(np.abs(y - yr) / bound)))
    assert np.all(np.abs(y - yr) <= bound), (what, "dmv against the oracle")
    assert same_bits(y, mv(F, x, y0)), (what, "dmv against a fresh handle")
    H = type("Arrays", (), dict(m=M, base=base, row_ptr=rp, col_ind=ci))
    for fill, op in (LOWER_N, UPPER_N):
        got = solve(A, fill, op, b)
        assert np.array_equal(got, _trsv_expect(H, fill, op, True, 0.75, b, 0)(v)), (what, "solve against the oracle", fill)
        assert same_bits(got, solve(F, fill, op, b)), (what, "solve against a fresh handle", fill)
    erp, eci, ev, _ = exported(A, np.float64)
    assert np.array_equal(erp, rp) and np.array_equal(eci, ci) and same_bits(ev, v), (what, "exported CSR")
    o, want = oracle_clean_values(M, base, rp, ci, v)
    c = export_clean(A, np.float64)
    assert c[6] and np.array_equal(c[1], o["ptr"]) and np.array_equal(c[2], o["ind"]) and same_bits(c[3], want), (what, "clean CSR")
    cf = export_clean(F, np.float64)
    assert all(np.array_equal(c[k], cf[k]) for k in (1, 2, 4, 5)) and same_bits(c[3], cf[3]), (what, "clean CSR against a fresh handle")


@pytest.mark.parametrize("base", [0, 1])
def test_mixed_sequence_double(case, base):
    order = case["order"]
    t0 = case["val"]
    rng = np.random.default_rng(9)
    x, y0, b = rng.uniform(-1, 1, M), rng.uniform(-1, 1, M), rng.uniform(-1, 1, M)
    A = handle(case, base, t0)
    assert A.clean_device() == 0
    check_double(A, case, base, t0[order], x, y0, b, "set-up")  # (the two solves build the plans)
    i = A.value_map_info()
    assert i.clean_map == 1 and i.plans_mapped >= 1 and i.clean_builds == 1
    # 1. refresh from triplets: nothing is kept, the next solves build their plans again
    t1, before = scaled(t0, 11), A.value_map_info()
    assert A.refresh_from_coo_device(dev(t1)) == 0
    i = A.value_map_info()
    assert (i.revalues, i.plans_mapped, i.clean_map) == (before.revalues, 0, 0) and A.spmv_info().device_resident == 1
    assert A.clean_device() == 0  # (a clean copy with its map again, for step 2)
    check_double(A, case, base, t1[order], x, y0, b, "refresh")
    i = A.value_map_info()
    assert i.plan_builds > before.plan_builds and i.clean_builds == before.clean_builds + 1 and i.plans_mapped >= 1
    # 2. revalue: the clean copy, the diagonal and both plans follow
    v2, before = scaled(t1[order], 12), A.value_map_info()
    assert A.revalue_device(dev(v2)) == 0
    i = A.value_map_info()
    assert i.revalues == before.revalues + 1 and i.last_kept_plans >= 1 and i.clean_map == 1
    check_double(A, case, base, v2, x, y0, b, "revalue")
    i = A.value_map_info()
    assert (i.plan_builds, i.clean_builds) == (before.plan_builds, before.clean_builds) and A.spmv_info().device_resident == 1
    # 3. update: nothing is kept
    v3, before = scaled(v2, 13), A.value_map_info()
    assert A.update_values_device(dev(v3)) == 0
    i = A.value_map_info()
    assert (i.revalues, i.plans_mapped, i.clean_map) == (before.revalues, 0, 0) and A.spmv_info().device_resident == 1
    assert A.clean_device() == 0  # (... for step 4)
    check_double(A, case, base, v3, x, y0, b, "update")
    i = A.value_map_info()
    assert i.plan_builds > before.plan_builds and i.clean_builds == before.clean_builds + 1
    # 4. revalue in place: the new values are written into the mirror's own array, and that array is the argument
    v4, before = scaled(v3, 14), A.value_map_info()
    addr = exported(A, np.float64)[3]
    mirror = dev(v4)
    hip = ctypes.CDLL(P.hip_runtime_path()[1])
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip.hipMemcpy(ctypes.c_void_p(addr), ctypes.c_void_p(mirror.data_ptr()), v4.nbytes, 3) == 0  # hipMemcpyDeviceToDevice
    torch.cuda.synchronize()
    assert A.revalue_device(addr) == 0
    i = A.value_map_info()
    assert i.revalues == before.revalues + 1 and i.last_kept_plans >= 1
    assert exported(A, np.float64)[3] == addr and A.spmv_info().device_resident == 1
    check_double(A, case, base, v4, x, y0, b, "revalue in place")
    i = A.value_map_info()
    assert (i.plan_builds, i.clean_builds) == (before.plan_builds, before.clean_builds)


@pytest.mark.parametrize("route", ["refresh", "revalue", "update"])
def test_behind_an_invalid_mirror(case, route):
    order, t0 = case["order"], case["val"]
    rng = np.random.default_rng(10)
    x, y0 = rng.uniform(-1, 1, M), rng.uniform(-1, 1, M)
    A = handle(case, 0, t0)
    assert A.spmv_info().device_resident == 1
    r, c = int(case["row"][order[5]]), int(case["ci"][5])
    assert L.aoclsparse_dset_value(A.h, r, c, 0.125) == 0 and A.spmv_info().device_resident == 0
    t1 = scaled(t0, 21)
    st = {"refresh": lambda: A.refresh_from_coo_device(dev(t1)), "revalue": lambda: A.revalue_device(dev(t1[order])),
          "update": lambda: A.update_values_device(dev(t1[order]))}[route]()
    assert st == 0, P.STATUS.get(st, st)
    print(route, "device_resident behind an invalid mirror:", A.spmv_info().device_resident)
    assert A.spmv_info().device_resident == RESIDENT_BEHIND_INVALID_MIRROR[route]
    y = mv(A, x, y0)
    so, yr = oracle.dcsrmv(-1, 0, 1.3, M, len(t1), t1[order], case["ci"], case["rp"], x, -0.4, y0)
    bound = (np.diff(case["rp"]) + 24) * EPS64 * abs_row_sums(case["rp"], case["ci"], t1[order], x) + 1e-300
    assert so == 0 and np.all(np.abs(y - yr) <= bound), route
    assert same_bits(y, mv(fresh(case, 0, t1[order]), x, y0)) and A.spmv_info().device_resident == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_value_type(case, dtype):
    """refresh, revalue, one solve (for c / z the conjugate-transposed one too): against a fresh handle bit for bit, the clean
    values against the oracle's (it moves values and never computes with them)"""
    order = case["order"]
    t0 = typed(case["val"], dtype)
    rng = np.random.default_rng(12)
    b = typed(rng.uniform(-1, 1, M), dtype, seed=4)
    ops = [P.OP_NONE] + ([P.OP_CONJ_TRANSPOSE] if np.dtype(dtype).kind == "c" else [])
    A = handle(case, 0, t0)
    assert A.clean_device() == 0
    old = [solve(A, P.FILL_LOWER, op, b) for op in ops]
    t1 = typed(scaled(case["val"], 31), dtype, seed=5)
    assert A.refresh_from_coo_device(dev(t1)) == 0
    assert A.clean_device() == 0
    mid = [solve(A, P.FILL_LOWER, op, b) for op in ops]
    F = fresh(case, 0, t1[order])
    for op, got, was in zip(ops, mid, old):
        assert same_bits(got, solve(F, P.FILL_LOWER, op, b)) and not same_bits(got, was), ("refresh", op)
    v2, before = typed(scaled(case["val"], 32), dtype, seed=6)[order], A.value_map_info()
    assert A.revalue_device(dev(v2)) == 0
    F = fresh(case, 0, v2)
    for op, was in zip(ops, mid):
        got = solve(A, P.FILL_LOWER, op, b)
        assert same_bits(got, solve(F, P.FILL_LOWER, op, b)) and not same_bits(got, was), ("revalue", op)
    i = A.value_map_info()
    assert (i.plan_builds, i.clean_builds) == (before.plan_builds, before.clean_builds) and i.last_kept_plans == len(ops)
    c = export_clean(A, dtype)
    o, want = oracle_clean_values(M, 0, case["rp"], case["ci"], v2)
    assert c[6] and np.array_equal(c[1], o["ptr"]) and np.array_equal(c[2], o["ind"]) and same_bits(c[3], want)
    assert same_bits(fetch(A.export_device()["val"], len(v2), dtype), v2)


# ---- every kind of copy on one handle ---------------------------------------------------------------------------------------------------
# The handles above hold the triplet map, a clean copy with its map, the diagonal and the mapped TRSV plans.  Here a handle holds,
# besides those, a device-built symmetric operator with its source map, a host-built triangular operator without one, and the
# SELL-64 copy of its own plan: handle "a" is the file's handle (its clean CSR is a mapped COPY), handle "b" is over the same grid with a
# full diagonal and sorted rows (its clean CSR is the user's arrays).  Each value change is followed by every observer there is
# (OBSERVED below), by the operators and copies being asked for again, and by the checks of the tests above.
EPS = {np.dtype(t): float(np.finfo(t).eps) for t in DTYPES}
STEPS = {"a": ["revalue", "refresh", "update", "revalue"], "b": ["revalue", "update", "revalue"]}


class Setup:
    """one handle of `kind` and value type, its descriptors and operands, and how a fresh handle over the same arrays is made"""

    def __init__(self, case, kind, dtype):
        self.kind, self.dtype, self.order = kind, np.dtype(dtype), case["order"]
        if kind == "a":
            self.rp, self.ci, self.r0 = case["rp"], case["ci"], case["val"][case["order"]]
        else:
            _, rp, ci, v = laplace5(GRID)
            self.rp, self.ci = np.asarray(rp, np.int32), np.asarray(ci, np.int32)
            self.r0 = v * np.random.default_rng(41).uniform(0.5, 1.5, len(v))
        self.v0 = typed(self.r0, dtype)  # (r0: the real values they are made from)
        rng = np.random.default_rng(13)
        self.x, self.y0, self.b = (typed(rng.uniform(-1, 1, M), dtype, seed=s) for s in (7, 8, 9))
        self.dgen, self.dsym = P.Descr(), P.Descr(mtype=P.TYPE_SYMMETRIC, fill=P.FILL_LOWER)
        self.dtri = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=P.FILL_UPPER)
        # the symmetric operator of the lower triangle as a CSR of its own, for the oracle: entry q of the handle's arrays, or its mirror
        rows = np.repeat(np.arange(M), np.diff(self.rp))
        low, strict = np.flatnonzero(self.ci <= rows), np.flatnonzero(self.ci < rows)
        r, c = np.concatenate([rows[low], self.ci[strict]]), np.concatenate([self.ci[low], rows[strict]])
        by = np.lexsort((c, r))
        self.sym_src, self.sym_ci = np.concatenate([low, strict])[by], c[by].astype(np.int32)
        self.sym_rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=M))]).astype(np.int32)
        if kind == "a":
            self.A = handle(case, 0, self.triplets(self.v0))
        else:
            self.A = self.fresh(self.v0, hint=False)
            assert self.A.keep_value_maps() == 0
        self.hint(self.A)

    def triplets(self, v):
        t = np.empty_like(v)
        t[self.order] = v
        return t

    def hint(self, A):
        assert L.aoclsparse_set_mv_hint(A.h, P.OP_NONE, self.dgen.h, 100) == 0

    def fresh(self, v, hint=True):
        F = P.Matrix.from_device(0, M, M, len(v), dev(self.rp), dev(self.ci), dev(v))
        assert F.status == 0, P.STATUS.get(F.status, F.status)
        if hint:
            self.hint(F)
            assert L.aoclsparse_optimize(F.h) == 0
        return F

    def arm(self):
        """whatever a value change has dropped that only a call of its own brings back with a map"""
        A = self.A
        if self.kind == "a":
            assert A.clean_device() == 0
        assert A.build_operator_device(self.dsym) == 0
        assert L.aoclsparse_optimize(A.h) == 0

    def observed(self):
        def fields(i):
            return tuple(int(getattr(i, k)) for k, _ in i._fields_)

        A = self.A
        return (fields(A.value_map_info()), fields(A.operator_info(self.dsym)), fields(A.operator_info(self.dtri)),
                fields(A.sell_keep_info(P.OP_NONE)), int(A.spmv_info().device_resident))

    def change(self, route, v):
        A = self.A
        st = {"revalue": lambda: A.revalue_device(dev(v)), "update": lambda: A.update_values_device(dev(v)),
              "refresh": lambda: A.refresh_from_coo_device(dev(self.triplets(v)))}[route]()
        assert st == 0, (route, P.STATUS.get(st, st))

    def against_the_oracle(self, d, y, v, what):
        """the bound of the tests above, (len + 24) eps sum |a||x| per row, with the eps of the value type; the oracle computes in
        double (oracle.dcsrmv for a real type, oracle.zmv for a complex one)"""
        if d is self.dsym:
            rp, ci, vv = self.sym_rp, self.sym_ci, v[self.sym_src]
        else:
            rp, ci, vv = self.rp, self.ci, v
        rows = np.repeat(np.arange(M), np.diff(rp))
        if self.dtype.kind == "c":
            yr, _ = oracle.zmv("n", "general", "lower", "non_unit", 0, 1.25 + 0.5j, M, M, rp, ci, vv, self.x, -0.5 + 0.25j, self.y0)
        else:
            so, yr = oracle.dcsrmv(-1, 0, 1.25, M, len(vv), vv.astype(np.float64), ci, rp, self.x.astype(np.float64), -0.5,
                                   self.y0.astype(np.float64))
            assert so == 0
        scale = np.bincount(rows, np.abs(vv).astype(np.float64) * np.abs(self.x[ci]).astype(np.float64), minlength=M)
        bound = (np.diff(rp) + 24) * EPS[self.dtype] * scale + 1e-300
        print(what, "max |got - oracle| / bound =", float(np.max(np.abs(y - yr) / bound)))
        assert np.all(np.abs(y - yr) <= bound), (what, "against the oracle")

    def check(self, v, what):
        """the checks of check_double for the handle's value type, and the products with the two operators"""
        A, F, dt = self.A, self.fresh(v), self.dtype
        for name, d in (("mv", self.dgen), ("symmetric mv", self.dsym), ("triangular mv", self.dtri)):
            y = op_mv(A, d, P.OP_NONE, self.x, self.y0)
            if d is not self.dtri:
                self.against_the_oracle(d, y, v, (what, name))
            assert same_bits(y, op_mv(F, d, P.OP_NONE, self.x, self.y0)), (what, name, "against a fresh handle")
        H = type("Arrays", (), dict(m=M, base=0, row_ptr=self.rp, col_ind=self.ci))
        for fill, op in (LOWER_N, UPPER_N):
            got = solve(A, fill, op, self.b)
            if dt == np.float64:
                assert np.array_equal(got, _trsv_expect(H, fill, op, True, 0.75, self.b, 0)(v)), (what, "solve against the oracle", fill)
            assert same_bits(got, solve(F, fill, op, self.b)), (what, "solve against a fresh handle", fill)
        erp, eci, ev, _ = exported(A, dt)
        assert np.array_equal(erp, self.rp) and np.array_equal(eci, self.ci) and same_bits(ev, v), (what, "exported CSR")
        o, want = oracle_clean_values(M, 0, self.rp, self.ci, v)
        c, cf = export_clean(A, dt), export_clean(F, dt)
        assert c[6] == (self.kind == "a") and np.array_equal(c[1], o["ptr"]) and np.array_equal(c[2], o["ind"]), (what, "clean CSR")
        assert same_bits(c[3], want), (what, "clean values")
        assert all(np.array_equal(c[k], cf[k]) for k in (1, 2, 4, 5)) and same_bits(c[3], cf[3]), (what, "clean CSR against a fresh handle")


# What the observers showed on the commit before the kept set became one value, the same for the four value types: per handle one
# entry for the set-up and two per step of STEPS -- right behind the value change, and after everything has been asked for again
# and checked.  Each entry: (ValueMapInfo, OperatorInfo of the symmetric operator, OperatorInfo of the triangular one,
# SellKeepInfo, device_resident), the fields in the order of their structs.
OBSERVED = {
    "a": [
        ((56, 1, 1, 2, 0, 2, 1, 0, 16968), (80, 1, 1, 1, 441, 441, 2121, 0, 1, 1, 8484, 1, 1, 0),
         (80, 1, 0, 0, 441, 441, 1281, 0, 1, 1, 0, 1, 1, 0), (56, 1, 1, 1, 0, 1, 1, 0, 0), 1),
        ((56, 1, 1, 2, 2, 2, 1, 1, 16968), (80, 1, 1, 1, 441, 441, 2121, 1, 1, 1, 8484, 1, 1, 1),
         (80, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1), (56, 1, 0, 1, 0, 1, 1, 0, 0), 1),
        ((56, 1, 1, 2, 2, 2, 1, 1, 16968), (80, 1, 1, 1, 441, 441, 2121, 1, 1, 2, 8484, 1, 2, 1),
         (80, 1, 0, 0, 441, 441, 1281, 1, 1, 1, 0, 1, 2, 1), (56, 1, 1, 2, 0, 1, 2, 0, 0), 1),
        ((56, 1, 0, 0, 2, 2, 1, 1, 0), (80, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 2, 3),
         (80, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 2, 3), (56, 0, 0, 2, 0, 1, 2, 0, 0), 1),
        ((56, 1, 1, 2, 2, 4, 2, 1, 16968), (80, 1, 1, 1, 441, 441, 2121, 1, 1, 1, 8484, 2, 3, 3),
         (80, 1, 0, 0, 441, 441, 1281, 1, 1, 1, 0, 2, 3, 3), (56, 1, 1, 1, 0, 2, 3, 0, 0), 1),
        ((56, 1, 0, 0, 2, 4, 2, 1, 0), (80, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 2, 3, 5),
         (80, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 2, 3, 5), (56, 0, 0, 1, 0, 2, 3, 0, 0), 1),
        ((56, 1, 1, 2, 2, 6, 3, 1, 16968), (80, 1, 1, 1, 441, 441, 2121, 1, 1, 1, 8484, 3, 4, 5),
         (80, 1, 0, 0, 441, 441, 1281, 1, 1, 1, 0, 3, 4, 5), (56, 1, 1, 1, 0, 3, 4, 0, 0), 1),
        ((56, 1, 1, 2, 2, 6, 3, 2, 16968), (80, 1, 1, 1, 441, 441, 2121, 1, 1, 1, 8484, 3, 4, 6),
         (80, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 3, 4, 6), (56, 1, 0, 1, 0, 3, 4, 0, 0), 1),
        ((56, 1, 1, 2, 2, 6, 3, 2, 16968), (80, 1, 1, 1, 441, 441, 2121, 1, 1, 2, 8484, 3, 5, 6),
         (80, 1, 0, 0, 441, 441, 1281, 1, 1, 1, 0, 3, 5, 6), (56, 1, 1, 2, 0, 3, 5, 0, 0), 1),
    ],
    "b": [
        ((56, 1, 1, 2, 0, 2, 1, 0, 8484), (80, 1, 1, 1, 441, 441, 2121, 0, 1, 1, 8484, 1, 1, 0),
         (80, 1, 0, 0, 441, 441, 1281, 0, 1, 1, 0, 1, 1, 0), (56, 1, 1, 1, 0, 1, 1, 0, 0), 1),
        ((56, 1, 1, 2, 2, 2, 1, 1, 8484), (80, 1, 1, 1, 441, 441, 2121, 1, 1, 1, 8484, 1, 1, 1),
         (80, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1), (56, 1, 0, 1, 0, 1, 1, 0, 0), 1),
        ((56, 1, 1, 2, 2, 2, 1, 1, 8484), (80, 1, 1, 1, 441, 441, 2121, 1, 1, 2, 8484, 1, 2, 1),
         (80, 1, 0, 0, 441, 441, 1281, 1, 1, 1, 0, 1, 2, 1), (56, 1, 1, 2, 0, 1, 2, 0, 0), 1),
        ((56, 1, 1, 0, 2, 2, 1, 1, 0), (80, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 2, 3),
         (80, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 2, 3), (56, 0, 0, 2, 0, 1, 2, 0, 0), 1),
        ((56, 1, 1, 2, 2, 4, 1, 1, 8484), (80, 1, 1, 1, 441, 441, 2121, 1, 1, 1, 8484, 2, 3, 3),
         (80, 1, 0, 0, 441, 441, 1281, 1, 1, 1, 0, 2, 3, 3), (56, 1, 1, 1, 0, 2, 3, 0, 0), 1),
        ((56, 1, 1, 2, 2, 4, 1, 2, 8484), (80, 1, 1, 1, 441, 441, 2121, 1, 1, 1, 8484, 2, 3, 4),
         (80, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 2, 3, 4), (56, 1, 0, 1, 0, 2, 3, 0, 0), 1),
        ((56, 1, 1, 2, 2, 4, 1, 2, 8484), (80, 1, 1, 1, 441, 441, 2121, 1, 1, 2, 8484, 2, 4, 4),
         (80, 1, 0, 0, 441, 441, 1281, 1, 1, 1, 0, 2, 4, 4), (56, 1, 1, 2, 0, 2, 4, 0, 0), 1),
    ],
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["a", "b"])
def test_every_kind_of_copy_at_once(case, kind, dtype):
    assert L.aoclsparse_mi355_set_option(P.OPTION_SELL, 1) == 0  # (a SELL-64 copy wherever the type has one, whatever the padding)
    try:
        S = Setup(case, kind, dtype)
        S.arm()
        S.check(S.v0, "set-up")
        seen, r = [S.observed()], S.r0
        for k, route in enumerate(STEPS[kind]):
            r = scaled(r, 50 + k)
            v = typed(r, dtype, seed=60 + k)
            S.change(route, v)
            seen.append(S.observed())
            S.arm()
            S.check(v, (k, route))
            seen.append(S.observed())
    finally:
        assert L.aoclsparse_mi355_set_option(P.OPTION_SELL, -1) == 0
    print("OBSERVED[%r] = %r" % (kind, seen))
    assert seen[1][3][1:3] == (1, 0), seen[1][3]  # (not vacuous: the revalue has kept the structure of the SELL-64 copy, stale)
    for k, (got, want) in enumerate(zip(seen, OBSERVED[kind])):
        assert got == want, (k, got, want)
    assert len(seen) == len(OBSERVED[kind])


# ---- the copies of the TRANSPOSE after a host ?set_value ------------------------------------------------------------------------------------
# The drop list resets the SELL-64 and the blocked-ELL copy of plan_trans next to those of plan_user; the products below read
# them (the observer says so before the value changes) and are compared with the oracle on the new values.
def test_transposed_sell_copy_after_set_value():
    from test_gpu_value_updates import mutate, options

    m, rp, ci, v = laplace5(40)
    v = v * np.random.default_rng(71).uniform(0.5, 1.5, len(v))
    A, d = P.Matrix(0, m, m, rp, ci, v), P.Descr()
    rng = np.random.default_rng(72)
    x, y0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)

    def run():
        y = dev(y0)
        assert P.dmv(P.OP_TRANSPOSE, 1.3, A, d, dev(x), -0.4, y) == 0
        torch.cuda.synchronize()
        return y.cpu().numpy()

    def check(vals, what):
        so, yr = oracle.dcsrmvt(0, 1.3, m, m, vals, ci, rp, x, -0.4, y0)
        st, cp, ri, cv = oracle.dcsr2csc(m, m, len(vals), 0, 0, rp, ci, vals)
        bound = (np.diff(cp) + 24) * EPS64 * abs_row_sums(np.asarray(cp), np.asarray(ri), np.asarray(cv), x) + 1e-300
        got = run()
        assert so == 0 and st == 0 and np.all(np.abs(got - yr) <= bound), (what, float(np.max(np.abs(got - yr) / bound)))
        return got

    with options(sell=1):
        assert L.aoclsparse_set_mv_hint(A.h, P.OP_TRANSPOSE, d.h, 100) == 0 and L.aoclsparse_optimize(A.h) == 0
        old = check(A.val.copy(), "old values")
        # (get_sell_keep_info answers for the handle's own operator alone; spmv_info shows the copy of the transpose)
        assert A.spmv_info(P.OP_TRANSPOSE).sell_slices > 0, "the transposed product did not run on a SELL-64 copy"
        new = check(mutate("set_value", A, m // 2), "new values")
    assert not np.array_equal(old, new)


def test_transposed_blocked_ell_copy_after_set_value():
    import standins
    from test_gpu_value_updates import mutate

    m, rp, ci, v = standins.block_dense(12, 16, 16, seed=5)
    A, d, n = P.Matrix(0, m, m, rp, ci, v), P.Descr(), 64
    rng = np.random.default_rng(73)
    B, C0 = rng.uniform(-1, 1, (m, n)), rng.uniform(-1, 1, (m, n))

    def oracle_product(vals, Bm, Cm):
        """2 A^T Bm + 0.5 Cm by oracle.dcsrmm over the CSC arrays (the CSR of A^T), and the entries per row of A^T"""
        st, cp, ri, cv = oracle.dcsr2csc(m, m, len(vals), 0, 0, rp, ci, vals)
        so, Cr = oracle.dcsrmm("col", 2.0, 0, cv, ri, cp, m, np.ascontiguousarray(Bm.T).ravel(), n, m, 0.5,
                               np.ascontiguousarray(Cm.T).ravel(), m)
        assert st == 0 and so == 0
        return np.asarray(Cr).reshape(n, m).T, np.diff(np.asarray(cp))

    def check(vals, what):
        C = C0.copy().ravel()
        assert P.dcsrmm(P.OP_TRANSPOSE, 2.0, A, d, P.ORDER_ROW, B.ravel(), n, n, 0.5, C, n) == 0
        ref, length = oracle_product(vals, B, C0)
        scale, _ = oracle_product(np.abs(vals), np.abs(B), np.abs(C0))  # alpha sum |a||b| + |beta c| per entry of C
        # the bound of this file's products, (len + 24) eps of the sum of magnitudes, with the length of the row of A^T
        bound = (length[:, None] + 24) * EPS64 * scale + 1e-300
        got = C.reshape(m, n)
        print(what, "max |got - oracle| / bound =", float(np.max(np.abs(got - ref) / bound)))
        assert np.all(np.abs(got - ref) <= bound), what
        return C

    old = check(A.val.copy(), "old values")
    assert A.spmv_info(P.OP_TRANSPOSE).mm_bell_width > 0, "the transposed product did not run on a blocked-ELL copy"
    new = check(mutate("set_value", A, m // 2), "new values")
    assert not np.array_equal(old, new)
