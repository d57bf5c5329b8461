"""GPU tier: aoclsparse_mi355_keep_value_maps / ?revalue_device / get_value_map_info (include/aoclsparse_mi355.h) -- new values in
HBM reach the clean CSR, the diagonal and the TRSV plans through the value maps the handle keeps, and nothing is analysed again.

Every case compares against a TWIN: a fresh host-created handle over the same structure with the new values, solved the ordinary
way; equality is bit for bit.  Double-precision cases also compare with the oracle's serial chain on oracle.dcsr_optimize of the
new values, as tests/test_gpu_value_updates.py does.  Every case asserts (a) the result on the old values was right, (b) the
result after revalue_device equals the twin's and differs from (a), (c) plan_builds and clean_builds did not move across
revalue + solve, (d) trsv_info reads the same before and after.  The fall-backs of group 7 are the control: there (c) DOES move."""
import ctypes
from ctypes import byref

import numpy as np
import pytest

import oracle
from clean_cases import HostMatrix, export_clean, same_bits
from order_cases import Raw
from util import pkg, triangular_system, trsv_schedule

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from test_gpu_trsv_blocks import node_mesh  # noqa: E402
from test_gpu_value_updates import KIND, _trsv_expect, _unclean, scaled  # noqa: E402

P = pkg()
L = P.lib()

SUCCESS, NOT_IMPLEMENTED, INVALID_POINTER, INVALID_SIZE, WRONG_TYPE = 0, 1, 2, 3, 9
assert [P.STATUS[k] for k in (1, 2, 3, 9)] == ["not_implemented", "invalid_pointer", "invalid_size", "wrong_type"]
LOWER_N, UPPER_T = (P.FILL_LOWER, P.OP_NONE), (P.FILL_UPPER, P.OP_TRANSPOSE)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    yield
    L.aoclsparse_mi355_set_pointer_mode(P.PTR_AUTO)


def dev(a):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a if len(a) else np.zeros(1, a.dtype)).cuda()
    torch.cuda.synchronize()
    return t


def device_matrix(base, m, rp, ci, v, maps=True):
    """a handle over arrays in HBM (Matrix.from_device), with the keep_value_maps flag set unless maps=False"""
    A = P.Matrix.from_device(base, m, m, len(v), dev(np.asarray(rp, np.int32)), dev(np.asarray(ci, np.int32)), dev(v))
    assert A.status == 0, P.STATUS.get(A.status, A.status)
    if maps:
        assert A.keep_value_maps() == SUCCESS
        assert A.value_map_info().enabled == 1
    return A


def solve(A, fill, op, unit, b, kid=None, alpha=0.75):
    """one ?trsv of the handle's value type -> x (host)"""
    d = P.Descr(base=A.base, mtype=P.TYPE_TRIANGULAR, fill=fill, diag=P.DIAG_UNIT if unit else P.DIAG_NON_UNIT)
    if b.dtype == np.complex128:
        x = np.zeros_like(b)
        st = L.aoclsparse_ztrsv(op, P.CDouble(alpha, alpha / 3), A.h, d.h, P._ptr(b), P._ptr(x))
        assert st == 0, P.STATUS.get(st, st)
        return x
    xd = torch.full((A.m,), 7.0, dtype=torch.float64 if b.dtype == np.float64 else torch.float32, device="cuda")
    st = (P.dtrsv if b.dtype == np.float64 else P.strsv)(op, alpha, A, d, dev(b), xd, kid=kid)
    assert st == 0, P.STATUS.get(st, st)
    torch.cuda.synchronize()
    return xd.cpu().numpy()


def info_of(A, fill, op):
    i = A.trsv_info(fill, op)
    return tuple(getattr(i, k) for k, _ in P.TrsvInfo._fields_)


def builds(A):
    i = A.value_map_info()
    return i.plan_builds, i.clean_builds


def revalue(A, v2):
    i0 = A.value_map_info()
    st = A.revalue_device(dev(v2))
    assert st == SUCCESS, P.STATUS.get(st, st)
    i1 = A.value_map_info()
    assert i1.revalues == i0.revalues + 1 and (i1.plan_builds, i1.clean_builds) == (i0.plan_builds, i0.clean_builds)
    return i1


def kept_protocol(A, Hold, Hnew, v2, cases, oracle_of=None):
    """cases: [(key, run(handle) -> x, (fill, op))].  (a) every case on the old values against the old twin (and the oracle on the
    old values), revalue_device once, (b) every case again against the new twin (and the oracle on the new values), (c), (d)."""
    old = {}
    for key, run, _ in cases:
        old[key] = run(A)
        assert np.array_equal(old[key], run(Hold)), ("old values", key)
        if oracle_of:
            assert np.array_equal(old[key], oracle_of(key, False)), ("old values against the oracle", key)
    before = builds(A)
    infos = {fo: info_of(A, *fo) for _, _, fo in cases}
    assert A.value_map_info().plans_mapped == len(infos), (A.value_map_info().plans_mapped, len(infos))
    i1 = revalue(A, v2)
    assert i1.last_kept_plans == len(infos) and i1.plans_mapped == len(infos)
    for key, run, fo in cases:
        got = run(A)
        assert np.array_equal(got, run(Hnew)), ("new values against the twin", key)
        if oracle_of:
            assert np.array_equal(got, oracle_of(key, True)), ("new values against the oracle", key)
        assert not np.array_equal(got, old[key]), ("the new values did not reach the output", key)
        assert info_of(A, *fo) == infos[fo], ("another plan after the revalue", key)
    assert builds(A) == before, ("something was analysed again", before, builds(A))


# --------------------------------------------------------------------------------------------------
# 1. every schedule
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", [0, 1, 2, 3, 4])
def test_every_schedule_double(sched):
    """all four (fill, op) plans of one handle, unit and non-unit, kid 0 and 3, carried over by ONE revalue"""
    m = 3000
    rp, ci, v = triangular_system(7 + sched, m, 4, band=60)
    v2 = scaled(v, 99)
    b = np.random.default_rng(11).uniform(-1, 1, m)
    with trsv_schedule(P, sched):
        A, Hold, Hnew = device_matrix(0, m, rp, ci, v), P.Matrix(0, m, m, rp, ci, v.copy()), P.Matrix(0, m, m, rp, ci, v2.copy())
        cases = [((fill, op, unit, kid), (lambda X, f=fill, o=op, u=unit, k=kid: solve(X, f, o, u, b, k)), (fill, op))
                 for fill, op in KIND for unit in (False, True) for kid in (0, 3)]

        def oracle_of(key, new):
            fill, op, unit, kid = key
            return _trsv_expect(Hold, fill, op, unit, 0.75, b, kid)(v2 if new else v)

        kept_protocol(A, Hold, Hnew, v2, cases, oracle_of)
        assert A.value_map_info().map_bytes >= 4 * (len(v) - m)  # every strict entry once at least


@pytest.mark.parametrize("sched", [0, 1, 2, 3, 4])
def test_every_schedule_float(sched):
    m = 3000
    rp, ci, v = triangular_system(7 + sched, m, 4, band=60, dtype=np.float32)
    v2 = scaled(v, 99)
    b = np.random.default_rng(11).uniform(-1, 1, m).astype(np.float32)
    with trsv_schedule(P, sched):
        A, Hold, Hnew = device_matrix(0, m, rp, ci, v), P.Matrix(0, m, m, rp, ci, v.copy()), P.Matrix(0, m, m, rp, ci, v2.copy())
        cases = [((fill, op, unit), (lambda X, f=fill, o=op, u=unit: solve(X, f, o, u, b, 0)), (fill, op))
                 for fill, op in KIND for unit in (False, True)]
        kept_protocol(A, Hold, Hnew, v2, cases)


@pytest.mark.parametrize("sched", [0, 1, 2, 3, 4])
def test_every_schedule_complex(sched):
    """op = N, T and H on both fills: H is the only user of the conjugating gather"""
    m = 3000
    rp, ci, vr = triangular_system(7 + sched, m, 4, band=60)
    rng = np.random.default_rng(17)
    v = (vr * np.exp(0.4j * rng.uniform(-1, 1, len(vr)))).astype(np.complex128)
    v2 = scaled(v, 99) * np.exp(0.2j * rng.uniform(-1, 1, len(vr)))
    b = (rng.uniform(-1, 1, m) + 1j * rng.uniform(-1, 1, m)).astype(np.complex128)
    with trsv_schedule(P, sched):
        A, Hold, Hnew = device_matrix(0, m, rp, ci, v), HostMatrix(0, m, m, rp, ci, v), HostMatrix(0, m, m, rp, ci, v2)
        assert Hold.status == 0 and Hnew.status == 0
        cases = [((fill, op), (lambda X, f=fill, o=op: solve(X, f, o, False, b)), (fill, op))
                 for fill in (P.FILL_LOWER, P.FILL_UPPER) for op in (P.OP_NONE, P.OP_TRANSPOSE, P.OP_CONJ_TRANSPOSE)]
        kept_protocol(A, Hold, Hnew, v2, cases)
        # the conjugated plans are plans of their own, and their values differ from the transposed ones'
        assert not np.array_equal(solve(A, P.FILL_LOWER, P.OP_TRANSPOSE, False, b), solve(A, P.FILL_LOWER, P.OP_CONJ_TRANSPOSE, False, b))


# --------------------------------------------------------------------------------------------------
# 2. / 3. the mesh factor: the two-level schedule; row and block layouts of one plan together
# --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mesh():
    nodes = 3000
    m, rp, ci, v = node_mesh(5, nodes, 40, np.full(nodes, 5))
    return m, rp, ci, v, scaled(v, 99), np.random.default_rng(3).uniform(-1, 1, m)


@pytest.fixture
def forced_chunks():
    assert L.aoclsparse_mi355_set_option(P.OPTION_TRSV_CHUNKS, 1) == 0
    yield
    assert L.aoclsparse_mi355_set_option(P.OPTION_TRSV_CHUNKS, -1) == 0


def test_two_level_schedule(forced_chunks, mesh):
    m, rp, ci, v, v2, b = mesh
    with trsv_schedule(P, 5):
        A, Hold, Hnew = device_matrix(0, m, rp, ci, v), P.Matrix(0, m, m, rp, ci, v.copy()), P.Matrix(0, m, m, rp, ci, v2.copy())
        cases = [((fill, op), (lambda X, f=fill, o=op: solve(X, f, o, False, b, None, 1.0)), (fill, op)) for fill, op in (LOWER_N, UPPER_T)]

        def oracle_of(key, new):
            return _trsv_expect(Hold, key[0], key[1], False, 1.0, b, 0)(v2 if new else v)

        for fill, op in (LOWER_N, UPPER_T):
            solve(A, fill, op, False, b, None, 1.0)
            assert A.trsv_info(fill, op).chunks >= 2
        kept_protocol(A, Hold, Hnew, v2, cases, oracle_of)
        for fill, op in (LOWER_N, UPPER_T):
            assert A.trsv_info(fill, op).chunks >= 2


def test_row_and_block_layouts_together(mesh):
    """the automatic schedule builds the block layout, a forced row schedule then adds the row layout late: one plan, two maps"""
    m, rp, ci, v, v2, b = mesh
    A, Hold, Hnew = device_matrix(0, m, rp, ci, v), P.Matrix(0, m, m, rp, ci, v.copy()), P.Matrix(0, m, m, rp, ci, v2.copy())

    def auto(X):
        return solve(X, P.FILL_LOWER, P.OP_NONE, False, b)

    def rows(X):
        with trsv_schedule(P, 1):
            return solve(X, P.FILL_LOWER, P.OP_NONE, False, b)

    x_auto = auto(A)
    assert A.trsv_info(P.FILL_LOWER, P.OP_NONE).blocks > 0
    one = A.value_map_info()
    x_rows = rows(A)
    two = A.value_map_info()
    strict = int(np.sum(ci < np.repeat(np.arange(m), np.diff(rp))))
    assert one.plans_mapped == two.plans_mapped == 1 and two.plan_builds == one.plan_builds + 1
    assert two.map_bytes - one.map_bytes >= 4 * strict and one.map_bytes >= 4 * strict and two.map_bytes >= 8 * strict
    assert np.array_equal(x_auto, auto(Hold)) and np.array_equal(x_rows, rows(Hold))
    before, info = builds(A), info_of(A, P.FILL_LOWER, P.OP_NONE)
    assert revalue(A, v2).last_kept_plans == 1
    y_auto, y_rows = auto(A), rows(A)
    ref = _trsv_expect(Hold, P.FILL_LOWER, P.OP_NONE, False, 0.75, b, 0)(v2)
    assert np.array_equal(y_auto, auto(Hnew)) and np.array_equal(y_rows, rows(Hnew))
    assert np.array_equal(y_auto, ref) and np.array_equal(y_rows, ref) and not np.array_equal(y_auto, x_auto)
    assert builds(A) == before and info_of(A, P.FILL_LOWER, P.OP_NONE) == info
    assert A.value_map_info().plans_mapped == 1 and A.value_map_info().map_bytes == two.map_bytes


# --------------------------------------------------------------------------------------------------
# 4. the clean copy through every route of clean_csr_device
# --------------------------------------------------------------------------------------------------
def _drop_diag(rp, ci, v, q):
    keep = np.ones(len(ci), bool)
    keep[rp[q] + int(np.nonzero(ci[rp[q]:rp[q + 1]] == q)[0][0])] = False
    counts = np.add.reduceat(keep.astype(int), rp[:-1])
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), ci[keep].copy(), v[keep].copy()


def _long_rows():
    """lower triangular, 2,200 rows, every row in DESCENDING column order; rows of 40, 300 and 2,100 entries among short ones: the
    lane, LDS and radix paths of the row sort and the wavefront path of the mark kernel"""
    rng = np.random.default_rng(41)
    m, want = 2200, {100: 40, 600: 300, 2150: 2100}
    rows, vals = [], []
    for i in range(m):
        k = min(i, want.get(i, int(rng.integers(0, 4)) + 1) - 1) if i in want else min(i, int(rng.integers(0, 4)))
        c = np.sort(np.concatenate([rng.choice(i, size=k, replace=False) if k else np.zeros(0, np.int64), [i]]))[::-1]
        x = rng.uniform(-0.5, 0.5, len(c)) / max(1, len(c) // 8)
        x[0] = rng.uniform(2.0, 4.0) * rng.choice([-1.0, 1.0])  # (the diagonal comes first in a descending row)
        rows.append(c), vals.append(x)
    assert sorted(len(r) for r in rows)[-3:] == [40, 300, 2100]
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int32)
    return rp, np.concatenate(rows).astype(np.int32), np.concatenate(vals)


def _clean_case(name):
    if name == "long rows":
        return _long_rows()
    m = 2000
    rp, ci, v = _unclean(21, m, name == "both") if name != "missing" else triangular_system(21, m, 4, band=40)
    return _drop_diag(rp, ci, v, m // 3) if name == "missing" else (rp, ci, v)


_clean_cache = {}


def clean_case(name):
    if name not in _clean_cache:
        _clean_cache[name] = _clean_case(name)
    return _clean_cache[name]


def oracle_clean_values(m, base, rp, ci, v):
    """the clean value array of oracle.dcsr_optimize for values of any type: it moves values and never computes with them, so a
    float array goes through as doubles (exact) and a complex one as its two halves"""
    v = np.asarray(v)
    parts = [v.real, v.imag] if np.iscomplexobj(v) else [v]
    outs = []
    for p in parts:
        o = oracle.dcsr_optimize(m, m, len(p), base, rp, ci, np.ascontiguousarray(p, dtype=np.float64))
        assert o["status"] == 0
        outs.append(o)
    val = outs[0]["val"] + 1j * outs[1]["val"] if len(outs) == 2 else outs[0]["val"]
    return outs[0], np.ascontiguousarray(val.astype(v.dtype))


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("name", ["missing", "reversed", "both", "long rows"])
def test_clean_copy_follows(name, base):
    rp0, ci0, vd = clean_case(name)
    m, rp, ci = len(rp0) - 1, rp0 + base, ci0 + base
    rng = np.random.default_rng(23)
    phase = np.exp(0.3j * rng.uniform(-1, 1, len(vd)))
    b = np.random.default_rng(5).uniform(-1, 1, m)
    for dtype in (np.float32, np.float64, np.complex128):
        v = (vd * phase).astype(dtype) if np.dtype(dtype).kind == "c" else vd.astype(dtype)
        v2 = np.ascontiguousarray(scaled(v, 99) * (phase ** 0.5 if np.dtype(dtype).kind == "c" else 1)).astype(dtype)
        A = device_matrix(base, m, rp, ci, v)
        assert A.clean_device() == SUCCESS
        i0 = A.value_map_info()
        assert i0.clean_map == 1 and i0.clean_builds == 1 and i0.map_bytes >= 4 * len(v)
        c0, d0 = export_clean(A, dtype), A.export_diag()
        assert c0[6], "a clean COPY"
        o, want0 = oracle_clean_values(m, base, rp, ci, v)
        assert same_bits(c0[3], want0), "old clean values"
        if dtype == np.float64:  # (a) the solve on the old values: unit diagonal, one entry may be missing
            Hold, Hnew = P.Matrix(base, m, m, rp, ci, v.copy()), P.Matrix(base, m, m, rp, ci, v2.copy())
            x0 = solve(A, P.FILL_LOWER, P.OP_NONE, True, b)
            assert np.array_equal(x0, solve(Hold, P.FILL_LOWER, P.OP_NONE, True, b))
            info = info_of(A, P.FILL_LOWER, P.OP_NONE)
        before = builds(A)
        revalue(A, v2)
        c1, d1 = export_clean(A, dtype), A.export_diag()
        assert np.array_equal(d0["idiag"], d1["idiag"]) and np.array_equal(d0["iurow"], d1["iurow"]) and d1["is_internal"]
        assert c1[0] == c0[0] and np.array_equal(c1[1], c0[1]) and np.array_equal(c1[2], c0[2])
        _, want1 = oracle_clean_values(m, base, rp, ci, v2)
        assert np.array_equal(c1[1], o["ptr"]) and np.array_equal(c1[2], o["ind"])
        assert same_bits(c1[3], want1), ("new clean values", name, base, dtype)
        assert not same_bits(c1[3], c0[3])
        if dtype == np.float64:
            x1 = solve(A, P.FILL_LOWER, P.OP_NONE, True, b)
            assert np.array_equal(x1, solve(Hnew, P.FILL_LOWER, P.OP_NONE, True, b)) and not np.array_equal(x1, x0)
            assert np.array_equal(x1, _trsv_expect(Hold, P.FILL_LOWER, P.OP_NONE, True, 0.75, b, 0)(v2))
            assert info_of(A, P.FILL_LOWER, P.OP_NONE) == info
        assert builds(A) == before
        assert A.value_map_info().clean_map == 1


def test_clean_copy_non_unit_solves_read_the_regathered_diagonal():
    """a reversed row only (nothing missing): the non-unit solve reads dev_diag, which clean_device() left in HBM with its map"""
    rp, ci, v = clean_case("reversed")
    m, v2 = len(rp) - 1, scaled(clean_case("reversed")[2], 99)
    b = np.random.default_rng(5).uniform(-1, 1, m)
    A, Hold, Hnew = device_matrix(0, m, rp, ci, v), P.Matrix(0, m, m, rp, ci, v.copy()), P.Matrix(0, m, m, rp, ci, v2.copy())
    assert A.clean_device() == SUCCESS
    cases = [((fill, op), (lambda X, f=fill, o=op: solve(X, f, o, False, b)), (fill, op)) for fill, op in KIND]
    kept_protocol(A, Hold, Hnew, v2, cases, lambda key, new: _trsv_expect(Hold, key[0], key[1], False, 0.75, b, 0)(v2 if new else v))


# --------------------------------------------------------------------------------------------------
# 5. two revalues in a row, then ?trsm
# --------------------------------------------------------------------------------------------------
def test_two_revalues_then_trsm():
    m, k = 2000, 4
    rp, ci, v = triangular_system(33, m, 4, band=50)
    v2, v3 = scaled(v, 99), scaled(v, 100)
    Bm = np.random.default_rng(6).uniform(-1, 1, m * k)
    d = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=P.FILL_LOWER)

    def trsm(X):
        Xo = np.zeros(m * k)
        assert L.aoclsparse_dtrsm(P.OP_NONE, 1.5, X.h, d.h, P.ORDER_COLUMN, P._ptr(Bm), k, m, P._ptr(Xo), m) == 0
        return Xo

    A, Hold, Hnew = device_matrix(0, m, rp, ci, v), P.Matrix(0, m, m, rp, ci, v.copy()), P.Matrix(0, m, m, rp, ci, v3.copy())
    x0 = trsm(A)
    assert np.array_equal(x0, trsm(Hold))
    before, info = builds(A), info_of(A, P.FILL_LOWER, P.OP_NONE)
    assert revalue(A, v2).plans_mapped == 1
    i2 = revalue(A, v3)  # the maps survived the first one
    assert i2.plans_mapped == 1 and i2.last_kept_plans == 1 and i2.revalues == 2
    x1 = trsm(A)
    assert np.array_equal(x1, trsm(Hnew)) and not np.array_equal(x1, x0)
    ref = np.concatenate([_trsv_expect(Hold, P.FILL_LOWER, P.OP_NONE, False, 1.5, Bm[j * m:(j + 1) * m], 0)(v3) for j in range(k)])
    assert np.array_equal(x1, ref)
    assert builds(A) == before and info_of(A, P.FILL_LOWER, P.OP_NONE) == info


# --------------------------------------------------------------------------------------------------
# 6. what is not kept is dropped, and rebuilt from the new values
# --------------------------------------------------------------------------------------------------
def test_what_is_not_kept():
    m = 1500
    rp, ci, v = triangular_system(44, m, 4, band=30)
    v2 = scaled(v, 99)
    rng = np.random.default_rng(8)
    b, x0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)
    A, Hnew = device_matrix(0, m, rp, ci, v), P.Matrix(0, m, m, rp, ci, v2.copy())
    dg, ds = P.Descr(), P.Descr(mtype=P.TYPE_SYMMETRIC, fill=P.FILL_LOWER)

    def everything(X):
        out = []
        for d in (dg, ds):
            y = dev(x0)
            assert P.dmv(P.OP_NONE, 1.25, X, d, dev(b), -0.5, y) == 0
            torch.cuda.synchronize()
            out.append(y.cpu().numpy())
        x = x0.copy()
        assert L.aoclsparse_dsymgs(P.OP_NONE, X.h, dg.h, 1.0, P._ptr(b), P._ptr(x)) == 0
        out.append(x)
        x = x0.copy()
        assert L.aoclsparse_dsorv(0, dg.h, X.h, 0.7, 1.0, P._ptr(x), P._ptr(b)) == 0
        out.append(x)
        return out

    old = everything(A)  # (the symmetric expansion, the plans and the diagonal exist now)
    assert np.array_equal(A.export()["val"], v)
    revalue(A, v2)
    new, ref = everything(A), everything(Hnew)
    for what, g, r, o in zip(("dmv general", "dmv symmetric", "dsymgs", "dsorv forward"), new, ref, old):
        assert np.array_equal(g, r), what
        assert not np.array_equal(g, o), what
    e = A.export()
    assert e["status"] == 0 and np.array_equal(e["val"], v2) and np.array_equal(e["col_ind"], ci)


# --------------------------------------------------------------------------------------------------
# 7. fall-backs: results equal to the twin's, and the plan IS built again (the control for counter (c))
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["flag never set", "plans built before the flag", "host clean copy", "update_values_device"])
def test_fall_backs_rebuild(how):
    m = 2000
    rp, ci, v = _unclean(21, m, False) if how == "host clean copy" else triangular_system(21, m, 4, band=40)
    v2 = scaled(v, 99)
    b = np.random.default_rng(5).uniform(-1, 1, m)
    A = device_matrix(0, m, rp, ci, v, maps=how not in ("flag never set", "plans built before the flag"))
    Hold, Hnew = P.Matrix(0, m, m, rp, ci, v.copy()), P.Matrix(0, m, m, rp, ci, v2.copy())
    if how == "host clean copy":  # the forward-SOR hint: aoclsparse_optimize builds the clean copy on the host, without a map
        d = P.Descr()
        assert L.aoclsparse_set_sorv_hint(A.h, d.h, 0, 1) == 0 and L.aoclsparse_optimize(A.h) == 0
        assert A.export_diag()["is_internal"] and A.value_map_info().clean_map == 0
    x0 = solve(A, P.FILL_LOWER, P.OP_NONE, False, b)
    assert np.array_equal(x0, solve(Hold, P.FILL_LOWER, P.OP_NONE, False, b))
    if how == "plans built before the flag":
        assert A.keep_value_maps() == SUCCESS
    i0 = A.value_map_info()
    assert i0.plans_mapped == (1 if how in ("host clean copy", "update_values_device") else 0)
    st = A.update_values_device(dev(v2)) if how == "update_values_device" else A.revalue_device(dev(v2))
    assert st == SUCCESS
    i1 = A.value_map_info()
    assert i1.plans_mapped == 0 and i1.last_kept_plans == 0 and i1.plan_builds == i0.plan_builds
    assert i1.revalues == (0 if how == "update_values_device" else 1)
    x1 = solve(A, P.FILL_LOWER, P.OP_NONE, False, b)
    assert np.array_equal(x1, solve(Hnew, P.FILL_LOWER, P.OP_NONE, False, b)) and not np.array_equal(x1, x0)
    i2 = A.value_map_info()
    assert i2.plan_builds == i0.plan_builds + 1, "the plan was built again"
    if how == "host clean copy":
        assert i2.clean_builds == i0.clean_builds + 1
    assert i2.plans_mapped == (0 if how == "flag never set" else 1)  # built under the flag this time


@pytest.mark.parametrize("how", ["aoclsparse_order_mat", "order_mat_device", "aoclsparse_mi355_invalidate", "keep_value_maps(0)"])
def test_what_releases_the_maps(how):
    m = 2000
    rp, ci, v = triangular_system(21, m, 4, band=40)
    b = np.random.default_rng(5).uniform(-1, 1, m)
    A, H = device_matrix(0, m, rp, ci, v), P.Matrix(0, m, m, rp, ci, v.copy())
    x0 = solve(A, P.FILL_LOWER, P.OP_NONE, False, b)
    i0 = A.value_map_info()
    assert i0.plans_mapped == 1 and i0.map_bytes > 0
    if how == "aoclsparse_order_mat":
        assert L.aoclsparse_order_mat(A.h) == 0
    elif how == "order_mat_device":
        assert A.order_device() == 0
    elif how == "aoclsparse_mi355_invalidate":
        assert L.aoclsparse_mi355_invalidate(A.h) == 0
    else:
        assert A.keep_value_maps(False) == SUCCESS
        assert A.value_map_info().enabled == 0
    i1 = A.value_map_info()
    assert i1.plans_mapped == 0 and i1.map_bytes == 0
    x1 = solve(A, P.FILL_LOWER, P.OP_NONE, False, b)
    assert np.array_equal(x1, x0) and np.array_equal(x1, solve(H, P.FILL_LOWER, P.OP_NONE, False, b))


# --------------------------------------------------------------------------------------------------
# 8. statuses: all decided before the device is touched, the handle unchanged
# --------------------------------------------------------------------------------------------------
def test_statuses():
    m = 60
    rp, ci, v = triangular_system(3, m, 3, band=10)
    b = np.random.default_rng(2).uniform(-1, 1, m)
    A = device_matrix(0, m, rp, ci, v)
    x0 = solve(A, P.FILL_LOWER, P.OP_NONE, False, b)
    i0 = A.value_map_info()
    t, n = dev(scaled(v, 5)), len(v)
    host = scaled(v, 5)
    rv = L.aoclsparse_mi355_drevalue_device
    assert rv(None, n, P._ptr(t)) == INVALID_POINTER
    assert rv(A.h, n, None) == INVALID_POINTER
    assert rv(A.h, n - 1, P._ptr(t)) == INVALID_SIZE and rv(A.h, n + 1, P._ptr(t)) == INVALID_SIZE
    for wrong in (L.aoclsparse_mi355_srevalue_device, L.aoclsparse_mi355_crevalue_device, L.aoclsparse_mi355_zrevalue_device):
        assert wrong(A.h, n, P._ptr(t)) == WRONG_TYPE
    assert rv(A.h, n, P._ptr(host)) == INVALID_POINTER  # a host array
    i1 = A.value_map_info()
    assert (i1.revalues, i1.plans_mapped, i1.plan_builds, i1.map_bytes) == (0, i0.plans_mapped, i0.plan_builds, i0.map_bytes)
    assert np.array_equal(solve(A, P.FILL_LOWER, P.OP_NONE, False, b), x0) and A.value_map_info().plan_builds == i0.plan_builds
    # handles whose first representation is not a CSR in HBM's reach
    i32 = lambda *a: np.array(a, np.int32)  # noqa: E731
    w = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    others = [("coo", Raw("aoclsparse_create_dcoo", 0, 3, 3, 5, i32(0, 0, 1, 2, 2), i32(1, 0, 1, 2, 0), w.copy()), 5),
              ("csc", Raw("aoclsparse_create_dcsc", 0, 3, 3, 5, i32(0, 2, 4, 5), i32(2, 0, 1, 0, 2), w.copy()), 5),
              ("tcsr", P.TcsrMatrix(0, 3, i32(0, 1, 2, 4), i32(0, 1, 0, 2), np.array([1.0, 2.0, 5.0, 4.0]),
                                    i32(0, 2, 3, 4), i32(0, 1, 1, 2), np.array([1.0, 3.0, 2.0, 4.0])), None),
              ("bsr", P.BsrMatrix(0, P.ORDER_ROW, 2, 2, 2, i32(0, 2, 3), i32(1, 0, 1), np.arange(12.0)), None)]
    t5 = dev(np.arange(16.0))
    for name, X, nnz in others:
        assert X.status == 0, name
        got = [rv(X.h, k, P._ptr(t5)) for k in ([nnz] if nnz is not None else range(0, 13))]
        assert NOT_IMPLEMENTED in got and set(got) <= {NOT_IMPLEMENTED, INVALID_SIZE}, (name, got)
        if name in ("tcsr", "bsr"):
            assert L.aoclsparse_mi355_keep_value_maps(X.h, 1) == NOT_IMPLEMENTED, name
    # empty handles
    for mm, rpe in ((0, i32(0)), (4, i32(0, 0, 0, 0, 0))):
        E = P.Matrix.from_device(0, mm, mm, 0, dev(rpe), dev(i32(0)), dev(np.zeros(1)))
        assert E.status == 0 and E.keep_value_maps() == SUCCESS
        assert rv(E.h, 0, P._ptr(t5)) == SUCCESS and E.value_map_info().revalues == 1
    # the flag and the observer
    assert L.aoclsparse_mi355_keep_value_maps(None, 1) == INVALID_POINTER
    info = P.ValueMapInfo(struct_size=ctypes.sizeof(P.ValueMapInfo))
    assert L.aoclsparse_mi355_get_value_map_info(None, byref(info)) == INVALID_POINTER
    assert L.aoclsparse_mi355_get_value_map_info(A.h, None) == INVALID_POINTER
    small = P.ValueMapInfo(struct_size=ctypes.sizeof(ctypes.c_size_t) + 4, plans_mapped=-7)
    assert L.aoclsparse_mi355_get_value_map_info(A.h, byref(small)) == SUCCESS
    assert small.enabled == 1 and small.plans_mapped == -7  # no more than struct_size bytes are written
    small.struct_size = 2
    assert L.aoclsparse_mi355_get_value_map_info(A.h, byref(small)) == INVALID_SIZE
