"""GPU tier: aoclsparse_mi355_build_operator_device / get_operator_info / export_operator (include/aoclsparse_mi355.h) -- the
operator of a symmetric, Hermitian or triangular descriptor built in HBM from the clean CSR, and kept through ?revalue_device.

The reference of every comparison is the HOST route: a TWIN handle over the same arrays whose operator ensure_derived builds with
build_derived (derived.cpp) at its first product.  Every comparison is bit for bit (np.array_equal on integers, same_bits on
values); there is no tolerance anywhere."""
import ctypes
from ctypes import byref

import numpy as np
import pytest

from clean_cases import HostMatrix, same_bits
from util import laplace5, pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

P = pkg()
L = P.lib()

SUCCESS, NOT_IMPLEMENTED = 0, 1
DTYPE = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}
N, T, H = P.OP_NONE, P.OP_TRANSPOSE, P.OP_CONJ_TRANSPOSE
CAP = 2048  # the longest mirrored row segment the device segment sort takes


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    yield
    L.aoclsparse_mi355_set_pointer_mode(P.PTR_AUTO)


@pytest.fixture
def forced_sell():
    """every operator of a real type gets its SELL-64 copy whatever the padding: the refill of a kept structure is then observable"""
    assert L.aoclsparse_mi355_set_option(P.OPTION_SELL, 1) == 0
    yield
    assert L.aoclsparse_mi355_set_option(P.OPTION_SELL, -1) == 0


def dev(a):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a if len(a) else np.zeros(1, a.dtype)).cuda()
    torch.cuda.synchronize()
    return t


def device_matrix(base, m, n, rp, ci, v, maps=False):
    """a handle over arrays in HBM (0-based arrays in, moved to `base`), with the keep_value_maps flag set when maps"""
    A = P.Matrix.from_device(base, m, n, len(v), dev(np.asarray(rp, np.int32) + base), dev(np.asarray(ci, np.int32) + base), dev(v))
    assert A.status == 0, P.STATUS.get(A.status, A.status)
    if maps:
        assert A.keep_value_maps() == SUCCESS
    return A


def twin(base, m, n, rp, ci, v):
    X = HostMatrix(base, m, n, np.asarray(rp, np.int32) + base, np.asarray(ci, np.int32) + base, v)
    assert X.status == 0, P.STATUS.get(X.status, X.status)
    return X


def mv(X, d, op, x, y0):
    """y = alpha op(X) x + beta y0 through the handle's own ?mv, host vectors"""
    letter, y = X._letter(), y0.copy()
    if letter in "ds":
        st = (P.dmv if letter == "d" else P.smv)(op, 1.25, X, d, x, -0.5, y)
    else:
        C = P.CDouble if letter == "z" else P.CFloat
        a, b = C(1.25, 0.5), C(-0.5, 0.25)
        st = getattr(L, "aoclsparse_%smv" % letter)(op, byref(a), X.h, d.h, P._ptr(x), byref(b), P._ptr(y))
    assert st == 0, P.STATUS.get(st, st)
    return y


def vectors(X, op, seed=5):
    """(x, y0) of the handle's value type for op(X)"""
    rng, dt = np.random.default_rng(seed), DTYPE[X._letter()]
    nx, ny = (X.n, X.m) if op == N else (X.m, X.n)

    def vec(k):
        r = rng.uniform(-1, 1, k)
        return (r + 1j * rng.uniform(-1, 1, k)).astype(dt) if np.dtype(dt).kind == "c" else r.astype(dt)

    return vec(nx), vec(ny)


def values(nnz, dtype, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.5, 1.5, nnz) * rng.choice([-1.0, 1.0], nnz)
    if np.dtype(dtype).kind == "c":
        v = v * np.exp(1j * rng.uniform(0.2, 1.2, nnz))
    return np.ascontiguousarray(v.astype(dtype))


def rescaled(v, seed):
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.5, 1.5, len(v))
    if np.iscomplexobj(v):
        f = f * np.exp(0.3j * rng.uniform(-1, 1, len(v)))
    return np.ascontiguousarray((v * f).astype(v.dtype))


# --------------------------------------------------------------------------------------------------
# the edge matrix: sorted rows; the strict LOWER triangle holds exactly col0 / 33 / 32 / 31 entries in columns 0 .. 3 (the
# wavefront sorter's cap, and either side of the lane sorter's cap), one row of 129 and one of 128 strict entries side by side near
# the end (either side of the row walk's wavefront threshold), a few short random rows; the strict UPPER triangle is its mirror
# image, so the upper fills meet the same edges.  Unless `full`: four rows are empty and three more lack their diagonal entry (the
# clean CSR is then a copy).
# --------------------------------------------------------------------------------------------------
_edge = {}


def edge_matrix(m, col0, full=False):
    key = (m, col0, full)
    if key in _edge:
        return _edge[key]
    rng = np.random.default_rng(1000 + m + col0)
    empty = set() if full else set(range(col0 + 50, col0 + 54))
    nodiag = set() if full else {50, m // 3, m - 40} | empty
    long_rows = {m - 10: 129, m - 9: 128}
    assert col0 + 54 < m - 10 and 100 + 129 < col0
    low = {(r, 0) for r in range(1, col0 + 1)}
    low |= {(r, 1) for r in range(2, 35)} | {(r, 2) for r in range(3, 35)} | {(r, 3) for r in range(4, 35)}
    for r, k in long_rows.items():
        low |= {(r, c) for c in range(100, 100 + k)}
    for r in range(6, m):
        if r in empty or r in long_rows:
            continue
        pool = [c for c in rng.integers(4, r, size=int(rng.integers(0, 4))) if c not in empty]
        low |= {(r, int(c)) for c in pool}
    lr, lc = np.array(sorted(low)).T
    cnt = np.bincount(lc, minlength=m)
    assert list(cnt[:4]) == [col0, 33, 32, 31], cnt[:4]
    per_row = np.bincount(lr, minlength=m)
    assert per_row[m - 10] == 129 and per_row[m - 9] == 128 and all(per_row[r] == 0 for r in empty)
    dg = np.array([i for i in range(m) if i not in nodiag])
    rows = np.concatenate([lr, dg, lc])
    cols = np.concatenate([lc, dg, lr])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    up = np.bincount(rows[cols > rows], minlength=m)
    assert list(up[:4]) == [col0, 33, 32, 31] and np.array_equal(np.bincount(cols[cols > rows], minlength=m), per_row)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int32)
    _edge[key] = (rp, cols.astype(np.int32))
    return _edge[key]


KEYS = {"symmetric lower": (P.TYPE_SYMMETRIC, P.FILL_LOWER, N), "symmetric upper": (P.TYPE_SYMMETRIC, P.FILL_UPPER, N),
        "lower N": (P.TYPE_TRIANGULAR, P.FILL_LOWER, N), "lower T": (P.TYPE_TRIANGULAR, P.FILL_LOWER, T),
        "upper N": (P.TYPE_TRIANGULAR, P.FILL_UPPER, N), "upper T": (P.TYPE_TRIANGULAR, P.FILL_UPPER, T)}


def same_operator(A, X, d, op, what=""):
    """export_operator of the two handles: the three arrays themselves"""
    a, x = A.export_operator(d, op), X.export_operator(d, op)
    assert a["status"] == 0 and x["status"] == 0, (what, a["status"], x["status"])
    assert (a["rows"], a["cols"], a["nnz"]) == (x["rows"], x["cols"], x["nnz"]), what
    assert np.array_equal(a["row_ptr"], x["row_ptr"]), (what, "row_ptr")
    assert np.array_equal(a["col_ind"], x["col_ind"]), (what, "col_ind")
    assert same_bits(a["val"], x["val"]), (what, "val")
    return a


def built_like_the_twin(A, X, d, op, what=""):
    """build on the device, one product of the twin builds on the host: info, arrays, one product"""
    i0 = A.operator_info(d, op)
    assert (i0.present, i0.device_builds, i0.host_builds) == (0, 0, 0)
    st = A.build_operator_device(d, op)
    assert st == SUCCESS, (what, P.STATUS.get(st, st))
    i1 = A.operator_info(d, op)
    assert (i1.present, i1.built_on_device, i1.device_builds, i1.host_builds) == (1, 1, 1, 0), what
    assert A.build_operator_device(d, op) == SUCCESS and A.operator_info(d, op).device_builds == 1  # it exists: nothing is done
    x, y0 = vectors(X, op)
    want = mv(X, d, op, x, y0)
    ix = X.operator_info(d, op)
    assert (ix.present, ix.built_on_device, ix.device_builds, ix.host_builds) == (1, 0, 0, 1), what
    e = same_operator(A, X, d, op, what)
    assert (i1.rows, i1.cols, i1.nnz) == (e["rows"], e["cols"], e["nnz"])
    assert same_bits(mv(A, d, op, x, y0), want), (what, "product")
    assert A.operator_info(d, op).host_builds == 0  # the product found the operator
    return e


# --------------------------------------------------------------------------------------------------
# 1. structure, every key
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", ["d", "s"])
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("diag", [P.DIAG_NON_UNIT, P.DIAG_UNIT, P.DIAG_ZERO])
@pytest.mark.parametrize("key", list(KEYS))
def test_structure_every_key(key, diag, base, letter):
    m = 2400  # m % 256 = 96, m % 64 = 32: the last workgroup and the last wavefront are partial
    rp, ci = edge_matrix(m, CAP)
    v = values(len(ci), DTYPE[letter], 3)
    mtype, fill, op = KEYS[key]
    d = P.Descr(base=base, mtype=mtype, fill=fill, diag=diag)
    A, X = device_matrix(base, m, m, rp, ci, v), twin(base, m, m, rp, ci, v)
    e = built_like_the_twin(A, X, d, op, (key, diag, base, letter))
    on_diag = e["col_ind"] == np.repeat(np.arange(e["rows"]), np.diff(e["row_ptr"]))
    if diag == P.DIAG_UNIT:
        assert int(on_diag.sum()) == m and np.all(e["val"][on_diag] == 1)
    if diag == P.DIAG_ZERO:
        assert not on_diag.any()


# --------------------------------------------------------------------------------------------------
# 2. complex: symmetric, Hermitian (the conjugated mirror), triangular with op = H
# --------------------------------------------------------------------------------------------------
CKEYS = {"symmetric lower": (P.TYPE_SYMMETRIC, P.FILL_LOWER, N), "symmetric upper": (P.TYPE_SYMMETRIC, P.FILL_UPPER, N),
         "hermitian lower": (P.TYPE_HERMITIAN, P.FILL_LOWER, N), "hermitian upper": (P.TYPE_HERMITIAN, P.FILL_UPPER, N),
         "lower H": (P.TYPE_TRIANGULAR, P.FILL_LOWER, H), "upper H": (P.TYPE_TRIANGULAR, P.FILL_UPPER, H)}


@pytest.mark.parametrize("letter", ["z", "c"])
@pytest.mark.parametrize("diag", [P.DIAG_NON_UNIT, P.DIAG_UNIT])
@pytest.mark.parametrize("key", list(CKEYS))
def test_complex(key, diag, letter):
    m = 600
    rp, ci = edge_matrix(m, 520)
    v = values(len(ci), DTYPE[letter], 4)
    mtype, fill, op = CKEYS[key]
    d = P.Descr(mtype=mtype, fill=fill, diag=diag)
    A, X = device_matrix(0, m, m, rp, ci, v), twin(0, m, m, rp, ci, v)
    e = built_like_the_twin(A, X, d, op, (key, diag, letter))
    if mtype == P.TYPE_TRIANGULAR:  # H folds to T: the same operator answers both
        assert A.operator_info(d, T).present == 1 and A.operator_info(d, N).present == 0
    if mtype == P.TYPE_HERMITIAN and diag == P.DIAG_UNIT:  # the mirrored half is the conjugate of the stored one
        D = np.zeros((m, m), DTYPE[letter])
        D[np.repeat(np.arange(m), np.diff(e["row_ptr"])), e["col_ind"]] = e["val"]
        assert np.array_equal(D, D.conj().T) and np.any(D.imag != 0)


# --------------------------------------------------------------------------------------------------
# 3. rectangular triangular operators: the col < rows filter and dim = min(m, n)
# --------------------------------------------------------------------------------------------------
def rectangular(m, n, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(m):
        c = set(int(x) for x in rng.integers(0, n, size=int(rng.integers(0, 7))))
        if i < n and i % 11:
            c.add(i)
        rows.append(sorted(c))
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int32)
    return rp, np.array([c for r in rows for c in r], np.int32)


@pytest.mark.parametrize("op", [N, T])
@pytest.mark.parametrize("fill", [P.FILL_LOWER, P.FILL_UPPER])
@pytest.mark.parametrize("shape", [(300, 200), (200, 300)])
def test_rectangular_triangular(shape, fill, op):
    m, n = shape
    rp, ci = rectangular(m, n, 9)
    v = values(len(ci), np.float64, 6)
    for diag in (P.DIAG_NON_UNIT, P.DIAG_UNIT):
        d = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=fill, diag=diag)
        A, X = device_matrix(0, m, n, rp, ci, v), twin(0, m, n, rp, ci, v)
        e = built_like_the_twin(A, X, d, op, (shape, fill, op, diag))
        assert (e["rows"], e["cols"]) == ((m, n) if op == N else (n, m))


# --------------------------------------------------------------------------------------------------
# 4. declined: a mirrored segment one entry over the cap
# --------------------------------------------------------------------------------------------------
def test_declined():
    m = 2400
    rp, ci = edge_matrix(m, CAP + 1)
    v = values(len(ci), np.float64, 3)
    d = P.Descr(mtype=P.TYPE_SYMMETRIC, fill=P.FILL_LOWER)
    A, X = device_matrix(0, m, m, rp, ci, v, maps=True), twin(0, m, m, rp, ci, v)
    assert A.build_operator_device(d) == NOT_IMPLEMENTED
    i = A.operator_info(d)
    assert (i.present, i.device_builds, i.host_builds, i.map_bytes) == (0, 0, 0, 0)
    freed = ctypes.c_size_t(1 << 60)
    assert L.aoclsparse_mi355_release_staging(byref(freed)) == 0 and freed.value < (1 << 60)  # nothing of the call holds staging
    x, y0 = vectors(X, N)
    assert same_bits(mv(A, d, N, x, y0), mv(X, d, N, x, y0))
    i = A.operator_info(d)
    assert (i.present, i.built_on_device, i.device_builds, i.host_builds) == (1, 0, 0, 1)
    same_operator(A, X, d, N)
    # the upper fill of the same matrix mirrors rows, not columns: its longest segment is short, and it is built
    du = P.Descr(mtype=P.TYPE_SYMMETRIC, fill=P.FILL_UPPER)
    assert A.build_operator_device(du) == SUCCESS and A.operator_info(du).built_on_device == 1
    mv(X, du, N, x, y0)
    same_operator(A, X, du, N)


# --------------------------------------------------------------------------------------------------
# 5. kept through ?revalue_device
# --------------------------------------------------------------------------------------------------
def unclean(rp, ci, v, m):
    """row m/2 in descending order and row m/5 without its diagonal entry: the handle's clean CSR is a sorted, completed COPY"""
    rp, ci, v = rp.copy(), ci.copy(), v.copy()
    r = m // 2
    assert rp[r + 1] - rp[r] >= 2
    ci[rp[r]:rp[r + 1]] = ci[rp[r]:rp[r + 1]][::-1].copy()
    v[rp[r]:rp[r + 1]] = v[rp[r]:rp[r + 1]][::-1].copy()
    q = m // 5
    keep = np.ones(len(ci), bool)
    keep[rp[q] + int(np.nonzero(ci[rp[q]:rp[q + 1]] == q)[0][0])] = False
    rp2 = np.concatenate([[0], np.cumsum(np.add.reduceat(keep.astype(int), rp[:-1]))]).astype(np.int32)
    return rp2, ci[keep].copy(), v[keep].copy(), keep


def kept_case(letter, copy, m=600):
    """-> (structure, values, two descriptors with their operations): the symmetric (Hermitian for a complex type) operator of the
    lower triangle and the unit triangular operator of op(upper triangle)"""
    rp, ci = edge_matrix(m, 520, full=True)
    v = values(len(ci), DTYPE[letter], 8)
    keep = np.ones(len(ci), bool)
    if copy:
        rp, ci, v, keep = unclean(rp, ci, v, m)
    cplx = letter in "cz"
    ops = [(P.Descr(mtype=P.TYPE_HERMITIAN if cplx else P.TYPE_SYMMETRIC, fill=P.FILL_LOWER), N),
           (P.Descr(mtype=P.TYPE_TRIANGULAR, fill=P.FILL_UPPER, diag=P.DIAG_UNIT), H if cplx else T)]
    return rp, ci, v, ops


@pytest.mark.parametrize("letter", ["d", "s", "z"])
@pytest.mark.parametrize("copy", [False, True], ids=["own clean arrays", "clean_csr_device copy"])
def test_kept_through_revalue(forced_sell, copy, letter):
    m = 600
    rp, ci, v, ops = kept_case(letter, copy)
    v2, v3, v4 = rescaled(v, 21), rescaled(v, 22), rescaled(v, 23)
    A = device_matrix(0, m, m, rp, ci, v, maps=True)
    if copy:
        assert A.clean_device() == SUCCESS and A.value_map_info().clean_map == 1
    Hold, Hnew, Hlast = twin(0, m, m, rp, ci, v), twin(0, m, m, rp, ci, v2), twin(0, m, m, rp, ci, v4)
    real = letter in "ds"
    old, e_old, i_old = [], [], []
    for d, op in ops:
        e_old.append(built_like_the_twin(A, Hold, d, op, (copy, letter)) if op == N else None)
        if op != N:  # (the second operator of the handle: the counters of built_like_the_twin do not apply)
            assert A.build_operator_device(d, op) == SUCCESS
            x, y0 = vectors(Hold, op)
            assert same_bits(mv(A, d, op, x, y0), mv(Hold, d, op, x, y0))
            e_old[-1] = same_operator(A, Hold, d, op)
        x, y0 = vectors(Hold, op)
        old.append(mv(A, d, op, x, y0))
        i = A.operator_info(d, op)
        assert (i.present, i.built_on_device, i.mapped) == (1, 1, 1) and i.map_bytes == 4 * max(i.nnz, 1)
        assert i.sell_copy == (1 if real else 0)
        i_old.append(i)
    assert A.operator_info(ops[0][0]).device_builds == 2
    vm0 = A.value_map_info()
    assert A.revalue_device(dev(v2)) == SUCCESS
    vm1 = A.value_map_info()
    assert (vm1.revalues, vm1.plan_builds, vm1.clean_builds, vm1.map_bytes) == (vm0.revalues + 1, vm0.plan_builds, vm0.clean_builds, vm0.map_bytes)
    for k, (d, op) in enumerate(ops):
        i = A.operator_info(d, op)
        assert (i.present, i.built_on_device, i.mapped, i.followed) == (1, 1, 1, 2)
        assert (i.device_builds, i.host_builds, i.dropped_by_value_change) == (2, 0, 0)
        x, y0 = vectors(Hnew, op)
        want = mv(Hnew, d, op, x, y0)
        e = same_operator(A, Hnew, d, op, ("after the revalue", k))  # val: the NEW twin's
        assert np.array_equal(e["row_ptr"], e_old[k]["row_ptr"]) and np.array_equal(e["col_ind"], e_old[k]["col_ind"])
        assert not same_bits(e["val"], e_old[k]["val"])
        got = mv(A, d, op, x, y0)
        assert same_bits(got, want) and not same_bits(got, old[k]), ("after the revalue", k)
        i = A.operator_info(d, op)
        assert (i.device_builds, i.host_builds) == (2, 0)
        if real:  # the product refilled the kept SELL-64 structure: one values stage, no structure build
            assert i.sell_copy == 1 and i.sell_value_fills == i_old[k].sell_value_fills + 1, (k, i.sell_value_fills)
    # the unit diagonal is still ones
    e = A.export_operator(*ops[1])
    on_diag = e["col_ind"] == np.repeat(np.arange(e["rows"]), np.diff(e["row_ptr"]))
    assert int(on_diag.sum()) == m and np.all(e["val"][on_diag] == 1)
    # twice in a row, then the products
    assert A.revalue_device(dev(v3)) == SUCCESS and A.revalue_device(dev(v4)) == SUCCESS
    for d, op in ops:
        x, y0 = vectors(Hlast, op)
        want = mv(Hlast, d, op, x, y0)
        assert same_bits(mv(A, d, op, x, y0), want)
        same_operator(A, Hlast, d, op, "after two more")
        i = A.operator_info(d, op)
        assert (i.followed, i.device_builds, i.host_builds, i.dropped_by_value_change) == (2, 2, 0, 0)


# --------------------------------------------------------------------------------------------------
# 6. controls: not kept, rebuilt right
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["flag never set", "built by a product", "host clean copy", "update_values_device"])
def test_controls_rebuild(how):
    m = 600
    rp, ci, v, _ = kept_case("d", how == "host clean copy")
    v2 = rescaled(v, 21)
    d = P.Descr(mtype=P.TYPE_SYMMETRIC, fill=P.FILL_LOWER)
    A = device_matrix(0, m, m, rp, ci, v, maps=how != "flag never set")
    Hold, Hnew = twin(0, m, m, rp, ci, v), twin(0, m, m, rp, ci, v2)
    if how == "host clean copy":  # the forward-SOR hint: aoclsparse_optimize builds the clean copy on the host, without a map
        g = P.Descr()
        assert L.aoclsparse_set_sorv_hint(A.h, g.h, 0, 1) == 0 and L.aoclsparse_optimize(A.h) == 0
        assert A.export_diag()["is_internal"] and A.value_map_info().clean_map == 0
    x, y0 = vectors(Hold, N)
    if how != "built by a product":
        assert A.build_operator_device(d) == SUCCESS
    y_old = mv(A, d, N, x, y0)
    assert same_bits(y_old, mv(Hold, d, N, x, y0))
    same_operator(A, Hold, d, N)
    i0 = A.operator_info(d)
    assert i0.present == 1 and i0.built_on_device == (0 if how == "built by a product" else 1)
    assert i0.mapped == (1 if how in ("host clean copy", "update_values_device") else 0)
    st = A.update_values_device(dev(v2)) if how == "update_values_device" else A.revalue_device(dev(v2))
    assert st == SUCCESS
    i1 = A.operator_info(d)
    assert (i1.present, i1.mapped, i1.map_bytes, i1.followed) == (0, 0, 0, 0)
    assert i1.dropped_by_value_change == i0.dropped_by_value_change + 1
    y_new = mv(A, d, N, x, y0)
    assert same_bits(y_new, mv(Hnew, d, N, x, y0)) and not same_bits(y_new, y_old)
    i2 = A.operator_info(d)
    assert (i2.present, i2.built_on_device, i2.host_builds, i2.device_builds) == (1, 0, i0.host_builds + 1, i0.device_builds)
    same_operator(A, Hnew, d, N)


# --------------------------------------------------------------------------------------------------
# 7. what releases the map, and what the operator with it
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["aoclsparse_order_mat", "order_mat_device", "aoclsparse_mi355_invalidate", "keep_value_maps(0)"])
def test_releases(how):
    m = 600
    rp, ci, v, _ = kept_case("d", False)
    d = P.Descr(mtype=P.TYPE_SYMMETRIC, fill=P.FILL_LOWER)
    A, X = device_matrix(0, m, m, rp, ci, v, maps=True), twin(0, m, m, rp, ci, v)
    assert A.build_operator_device(d) == SUCCESS
    i0 = A.operator_info(d)
    assert (i0.present, i0.mapped) == (1, 1) and i0.map_bytes == 4 * i0.nnz
    if how == "aoclsparse_order_mat":
        assert L.aoclsparse_order_mat(A.h) == 0
    elif how == "order_mat_device":
        assert A.order_device() == 0
    elif how == "aoclsparse_mi355_invalidate":
        assert L.aoclsparse_mi355_invalidate(A.h) == 0
    else:
        assert A.keep_value_maps(False) == SUCCESS
    i1 = A.operator_info(d)
    assert (i1.present, i1.mapped, i1.map_bytes) == ((1, 0, 0) if how == "keep_value_maps(0)" else (0, 0, 0))
    assert i1.dropped_by_value_change == 0  # (no value has changed)
    x, y0 = vectors(X, N)
    assert same_bits(mv(A, d, N, x, y0), mv(X, d, N, x, y0))
    same_operator(A, X, d, N)
    if how == "keep_value_maps(0)":  # without its map the operator no longer follows: the next revalue drops it
        v2 = rescaled(v, 21)
        assert A.revalue_device(dev(v2)) == SUCCESS
        i2 = A.operator_info(d)
        assert (i2.present, i2.dropped_by_value_change) == (0, 1)
        Xn = twin(0, m, m, rp, ci, v2)
        assert same_bits(mv(A, d, N, x, y0), mv(Xn, d, N, x, y0))


# --------------------------------------------------------------------------------------------------
# 8. the other consumers: csrmm and the iterative solvers
# --------------------------------------------------------------------------------------------------
def test_csrmm_on_the_kept_operator():
    m, k = 600, 8
    rp, ci, v, _ = kept_case("d", False)
    v2 = rescaled(v, 21)
    d = P.Descr(mtype=P.TYPE_SYMMETRIC, fill=P.FILL_LOWER)
    A = device_matrix(0, m, m, rp, ci, v, maps=True)
    Hold, Hnew = twin(0, m, m, rp, ci, v), twin(0, m, m, rp, ci, v2)
    rng = np.random.default_rng(12)
    B, C0 = rng.uniform(-1, 1, m * k), rng.uniform(-1, 1, m * k)

    def mm(X, order):
        C = C0.copy()
        ld = m if order == P.ORDER_COLUMN else k
        assert P.dcsrmm(N, 1.5, X, d, order, B, k, ld, -0.25, C, ld) == 0
        return C

    assert A.build_operator_device(d) == SUCCESS
    old = {}
    for order in (P.ORDER_COLUMN, P.ORDER_ROW):
        old[order] = mm(A, order)
        assert same_bits(old[order], mm(Hold, order))
    assert A.revalue_device(dev(v2)) == SUCCESS
    for order in (P.ORDER_COLUMN, P.ORDER_ROW):
        got = mm(A, order)
        assert same_bits(got, mm(Hnew, order)) and not same_bits(got, old[order])
    i = A.operator_info(d)
    assert (i.present, i.built_on_device, i.followed, i.device_builds, i.host_builds) == (1, 1, 1, 1, 0)


def test_cg_on_the_kept_operator():
    """CG with the symmetric descriptor on the lower-stored Laplacian (16 on the diagonal: the rescaled matrix stays diagonally
    dominant): the twin's iterate and iteration count, before and after the revalue"""
    n, rp, ci, v = laplace5(40)
    v = np.where(v > 0, 16.0, v)
    keep = ci <= np.repeat(np.arange(n), np.diff(rp))
    lrp = np.concatenate([[0], np.cumsum(np.add.reduceat(keep.astype(int), rp[:-1]))]).astype(np.int32)
    lci, lv = ci[keep].copy(), v[keep].copy()
    lv2 = rescaled(lv, 31)
    d = P.Descr(mtype=P.TYPE_SYMMETRIC, fill=P.FILL_LOWER)
    b = np.random.default_rng(71).uniform(-1, 1, n)

    def cg(X):
        h = ctypes.c_void_p()
        assert L.aoclsparse_itsol_d_init(byref(h)) == 0
        try:
            for key, val in {"CG Rel Tolerance": 1e-9, "CG Abs Tolerance": 0.0, "CG Preconditioner": "None", "CG Iteration Limit": 500}.items():
                assert L.aoclsparse_itsol_option_set(h, key.encode(), str(val).encode()) == 0
            x, rinfo = np.zeros(n), np.zeros(100)
            assert L.aoclsparse_itsol_d_solve(h, n, X.h, d.h, P._ptr(b), P._ptr(x), P._ptr(rinfo), None, None, None) == 0
            return x, rinfo[30]
        finally:
            L.aoclsparse_itsol_destroy(byref(h))

    A = device_matrix(0, n, n, lrp, lci, lv, maps=True)
    assert A.build_operator_device(d) == SUCCESS
    x0, it0 = cg(A)
    r0, rit0 = cg(twin(0, n, n, lrp, lci, lv))
    assert same_bits(x0, r0) and it0 == rit0 and it0 > 1
    assert A.revalue_device(dev(lv2)) == SUCCESS
    x1, it1 = cg(A)
    r1, rit1 = cg(twin(0, n, n, lrp, lci, lv2))
    assert same_bits(x1, r1) and it1 == rit1 and not same_bits(x1, x0)
    i = A.operator_info(d)
    assert (i.present, i.built_on_device, i.followed, i.device_builds, i.host_builds) == (1, 1, 1, 1, 0)
