"""Small calls of every entry point that accepts host or device pointers, shared by tests/test_gpu_pointer_paths.py and
tools/staging_evidence.py.  A case is (modes, run, check): run(ctx) makes the call with its arrays placed by ctx (host arrays,
or torch device tensors) and returns {name: numpy array} of everything the call may write; check(out) holds the family's
oracle check and the sentinels.  Shapes are the smallest that cross a boundary: 70 rows (more than one 64-row slice), one long
row, leading dimensions with padding, strides with gaps."""
import ctypes

import numpy as np

from util import EPS64, banded_rows, pkg, random_csr  # (puts the repository root on sys.path)

import oracle  # noqa: E402

P = pkg()
SENTINEL = np.frombuffer(np.uint64(0x7FF8DEADBEEF1234).tobytes(), np.float64)[0]  # a NaN with a payload: compared as bits
M = 70


class Ctx:
    """mode 'host': numpy arrays; 'auto' / 'device': torch device tensors (the pointer mode is set by the caller)"""

    def __init__(self, mode):
        self.mode, self.keep = mode, []

    def put(self, a):
        a = np.ascontiguousarray(a).copy()
        if self.mode == "host":
            t = a
        else:
            import torch
            host = a.view(np.float32 if a.dtype == np.complex64 else np.float64) if a.dtype.kind == "c" else a
            t = torch.from_numpy(host).cuda()
        self.keep.append((t, a.dtype))
        return t

    def get(self, t):
        if isinstance(t, np.ndarray):
            return t
        import torch
        torch.cuda.synchronize()
        dt = next(d for k, d in self.keep if k is t)
        a = t.cpu().numpy()
        return a.view(dt) if np.dtype(dt).kind == "c" else a


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def tri_plus_long_row(dtype=np.float64, seed=3):
    """70 x 70, tridiagonal with a dominant diagonal, row 35 full (small entries): sorted rows, full diagonal"""
    rng = np.random.default_rng(seed)
    rows, vals = [], []
    for i in range(M):
        c = np.arange(M) if i == 35 else np.arange(max(0, i - 1), min(M, i + 2))
        v = rng.uniform(-1, 1, len(c)) * (0.01 if i == 35 else 1.0)
        v[c == i] = 4.0 + rng.uniform(0, 1)
        rows.append(c), vals.append(v)
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int32)
    ci, v = np.concatenate(rows).astype(np.int32), np.concatenate(vals)
    if np.dtype(dtype).kind == "c":
        v = v + 1j * rng.uniform(-0.5, 0.5, len(v))
    return rp, ci, v.astype(dtype)


def dense_of(rp, ci, v, n=M):
    D = np.zeros((len(rp) - 1, n), v.dtype)
    D[np.repeat(np.arange(len(rp) - 1), np.diff(rp)), ci] = v
    return D


def within(got, D, alpha, x, beta, y0, dtype):
    """componentwise forward bound of one chain per row: (L + 4) u (|alpha| |A| |x| + |beta| |y0|), u doubled for complex
    arithmetic (a complex multiply-add rounds four products and four sums)"""
    W = np.complex128 if np.dtype(dtype).kind == "c" else np.float64
    u = float(np.finfo(dtype).eps) * (2 if np.dtype(dtype).kind == "c" else 1)
    ex = W(alpha) * (D.astype(W) @ x.astype(W)) + (W(beta) * y0.astype(W) if beta != 0 else 0)
    L = np.count_nonzero(D, axis=1).max()
    bound = (L + 4) * u * (abs(alpha) * (np.abs(D) @ np.abs(x)) + abs(beta) * np.abs(np.nan_to_num(y0))) + 1e-300
    return bool(np.all(np.abs(got.astype(W) - ex) <= bound))


def exact_below_the_tree(got, want, rp):
    """double-precision products in the scalar order: a row of fewer than 32 entries (SPMV_TREE_MIN) is one lane's chain, bit for
    bit the reference's; a longer row is summed by a wavefront and carries the bound of within() instead"""
    short = np.diff(rp) < 32
    assert not short.all()  # the matrix has its long row
    bad = np.flatnonzero(short & (got != want))
    assert bad.size == 0, ("rows that differ from the oracle", bad, got[bad], want[bad])


class Handle:
    """CSR handle of any of the four types over host arrays it keeps alive"""

    def __init__(self, rp, ci, v, base=0, n=M):
        self.arrays = (np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32), np.ascontiguousarray(v))
        t = {np.dtype(np.float64): "d", np.dtype(np.float32): "s", np.dtype(np.complex128): "z", np.dtype(np.complex64): "c"}[v.dtype]
        self.h = ctypes.c_void_p()
        fn = getattr(P.lib(), "aoclsparse_create_%scsr" % t)
        st = fn(ctypes.byref(self.h), base, len(rp) - 1, n, len(v), *[P._ptr(a) for a in self.arrays])
        assert st == 0

    def __del__(self):
        try:
            P.lib().aoclsparse_destroy(ctypes.byref(self.h))
        except Exception:
            pass


CASES = {}
ALL = ("host", "auto", "device")


def case(name, modes=ALL):
    def reg(factory):
        CASES[name] = (modes, factory)
        return factory
    return reg


def scal(t, v):
    """scalar argument passed by pointer"""
    return np.array([v], {"d": np.float64, "s": np.float32, "z": np.complex128, "c": np.complex64}[t])


# ---- ?mv, ?csrmv, ?dotmv ---------------------------------------------------------------------------------------------------
def _mv_case(t, beta):
    dt = scal(t, 0).dtype
    rp, ci, v = tri_plus_long_row(dt)
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, M).astype(dt)
    y0 = rng.uniform(-1, 1, M).astype(dt) if beta != 0 else np.full(M, np.nan, dt)
    alpha = 1.5
    A, d = Handle(rp, ci, v), P.Descr()
    a, b = scal(t, alpha), scal(t, beta)

    def run(c):
        xd, yd = c.put(x), c.put(y0)
        st = getattr(P.lib(), "aoclsparse_%smv" % t)(P.OP_NONE, P._ptr(a), A.h, d.h, P._ptr(xd), P._ptr(b), P._ptr(yd))
        assert st == 0, P.STATUS[st]
        return {"y": c.get(yd)}

    def check(o):
        assert np.all(np.isfinite(o["y"]))
        if t == "d":
            st, yr = oracle.dcsrmv(-1, 0, alpha, M, len(v), v, ci, rp, x, beta, np.nan_to_num(y0))
            assert st == 0
            exact_below_the_tree(o["y"], yr, rp)
        assert within(o["y"], dense_of(rp, ci, v), alpha, x, beta, y0, dt)
    return run, check


for _t in "dszc":
    case("%smv" % _t)(lambda _t=_t: _mv_case(_t, -0.5))
    case("%smv_beta0_nan_y" % _t)(lambda _t=_t: _mv_case(_t, 0.0))


def _csrmv_case(t, beta, mixed):
    dt = scal(t, 0).dtype
    rp, ci, v = tri_plus_long_row(dt)
    rng = np.random.default_rng(12)
    x = rng.uniform(-1, 1, M).astype(dt)
    y0 = rng.uniform(-1, 1, M).astype(dt) if beta != 0 else np.full(M, np.nan, dt)
    alpha, d = 0.75, P.Descr()
    a, b = scal(t, alpha), scal(t, beta)

    def run(c):
        vd, cd, rd = c.put(v), c.put(ci), c.put(rp)
        host = Ctx("host")
        xd, yd = (host.put(x), host.put(y0)) if mixed else (c.put(x), c.put(y0))
        st = getattr(P.lib(), "aoclsparse_%scsrmv" % t)(P.OP_NONE, P._ptr(a), M, M, len(v), P._ptr(vd), P._ptr(cd), P._ptr(rd), d.h,
                                                       P._ptr(xd), P._ptr(b), P._ptr(yd))
        assert st == 0, P.STATUS[st]
        return {"y": (host if mixed else c).get(yd)}

    def check(o):
        assert np.all(np.isfinite(o["y"]))
        if t == "d":
            st, yr = oracle.dcsrmv(-1, 0, alpha, M, len(v), v, ci, rp, x, beta, np.nan_to_num(y0))
            assert st == 0
            exact_below_the_tree(o["y"], yr, rp)
        assert within(o["y"], dense_of(rp, ci, v), alpha, x, beta, y0, dt)
    return run, check


for _t in "ds":
    case("%scsrmv" % _t)(lambda _t=_t: _csrmv_case(_t, 2.0, False))
    case("%scsrmv_beta0_nan_y" % _t)(lambda _t=_t: _csrmv_case(_t, 0.0, False))
    # matrix arrays where the mode puts them, x and y always on the host: host mode and the automatic mode only
    case("%scsrmv_matrix_device_vectors_host" % _t, ("host", "auto"))(lambda _t=_t: _csrmv_case(_t, 2.0, True))


def _dotmv_case(t, host_d):
    dt = scal(t, 0).dtype
    rp, ci, v = tri_plus_long_row(dt)
    rng = np.random.default_rng(13)
    x, y0 = rng.uniform(-1, 1, M).astype(dt), rng.uniform(-1, 1, M).astype(dt)
    alpha, beta = 1.25, 0.5
    A, d = Handle(rp, ci, v), P.Descr()

    def run(c):
        xd, yd = c.put(x), c.put(y0)
        dd = (Ctx("host") if host_d else c).put(np.zeros(1, dt))
        if t == "d":
            st = P.lib().aoclsparse_ddotmv(P.OP_NONE, alpha, A.h, d.h, P._ptr(xd), beta, P._ptr(yd), P._ptr(dd))
        else:
            st = P.lib().aoclsparse_zdotmv(P.OP_NONE, P.CDouble(alpha, 0.0), A.h, d.h, P._ptr(xd), P.CDouble(beta, 0.0), P._ptr(yd),
                                           P._ptr(dd))
        assert st == 0, P.STATUS[st]
        return {"y": c.get(yd), "d": dd if host_d else c.get(dd)}

    def check(o):
        D = dense_of(rp, ci, v)
        if t == "d":
            st, yr = oracle.dcsrmv(-1, 0, alpha, M, len(v), v, ci, rp, x, beta, y0)
            assert st == 0
            exact_below_the_tree(o["y"], yr, rp)
        assert within(o["y"], D, alpha, x, beta, y0, dt)
        # the dot of the result actually stored, within n u sum |x y| of the exact sum (u doubled for complex products)
        ex = np.sum(np.conj(x) * o["y"])
        assert abs(o["d"][0] - ex) <= M * float(np.finfo(dt).eps) * 2 * np.sum(np.abs(x * o["y"]))
    return run, check


for _t in "dz":
    case("%sdotmv_d_with_the_vectors" % _t)(lambda _t=_t: _dotmv_case(_t, False))
    case("%sdotmv_host_d" % _t, ("host", "auto"))(lambda _t=_t: _dotmv_case(_t, True))


# ---- ?csrmm ------------------------------------------------------------------------------------------------------------------
def _csrmm_case(colmaj, n, alpha, nine=False, t="d"):
    dt = scal(t, 0).dtype
    if nine:  # 9 entries in every row, columns anywhere: column-major with n >= 16 takes the relayout detour
        rp, ci, v = random_csr(21, M, M, lambda r, i: 9)
        v = v.astype(dt)
    else:
        rp, ci, v = tri_plus_long_row(dt)
    k, beta = M, -0.5
    ldb, ldc = (k + 3, M + 2) if colmaj else (n + 3, n + 2)
    bo, co = (n, n) if colmaj else (k, M)
    bi, cin = (k, M) if colmaj else (n, n)
    rng = np.random.default_rng(14)

    def strided(outer, inner, ld):
        S = np.full(outer * ld, SENTINEL, np.float64).astype(dt)
        S = S.reshape(outer, ld)
        S[:, :inner] = rng.uniform(-1, 1, (outer, inner))
        return S.ravel().copy()
    B, C0 = strided(bo, bi, ldb), strided(co, cin, ldc)
    A, d = Handle(rp, ci, v), P.Descr()
    order = P.ORDER_COLUMN if colmaj else P.ORDER_ROW

    def run(c):
        Bd, Cd = c.put(B), c.put(C0)
        if t == "d":
            st = P.lib().aoclsparse_dcsrmm(P.OP_NONE, alpha, A.h, d.h, order, P._ptr(Bd), n, ldb, beta, P._ptr(Cd), ldc)
        else:
            st = P.lib().aoclsparse_zcsrmm(P.OP_NONE, P.CDouble(alpha, 0.0), A.h, d.h, order, P._ptr(Bd), n, ldb, P.CDouble(beta, 0.0),
                                           P._ptr(Cd), ldc)
        assert st == 0, P.STATUS[st]
        return {"C": c.get(Cd), "B": c.get(Bd)}

    def check(o):
        assert same_bits(o["B"], B)
        got, was = o["C"].reshape(co, ldc), C0.reshape(co, ldc)
        assert same_bits(got[:, cin:], was[:, cin:]), "the padding of C changed"
        if t == "d":
            st, Cr = oracle.dcsrmm("col" if colmaj else "row", alpha, 0, v, ci, rp, M, np.nan_to_num(B), n, ldb, beta, np.nan_to_num(C0), ldc)
            assert st == 0
            want = Cr.reshape(co, ldc)[:, :cin]
            if colmaj:  # csrmm_col_major_ref bit for bit (rows of 32 entries and more: the bound below)
                for j in range(n):
                    if nine:
                        assert np.array_equal(got[j, :cin], want[j]), j
                    else:
                        exact_below_the_tree(got[j, :cin], want[j], rp)
            else:  # row-major: within (len + 3) eps |alpha| sum |a b| + 2 eps |beta c| of the reference kernel (tests/test_gpu_parity.py)
                Bm, Cm = np.nan_to_num(B.reshape(bo, ldb)[:, :bi]), np.nan_to_num(was[:, :cin])
                scale = np.abs(dense_of(rp, ci, v)) @ np.abs(Bm)
                bound = (np.diff(rp)[:, None] + 3) * EPS64 * scale * abs(alpha) + 2 * EPS64 * np.abs(beta * Cm) + 1e-300
                assert np.all(np.abs(got[:, :cin] - want) <= bound)
        D, Bm, Cm = dense_of(rp, ci, v), np.nan_to_num(B.reshape(bo, ldb)[:, :bi]), np.nan_to_num(was[:, :cin])
        for j in range(n):
            bj, cj, gj = (Bm[j], Cm[j], got[j, :cin]) if colmaj else (Bm[:, j], Cm[:, j], got[:, j])
            assert within(gj, D, alpha, bj, beta, cj, dt)
    return run, check


case("dcsrmm_row_major")(lambda: _csrmm_case(False, 5, 1.5))
case("dcsrmm_column_major")(lambda: _csrmm_case(True, 5, 1.5))
case("dcsrmm_column_major_relayout_detour")(lambda: _csrmm_case(True, 16, 1.5, nine=True))
case("dcsrmm_alpha_zero")(lambda: _csrmm_case(False, 5, 0.0))
case("zcsrmm_row_major")(lambda: _csrmm_case(False, 5, 1.5, t="z"))
case("zcsrmm_column_major")(lambda: _csrmm_case(True, 5, 1.5, t="z"))


# ---- ?trsv_strided, ?trsm ----------------------------------------------------------------------------------------------------
def _trsv_case():
    rp, ci, v = tri_plus_long_row()
    incb, incx, alpha = 3, 2, 1.25
    rng = np.random.default_rng(15)
    b = np.full((M - 1) * incb + 1, SENTINEL)
    b[::incb] = rng.uniform(-1, 1, M)
    x0 = np.full((M - 1) * incx + 1, SENTINEL)
    A, d = Handle(rp, ci, v), P.Descr(mtype=P.TYPE_TRIANGULAR, fill=P.FILL_LOWER)

    def run(c):
        bd, xd = c.put(b), c.put(x0)
        st = P.lib().aoclsparse_dtrsv_strided(P.OP_NONE, alpha, A.h, d.h, P._ptr(bd), incb, P._ptr(xd), incx)
        assert st == 0, P.STATUS[st]
        return {"x": c.get(xd)}

    def check(o):
        gaps = np.ones(len(x0), bool)
        gaps[::incx] = False
        assert same_bits(o["x"][gaps], x0[gaps]), "the gaps of x changed"
        st, idiag, iurow = oracle.csr_indices(M, 0, rp, ci)
        st2, xr = oracle.dtrsv("l", alpha, M, 0, v, ci, rp, idiag, np.nan_to_num(b), False, incb, incx)
        assert st == 0 and st2 == 0 and np.array_equal(o["x"][::incx], xr[::incx])
    return run, check


case("dtrsv_strided")(_trsv_case)


def _trsm_case(colmaj):
    rp, ci, v = tri_plus_long_row()
    n, alpha = 5, 0.5
    ldb, ldx = (M + 3, M + 2) if colmaj else (n + 3, n + 2)
    outer, inner = (n, M) if colmaj else (M, n)
    rng = np.random.default_rng(16)
    B = np.full((outer, ldb), SENTINEL)
    B[:, :inner] = rng.uniform(-1, 1, (outer, inner))
    X0 = np.full((outer, ldx), SENTINEL)
    A, d = Handle(rp, ci, v), P.Descr(mtype=P.TYPE_TRIANGULAR, fill=P.FILL_UPPER)

    def run(c):
        Bd, Xd = c.put(B.ravel()), c.put(X0.ravel())
        st = P.lib().aoclsparse_dtrsm(P.OP_NONE, alpha, A.h, d.h, P.ORDER_COLUMN if colmaj else P.ORDER_ROW, P._ptr(Bd), n, ldb,
                                      P._ptr(Xd), ldx)
        assert st == 0, P.STATUS[st]
        return {"X": c.get(Xd)}

    def check(o):
        X = o["X"].reshape(outer, ldx)
        assert same_bits(X[:, inner:], X0[:, inner:]), "the padding of X changed"
        st, idiag, iurow = oracle.csr_indices(M, 0, rp, ci)
        for j in range(n):
            bj, xj = (B[j, :M], X[j, :M]) if colmaj else (B[:, j], X[:, j])
            st2, xr = oracle.dtrsv("u", alpha, M, 0, v, ci, rp, iurow, np.ascontiguousarray(bj), False)
            assert st2 == 0 and np.array_equal(xj, xr), j
    return run, check


case("dtrsm_row_major")(lambda: _trsm_case(False))
case("dtrsm_column_major")(lambda: _trsm_case(True))


# ---- level 1, nnz = 100 ------------------------------------------------------------------------------------------------------
NNZ, EXT = 100, 400


def _l1_data(dt=np.float64):
    rng = np.random.default_rng(17)
    ix = rng.permutation(EXT)[:NNZ].astype(np.int32)
    ix[0] = EXT - 1  # the extent a host call stages is max + 1
    x, y = rng.uniform(-1, 1, NNZ).astype(dt), rng.uniform(-1, 1, EXT).astype(dt)
    if np.dtype(dt).kind == "c":
        x, y = x + 1j * rng.uniform(-1, 1, NNZ).astype(dt), y + 1j * rng.uniform(-1, 1, EXT).astype(dt)
    return ix, x.astype(dt), y.astype(dt)


@case("daxpyi")
def _axpyi():
    ix, x, y = _l1_data()

    def run(c):
        xd, id_, yd = c.put(x), c.put(ix), c.put(y)
        assert P.lib().aoclsparse_daxpyi(NNZ, 0.3, P._ptr(xd), P._ptr(id_), P._ptr(yd)) == 0
        return {"y": c.get(yd), "x": c.get(xd)}

    def check(o):
        st, yr = oracle.daxpyi(0.3, x, ix, y)
        assert st == 0 and np.array_equal(o["y"], yr) and same_bits(o["x"], x)
    return run, check


@case("ddoti")
def _doti():
    ix, x, y = _l1_data()

    def run(c):
        xd, id_, yd = c.put(x), c.put(ix), c.put(y)
        return {"dot": np.array([P.lib().aoclsparse_ddoti(NNZ, P._ptr(xd), P._ptr(id_), P._ptr(yd))])}

    def check(o):
        assert abs(o["dot"][0] - oracle.ddoti(x, ix, y)) <= NNZ * EPS64 * np.sum(np.abs(x * y[ix]))
    return run, check


def _zdot(conj):
    ix, x, y = _l1_data(np.complex128)

    def run(c):
        xd, id_, yd = c.put(x), c.put(ix), c.put(y)
        dot = np.zeros(1, np.complex128)  # a host scalar in the reference's interface, whatever the mode
        fn = P.lib().aoclsparse_zdotci if conj else P.lib().aoclsparse_zdotui
        assert fn(NNZ, P._ptr(xd), P._ptr(id_), P._ptr(yd), P._ptr(dot)) == 0
        return {"dot": dot}

    def check(o):
        ex = np.sum((np.conj(x) if conj else x) * y[ix])
        assert abs(o["dot"][0] - ex) <= NNZ * 2 * EPS64 * np.sum(np.abs(x * y[ix]))
    return run, check


case("zdotci")(lambda: _zdot(True))
case("zdotui")(lambda: _zdot(False))


def _move(kind):
    ix, x, y = _l1_data()
    stride = 3

    def run(c):
        L = P.lib()
        xd, id_, yd = c.put(x if kind.startswith("sctr") else np.zeros(NNZ)), c.put(ix), c.put(y)
        if kind == "gthr":
            st = L.aoclsparse_dgthr(NNZ, P._ptr(yd), P._ptr(xd), P._ptr(id_))
        elif kind == "gthrz":
            st = L.aoclsparse_dgthrz(NNZ, P._ptr(yd), P._ptr(xd), P._ptr(id_))
        elif kind == "gthrs":
            st = L.aoclsparse_dgthrs(NNZ, P._ptr(yd), P._ptr(xd), stride)
        elif kind == "sctr":
            st = L.aoclsparse_dsctr(NNZ, P._ptr(xd), P._ptr(id_), P._ptr(yd))
        else:
            st = L.aoclsparse_dsctrs(NNZ, P._ptr(xd), stride, P._ptr(yd))
        assert st == 0, P.STATUS[st]
        return {"x": c.get(xd), "y": c.get(yd)}

    def check(o):
        if kind in ("gthr", "gthrz"):
            xr, yr = oracle.gthr(y, ix, zero=kind == "gthrz")
        elif kind == "gthrs":
            xr, yr = y[0:stride * NNZ:stride], y
        elif kind == "sctr":
            xr, yr = x, oracle.sctr(x, ix, y)
        else:
            xr, yr = x, y.copy()
            yr[0:stride * NNZ:stride] = x
        assert np.array_equal(o["x"], xr) and np.array_equal(o["y"], yr)
    return run, check


for _k in ("gthr", "gthrz", "gthrs", "sctr", "sctrs"):
    case("d" + _k)(lambda _k=_k: _move(_k))


@case("droti")
def _roti():
    ix, x, y = _l1_data()

    def run(c):
        xd, id_, yd = c.put(x), c.put(ix), c.put(y)
        assert P.lib().aoclsparse_droti(NNZ, P._ptr(xd), P._ptr(id_), P._ptr(yd), 0.6, -0.8) == 0
        return {"x": c.get(xd), "y": c.get(yd)}

    def check(o):
        st, xr, yr = oracle.droti(x, ix, y, 0.6, -0.8)
        assert st == 0 and np.array_equal(o["x"], xr) and np.array_equal(o["y"], yr)
    return run, check


# ---- the raw-array formats ---------------------------------------------------------------------------------------------------
def _rows_with_a_long_one():
    """70 x 60, 1-5 entries a row, every 23rd row 20 entries (the long rows of the hybrid format)"""
    return random_csr(51, M, 60, lambda r, i: 20 if i % 23 == 7 else 1 + i % 5)


def _ell_case(layout):
    n = 60
    rp, ci, v = _rows_with_a_long_one()
    rng = np.random.default_rng(18)
    x, y0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, M)
    alpha, beta = 1.5, -0.5
    a, b, d = scal("d", alpha), scal("d", beta), P.Descr()
    if layout == "hyb":
        w, em, mp, hc, hv = oracle.csr2ell("hyb", M, 0, rp, ci, v)
        assert 0 < len(mp) < M
    else:
        w, ec, ev = oracle.csr2ell(layout, M, 0, rp, ci, v)

    def run(c):
        L = P.lib()
        xd, yd = c.put(x), c.put(y0)
        if layout == "hyb":
            t = [c.put(z) for z in (hv, hc, v, rp, ci, mp)]
            st = L.aoclsparse_dellthybmv(P.OP_NONE, P._ptr(a), M, n, len(v), P._ptr(t[0]), P._ptr(t[1]), w, em, P._ptr(t[2]), P._ptr(t[3]),
                                         P._ptr(t[4]), None, P._ptr(t[5]), d.h, P._ptr(xd), P._ptr(b), P._ptr(yd))
        else:
            fn = L.aoclsparse_dellmv if layout == "ell" else L.aoclsparse_delltmv
            evd, ecd = c.put(ev), c.put(ec)
            st = fn(P.OP_NONE, P._ptr(a), M, n, len(v), P._ptr(evd), P._ptr(ecd), w, d.h, P._ptr(xd), P._ptr(b), P._ptr(yd))
        assert st == 0, P.STATUS[st]
        return {"y": c.get(yd)}

    def check(o):
        if layout == "hyb":
            st, yr = oracle.dellthybmv(0, alpha, M, hv, hc, w, em, v, rp, ci, mp, x, beta, y0)
        else:
            st, yr = oracle.dellmv(layout, 0, alpha, M, ev, ec, w, x, beta, y0)
        assert np.array_equal(o["y"], yr)
    return run, check


case("dellmv")(lambda: _ell_case("ell"))
case("delltmv")(lambda: _ell_case("ellt"))
case("dellthybmv")(lambda: _ell_case("hyb"))


@case("dblkcsrmv")
def _blk():
    m, n, rows = 50, 8, 2
    rp, ci, v = banded_rows(3, m, n, lambda r, i: 1 + i % 8, 0)
    so, brp, bc, bv, mk = oracle.csr2blkcsr(m, n, 0, rp, ci, v, rows)
    rng = np.random.default_rng(19)
    x, y0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, m)
    alpha, beta = 2.0, 1.0
    a, b, d = scal("d", alpha), scal("d", beta), P.Descr()

    def run(c):
        t = [c.put(z) for z in (mk, bv, bc, brp, x, y0)]
        st = P.lib().aoclsparse_dblkcsrmv(P.OP_NONE, P._ptr(a), m, n, len(v), P._ptr(t[0]), P._ptr(t[1]), P._ptr(t[2]), P._ptr(t[3]), d.h,
                                          P._ptr(t[4]), P._ptr(b), P._ptr(t[5]), rows)
        assert st == 0, P.STATUS[st]
        return {"y": c.get(t[5])}

    def check(o):
        so, yr = oracle.dblkcsrmv(0, alpha, m, mk, bv, bc, brp, x, beta, y0, rows)
        assert so == 0 and np.array_equal(o["y"], yr)
    return run, check


def _dia_bsr(which):
    n = 60
    rp, ci, v = _rows_with_a_long_one()
    rng = np.random.default_rng(20)
    alpha, beta, dim = -0.75, 1.0, 3
    d = P.Descr()
    if which == "dia":
        nd, off, dv = oracle.csr2dia(M, n, 0, rp, ci, v)
        x, y0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, M)
    else:
        mb, nb = (M + dim - 1) // dim, (n + dim - 1) // dim
        bp, bi, bv = oracle.csr2bsr(M, n, 0, rp, ci, v, dim, False)
        x, y0 = rng.uniform(-1, 1, nb * dim), rng.uniform(-1, 1, mb * dim)

    def run(c):
        a, b = ctypes.c_double(alpha), ctypes.c_double(beta)
        xd, yd = c.put(x), c.put(y0)
        if which == "dia":
            dvd, offd = c.put(dv), c.put(off)
            st = P.lib().aoclsparse_ddiamv(P.OP_NONE, ctypes.byref(a), M, n, len(v), P._ptr(dvd), P._ptr(offd), nd, d.h, P._ptr(xd),
                                           ctypes.byref(b), P._ptr(yd))
        else:
            t = [c.put(z) for z in (bv, bi, bp)]
            st = P.lib().aoclsparse_dbsrmv(P.OP_NONE, ctypes.byref(a), mb, nb, dim, P._ptr(t[0]), P._ptr(t[1]), P._ptr(t[2]), d.h, P._ptr(xd),
                                           ctypes.byref(b), P._ptr(yd))
        assert st == 0, P.STATUS[st]
        return {"y": c.get(yd)}

    def check(o):
        want = oracle.ddiamv(alpha, M, n, dv, off, x, beta, y0) if which == "dia" else oracle.dbsrmv(alpha, mb, dim, 0, bv, bi, bp, x, beta, y0)
        assert np.array_equal(o["y"], want)
    return run, check


case("ddiamv")(lambda: _dia_bsr("dia"))
case("dbsrmv")(lambda: _dia_bsr("bsr"))


# ---- dense results: sp2md / spmmd / csr2dense / syrkd / syprd ----------------------------------------------------------------
def _sp2md_case(spmmd):
    ma, ka, nb = 45, M, 33
    a = (ma, ka, 0) + random_csr(31, ma, ka, lambda r, i: 1 + i % 6)
    b = (ka, nb, 0) + random_csr(32, ka, nb, lambda r, i: 1 + i % 4)
    ldc = nb + 3
    alpha, beta = (1.0, 0.0) if spmmd else (1.5, -0.5)
    rng = np.random.default_rng(33)
    C0 = np.full((ma, ldc), SENTINEL)
    C0[:, :nb] = rng.uniform(-1, 1, (ma, nb))
    A, B, d = Handle(*a[3:], n=ka), Handle(*b[3:], n=nb), P.Descr()

    def run(c):
        Cd = c.put(C0.ravel())
        if spmmd:
            st = P.lib().aoclsparse_dspmmd(P.OP_NONE, A.h, B.h, P.ORDER_ROW, P._ptr(Cd), ldc)
        else:
            st = P.lib().aoclsparse_dsp2md(P.OP_NONE, d.h, A.h, P.OP_NONE, d.h, B.h, alpha, beta, P._ptr(Cd), P.ORDER_ROW, ldc)
        assert st == 0, P.STATUS[st]
        return {"C": c.get(Cd)}

    def check(o):
        C = o["C"].reshape(ma, ldc)
        assert same_bits(C[:, nb:], C0[:, nb:]), "the padding of C changed"
        want = oracle.dsp2md(a, False, b, False, alpha, beta, np.nan_to_num(C0).ravel(), True, ldc).reshape(ma, ldc)
        assert np.array_equal(C[:, :nb], want[:, :nb])
    return run, check


case("dsp2md_ldc_padding")(lambda: _sp2md_case(False))
case("dspmmd_ldc_padding")(lambda: _sp2md_case(True))


@case("dcsr2dense_ld_padding")
def _csr2dense():
    n, ld = 60, 64
    rp, ci, v = _rows_with_a_long_one()
    A0 = np.full(M * ld, SENTINEL)
    d = P.Descr()

    def run(c):
        t = [c.put(z) for z in (v, rp, ci, A0)]
        st = P.lib().aoclsparse_dcsr2dense(M, n, d.h, P._ptr(t[0]), P._ptr(t[1]), P._ptr(t[2]), P._ptr(t[3]), ld, P.ORDER_ROW)
        assert st == 0, P.STATUS[st]
        return {"A": c.get(t[3])}

    def check(o):
        assert same_bits(o["A"], oracle.dcsr2dense(M, n, 0, rp, ci, v, A0, ld, False))
        assert same_bits(o["A"].reshape(M, ld)[:, n:], A0.reshape(M, ld)[:, n:])
    return run, check


def _sy_dense(which):
    m, n = 45, M
    a = (m, n, 0) + random_csr(41, m, n, lambda r, i: 2 + i % 5)
    alpha, beta, ldc = 1.5, -0.5, m + 3
    rng = np.random.default_rng(42)
    C0 = np.full((m, ldc), SENTINEL)
    C0[:, :m] = rng.uniform(-1, 1, (m, m))
    Bm = rng.uniform(-1, 1, (n, n))
    A = Handle(*a[3:], n=n)
    up = np.triu_indices(m)

    def run(c):
        Cd = c.put(C0.ravel())
        if which == "syrkd":
            st = P.lib().aoclsparse_dsyrkd(P.OP_NONE, A.h, alpha, beta, P._ptr(Cd), P.ORDER_ROW, ldc)
        else:
            st = P.lib().aoclsparse_dsyprd(P.OP_NONE, A.h, P._ptr(c.put(Bm.ravel())), P.ORDER_ROW, n, alpha, beta, P._ptr(Cd), P.ORDER_ROW, ldc)
        assert st == 0, P.STATUS[st]
        return {"C": c.get(Cd)}

    def check(o):
        C = o["C"].reshape(m, ldc)
        assert same_bits(C[:, m:], C0[:, m:]) and same_bits(C[:, :m][np.tril_indices(m, -1)], C0[:, :m][np.tril_indices(m, -1)])
        if which == "syrkd":
            want = oracle.dsp2md(a, False, a, True, alpha, beta, C0[:, :m], True, m).reshape(m, m)
            assert np.array_equal(C[:, :m][up], want[up])
        else:
            # C = alpha A sym(B) A^T + beta C on the upper triangle: chains of at most 2 L terms, so (2 L + 4) u times the same
            # product of absolute values (the bound of tests/test_sy_dense_gpu.py)
            D, Bs = dense_of(*a[3:], n=n), np.triu(Bm) + np.triu(Bm, 1).T
            ex = alpha * (D @ Bs @ D.T) + beta * C0[:, :m]
            bound = (2 * np.count_nonzero(D, axis=1).max() + 4) * EPS64 * (abs(alpha) * (np.abs(D) @ np.abs(Bs) @ np.abs(D.T)) + abs(beta) * np.abs(C0[:, :m]))
            assert np.all(np.abs(C[:, :m] - ex)[up] <= bound[up])
    return run, check


case("dsyrkd")(lambda: _sy_dense("syrkd"))
case("dsyprd")(lambda: _sy_dense("syprd"))


# ---- composite routines on the 70-row matrix ---------------------------------------------------------------------------------
@case("dsymgs")
def _symgs():
    rp, ci, v = tri_plus_long_row()
    rng = np.random.default_rng(43)
    b, x0 = rng.uniform(-1, 1, M), rng.uniform(-1, 1, M)
    A, d = Handle(rp, ci, v), P.Descr()

    def run(c):
        bd, xd = c.put(b), c.put(x0)
        st = P.lib().aoclsparse_dsymgs(P.OP_NONE, A.h, d.h, 0.9, P._ptr(bd), P._ptr(xd))
        assert st == 0, P.STATUS[st]
        return {"x": c.get(xd)}

    def check(o):
        q = oracle.dcsr_optimize(M, M, len(v), 0, rp, ci, v)
        st, xr = oracle.dsymgs(0, 0, 0, 0, 0.9, M, q["val"], q["ind"], q["ptr"], q["idiag"], q["iurow"], b, x0)
        assert st == 0 and np.max(np.abs(o["x"] - xr)) <= 64 * EPS64 * max(1.0, np.abs(xr).max())  # (as tests/test_gpu_parity.py)
    return run, check


@case("dilu_smoother")
def _ilu():
    rp, ci, v = tri_plus_long_row()
    rng = np.random.default_rng(44)
    b = rng.uniform(-1, 1, M)
    A, d = Handle(rp, ci, v), P.Descr()
    assert P.lib().aoclsparse_set_lu_smoother_hint(A.h, P.OP_NONE, d.h, 10) == 0 and P.lib().aoclsparse_optimize(A.h) == 0

    def run(c):
        bd, xd = c.put(b), c.put(np.zeros(M))
        pv = ctypes.c_void_p()
        st = P.lib().aoclsparse_dilu_smoother(P.OP_NONE, A.h, d.h, ctypes.byref(pv), None, P._ptr(xd), P._ptr(bd))
        assert st == 0, P.STATUS[st]
        fac = np.ctypeslib.as_array(ctypes.cast(pv, ctypes.POINTER(ctypes.c_double)), (len(v),)).copy()
        return {"x": c.get(xd), "factors": fac}

    def check(o):
        st, lu, diag = oracle.dilu0(M, 0, rp, ci, v)
        st2, xr = oracle.dilu_solve(M, 0, diag, lu, rp, ci, b)
        assert st == 0 and st2 == 0 and np.array_equal(o["factors"], lu) and np.array_equal(o["x"], xr)
    return run, check


@case("dsorv")
def _sorv():
    rp, ci, v = tri_plus_long_row()
    rng = np.random.default_rng(45)
    b, x0 = rng.uniform(-1, 1, M), rng.uniform(-1, 1, M)
    A, d = Handle(rp, ci, v), P.Descr()

    def run(c):
        bd, xd = c.put(b), c.put(x0)
        st = P.lib().aoclsparse_dsorv(0, d.h, A.h, 1.2, 0.5, P._ptr(xd), P._ptr(bd))
        assert st == 0, P.STATUS[st]
        return {"x": c.get(xd)}

    def check(o):
        st, xr = oracle.dsorv(M, 0, rp, ci, v, 1.2, 0.5, x0, b)
        assert st == 0 and np.array_equal(o["x"], xr)
    return run, check


# ---- running a case ------------------------------------------------------------------------------------------------------------
def run_case(name, mode):
    """one call of case `name` with its arrays placed for `mode`; the pointer mode is restored whatever happens"""
    modes, factory = CASES[name]
    assert mode in modes
    run, check = factory()
    L = P.lib()
    try:
        if mode == "device":
            assert L.aoclsparse_mi355_set_pointer_mode(P.PTR_DEVICE) == 0
        out = run(Ctx(mode))
    finally:
        assert L.aoclsparse_mi355_set_pointer_mode(P.PTR_AUTO) == 0
    return out, check
