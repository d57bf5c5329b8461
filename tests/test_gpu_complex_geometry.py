"""The complex kernels (csrc/complex_kernels.hip) where their launch geometry changes: triangular levels on both sides of
TRSV_NARROW, the 16- and 64-lane SpMV groups, every tile width of csrmm, and the loops that split a launch at the 65,535
limit of a grid's y dimension or at the 1024 workgroups of the dot product.

Every case compares EVERY output entry with an extended-precision reference computed on the CSR arrays (tests/complex_ref.py)
within a bound derived from the operations the kernel performs (same file; tests/test_complex_ref_cpu.py shows that the bounds
tell a correct result from a subtly wrong one).  Padding must keep its bits.  Each case first asserts, from its own inputs and
from the constant in the source it names, that it runs on the path it is meant for.  The largest error / bound ratio of each
case is printed as `RATIO <group> <prec> <value>` (DESIGN.md section 3 records them)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import complex_ref as cr
from util import ROOT, pkg

pytestmark = pytest.mark.gpu
PREC = pytest.mark.parametrize("prec", ["z", "c"])

torch = pytest.importorskip("torch")
P = pkg()
L = P.lib()

DTYPE = {"z": np.complex128, "c": np.complex64}
OPS = {"n": P.OP_NONE, "t": P.OP_TRANSPOSE, "h": P.OP_CONJ_TRANSPOSE}
FILLS = {"lower": P.FILL_LOWER, "upper": P.FILL_UPPER}
GRID_Y = 65535  # the y limit of a grid: the literal of the c0 / j0 / o0 loops in complex_kernels.hip
PAD = 9 - 9j


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    st, d, cus, name = P.device_info()
    assert st == 0 and cus > 0


# ---- the constants the cases depend on, read where they live: a changed threshold fails here instead of covering less ----------

@functools.lru_cache(maxsize=None)
def source(name):
    with open(os.path.join(ROOT, "aocl-sparse_amd", "csrc", name)) as f:
        return f.read()


def source_int(name, pattern):
    found = re.findall(pattern, source(name))
    assert len(found) == 1, (name, pattern, found)
    return int(found[0])


def trsv_narrow():
    return source_int("internal.hpp", r"constexpr int TRSV_NARROW\s*=\s*(\d+);")


def spmv_group(mean):
    """lanes per row of launch_cspmv (complex_kernels.hip) for a mean row length nnz / m"""
    body = source("complex_kernels.hip")
    body = body[body.index("aoclsparse_status launch_cspmv("):]
    body = body[:body.index("MI355_HIP_TRY")]
    bands = [int(b) for b in re.findall(r"mean <= (\d+)", body)]
    groups = [int(g) for g in re.findall(r"integral_constant<int, (\d+)>", body)]
    assert bands == [6, 24, 96] and groups == [4, 8, 16, 64], (bands, groups)
    return groups[sum(mean > b for b in bands)]


def csrmm_tile(n):
    """columns per workgroup of the row-major launch of launch_ccsrmm (complex_kernels.hip)"""
    assert "const int tx = n >= 64 ? 64 : (n >= 16 ? 16 : 4), ty = 256 / tx;" in source("complex_kernels.hip")
    return 64 if n >= 64 else (16 if n >= 16 else 4)


def grid_loops():
    """the launch loops step by the y limit of a grid"""
    s = source("complex_kernels.hip")
    for loop in ("c0 += 65535)", "j0 += 65535 * 4)", "j0 += 65535 * tx)", "o0 += 65535)"):
        assert loop in s, loop
    return GRID_Y


# ---- helpers ------------------------------------------------------------------------------------------------------------------

def fn(prec, stem):
    return getattr(L, "aoclsparse_" + stem.replace("?", prec))


def scalar(prec, z):
    return (P.CDouble if prec == "z" else P.CFloat)(float(z.real), float(z.imag))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def report(group, prec, value):
    print("RATIO %s %s %.4g" % (group, prec, value))
    return value


class Handle:
    """a complex CSR handle over arrays it keeps alive (the library aliases them); no hint is ever set on it"""

    def __init__(self, prec, base, m, n, rp, ci, v):
        self.prec, self.base, self.m, self.n = prec, base, m, n
        self.rp, self.ci, self.v = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32), np.ascontiguousarray(v, DTYPE[prec])
        self.h = ctypes.c_void_p()
        assert fn(prec, "create_?csr")(ctypes.byref(self.h), base, m, n, len(self.v), P._ptr(self.rp), P._ptr(self.ci), P._ptr(self.v)) == 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        L.aoclsparse_destroy(ctypes.byref(self.h))

    def coo(self):
        return cr.coo(self.rp, self.ci, self.v, self.base)

    def trsv_levels(self, fill, op):
        lv = ctypes.c_int32(-2)
        assert L.aoclsparse_mi355_get_trsv_levels(self.h, FILLS[fill], OPS[op], ctypes.byref(lv)) == 0
        return lv.value


# ---- triangular solves on the designed levels ------------------------------------------------------------------------------------

ALPHA = 0.8 - 0.6j
NRHS = 5


@functools.lru_cache(maxsize=None)
def designed(prec, base):
    rp, ci, v = cr.level_triangle(cr.DESIGN_WIDTHS, 41, DTYPE[prec], 0)  # one matrix, two index bases
    return (rp + base).astype(np.int32), (ci + base).astype(np.int32), v


@functools.lru_cache(maxsize=None)
def rhs(prec):
    return cr.crand(np.random.default_rng(5), (5225, NRHS), DTYPE[prec])


@functools.lru_cache(maxsize=None)
def solve_reference(prec, fill, op, unit, nrhs):
    """the operator of the solve and the extended-precision solution of its first nrhs right-hand sides (shared, read only)"""
    t = cr.TriOp(*designed(prec, 0), 0, fill, op, unit)
    ref = t.solve(DTYPE[prec](ALPHA), rhs(prec)[:, :nrhs], cr.ext_type(DTYPE[prec]))
    ref.setflags(write=False)
    return t, ref


def check_solution(prec, t, ref, X, group="solve"):
    X = np.asarray(X).reshape(ref.shape)
    r = report(group, prec, cr.ratio(np.abs(X.astype(ref.dtype) - ref), t.bound(X, DTYPE[prec])))
    assert r < 1.0
    return r


def assert_designed_path(A, fill, op):
    """op = N: exactly the designed widths -- 1024 is a narrow level and 1025 a wide one (TRSV_NARROW, internal.hpp), so the plan
    of build_levels (trsv_plan.cpp) is wide | lone narrow (level kernel, 64 lanes) | wide | run of three narrow | wide | lone
    narrow (level kernel, 256 lanes, ragged).  op = T / H: the seeds are rows of more than 1000 entries, one long chain on one
    lane, and at least one level is wide."""
    narrow = trsv_narrow()
    widths = cr.level_widths(A.rp, A.ci, A.base, fill, op)
    if op == "n":
        assert widths == list(cr.DESIGN_WIDTHS) and narrow == 1024
        assert [w <= narrow for w in widths] == [False, True, False, True, True, True, False, True]
        assert any(w > narrow and w % 256 for w in widths) and widths[-1] >= 256 and widths[-1] % 256 and widths[1] < 64
    else:
        t = cr.TriOp(A.rp, A.ci, A.v, A.base, fill, op, True)
        assert max(widths) > narrow and t.p.max() > 1000
    assert A.trsv_levels(fill, op) == len(widths)
    if op == "n":
        assert len(widths) == 8


@PREC
@pytest.mark.parametrize("unit", [False, True], ids=["nonunit", "unit"])
@pytest.mark.parametrize("op", ["n", "t", "h"])
@pytest.mark.parametrize("fill", ["lower", "upper"])
def test_trsv_on_designed_levels(prec, fill, op, unit):
    dtype = DTYPE[prec]
    t, ref = solve_reference(prec, fill, op, unit, 1)
    b = np.ascontiguousarray(rhs(prec)[:, 0])
    for base in (0, 1):
        with Handle(prec, base, 5225, 5225, *designed(prec, base)) as A:
            d = P.Descr(base=base, mtype=P.TYPE_TRIANGULAR, fill=FILLS[fill], diag=P.DIAG_UNIT if unit else P.DIAG_NON_UNIT)
            x = np.full(5225, np.nan, dtype)
            assert fn(prec, "?trsv")(OPS[op], scalar(prec, dtype(ALPHA)), A.h, d.h, P._ptr(b), P._ptr(x)) == 0
            assert_designed_path(A, fill, op)
            check_solution(prec, t, ref, x)


@PREC
def test_trsv_strided(prec):
    """incb 3, incx 2, op = H: the slots between the entries keep their bits"""
    dtype = DTYPE[prec]
    n = 5225
    t, ref = solve_reference(prec, "lower", "h", False, 1)
    with Handle(prec, 1, n, n, *designed(prec, 1)) as A:
        d = P.Descr(base=1, mtype=P.TYPE_TRIANGULAR, fill=P.FILL_LOWER)
        bs, xs = np.zeros(3 * n, dtype), np.full(2 * n, PAD, dtype)
        bs[::3] = rhs(prec)[:, 0]
        args = (OPS["h"], scalar(prec, dtype(ALPHA)), A.h, d.h)
        assert fn(prec, "?trsv_strided")(*args, P._ptr(bs), 3, P._ptr(xs), 2) == 0
        assert_designed_path(A, "lower", "h")
        check_solution(prec, t, ref, xs[::2])
        assert same_bits(xs[1::2], np.full(n, PAD, dtype))
        xd = dev(np.full(2 * n, PAD, dtype))
        assert fn(prec, "?trsv_strided")(*args, P._ptr(dev(bs)), 3, P._ptr(xd), 2) == 0
        assert same_bits(host(xd), xs)  # one arithmetic whatever the operands' home


def layout(M, order, ld, fill, dtype):
    """M (rows x k) laid out row- or column-major with leading dimension ld, the padding set to `fill`; `cut` takes such an array
    back to rows x k and `pad` returns its padding"""
    rows, k = M.shape
    if order == P.ORDER_ROW:
        buf = np.full((rows, ld), fill, dtype)
        buf[:, :k] = M
        return buf, (lambda X: X[:, :k]), (lambda X: X[:, k:])
    buf = np.full((k, ld), fill, dtype)
    buf[:, :rows] = M.T
    return buf, (lambda X: X[:, :rows].T), (lambda X: X[:, rows:])


def dense_operands(Bm, order, ldb, ldx, dtype):
    """B from Bm (n x k) and an X of the same extent full of PAD, with their leading dimensions"""
    return (layout(Bm, order, ldb, 0, dtype)[0],) + layout(np.full(Bm.shape, PAD, dtype), order, ldx, PAD, dtype)


@PREC
@pytest.mark.parametrize("fill", ["lower", "upper"])
def test_trsm_five_right_hand_sides(prec, fill):
    """op = T, both layouts, padded leading dimensions, both index bases; host and device operands give the same bits"""
    dtype = DTYPE[prec]
    n, k = 5225, NRHS
    t, ref = solve_reference(prec, fill, "t", False, k)
    for base in (0, 1):
        with Handle(prec, base, n, n, *designed(prec, base)) as A:
            d = P.Descr(base=base, mtype=P.TYPE_TRIANGULAR, fill=FILLS[fill])
            for order, ldb, ldx in ((P.ORDER_ROW, k + 2, k + 1), (P.ORDER_COLUMN, n + 3, n + 4)):
                Bb, Xb, cut, pad = dense_operands(rhs(prec), order, ldb, ldx, dtype)
                args = (OPS["t"], scalar(prec, dtype(ALPHA)), A.h, d.h, order)
                assert fn(prec, "?trsm")(*args, P._ptr(Bb), k, ldb, P._ptr(Xb), ldx) == 0
                assert_designed_path(A, fill, "t")
                check_solution(prec, t, ref, cut(Xb))
                assert same_bits(pad(Xb), np.full(pad(Xb).shape, PAD, dtype))
                if base == 0:
                    Xd = dev(np.full(Xb.shape, PAD, dtype))
                    assert fn(prec, "?trsm")(*args, P._ptr(dev(Bb)), k, ldb, P._ptr(Xd), ldx) == 0
                    assert same_bits(host(Xd), Xb)


@PREC
def test_trsv_host_and_device_operands_give_the_same_bits(prec):
    dtype = DTYPE[prec]
    n = 5225
    b = np.ascontiguousarray(rhs(prec)[:, 0])
    with Handle(prec, 0, n, n, *designed(prec, 0)) as A:
        d = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=P.FILL_UPPER)
        x, xd = np.full(n, np.nan, dtype), dev(np.full(n, np.nan, dtype))
        args = (OPS["n"], scalar(prec, dtype(ALPHA)), A.h, d.h)
        assert fn(prec, "?trsv")(*args, P._ptr(b), P._ptr(x)) == 0 and fn(prec, "?trsv")(*args, P._ptr(dev(b)), P._ptr(xd)) == 0
        assert_designed_path(A, "upper", "n")
        assert same_bits(host(xd), x) and not np.any(np.isnan(x))


@PREC
@pytest.mark.parametrize("fill,op", [("lower", "n"), ("upper", "h")])
def test_trsm_more_right_hand_sides_than_a_grid_is_high(prec, fill, op):
    """65,537 right-hand sides of a 6 x 6 triangle, both layouts: launch_ctrsv walks them in chunks of 65,535 (its c0 loop), the
    second chunk at b + c0 * b_off, xp + c0 * m, x + c0 * x_off.  Every column is checked."""
    dtype = DTYPE[prec]
    n, k = 6, 65537
    assert k > grid_loops()
    rng = np.random.default_rng(77)
    rows = [np.arange(n) for _ in range(n)]  # a full 6 x 6 matrix: both triangles are chains of six levels
    rp = np.arange(0, n * n + 1, n)
    ci = np.concatenate(rows)
    v = 0.5 * cr.crand(rng, n * n, np.complex128)
    v[ci == np.repeat(np.arange(n), n)] = rng.uniform(3, 4, n) * np.exp(1j * rng.uniform(0, 2 * np.pi, n))
    Bm = cr.crand(rng, (n, k), dtype)
    with Handle(prec, 0, n, n, rp, ci, v.astype(dtype)) as A:
        t = cr.TriOp(A.rp, A.ci, A.v, 0, fill, op, False)
        ref = t.solve(dtype(ALPHA), Bm, cr.ext_type(dtype))
        d = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=FILLS[fill])
        for order, ldb, ldx in ((P.ORDER_ROW, k + 2, k + 1), (P.ORDER_COLUMN, n + 3, n + 1)):
            Bb, Xb, cut, pad = dense_operands(Bm, order, ldb, ldx, dtype)
            assert fn(prec, "?trsm")(OPS[op], scalar(prec, dtype(ALPHA)), A.h, d.h, order, P._ptr(Bb), k, ldb, P._ptr(Xb), ldx) == 0
            assert A.trsv_levels(fill, op) == n
            check_solution(prec, t, ref, cut(Xb))
            assert same_bits(pad(Xb), np.full(pad(Xb).shape, PAD, dtype))


# ---- ?mv on the lane-group kernel ----------------------------------------------------------------------------------------------------

MV_ALPHA, MV_BETA = 0.7 - 0.2j, -0.4 + 0.3j
MV_MATRICES = {  # name: (row lengths, transposed, the op that runs its designed rows, lanes per row expected)
    "mid": ((0, 1, 15, 16, 17, 33, 200), False, "n", 16),
    "long": ((0, 1, 63, 64, 65, 129, 500), False, "n", 64),
    "mid_t": ((0, 1, 15, 16, 17, 33, 200), True, "h", 16),  # 700 x 131: op = H runs on its transpose, the designed rows conjugated
    "long_t": ((0, 1, 63, 64, 65, 129, 500), True, "h", 64),
}


def check_product(prec, group, r, c, a, shape, alpha, B, beta, C0, t, got):
    """every entry of got against alpha A B + beta C0 (triples of the operator A) within (p_i + t + 3) c scale_i"""
    dtype = DTYPE[prec]
    ref = cr.product(r, c, a, shape, alpha, B, beta, C0, cr.ext_type(dtype))
    scale, p = cr.product_scale(r, c, a, shape, alpha, B, beta, C0)
    got = np.asarray(got).reshape(ref.shape)
    val = report(group, prec, cr.ratio(np.abs(got.astype(ref.dtype) - ref), cr.product_bound(p, t, scale, dtype)))
    assert val < 1.0


def run_mv(prec, A, descr, op, r, c, a, shape, lanes):
    """general alpha and beta, then beta = 0 on a y full of NaN; host and device operands"""
    dtype = DTYPE[prec]
    rng = np.random.default_rng(12)
    alpha, beta, zero = np.array([MV_ALPHA], dtype), np.array([MV_BETA], dtype), np.zeros(1, dtype)
    x, y0 = cr.crand(rng, shape[1], dtype), cr.crand(rng, shape[0], dtype)
    t = int(np.log2(lanes))
    y = y0.copy()
    assert fn(prec, "?mv")(OPS[op], P._ptr(alpha), A.h, descr.h, P._ptr(x), P._ptr(beta), P._ptr(y)) == 0
    check_product(prec, "mv", r, c, a, shape, alpha[0], x[:, None], beta[0], y0[:, None], t, y)
    yd = dev(y0)
    assert fn(prec, "?mv")(OPS[op], P._ptr(alpha), A.h, descr.h, P._ptr(dev(x)), P._ptr(beta), P._ptr(yd)) == 0
    assert same_bits(host(yd), y)
    yn = np.full(shape[0], np.nan + 1j * np.nan, dtype)
    assert fn(prec, "?mv")(OPS[op], P._ptr(alpha), A.h, descr.h, P._ptr(x), P._ptr(zero), P._ptr(yn)) == 0
    assert not np.any(np.isnan(yn))  # beta = 0 never reads y
    check_product(prec, "mv", r, c, a, shape, alpha[0], x[:, None], zero[0], np.zeros((shape[0], 1), dtype), t, yn)


@PREC
@pytest.mark.parametrize("name", list(MV_MATRICES))
def test_mv_lane_groups(prec, name):
    """cspmv_kernel<R, 16> (mean row length 25-96) and <R, 64> (above 96) of launch_cspmv, complex_kernels.hip: rows shorter than,
    equal to and longer than the lane group, empty first and last rows, 131 rows (no multiple of the 16 or 4 rows of a
    workgroup); the handle carries no hint, so no SELL-64 copy is built (complex_api.cpp)."""
    dtype = DTYPE[prec]
    lengths, transposed, op, lanes = MV_MATRICES[name]
    m, n = 131, 700
    rp, ci, v = cr.rows_of_lengths(dtype, m, n, lengths, 90 + len(name), base=1)
    assert rp[1] == rp[0] and rp[-1] == rp[-2] and set(np.diff(rp)) == set(lengths)
    shape = (m, n)
    if transposed:
        rp, ci, v = cr.transpose_csr(rp, ci, v, 1, shape)
        shape = (n, m)
    with Handle(prec, 1, *shape, rp, ci, v) as A:
        r, c, a, oshape = cr.op_coo(*A.coo(), shape, op)
        assert oshape[0] == 131 and 131 % (256 // lanes) != 0
        assert spmv_group(len(a) // oshape[0]) == lanes  # the band of nnz // (rows of the operator the kernel runs on)
        rows = np.bincount(r, minlength=131)
        assert rows.max() > lanes and np.any((rows > 0) & (rows < lanes)) and np.any(rows == lanes)
        run_mv(prec, A, P.Descr(base=1), op, r, c, a, oshape, lanes)


@PREC
def test_mv_hermitian_lane_group(prec):
    """a hermitian descriptor on a square matrix: the kernel runs on the expansion of the stored lower triangle, 16 lanes per row"""
    dtype = DTYPE[prec]
    n = 131
    rng = np.random.default_rng(23)
    lens = np.minimum(np.arange(n), rng.choice([0, 1, 15, 16, 17, 33, 100], size=n))
    rows = [np.concatenate([np.sort(rng.choice(i, size=k, replace=False)) if k else np.zeros(0, np.int64), [i]]) for i, k in enumerate(lens)]
    rp = np.concatenate([[0], np.cumsum([len(q) for q in rows])])
    ci = np.concatenate(rows)
    with Handle(prec, 0, n, n, rp, ci, cr.crand(rng, len(ci), dtype)) as A:
        r, c, a = cr.hermitian_coo(*A.coo(), "lower")
        lanes = spmv_group(len(a) // n)
        assert lanes == 16 and np.bincount(r, minlength=n).max() > lanes
        run_mv(prec, A, P.Descr(mtype=P.TYPE_HERMITIAN, fill=P.FILL_LOWER), "n", r, c, a, (n, n), lanes)


# ---- ?csrmm ------------------------------------------------------------------------------------------------------------------------

def run_csrmm(prec, A, op, order, n, ldb, ldc, alpha, beta, device, group="csrmm", pad=PAD):
    """C = alpha op(A) B + beta C0 through ?csrmm with the layout and leading dimensions given; every entry checked, padding
    unchanged; returns C as the caller's array (host copy for device operands)"""
    dtype = DTYPE[prec]
    r, c, a, shape = cr.op_coo(*A.coo(), (A.m, A.n), op)
    rng = np.random.default_rng(31)
    Bm, C0 = cr.crand(rng, (shape[1], n), dtype), cr.crand(rng, (shape[0], n), dtype)
    Bb = layout(Bm, order, ldb, 0, dtype)[0]
    Cb, cut, padding = layout(C0, order, ldc, pad, dtype)
    before = padding(Cb).copy()
    d = P.Descr(base=A.base)
    args = (OPS[op], scalar(prec, dtype(alpha)), A.h, d.h, order)
    if device:
        Cd = dev(Cb)
        assert fn(prec, "?csrmm")(*args, P._ptr(dev(Bb)), n, ldb, scalar(prec, dtype(beta)), P._ptr(Cd), ldc) == 0
        Cb = host(Cd)
    else:
        assert fn(prec, "?csrmm")(*args, P._ptr(Bb), n, ldb, scalar(prec, dtype(beta)), P._ptr(Cb), ldc) == 0
    if complex(dtype(alpha)) == 0:
        r, c, a = r[:0], c[:0], a[:0]  # alpha = 0: C = beta C0, one multiplication (launch_cscale_dense)
    check_product(prec, group, r, c, a, shape, dtype(alpha), Bm, dtype(beta), C0, 0, cut(Cb))
    assert same_bits(padding(Cb), before)
    return Cb


@PREC
@pytest.mark.parametrize("op", ["n", "h"])
@pytest.mark.parametrize("n", [1, 3, 15, 16, 17, 63, 64, 65, 130])
def test_csrmm_row_major_tiles(prec, op, n):
    """131 x 90, row-major: 4, 16 and 64 columns per workgroup of launch_ccsrmm on both sides of n = 16 and n = 64; ldb = n + 2,
    ldc = n + 1.  Host and device operands give the same bits (n = 65)."""
    assert csrmm_tile(n) == {1: 4, 3: 4, 15: 4, 16: 16, 17: 16, 63: 16, 64: 64, 65: 64, 130: 64}[n]
    with Handle(prec, 1, 131, 90, *cr.product_matrix(DTYPE[prec], 131, 90, base=1)) as A:
        C = run_csrmm(prec, A, op, P.ORDER_ROW, n, n + 2, n + 1, MV_ALPHA, MV_BETA, False)
        if n == 65:
            assert same_bits(run_csrmm(prec, A, op, P.ORDER_ROW, n, n + 2, n + 1, MV_ALPHA, MV_BETA, True), C)


@PREC
@pytest.mark.parametrize("op", ["n", "h"])
@pytest.mark.parametrize("n", [1, 5, 9])
@pytest.mark.parametrize("m", [1, 63, 65])
def test_csrmm_column_major(prec, op, n, m):
    """m x 90, column-major (64 rows x 4 columns per workgroup): rows and columns short of, at and past a workgroup's, padded
    leading dimensions.  Host and device operands give the same bits (m = 65, n = 9)."""
    with Handle(prec, 0, m, 90, *cr.product_matrix(DTYPE[prec], m, 90, seed=50 + m)) as A:
        rows_b, rows_c = (90, m) if op == "n" else (m, 90)
        C = run_csrmm(prec, A, op, P.ORDER_COLUMN, n, rows_b + 3, rows_c + 4, MV_ALPHA, MV_BETA, False)
        if (m, n) == (65, 9):
            assert same_bits(run_csrmm(prec, A, op, P.ORDER_COLUMN, n, rows_b + 3, rows_c + 4, MV_ALPHA, MV_BETA, True), C)


@PREC
def test_csrmm_column_major_past_the_grid(prec):
    """2 x 3, column-major, n = 65,535 * 4 + 3 on device operands: the j0 loop of launch_ccsrmm starts a second grid at
    B + j0 * ldb, C + j0 * ldc"""
    n = grid_loops() * 4 + 3
    assert n > GRID_Y * 4
    rp, ci = np.array([0, 2, 5]), np.array([0, 2, 0, 1, 2])
    with Handle(prec, 0, 2, 3, rp, ci, cr.crand(np.random.default_rng(4), 5, DTYPE[prec])) as A:
        run_csrmm(prec, A, "n", P.ORDER_COLUMN, n, 3 + 1, 2 + 1, MV_ALPHA, MV_BETA, True)


def test_ccsrmm_row_major_past_the_grid():
    """1 x 2, row-major, n = 65,535 * 64 + 5 on device operands, float complex only: the j0 loop of launch_ccsrmm starts a
    second grid at B + j0, C + j0"""
    n = grid_loops() * 64 + 5
    assert csrmm_tile(n) == 64 and n > GRID_Y * csrmm_tile(n)
    rp, ci = np.array([0, 2]), np.array([0, 1])
    with Handle("c", 0, 1, 2, rp, ci, cr.crand(np.random.default_rng(4), 2, np.complex64)) as A:
        run_csrmm("c", A, "n", P.ORDER_ROW, n, n + 2, n + 1, MV_ALPHA, MV_BETA, True)


@PREC
def test_csrmm_alpha_zero_past_the_grid(prec):
    """alpha = 0, beta = 2 - i, column-major, m = 3, n = 65,540 on device operands: the o0 loop of launch_cscale_dense"""
    n = 65540
    assert n > grid_loops()
    rp, ci = np.array([0, 1, 2, 4]), np.array([0, 3, 1, 2])
    with Handle(prec, 0, 3, 4, rp, ci, cr.crand(np.random.default_rng(4), 4, DTYPE[prec])) as A:
        run_csrmm(prec, A, "n", P.ORDER_COLUMN, n, 4 + 1, 3 + 2, 0.0, 2 - 1j, True)


# ---- ?dotmv ------------------------------------------------------------------------------------------------------------------------

@PREC
def test_dotmv_grid_stride_and_final_loop(prec):
    """bidiagonal, m = n = 262,144 + 300, op = N: launch_cdot (complex_kernels.hip) runs CDOT_BLOCKS = 1024 workgroups of 256, so
    the partial kernel's grid-stride loop takes a second turn for the last 300 entries (weighted 100 x: tail_weighted) and every
    thread of the final kernel adds four partials.  y has the bits of ?mv; host and device results are identical."""
    dtype = DTYPE[prec]
    n = cr.DOT_N
    blocks = source_int("complex_kernels.hip", r"constexpr int CDOT_BLOCKS\s*=\s*(\d+);")
    assert blocks == 1024 == cr.cdot_blocks(n) and n > blocks * 256 and blocks > 256
    assert "i += (long long)gridDim.x * 256" in source("complex_kernels.hip") and "i < count; i += 256" in source("complex_kernels.hip")
    rng = np.random.default_rng(6)
    x, y0 = cr.tail_weighted(n, 8, dtype), cr.crand(rng, n, dtype)
    alpha, beta = np.array([MV_ALPHA], dtype), np.array([MV_BETA], dtype)
    with Handle(prec, 0, n, n, *cr.bidiagonal(n, 7, dtype, 0)) as A:
        d = P.Descr()
        ymv = y0.copy()
        assert fn(prec, "?mv")(OPS["n"], P._ptr(alpha), A.h, d.h, P._ptr(x), P._ptr(beta), P._ptr(ymv)) == 0
        r, c, a = A.coo()
        check_product(prec, "mv", r, c, a, (n, n), alpha[0], x[:, None], beta[0], y0[:, None], int(np.log2(spmv_group(len(a) // n))), ymv)
        y, dot = y0.copy(), np.zeros(1, dtype)
        args = (OPS["n"], scalar(prec, alpha[0]), A.h, d.h)
        assert fn(prec, "?dotmv")(*args, P._ptr(x), scalar(prec, beta[0]), P._ptr(y), P._ptr(dot)) == 0
        assert same_bits(y, ymv)
        ref = cr.cdot(x, y, cr.ext_type(dtype))
        val = report("dot", prec, float(abs(cr.ext_type(dtype)(dot[0]) - ref)) / cr.cdot_bound(x, y, dtype))
        assert val < 1.0
        yd, dd = dev(y0), dev(np.zeros(1, dtype))
        assert fn(prec, "?dotmv")(*args, P._ptr(dev(x)), scalar(prec, beta[0]), P._ptr(yd), P._ptr(dd)) == 0
        assert same_bits(host(yd), y) and same_bits(host(dd), dot)
