"""BSR handles on the GPU: aoclsparse_dmv bit for bit against the oracle's dbsrmv (the reference's chain per scalar row,
level2/aoclsparse_bsrmv_kr.hpp:32-153), float within the raw routine's bound, the complex types against a complex128 product on the
densified matrix within a derived componentwise bound, aoclsparse_convert_bsr followed by a product, and stale values."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from util import EPS32, EPS64, abs_row_sums, laplace5, pkg

pytestmark = pytest.mark.gpu
P = pkg()
L = P.lib()
ST = {v: k for k, v in P.STATUS.items()}
BLOCKS = (0, 1, 2, 40)  # blocks of a block row, cycled
AB = ((1.0, 0.0), (-1.5, 0.25), (1.0, 1.0))


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared cases are read-only)


def block_rows(dim):
    """block-row counts whose scalar rows land on 63, 64, 65, 255, 256, 257 where dim divides them, otherwise on the nearest counts on
    either side of the wavefront (64) and workgroup (256) edges; and one block row alone"""
    out = {1}
    for edge in (64, 256):
        out |= {(edge - 1) // dim, edge // dim + 1}
        if edge % dim == 0:
            out.add(edge // dim)
    return sorted(b for b in out if b > 0)


_CASES = {}


def bsr_case(dim, bm, base, dtype=np.float64):
    """bm x bn blocks (bn != bm), block row i holds BLOCKS[i % 4] blocks at random block columns in random (stored) order; built once"""
    key = (dim, bm, base, np.dtype(dtype).str)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * dim + bm)
        bn = max(bm + 3, 41)
        cnt = [BLOCKS[(i + bm) % 4] for i in range(bm)]
        rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        ci = np.concatenate([rng.choice(bn, c, replace=False) for c in cnt] + [np.zeros(0, np.int64)]).astype(np.int32)
        n = int(rp[-1]) * dim * dim
        v = rng.uniform(-1, 1, n)
        x, y0 = rng.uniform(-1, 1, bn * dim), rng.uniform(-1, 1, bm * dim)
        if np.issubdtype(dtype, np.complexfloating):
            v, x, y0 = (a + 1j * rng.uniform(-1, 1, len(a)) for a in (v, x, y0))
        arrs = tuple(np.ascontiguousarray(a.astype(dtype)) for a in (v, x, y0))
        for a in arrs:
            a.setflags(write=False)
        _CASES[key] = (bn, rp + base, ci + base, np.array(cnt)) + arrs
    return _CASES[key]


def handle(base, bm, bn, dim, rp, ci, v, order=None):
    A = P.BsrMatrix(base, P.ORDER_COLUMN if order is None else order, bm, bn, dim, rp, ci, v)
    assert A.status == 0
    return A


# ---- double: bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3, 4, 5, 7, 8, 16, 9, 17])
def test_dmv_bit_exact(dim):
    k = 0
    for bm in block_rows(dim):
        for base in (0, 1):
            bn, rp, ci, cnt, v, x, y0 = bsr_case(dim, bm, base)
            if int(rp[-1]) == base:  # (one block row with no block: the quick return, covered below)
                continue
            A = handle(base, bm, bn, dim, rp, ci, v)
            d = P.Descr(base=base)
            for alpha, beta in AB:
                want = oracle.dbsrmv(alpha, bm, dim, base, v, ci, rp, x, beta, y0)
                y = y0.copy() if beta != 0 else np.full(bm * dim, np.nan)
                assert P.dmv(P.OP_NONE, alpha, A, d, x, beta, y) == 0
                assert np.array_equal(y, want), (dim, bm, base, alpha, beta, "host")
                k += 1
                if k % 3 == 0:  # device operands: one (alpha, beta) of every handle, in rotation
                    tx, ty = dev(x), dev(y0 if beta != 0 else np.full(bm * dim, np.nan))
                    assert P.dmv(P.OP_NONE, alpha, A, d, tx, beta, ty) == 0
                    torch.cuda.synchronize()
                    assert np.array_equal(ty.cpu().numpy(), want), (dim, bm, base, alpha, beta, "device")
            info = A.spmv_info()
            assert info.kernel == 6 and info.device_resident == 1
            assert info.row_blocks == (bm * dim + 255) // 256


def test_the_handle_has_one_base_and_an_empty_handle_scales_y():
    """mv.cpp:71-72 refuses a descriptor whose base is not the handle's before anything runs, so the base the kernel subtracts
    (mv.cpp:165) is always the handle's: a one-based handle multiplied with a one-based descriptor reads its one-based indices
    right (a zero-based reading would address block column bn), and the zero-based descriptor is refused with y untouched."""
    dim, bm = 4, 17
    bn, rp, ci, cnt, v, x, y0 = bsr_case(dim, bm, 1)
    A = handle(1, bm, bn, dim, rp, ci, v)
    y = y0.copy()
    assert P.dmv(P.OP_NONE, 1.0, A, P.Descr(base=0), x, 0.0, y) == ST["invalid_value"]
    assert np.array_equal(y, y0) and A.spmv_info().device_resident == 0
    assert P.dmv(P.OP_NONE, -1.5, A, P.Descr(base=1), x, 0.25, y) == 0
    assert np.array_equal(y, oracle.dbsrmv(-1.5, bm, dim, 1, v, ci, rp, x, 0.25, y0))
    # mv.cpp:116-121: a handle without blocks gives y = beta * y, whatever the operation
    E = handle(0, 3, 5, 2, np.zeros(4, np.int32), np.zeros(1, np.int32), np.zeros(4))
    y = np.arange(6.0)
    assert P.dmv(P.OP_NONE, 1.0, E, P.Descr(), np.ones(10), 0.5, y) == 0
    assert np.array_equal(y, 0.5 * np.arange(6.0))
    y = np.arange(10.0)
    assert P.dmv(P.OP_TRANSPOSE, 1.0, E, P.Descr(), np.ones(6), 2.0, y) == 0
    assert np.array_equal(y, 2.0 * np.arange(10.0))


def test_dotmv_and_the_runtime_stream():
    dim, bm = 5, 13
    bn, rp, ci, cnt, v, x, y0 = bsr_case(dim, bm, 0)
    A = handle(0, bm, bn, dim, rp, ci, v)
    want = oracle.dbsrmv(2.0, bm, dim, 0, v, ci, rp, x, 0.5, y0)
    y, dot = y0.copy(), np.zeros(1)
    assert L.aoclsparse_ddotmv(P.OP_NONE, 2.0, A.h, P.Descr().h, P._ptr(x), 0.5, P._ptr(y), P._ptr(dot)) == 0
    assert np.array_equal(y, want)
    k = min(bm, bn) * dim
    assert abs(dot[0] - np.dot(x[:k], want[:k])) <= (k + 4) * EPS64 * np.dot(np.abs(x[:k]), np.abs(want[:k]))
    s = torch.cuda.Stream()
    assert L.aoclsparse_mi355_set_stream(ctypes.c_void_p(s.cuda_stream)) == 0
    try:
        with torch.cuda.stream(s):
            tx, ty = dev(x), dev(y0)
            s.synchronize()
            assert P.dmv(P.OP_NONE, 2.0, A, P.Descr(), tx, 0.5, ty) == 0
        s.synchronize()  # the product ran on the runtime's stream: waiting for that stream alone is enough
        assert np.array_equal(ty.cpu().numpy(), want)
    finally:
        assert L.aoclsparse_mi355_set_stream(None) == 0


# ---- float -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [4, 5])
def test_smv_within_the_raw_routines_bound(dim):
    worst = 0.0
    for bm in block_rows(dim):
        for base in (0, 1):
            bn, rp, ci, cnt, v, x, y0 = bsr_case(dim, bm, base, np.float32)
            if int(rp[-1]) == base:
                continue
            A = handle(base, bm, bn, dim, rp, ci, v)
            d = P.Descr(base=base)
            v64, x64, y64 = v.astype(np.float64), x.astype(np.float64), y0.astype(np.float64)
            for alpha, beta in AB:
                want = oracle.dbsrmv(alpha, bm, dim, base, v64, ci, rp, x64, beta, y64)
                scale = abs(alpha) * oracle.dbsrmv(1.0, bm, dim, base, np.abs(v64), ci, rp, np.abs(x64), 0.0, y64) + abs(beta) * np.abs(y64)
                for where in ("host", "device"):
                    y = y0.copy() if beta != 0 else np.full(bm * dim, np.nan, np.float32)
                    ty = dev(y) if where == "device" else y
                    assert P.smv(P.OP_NONE, alpha, A, d, dev(x) if where == "device" else x, beta, ty) == 0
                    torch.cuda.synchronize()
                    got = ty.cpu().numpy() if where == "device" else y
                    err = np.abs(got.astype(np.float64) - want)
                    bound = 64 * EPS32 * scale + 1e-30
                    worst = max(worst, float(np.max(err / bound)))
                    assert np.all(err <= bound), (dim, bm, base, alpha, beta, where)
            assert A.spmv_info().kernel == 6
    print("smv dim %d: max error / bound = %.3g" % (dim, worst))


# ---- complex -----------------------------------------------------------------------------------------------------------------
def abs1(z):
    return np.abs(z.real) + np.abs(z.imag)


def dense(bm, bn, dim, base, rp, ci, v):
    """the matrix of column-major BSR arrays, complex128"""
    A = np.zeros((bm * dim, bn * dim), np.complex128)
    for i in range(bm):
        for p in range(rp[i] - base, rp[i + 1] - base):
            j = ci[p] - base
            A[i * dim:(i + 1) * dim, j * dim:(j + 1) * dim] = v[p * dim * dim:(p + 1) * dim * dim].reshape(dim, dim).T
    return A


def complex_bound(Ad, cnt, dim, alpha, beta, x, y0, eps, tiny):
    """|y - y_ref| <= (2 L + 8) eps S per component, L = dim * (blocks of the block row),
    S = |alpha|_1 sum |a|_1 |x|_1 + |beta|_1 |y0|_1: each component is a real sum of 2 L products, then two complex scalings"""
    Lrow = np.repeat(dim * cnt, dim)
    S = abs1(np.complex128(alpha)) * (abs1(Ad) @ abs1(x.astype(np.complex128))) + abs1(np.complex128(beta)) * abs1(y0.astype(np.complex128))
    return (2 * Lrow + 8) * eps * S + tiny


def check_complex(got, ref, bound, what):
    got = got.astype(np.complex128)
    er, ei = np.abs(got.real - ref.real), np.abs(got.imag - ref.imag)
    assert np.all(er <= bound) and np.all(ei <= bound), what
    return float(max(np.max(er / bound), np.max(ei / bound)))


CAB = ((1.0 + 0j, 0j), (-1.5 + 0.5j, 0.25 - 1j), (1.0 + 0j, 1.0 + 0j))


@pytest.mark.parametrize("t", ["z", "c"])
@pytest.mark.parametrize("dim", [2, 3, 4, 8, 16, 9])
def test_complex_mv_within_the_derived_bound(dim, t):
    dt, C, fn, eps, tiny = ((np.complex128, P.CDouble, L.aoclsparse_zmv, EPS64, 1e-300) if t == "z"
                            else (np.complex64, P.CFloat, L.aoclsparse_cmv, EPS32, 1e-30))
    worst, k = 0.0, 0
    for bm in block_rows(dim):
        for base in (0, 1):
            bn, rp, ci, cnt, v, x, y0 = bsr_case(dim, bm, base, dt)
            if int(rp[-1]) == base:
                continue
            A = handle(base, bm, bn, dim, rp, ci, v)
            d = P.Descr(base=base)
            Ad = dense(bm, bn, dim, base, rp, ci, v)
            for alpha, beta in CAB:
                ref = alpha * (Ad @ x.astype(np.complex128)) + beta * y0.astype(np.complex128)
                bound = complex_bound(Ad, cnt, dim, alpha, beta, x, y0, eps, tiny)
                a, b = C(alpha.real, alpha.imag), C(beta.real, beta.imag)
                y = y0.copy() if beta != 0 else np.full(bm * dim, np.nan + 1j * np.nan, dt)  # beta = 0: y is not read
                assert fn(P.OP_NONE, ctypes.byref(a), A.h, d.h, P._ptr(x), ctypes.byref(b), P._ptr(y)) == 0
                worst = max(worst, check_complex(y, ref, bound, (t, dim, bm, base, alpha, beta, "host")))
                k += 1
                if k % 3 == 0:
                    tx, ty = dev(x), dev(y0 if beta != 0 else np.full(bm * dim, np.nan + 1j * np.nan, dt))
                    assert fn(P.OP_NONE, ctypes.byref(a), A.h, d.h, P._ptr(tx), ctypes.byref(b), P._ptr(ty)) == 0
                    torch.cuda.synchronize()
                    worst = max(worst, check_complex(ty.cpu().numpy(), ref, bound, (t, dim, bm, base, alpha, beta, "device")))
            info = A.spmv_info()
            assert info.kernel == 6 and info.device_resident == 1
    print("%smv dim %d: max error / bound = %.3g" % (t, dim, worst))


def test_zdotmv_on_a_bsr_handle():
    dim, bm = 4, 41  # square: bn = max(bm + 3, 41) would not be, so the arrays are made here
    rng = np.random.default_rng(7)
    cnt = np.array([BLOCKS[i % 4] for i in range(bm)])
    rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    ci = np.concatenate([rng.choice(bm, c, replace=False) for c in cnt]).astype(np.int32)
    v = rng.uniform(-1, 1, int(rp[-1]) * 16) + 1j * rng.uniform(-1, 1, int(rp[-1]) * 16)
    x, y0 = (rng.uniform(-1, 1, bm * dim) + 1j * rng.uniform(-1, 1, bm * dim) for _ in range(2))
    A = handle(0, bm, bm, dim, rp, ci, v)
    alpha, beta = 0.5 - 2j, -1 + 0.5j
    Ad = dense(bm, bm, dim, 0, rp, ci, v)
    ref = alpha * (Ad @ x) + beta * y0
    y, dot = y0.copy(), np.zeros(1, np.complex128)
    assert L.aoclsparse_zdotmv(P.OP_NONE, P.CDouble(alpha.real, alpha.imag), A.h, P.Descr().h, P._ptr(x), P.CDouble(beta.real, beta.imag),
                               P._ptr(y), P._ptr(dot)) == 0
    r = check_complex(y, ref, complex_bound(Ad, cnt, dim, alpha, beta, x, y0, EPS64, 1e-300), "zdotmv")
    # the dot of the y it produced: d = sum conj(x_i) y_i (level1/aoclsparse_dense_dot.hpp:36-49), 2 n real products per component
    n = bm * dim
    assert abs1(dot[0] - np.vdot(x, y)) <= (2 * n + 8) * EPS64 * float(abs1(x) @ abs1(y))
    print("zdotmv: max error / bound = %.3g" % r)


def test_the_complex_check_tells_chain_orders_apart():
    """A condition on the test, not on the kernel: at about 1000 scalar rows and block_dim = 4, summing the blocks of a block row in
    reversed order changes the rounded result in some rows, so a comparison against one order is a comparison of orders.  (The
    kernel itself is held to the derived bound above: its complex multiply-add is four contracted real ones, which numpy's is not.)"""
    dim, bm, bn = 4, 250, 260
    rng = np.random.default_rng(3)
    cnt = np.array([BLOCKS[i % 4] for i in range(bm)])
    rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    ci = np.concatenate([rng.choice(bn, c, replace=False) for c in cnt]).astype(np.int32)
    v = rng.uniform(-1, 1, int(rp[-1]) * 16) + 1j * rng.uniform(-1, 1, int(rp[-1]) * 16)
    x = rng.uniform(-1, 1, bn * dim) + 1j * rng.uniform(-1, 1, bn * dim)

    def chain(order):
        y = np.zeros(bm * dim, np.complex128)
        for i in range(bm):
            ps = list(range(rp[i], rp[i + 1]))
            for p in (ps if order > 0 else ps[::-1]):
                blk = v[p * 16:(p + 1) * 16].reshape(4, 4).T
                for bj in range(4):
                    y[i * 4:(i + 1) * 4] += blk[:, bj] * x[ci[p] * 4 + bj]
        return y

    fwd, rev = chain(1), chain(-1)
    differ = np.flatnonzero(fwd != rev)
    assert len(differ) >= bm * dim // 8, len(differ)
    A = handle(0, bm, bn, dim, rp, ci, v)
    y = np.full(bm * dim, np.nan + 1j * np.nan)
    one, zero = P.CDouble(1, 0), P.CDouble(0, 0)
    assert L.aoclsparse_zmv(P.OP_NONE, ctypes.byref(one), A.h, P.Descr().h, P._ptr(x), ctypes.byref(zero), P._ptr(y)) == 0
    Ad = dense(bm, bn, dim, 0, rp, ci, v)
    check_complex(y, Ad @ x, complex_bound(Ad, cnt, dim, 1 + 0j, 0j, x, y, EPS64, 1e-300), "1000 rows")


# ---- convert_bsr, then a product -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_convert_bsr_then_mv(dim):
    m, rp, ci, v = laplace5(30)
    v = v * (1.0 + 0.25 * np.sin(np.arange(len(v))))  # values that round
    C = P.Matrix(0, m, m, rp, ci, v)
    st, B = P.convert_bsr(C, dim, P.ORDER_COLUMN, P.OP_NONE)
    assert st == 0
    bp, bi, bv = oracle.csr2bsr(m, m, 0, rp, ci, v, dim, False)
    mb = (m + dim - 1) // dim
    assert B.bm == mb and B.bn == mb and np.array_equal(B.row_ptr, bp) and np.array_equal(B.col_ind, bi) and np.array_equal(B.val, bv)
    rng = np.random.default_rng(9)
    x, y0 = rng.uniform(-1, 1, mb * dim), rng.uniform(-1, 1, mb * dim)
    alpha, beta = -0.75, 0.5
    y = y0.copy()
    assert P.dmv(P.OP_NONE, alpha, B, P.Descr(), x, beta, y) == 0
    assert np.array_equal(y, oracle.dbsrmv(alpha, mb, dim, 0, bv, bi, bp, x, beta, y0))
    assert np.array_equal(y[m:], beta * y0[m:])  # the padded tail: rows without an entry
    yc = y0[:m].copy()
    assert P.dmv(P.OP_NONE, alpha, C, P.Descr(), x[:m], beta, yc) == 0
    # the CSR path's componentwise bound: (row length + 4) eps (|alpha| sum |a x| + |beta y0|), for either product
    scale = abs(alpha) * abs_row_sums(rp, ci, v, x[:m]) + abs(beta) * np.abs(y0[:m])
    assert np.all(np.abs(y[:m] - yc) <= 2 * (5 + 4) * EPS64 * scale)
    assert B.spmv_info().kernel == 6


# ---- stale values ------------------------------------------------------------------------------------------------------------
def test_value_change_in_place_then_invalidate():
    dim, bm = 3, 22
    bn, rp, ci, cnt, v, x, y0 = bsr_case(dim, bm, 0)
    v = v.copy()
    A = handle(0, bm, bn, dim, rp, ci, v)
    d = P.Descr()
    y1 = np.zeros(bm * dim)
    assert P.dmv(P.OP_NONE, 1.0, A, d, x, 0.0, y1) == 0
    assert np.array_equal(y1, oracle.dbsrmv(1.0, bm, dim, 0, v, ci, rp, x, 0.0, y0))
    A.val[:] = -2.0 * A.val + 0.125  # the caller's array, which the handle aliases
    assert L.aoclsparse_mi355_invalidate(A.h) == 0
    assert A.spmv_info().device_resident == 0
    y2 = np.zeros(bm * dim)
    assert P.dmv(P.OP_NONE, 1.0, A, d, x, 0.0, y2) == 0
    assert np.array_equal(y2, oracle.dbsrmv(1.0, bm, dim, 0, A.val, ci, rp, x, 0.0, y0))
    assert not np.array_equal(y1, y2) and A.spmv_info().device_resident == 1
