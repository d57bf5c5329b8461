"""?syrkd / ?syprd without a GPU: every status that is decided before the device is touched, in the reference's order
(level3/aoclsparse_syrkd.hpp:170-263, level3/aoclsparse_syprd.cpp:42-168, level3/aoclsparse_syprd.hpp:267-402), and the
restatement of the two double-precision chains that tests/test_sy_dense_gpu.py compares the GPU against bit for bit,
itself checked here against the CPU oracle's dsp2md."""
from ctypes import byref, c_void_p
from fractions import Fraction

import numpy as np
import pytest

import oracle
from util import pkg

P = pkg()
L = P.lib()
ST = {v: k for k, v in P.STATUS.items()}
TYPES = (("s", np.float32), ("d", np.float64), ("c", np.complex64), ("z", np.complex128))
ROW, COL = P.ORDER_ROW, P.ORDER_COLUMN
N, T, H = P.OP_NONE, P.OP_TRANSPOSE, P.OP_CONJ_TRANSPOSE


def fma(a, b, c):
    """correctly rounded a * b + c (exact rational arithmetic, one rounding)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


class Handle:
    """aoclsparse_matrix of any of the four value types from CSR or CSC arrays; keeps the aliased arrays alive"""

    def __init__(self, base, m, n, ptr, ind, val, csc=False):
        self.ptr, self.ind = np.ascontiguousarray(ptr, np.int32), np.ascontiguousarray(ind, np.int32)
        self.val = np.ascontiguousarray(val)
        self.t = {np.dtype(d): t for t, d in TYPES}[self.val.dtype]
        self.h = c_void_p()
        nnz = int(self.ptr[n if csc else m]) - base
        fn = getattr(L, "aoclsparse_create_%s%s" % (self.t, "csc" if csc else "csr"))
        self.status = fn(byref(self.h), base, m, n, nnz, P._ptr(self.ptr), P._ptr(self.ind), P._ptr(self.val))
        assert self.status == 0, P.STATUS[self.status]

    def __del__(self):
        try:
            if self.h:
                L.aoclsparse_destroy(byref(self.h))
        except Exception:
            pass


def scalar(t, v):
    v = complex(v)
    return {"s": v.real, "d": v.real, "c": P.CFloat(v.real, v.imag), "z": P.CDouble(v.real, v.imag)}[t]


def syrkd(t, op, A, alpha, beta, C, layout, ldc):
    return P.STATUS[getattr(L, "aoclsparse_%ssyrkd" % t)(op, A, scalar(t, alpha), scalar(t, beta), P._ptr(C), layout, ldc)]


def syprd(t, op, A, B, order_b, ldb, alpha, beta, C, order_c, ldc):
    return P.STATUS[getattr(L, "aoclsparse_%ssyprd" % t)(op, A, P._ptr(B), order_b, ldb, scalar(t, alpha), scalar(t, beta),
                                                          P._ptr(C), order_c, ldc)]


def small(dt, base=0, sort=True):
    """3 x 4: rows {0, 2}, {1}, {0, 3}; unsorted: row 0 stored as {2, 0}"""
    ptr = np.array([0, 2, 3, 5], np.int32) + base
    ind = np.array([0, 2, 1, 0, 3] if sort else [2, 0, 1, 0, 3], np.int32) + base
    return 3, 4, ptr, ind, (np.arange(5) + 1.0).astype(dt)


def tcsr(dt):
    one = np.ones(2, dt)
    return P.TcsrMatrix(0, 2, [0, 1, 2], [0, 1], one, [0, 1, 2], [0, 1], one)


def bsr(dt):
    return P.BsrMatrix(0, COL, 1, 1, 2, [0, 1], [0], np.ones(4, dt))


@pytest.mark.parametrize("t,dt", TYPES, ids=[t for t, _ in TYPES])
def test_syrkd_statuses_in_the_reference_order(t, dt):
    m, n, ptr, ind, val = small(dt)
    A, U = Handle(0, m, n, ptr, ind, val), Handle(0, *small(dt, sort=False))
    other = Handle(0, *small(np.float32 if dt != np.float32 else np.float64))
    A1 = Handle(1, *small(dt, base=1))
    csc_ptr, csc_ind, csc_val = np.array([0, 2, 2, 3], np.int32), np.array([0, 2, 1], np.int32), np.ones(3, dt)
    K = Handle(0, 4, 3, csc_ptr, csc_ind, csc_val, csc=True)  # 4 x 3 from sorted CSC arrays
    KU = Handle(0, 4, 3, csc_ptr, np.array([2, 0, 1], np.int32), csc_val, csc=True)  # column 0 stored as rows {2, 0}
    TC, BS = tcsr(dt), bsr(dt)
    C = np.zeros(64, dt)
    cplx = t in "cz"
    big = 1 << 30
    table = [  # (call, expected, line of syrkd.hpp)
        (dict(A=None), "invalid_pointer", 179),
        (dict(C=None), "invalid_pointer", 179),
        (dict(A=None, op=7, layout=7), "invalid_pointer", 179),
        (dict(op=7, layout=7), "invalid_value", 182),
        (dict(op=110, A=TC.h), "invalid_value", 182),
        (dict(layout=7, A=TC.h), "invalid_value", 186),
        (dict(A=TC.h, ldc=0), "not_implemented", 189),  # TCSR: a handle without a CSR
        (dict(A=BS.h, ldc=0), "not_implemented", 189),  # BSR
        (dict(A=other.h, op=T, ldc=0), "wrong_type", 192),
        (dict(op=T, ldc=0), "not_implemented" if cplx else "invalid_value", 197),  # complex + transpose; real: falls to :253
        (dict(A=U.h, op=T if not cplx else H, ldc=0), "unsorted_input", 239),
        (dict(A=U.h, op=N, ldc=0), "invalid_value", 253),  # unsorted rows are legal for op = none
        (dict(A=KU.h, op=N, ldc=0), "unsorted_input", 239),  # from CSC the reference's effective op is flipped (:231-236)
        (dict(A=KU.h, op=H, ldc=0), "invalid_value", 253),
        (dict(op=N, ldc=m - 1), "invalid_value", 253),  # m_C = m for op = none
        (dict(op=H, ldc=n - 1), "invalid_value", 253),  # m_C = n for op = H
        (dict(A=A1.h, op=H, ldc=n - 1), "invalid_value", 253),
        (dict(A=K.h, op=N, ldc=3), "invalid_value", 253),  # CSC handle, 4 x 3: m_C = 4
        (dict(A=K.h, op=H, ldc=2), "invalid_value", 253),  # m_C = 3
        (dict(op=N, ldc=big), "invalid_size", 260),  # 3 * 2^30 overflows
        (dict(op=H, ldc=big, layout=COL), "invalid_size", 260),
    ]
    for kw, want, line in table:
        a = dict(op=N, A=A.h, alpha=1.0, beta=0.0, C=C, layout=ROW, ldc=8)
        a.update(kw)
        got = syrkd(t, a["op"], a["A"], a["alpha"], a["beta"], a["C"], a["layout"], a["ldc"])
        assert got == want, (kw, line, got)
    assert not C.any()


@pytest.mark.parametrize("t,dt", TYPES, ids=[t for t, _ in TYPES])
def test_syprd_statuses_in_the_reference_order(t, dt):
    m, n, ptr, ind, val = small(dt)
    A = Handle(0, m, n, ptr, ind, val)
    other = Handle(0, *small(np.float32 if dt != np.float32 else np.float64))
    E = Handle(0, 0, 4, np.array([0], np.int32), np.zeros(1, np.int32), np.zeros(1, dt))  # m = 0
    K = Handle(0, 4, 3, np.array([0, 2, 2, 3], np.int32), np.array([0, 2, 1], np.int32), np.ones(3, dt), csc=True)
    TC, BS = tcsr(dt), bsr(dt)
    B, C = np.zeros(64, dt), np.full(64, 7.0, dt)
    cplx = t in "cz"
    big = 1 << 30
    table = [  # (call, expected, line of syprd.hpp unless it says .cpp)
        (dict(A=None), "invalid_pointer", ".cpp:55"),
        (dict(B=None), "invalid_pointer", ".cpp:55"),
        (dict(C=None, op=7), "invalid_pointer", ".cpp:55"),
        (dict(A=other.h, op=7, order_b=7), "wrong_type", ".cpp:60"),
        (dict(op=7, order_b=7), "invalid_value", 282),
        (dict(order_b=7, order_c=COL), "invalid_value", 286),
        (dict(order_c=7, order_b=COL), "invalid_value", 289),
        (dict(order_b=ROW, order_c=COL, A=TC.h), "invalid_operation", 292),
        (dict(order_b=COL, order_c=ROW, A=TC.h), "invalid_operation", 292),
        (dict(A=TC.h, op=T), "invalid_pointer", 304),  # TCSR: a handle without a CSR, before the complex + T rule
        (dict(A=BS.h, op=T), "invalid_pointer", 304),  # BSR
        (dict(op=T, ldb=0), "not_implemented" if cplx else "invalid_size", 319),
        (dict(A=E.h, ldb=0, ldc=0), "success", 357),  # m = 0 returns before the leading dimensions
        (dict(alpha=0.0, beta=1.0, ldb=0, ldc=0), "success", 368),  # alpha = 0 and beta = 1 likewise
        (dict(alpha=0.0, beta=0.5, ldb=0), "invalid_size", 381),
        (dict(op=N, ldb=n - 1), "invalid_size", 381),  # op = none: B is n x n
        (dict(op=H, ldb=m - 1), "invalid_size", 381),  # op = H: B is m x m
        (dict(op=N, ldb=n, ldc=m - 1), "invalid_size", 389),  # C is m x m
        (dict(op=H, ldb=m, ldc=n - 1), "invalid_size", 389),  # C is n x n
        (dict(A=K.h, op=N, ldb=2), "invalid_size", 381),  # CSC handle, 4 x 3: the caller's op (:373-376), B is 3 x 3
        (dict(A=K.h, op=N, ldb=3, ldc=3), "invalid_size", 389),  # C is 4 x 4
        (dict(A=K.h, op=H, ldb=3), "invalid_size", 381),  # B is 4 x 4
        (dict(op=N, ldc=big), "invalid_size", 398),
        (dict(op=N, ldb=big), "invalid_size", 398),
    ]
    if cplx:
        # syprd.cpp:125-126 hands alpha and beta on whole (syrkd.cpp:88-89 keeps the real parts: checked on the GPU, where it
        # shows): an imaginary part keeps the call from the quick return of :368
        table += [(dict(alpha=1j, beta=1.0, ldb=0), "invalid_size", 368), (dict(alpha=0.0, beta=1 + 1j, ldb=0), "invalid_size", 368)]
    for kw, want, line in table:
        a = dict(op=N, A=A.h, B=B, order_b=ROW, ldb=8, alpha=1.0, beta=0.0, C=C, order_c=ROW, ldc=8)
        a.update(kw)
        got = syprd(t, a["op"], a["A"], a["B"], a["order_b"], a["ldb"], a["alpha"], a["beta"], a["C"], a["order_c"], a["ldc"])
        assert got == want, (kw, line, got)
    assert (C == 7.0).all()


# ---- the two double-precision chains, restated ---------------------------------------------------------------------------
def rows_of(m, base, ptr, ind, val):
    """[[(column, value), ...] per row], zero-based, in stored order"""
    return [[(int(ind[p]) - base, float(val[p])) for p in range(ptr[i] - base, ptr[i + 1] - base)] for i in range(m)]


def stable_transpose(n, rows):
    out = [[] for _ in range(n)]
    for r, row in enumerate(rows):
        for c, v in row:
            out[c].append((r, v))
    return out


def dsyrkd_chain(op, m, n, base, ptr, ind, val, alpha, beta, C0):
    """syrkd.hpp:86-165 on M = A (op = T) or M = the stable transpose of A (op = none): C(i,j), j >= i, starts at beta*C0
    (0 for beta = 0) and receives fma(alpha*M(r,i) rounded, M(r,j), C) for r ascending.  C0: m_C x m_C; returns the same shape,
    the strict lower triangle untouched."""
    rows = rows_of(m, base, ptr, ind, val)
    M = rows if op != N else stable_transpose(n, rows)
    k = n if op != N else m
    C = np.array(C0, np.float64)
    for i in range(k):
        for j in range(i, k):
            C[i, j] = beta * C[i, j] if beta != 0 else 0.0
    for r, row in enumerate(M):  # for every i the rows r ascend; the elements C(i, .) of different i are independent
        for i, a in row:
            va = alpha * a
            for j, w in row:
                if j >= i:
                    C[i, j] = fma(va, w, C[i, j])
    return C


def dsyprd_chain(op, m, n, base, ptr, ind, val, B, alpha, beta, C0, rowmajor):
    """syprd.hpp:111-153 (row-major) / :227-260 (column-major) on M = A (op = none) or its stable transpose.  B: the full
    square array, of which only the upper triangle is read; C0 as in dsyrkd_chain."""
    rows = rows_of(m, base, ptr, ind, val)
    M = rows if op == N else stable_transpose(n, rows)
    mc, nin = (m, n) if op == N else (n, m)
    C = np.array(C0, np.float64)
    for i in range(mc):
        for j in range(i, mc):
            C[i, j] = beta * C[i, j] if beta != 0 else 0.0
    if alpha == 0:
        return C
    for i in range(mc):
        t = [0.0] * nin
        for j in range(nin):
            for c, a in M[i]:
                b = float(B[min(j, c), max(j, c)])
                t[j] = fma(b, alpha * a, t[j]) if rowmajor else fma(a, b, t[j])
            if not rowmajor:
                t[j] *= alpha
        for j in range(i, mc):
            acc = C[i, j]
            for c, a in M[j]:
                acc = fma(t[c], a, acc)
            C[i, j] = acc
    return C


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("shape", [(23, 17), (17, 23)])
def test_restated_dsyrkd_is_the_oracles_dsp2md_upper_triangle(shape, base):
    from util import random_csr

    m, n = shape
    ptr, ind, val = random_csr(5 * m + base, m, n, lambda rng, i: rng.integers(0, 7), base=base)
    a = (m, n, base, ptr, ind, val)
    rng = np.random.default_rng(m)
    for op, k in ((T, n), (N, m)):
        C0 = rng.uniform(-1, 1, (k, k))
        for alpha, beta in ((1.5, 0.0), (1.5, -0.5), (-0.75, 1.0)):
            mine = dsyrkd_chain(op, m, n, base, ptr, ind, val, alpha, beta, C0)
            ref = oracle.dsp2md(a, op == T, a, op == N, alpha, beta, C0, True, k).reshape(k, k)
            up = np.triu_indices(k)
            assert np.array_equal(mine[up], ref[up]), (op, alpha, beta)
            assert np.array_equal(np.tril(mine, -1), np.tril(C0, -1))


def test_restated_dsyprd_with_b_the_identity_is_the_product_itself():
    """B = I makes stage 1 exact (T = alpha*M rounded once), so the row-major chain is dsyrkd's with the roles of the two
    factors kept: the same upper triangle as the oracle's dsp2md(A, N, A, T) for op = none."""
    from util import random_csr

    m, n, base = 19, 13, 0
    ptr, ind, val = random_csr(3, m, n, lambda rng, i: rng.integers(0, 6), base=base)
    a = (m, n, base, ptr, ind, val)
    C0 = np.random.default_rng(1).uniform(-1, 1, (m, m))
    mine = dsyprd_chain(N, m, n, base, ptr, ind, val, np.eye(n), 1.5, -0.5, C0, True)
    ref = oracle.dsp2md(a, False, a, True, 1.5, -0.5, C0, True, m).reshape(m, m)
    up = np.triu_indices(m)
    assert np.array_equal(mine[up], ref[up])
