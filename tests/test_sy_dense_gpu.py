"""?syrkd / ?syprd on the GPU.  Double precision bit for bit: dsyrkd against the upper triangle of the CPU oracle's dsp2md,
dsyprd against the chains restated in tests/test_sy_dense_cpu.py.  The other three types within the derived componentwise
bound |got - exact| <= (L + 4) u (|alpha| S + |beta| |C0|): S the same product formed from absolute values, L the longest
chain of the test matrix (for syprd the sum of the two nested chains), u the real type's epsilon, doubled for complex
types (a complex product is two real ones per component); `exact` is evaluated one precision up.  The lower triangle and
the padding of C, and the strict lower triangle of B, are NaN before the call and must come back bitwise unchanged."""
import functools
import glob
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle
from test_sy_dense_cpu import COL, H, Handle, N, ROW, T, dsyprd_chain, dsyrkd_chain, syprd, syrkd
from util import ROOT, pkg

pytestmark = pytest.mark.gpu
P = pkg()
L = P.lib()
SHAPES = ((45, 70), (70, 45))
WIDER = {np.dtype(np.float32): np.float64, np.dtype(np.float64): np.longdouble, np.dtype(np.complex64): np.complex128, np.dtype(np.complex128): np.clongdouble}


@functools.lru_cache(maxsize=None)
def pattern(m, n):
    """sorted CSR pattern, zero-based: rows 3, 10 and m - 1 and columns 2, 11 and n - 2 are empty; every fifth row ends exactly
    at its diagonal; on 45 x 70 row 7 holds every non-empty column (67 entries: the lanes wrap), on 70 x 45 column 5 sits in
    every non-empty row (67 entries of the transpose's row)"""
    rng = np.random.default_rng(100 * m + n)
    empty_r, empty_c = {3, 10, m - 1}, {2, 11, n - 2}
    live = [c for c in range(n) if c not in empty_c]
    rows = []
    for i in range(m):
        if i in empty_r:
            rows.append([])
            continue
        cols = set(rng.choice(live, size=int(rng.integers(2, 8)), replace=False).tolist())
        if i % 5 == 0 and i < n and i not in empty_c:
            cols = {c for c in cols if c < i} | {i}
        if m < n and i == 7:
            cols = set(live)
        if m > n:
            cols.add(5)
        rows.append(sorted(cols))
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ind = np.array([c for r in rows for c in r], np.int32)
    assert max(len(r) for r in rows) > 64 or np.bincount(ind, minlength=n).max() > 64
    return ptr, ind


def values(k, dt, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, k)
    if np.dtype(dt).kind == "c":
        v = v + 1j * rng.uniform(-1, 1, k)
    return v.astype(dt)


def matrix(shape, dt, base=0):
    m, n = shape
    ptr, ind = pattern(m, n)
    return m, n, base, ptr + base, ind + base, values(len(ind), dt, m)


def dense(m, n, base, ptr, ind, val, dt):
    D = np.zeros((m, n), dt)
    rows = np.repeat(np.arange(m), np.diff(ptr))
    np.add.at(D, (rows, ind - base), val.astype(dt))
    return D


def positions(k, ld, rowmajor):
    """flat positions of the upper triangle, in np.triu_indices order"""
    i, j = np.triu_indices(k)
    return i * ld + j if rowmajor else i + j * ld


def embed(Cm, ld, rowmajor):
    """k x k matrix -> flat k x ld storage: the upper triangle at its place, NaN everywhere else"""
    k = Cm.shape[0]
    S = np.full(k * ld, np.nan, Cm.dtype)
    S[positions(k, ld, rowmajor)] = Cm[np.triu_indices(k)]
    return S


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def run(call, S, dev, Bs=None):
    """call(C, B) on host arrays or on device copies -> (status, C after, B after)"""
    if not dev:
        C, B = S.copy(), None if Bs is None else Bs.copy()
        st = call(C, B)
        return st, C, B
    C, B = torch.from_numpy(S.copy()).cuda(), None if Bs is None else torch.from_numpy(Bs.copy()).cuda()
    st = call(C, B)
    torch.cuda.synchronize()
    return st, C.cpu().numpy(), None if B is None else B.cpu().numpy()


def check_untouched(before, after, pos):
    keep = np.ones(before.shape, bool)
    keep[pos] = False
    assert np.array_equal(bits(before[keep]), bits(after[keep])), "bytes outside the upper triangle changed"


COMBOS = [(base, pad, rowmajor, alpha, beta, dev) for base in (0, 1) for pad in (0, 3) for rowmajor in (True, False)
          for alpha in (0.0, 1.5) for beta in (0.0, 1.0, -0.5) for dev in (False, True)]


# ---- double precision, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [N, T], ids=["N", "T"])
@pytest.mark.parametrize("shape", SHAPES, ids=["45x70", "70x45"])
def test_dsyrkd_bit_exact_against_the_oracle(shape, op):
    m, n = shape
    k = m if op == N else n
    C0 = np.random.default_rng(k).uniform(-1, 1, (k, k))
    a0 = matrix(shape, np.float64)
    up = np.triu_indices(k)
    ref = {(al, be): oracle.dsp2md(a0, op == T, a0, op == N, al, be, C0, True, k).reshape(k, k)[up]
           for al in (0.0, 1.5) for be in (0.0, 1.0, -0.5)}
    assert np.array_equal(ref[(1.5, -0.5)], dsyrkd_chain(op, *a0, 1.5, -0.5, C0)[up])  # the two references agree here too
    for base in (0, 1):
        A = Handle(base, m, n, *matrix(shape, np.float64, base)[3:])
        for b, pad, rowmajor, alpha, beta, dev in COMBOS:
            if b != base:
                continue
            ld, S = k + pad, embed(C0, k + pad, rowmajor)
            st, C, _ = run(lambda C, B: syrkd("d", op, A.h, alpha, beta, C, ROW if rowmajor else COL, ld), S, dev)
            assert st == "success"
            pos = positions(k, ld, rowmajor)
            assert np.array_equal(C[pos], ref[(alpha, beta)]), (base, pad, rowmajor, alpha, beta, dev)
            check_untouched(S, C, pos)


@pytest.mark.parametrize("rowmajor", [True, False], ids=["row", "col"])
@pytest.mark.parametrize("op", [N, T], ids=["N", "T"])
@pytest.mark.parametrize("shape", SHAPES, ids=["45x70", "70x45"])
def test_dsyprd_bit_exact_against_the_restated_chain(shape, op, rowmajor):
    m, n = shape
    mc, nin = (m, n) if op == N else (n, m)
    rng = np.random.default_rng(mc)
    C0, Bm = rng.uniform(-1, 1, (mc, mc)), rng.uniform(-1, 1, (nin, nin))
    a0 = matrix(shape, np.float64)
    up = np.triu_indices(mc)
    ref = {(al, be): dsyprd_chain(op, *a0, Bm, al, be, C0, rowmajor)[up] for al in (0.0, 1.5) for be in (0.0, 1.0, -0.5)}
    ldb = nin + 2
    Bs = embed(Bm, ldb, rowmajor)  # strict lower triangle and padding: NaN, so any read of them shows in C
    order = ROW if rowmajor else COL
    for base in (0, 1):
        A = Handle(base, m, n, *matrix(shape, np.float64, base)[3:])
        for b, pad, rm, alpha, beta, dev in COMBOS:
            if b != base or rm != rowmajor:
                continue
            ld, S = mc + pad, embed(C0, mc + pad, rowmajor)
            st, C, B = run(lambda C, B: syprd("d", op, A.h, B, order, ldb, alpha, beta, C, order, ld), S, dev, Bs)
            assert st == "success"
            pos = positions(mc, ld, rowmajor)
            assert np.array_equal(C[pos], ref[(alpha, beta)]), (base, pad, alpha, beta, dev)
            check_untouched(S, C, pos)
            assert np.array_equal(bits(B), bits(Bs))


# ---- the other types: the derived bound --------------------------------------------------------------------------------------
def herm_upper(Bm):
    return np.triu(Bm) + np.triu(Bm, 1).conj().T


def exact_and_bound(family, op, D, Bm, alpha, beta, C0, dt):
    """the dense formulas of syrkd.hpp:213-218 / syprd.hpp:306-311 one precision up, and the bound of the module docstring"""
    W = WIDER[np.dtype(dt)]
    cplx = np.dtype(dt).kind == "c"
    Dw = D.astype(W)
    left, right = (Dw, Dw.conj().T) if op == N else (Dw.conj().T, Dw)
    lens = np.count_nonzero(D, axis=1).max() if op == N else np.count_nonzero(D, axis=0).max()  # the longest row of op(A)
    if family == "syrkd":
        prod, S = left @ right, np.abs(left) @ np.abs(right)
        chain = lens  # C(i,j) sums over the entries of row i of op(A)
    else:
        Bh = herm_upper(Bm.astype(W))
        prod, S = left @ Bh @ right, np.abs(left) @ np.abs(Bh) @ np.abs(right)
        chain = 2 * lens
    exact = W(alpha) * prod + (W(beta) * C0.astype(W) if beta != 0 else 0)
    u = float(np.finfo(dt).eps) * (2 if cplx else 1)
    return exact, (chain + 4) * u * (abs(alpha) * S + abs(beta) * np.abs(C0)).astype(np.float64)


def within(got, exact, bound):
    d = got.astype(exact.dtype) - exact
    parts = (d.real, d.imag) if np.iscomplexobj(d) else (d,)
    return all((np.abs(p).astype(np.float64) <= bound).all() for p in parts)


@pytest.mark.parametrize("family", ["syrkd", "syprd"])
@pytest.mark.parametrize("t,dt", [("s", np.float32), ("c", np.complex64), ("z", np.complex128)], ids=["s", "c", "z"])
@pytest.mark.parametrize("shape", SHAPES, ids=["45x70", "70x45"])
def test_other_types_within_the_derived_bound(shape, t, dt, family):
    m, n = shape
    cplx = t in "cz"
    a0 = matrix(shape, dt)
    D = dense(*a0, dt)
    A = {base: Handle(base, m, n, *matrix(shape, dt, base)[3:]) for base in (0, 1)}
    for op in (N, H if cplx else T):
        mc, nin = (m, n) if op == N else (n, m)
        C0, Bm = values(mc * mc, dt, 1).reshape(mc, mc), values(nin * nin, dt, 2).reshape(nin, nin)
        up = np.triu_indices(mc)
        for base, pad, rowmajor, al, beta, dev in COMBOS:
            if beta == 1.0 and al == 0.0:
                continue  # (syprd returns at once; covered bit for bit in double)
            # complex: syprd takes alpha and beta whole; syrkd keeps their real parts (syrkd.cpp:88-89, :109-110)
            alpha, b = (al + 0.5j if al else 0.0, beta + 0.25j if beta else 0.0) if cplx else (al, beta)
            used = (alpha, b) if family == "syprd" or not cplx else (complex(alpha).real, complex(b).real)
            exact, bound = exact_and_bound(family, op, D, Bm, used[0], used[1], C0, dt)
            ld, order = mc + pad, ROW if rowmajor else COL
            S = embed(C0, ld, rowmajor)
            if family == "syrkd":
                st, C, _ = run(lambda C, B: syrkd(t, op, A[base].h, alpha, b, C, order, ld), S, dev)
            else:
                Bs = embed(Bm, nin + 2, rowmajor)
                st, C, B = run(lambda C, B: syprd(t, op, A[base].h, B, order, nin + 2, alpha, b, C, order, ld), S, dev, Bs)
                assert np.array_equal(bits(B), bits(Bs))
            assert st == "success"
            pos = positions(mc, ld, rowmajor)
            assert within(C[pos], exact[up], bound[up]), (op, base, pad, rowmajor, alpha, b, dev)
            check_untouched(S, C, pos)
    if cplx:  # complex + transpose: not_implemented (syrkd.hpp:197, syprd.hpp:319)
        C, B = np.zeros(80 * 80, dt), np.zeros(80 * 80, dt)
        assert syrkd(t, T, A[0].h, 1.0, 0.0, C, ROW, 80) == "not_implemented"
        assert syprd(t, T, A[0].h, B, ROW, 80, 1.0, 0.0, C, ROW, 80) == "not_implemented"


@pytest.mark.parametrize("t,dt", [("d", np.float64), ("z", np.complex128)], ids=["d", "z"])
@pytest.mark.parametrize("shape", SHAPES, ids=["45x70", "70x45"])
def test_handles_made_from_csc(shape, t, dt):
    """the CSC rows of the two dispatch tables: in terms of the caller's matrix the same dense formulas"""
    m, n = shape
    a0 = matrix(shape, dt)
    D = dense(*a0, dt)
    tm, tn, _, tp, ti, tv = matrix((n, m), dt, 1)  # the CSR arrays of an n x m matrix are the CSC arrays of its m x n transpose
    K = Handle(1, tn, tm, tp, ti, tv, csc=True)
    Dk = dense(tm, tn, 1, tp, ti, tv, dt).T
    assert Dk.shape == D.shape
    for op in (N, H if t == "z" else T):
        mc, nin = (m, n) if op == N else (n, m)
        C0, Bm = values(mc * mc, dt, 3).reshape(mc, mc), values(nin * nin, dt, 4).reshape(nin, nin)
        up, pos = np.triu_indices(mc), positions(mc, mc + 1, True)
        S = embed(C0, mc + 1, True)
        alpha, beta = (1.5 + 0.5j, -0.5 + 0.25j) if t == "z" else (1.5, -0.5)
        for dev in (False, True):
            st, C, _ = run(lambda C, B: syrkd(t, op, K.h, alpha, beta, C, ROW, mc + 1), S, dev)
            exact, bound = exact_and_bound("syrkd", op, Dk, Bm, complex(alpha).real, complex(beta).real, C0, dt)
            assert st == "success" and within(C[pos], exact[up], bound[up]), ("syrkd", op, dev)
            check_untouched(S, C, pos)
            Bs = embed(Bm, nin, True)
            st, C, _ = run(lambda C, B: syprd(t, op, K.h, B, ROW, nin, alpha, beta, C, ROW, mc + 1), S, dev, Bs)
            exact, bound = exact_and_bound("syprd", op, Dk, Bm, alpha, beta, C0, dt)
            assert st == "success" and within(C[pos], exact[up], bound[up]), ("syprd", op, dev)
            check_untouched(S, C, pos)


def test_unsorted_rows_and_repeated_columns():
    m, n = 45, 70
    _, _, _, ptr, ind, val = matrix((m, n), np.float64)
    rng = np.random.default_rng(9)
    uind, uval = ind.copy(), val.copy()
    for i in range(m):  # the same matrix, every row in a random order
        p = rng.permutation(ptr[i + 1] - ptr[i]) + ptr[i]
        uind[ptr[i]:ptr[i + 1]], uval[ptr[i]:ptr[i + 1]] = ind[p], val[p]
    U = Handle(0, m, n, ptr, uind, uval)
    C0 = rng.uniform(-1, 1, (m, m))
    up, pos = np.triu_indices(m), positions(m, m, True)
    S = embed(C0, m, True)
    # op = none succeeds and walks the reference's chain: r ascends along the SORTED row (the csr2csc copy of syrkd.hpp:338)
    ref = dsyrkd_chain(N, m, n, 0, ptr, ind, val, 1.5, -0.5, C0)[up]
    for dev in (False, True):
        st, C, _ = run(lambda C, B: syrkd("d", N, U.h, 1.5, -0.5, C, ROW, m), S, dev)
        assert st == "success" and np.array_equal(C[pos], ref)
    assert syrkd("d", T, U.h, 1.5, -0.5, np.zeros(n * n), ROW, n) == "unsorted_input"
    # a fully sorted row may repeat a column (the handle check lets it through): lanes must not meet on an element of C
    dptr = np.array([0, 4, 6, 9], np.int32)
    dind = np.array([0, 1, 1, 3, 1, 2, 0, 3, 3], np.int32)
    dval = rng.uniform(-1, 1, 9)
    R = Handle(0, 3, 4, dptr, dind, dval)
    D = dense(3, 4, 0, dptr, dind, dval, np.float64)
    for op, k in ((N, 3), (T, 4)):
        Ck = rng.uniform(-1, 1, (k, k))
        st, C, _ = run(lambda C, B: syrkd("d", op, R.h, 1.5, -0.5, C, ROW, k), embed(Ck, k, True), False)
        exact = 1.5 * (D @ D.T if op == N else D.T @ D) - 0.5 * Ck
        scale = 1.5 * (np.abs(D) @ np.abs(D).T if op == N else np.abs(D).T @ np.abs(D)) + 0.5 * np.abs(Ck)
        i = np.triu_indices(k)
        assert st == "success" and (np.abs(C[positions(k, k, True)] - exact[i]) <= (9 + 4) * np.finfo(np.float64).eps * scale[i]).all()


def test_empty_matrix_with_beta_zero_zeroes_the_upper_triangle():
    A = Handle(0, 5, 4, np.zeros(6, np.int32), np.zeros(1, np.int32), np.zeros(1))
    for op, k in ((N, 5), (T, 4)):
        for rowmajor in (True, False):
            for dev in (False, True):
                S = embed(np.ones((k, k)), k + 2, rowmajor)
                st, C, _ = run(lambda C, B: syrkd("d", op, A.h, 1.5, 0.0, C, ROW if rowmajor else COL, k + 2), S, dev)
                pos = positions(k, k + 2, rowmajor)
                assert st == "success" and not C[pos].any() and not np.signbit(C[pos]).any()
                check_untouched(S, C, pos)


def test_reference_samples_built_and_pass():
    d = os.path.join(ROOT, "oracle", "_ref", "samples")
    if not glob.glob(os.path.join(d, "sample_*")):
        return  # no reference on the build machine: nothing was built (test_reference_samples_run_unchanged says the same)
    for name in ("sample_dsyrkd", "sample_syprd"):
        exe = os.path.join(d, name)
        assert os.path.exists(exe), name
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.stdout[-400:], r.stderr[-400:])
