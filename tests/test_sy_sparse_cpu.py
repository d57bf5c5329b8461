"""aoclsparse_syrk / aoclsparse_sypr without a GPU.

1. A plain restatement of the reference's algorithms (level3/aoclsparse_syrk.hpp:46-113, :216-332; level3/aoclsparse_sypr.hpp:
   51-109 first-touch accumulation, :120-243 the linked-list walk, :253-398 the symmetrised stage 1, :400-527 the upper-triangle
   A^T*B), which tests/test_sy_sparse_gpu.py compares the GPU against: structure always, double-precision values bit for bit.  It is
   checked here against what the reference's two example programs expect (tests/golden/sy_sparse_kats.json) and against dense
   numpy products: the pattern must contain the numeric pattern and the values must lie within (L + 4) u S, with S the same
   product of absolute values and L the longest chain (for sypr the sum of the two nested chains).
2. Every status that is decided before the device is touched, in the reference's order (aoclsparse_syrk.cpp:38-58, syrk.hpp:
   124-214; aoclsparse_sypr.cpp:33-46, sypr.hpp:548-729), through the library."""
import json
import os
from ctypes import byref, c_int, c_void_p
from fractions import Fraction

import numpy as np
import pytest

from test_sy_dense_cpu import Handle, bsr, tcsr
from util import ROOT, pkg, random_csr

P = pkg()
L = P.lib()
TYPES = (("s", np.float32), ("d", np.float64), ("c", np.complex64), ("z", np.complex128))
DT = dict(TYPES)
N, T, H = P.OP_NONE, P.OP_TRANSPOSE, P.OP_CONJ_TRANSPOSE
OPS = {"N": N, "T": T, "H": H}
FULL, COUNT, FINAL = P.STAGE_FULL, P.STAGE_NNZ_COUNT, P.STAGE_FINALIZE
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "sy_sparse_kats.json")))


# ---- arithmetic of the restatement: double precision, one rounding per fused multiply-add -----------------------------------
def fma(a, b, c):
    """correctly rounded a * b + c"""
    if a == 0 or b == 0:
        return a * b + c  # (keeps the sign rules of zero; the product is exact)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def mul(a, b, cplx):
    return cfma(a, b, 0j) if cplx else a * b


def cfma(a, b, c):
    """the multiply-add on complex values: four real ones, in the order of spgemm_kernels.hip's sp_fma"""
    re = fma(-a.imag, b.imag, fma(a.real, b.real, c.real))
    im = fma(a.imag, b.real, fma(a.real, b.imag, c.imag))
    return complex(re, im)


def madd(a, b, c, cplx):
    return cfma(a, b, c) if cplx else fma(a, b, c)


def cj(v, on):
    return v.conjugate() if on else v


# ---- the pieces ----------------------------------------------------------------------------------------------------------------
def rows_of(m, base, ptr, ind, val):
    """[[(column, value), ...] per row], zero-based, in stored order"""
    cplx = np.iscomplexobj(val)
    return [[(int(ind[p]) - base, complex(val[p]) if cplx else float(val[p])) for p in range(ptr[i] - base, ptr[i + 1] - base)]
            for i in range(m)]


def stable_transpose(n, rows):
    """aoclsparse_csr2csc_template: counting sort, so the rows of the transpose list their columns ascending"""
    out = [[] for _ in range(n)]
    for r, row in enumerate(rows):
        for c, v in row:
            out[c].append((r, v))
    return out


def walk(k, rows, first=None, last=None):
    """oftrans (sypr.hpp:120-243): for i = 0 .. k - 1 the (row, position) pairs in the order the reference visits them.  Rows are
    pushed, ascending, onto the stack of their first column; the stack of column i is walked from the top; a visited row moves to
    the stack of its next entry's column at that moment.  Only positions [first[r], last[r]) of row r take part.  A row that
    repeats a column is visited once per stored entry (the reference would lose the rest of that row: not reproduced)."""
    m = len(rows)
    first = [0] * m if first is None else first
    last = [len(r) for r in rows] if last is None else last
    cur, head, nxt = list(first), [-1] * k, [-1] * m
    for r in range(m):
        if cur[r] < last[r]:
            j = rows[r][cur[r]][0]
            nxt[r], head[j] = head[j], r
    out = []
    for i in range(k):
        visits, row = [], head[i]
        while row >= 0:
            after = nxt[row]
            while True:
                visits.append((row, cur[row]))
                cur[row] += 1
                if not (cur[row] < last[row] and rows[row][cur[row]][0] == i):
                    break
            if cur[row] < last[row]:
                j = rows[row][cur[row]][0]
                nxt[row], head[j] = head[j], row
            row = after
        out.append(visits)
    return out


def first_touch(i, steps, upper, cplx):
    """add_sprow (sypr.hpp:66-107) over `steps` = [(alpha, row of W), ...]: a column's first product is stored as alpha * w, later
    ones are added with one multiply-add; columns in first-touch order; sums that cancel stay; upper: columns < i are skipped"""
    cols, acc = [], {}
    for alpha, row in steps:
        for c, w in row:
            if upper and c < i:
                continue
            if c in acc:
                acc[c] = madd(alpha, w, acc[c], cplx)
            else:
                cols.append(c)
                acc[c] = mul(alpha, w, cplx)
    return [(c, acc[c]) for c in cols]


def atb_upper(k, left, right, conj_l, conj_r, cplx):
    """sp2m_online_atb with BUILD_ONLY_U (sypr.hpp:400-527): row i of C from the rows of `left` that hold column i, in walk order"""
    out = []
    for i, visits in enumerate(walk(k, left)):
        steps = [(cj(left[r][p][1], conj_l), [(c, cj(w, conj_r)) for c, w in right[r]]) for r, p in visits]
        out.append(first_touch(i, steps, True, cplx))
    return out


def dense_row(m, rows, cplx):
    """aoclsparse_aat_dense_row (syrk.hpp:46-113): row i scattered densely, C(i,j) for j = i .. m - 1 one multiply-add per entry
    of row j in stored order; sums that are exactly zero are dropped.  In the reference a later repeat of a column in row i
    overwrites the earlier one; such rows are outside the parity contract, and like the walk this restatement gives them the
    complete product: the repeats are summed"""
    out = []
    for i in range(m):
        trow = {}
        for col, v in rows[i]:
            trow[col] = trow.get(col, 0) + v
        keep = []
        for j in range(i, m):
            c = 0j if cplx else 0.0
            for col, v in rows[j]:
                c = madd(trow.get(col, 0j if cplx else 0.0), cj(v, True), c, cplx)
            if c != 0:
                keep.append((j, c))
        out.append(keep)
    return out


def takes_dense_row_path(csc, op, m, n, nnz):
    """syrk.hpp:221"""
    return not csc and op == N and m < 3000 and m < n and nnz <= 10 * m


def csr_out(rows, base, dt):
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32) + base
    ind = np.array([c for r in rows for c, _ in r], np.int32) + base
    val = np.array([v for r in rows for _, v in r], dt)
    return ptr, ind, val


def restated_syrk(op, csc, m, n, base, ptr, ind, val):
    """aoclsparse_syrk_t.  (m, n): the caller's dimensions; csc: the arrays are col_ptr / row_ind, i.e. the CSR of A^T, which is
    what the reference stores (syrk.hpp:150-173).  -> (m_C, base, row_ptr, col_ind, val)"""
    cplx = np.iscomplexobj(val)
    ms, ns = (n, m) if csc else (m, n)
    S = rows_of(ms, base, ptr, ind, val)
    eff_none = (op != N) if csc else (op == N)
    if eff_none and takes_dense_row_path(csc, op, ms, ns, len(val)):
        C, mc = dense_row(ms, S, cplx), ms
    elif eff_none:  # :228-283: the csr2csc transpose; CSR: conjugated, then CONJ_A on top; CSC: CONJ_A only
        Lt, mc = stable_transpose(ns, S), ms
        C = atb_upper(mc, Lt, Lt, csc, not csc, cplx)
    else:  # :286-331
        mc = ns
        C = atb_upper(mc, S, S, not csc, csc, cplx)
    return (mc, base) + csr_out(C, base, val.dtype)


def clean_rows(m, rows):
    """aoclsparse_csr_csc_optimize on sorted rows: an explicit zero on every missing diagonal"""
    out = []
    for i, row in enumerate(rows):
        if any(c == i for c, _ in row):
            out.append(list(row))
            continue
        zero = 0j if row and isinstance(row[0][1], complex) else 0.0
        out.append(sorted(row + [(i, zero)], key=lambda e: e[0]))
    return out


def restated_sypr(op, A, B, lower):
    """aoclsparse_sypr_t.  A = (csc, m, n, base, ptr, ind, val) as for restated_syrk; B = (m, base, ptr, ind, val), fully
    sorted.  -> (n_C, 0, row_ptr, col_ind, val), plus the intermediate T for the chain lengths"""
    csc, am, an, abase, aptr, aind, aval = A
    bm, bbase, bptr, bind, bval = B
    cplx = np.iscomplexobj(aval)
    ms, ns = (an, am) if csc else (am, an)
    S = rows_of(ms, abase, aptr, aind, aval)
    none = op == N
    eff_none = (not none) if csc else none
    conj_flip = csc and none and cplx
    if eff_none:  # sypr.hpp:750-786
        Lm = stable_transpose(ns, S)
        conj1, conj2 = cplx and not csc, cplx and csc
    else:  # :737-743, :824, :945
        Lm = S
        conj1, conj2 = conj_flip, cplx and not conj_flip
    nc = ns if not eff_none else ms
    Bc = clean_rows(bm, rows_of(bm, bbase, bptr, bind, bval.astype(aval.dtype)))
    if cplx:
        Bc = [[(c, complex(v)) for c, v in r] for r in Bc]
    diag = [[c for c, _ in r].index(i) for i, r in enumerate(Bc)]
    if lower:  # :303-322
        s_first, s_last, t_first, t_last = [0] * bm, [d + 1 for d in diag], [0] * bm, diag
    else:
        s_first, s_last, t_first, t_last = diag, [len(r) for r in Bc], [d + 1 for d in diag], [len(r) for r in Bc]
    other = walk(bm, Bc, t_first, t_last)
    Tm = []
    for i in range(bm):  # :333-390
        steps = [(Bc[i][p][1], [(c, cj(w, conj1)) for c, w in Lm[Bc[i][p][0]]]) for p in range(s_first[i], s_last[i])]
        steps += [(cj(Bc[r][p][1], True), [(c, cj(w, conj1)) for c, w in Lm[r]]) for r, p in other[i]]
        Tm.append(first_touch(i, steps, False, cplx))
    C = atb_upper(nc, Lm, Tm, conj2, False, cplx)
    return (nc, 0) + csr_out(C, 0, aval.dtype), Tm


# ---- through the library -------------------------------------------------------------------------------------------------------
def export(h, t):
    """-> dict(base, m, n, nnz, row_ptr, col_ind, val): copies of what aoclsparse_export_?csr hands out"""
    base, m, n, nnz = c_int(), c_int(), c_int(), c_int()
    rp, ci, v = c_void_p(), c_void_p(), c_void_p()
    st = getattr(L, "aoclsparse_export_%scsr" % t)(h, byref(base), byref(m), byref(n), byref(nnz), byref(rp), byref(ci), byref(v))
    assert st == 0, P.STATUS[st]
    from ctypes import POINTER, cast, c_byte

    def arr(p, count, dt):
        if count == 0:
            return np.zeros(0, dt)
        nb = count * np.dtype(dt).itemsize
        return np.frombuffer(bytes(cast(p, POINTER(c_byte * nb)).contents), dt).copy()

    return dict(base=base.value, m=m.value, n=n.value, nnz=nnz.value, row_ptr=arr(rp, m.value + 1, np.int32),
                col_ind=arr(ci, nnz.value, np.int32), val=arr(v, nnz.value, DT[t]))


class Result:
    """the C of one call; destroyed with the object"""

    def __init__(self):
        self.h = c_void_p()

    def __del__(self):
        try:
            if self.h:
                L.aoclsparse_destroy(byref(self.h))
        except Exception:
            pass


def syrk(op, A, C="new"):
    """-> (status name, Result)"""
    r = Result()
    st = L.aoclsparse_syrk(op, A, None if C is None else byref(r.h))
    return P.STATUS[st], r


def sypr(op, A, B, descr, request=FULL, C="new"):
    """C: "new" (a fresh null handle), None (a null pointer) or a Result to continue with"""
    r = Result() if C == "new" or C is None else C
    st = L.aoclsparse_sypr(op, A, B, descr, None if C is None else byref(r.h), request)
    return P.STATUS[st], r


def values_of(t, vals):
    dt = DT[t]
    if np.dtype(dt).kind == "c":
        return np.array([complex(*v) for v in vals], dt)
    return np.array(vals, dt)


def kat_handle(t, d):
    val = values_of(t, d["val"])
    return Handle(d["base"], d["m"], d["n"], d["ptr"], d["ind"], val, csc=d.get("csc", False)), val


# ---- 1a. the restatement against what the reference's programs expect ----------------------------------------------------------
def check_expected(got, e, dt):
    mc, base, ptr, ind, val = got
    assert (mc, base) == (e["m"], e["base"]) and e["m"] == e["n"]
    assert ptr.tolist() == e["row_ptr"] and ind.tolist() == e["col_ind"]
    want = values_of({np.dtype(d): t for t, d in TYPES}[np.dtype(dt)], e["val"])
    d = val - want
    assert max([0.0] + [max(abs(x.real), abs(x.imag)) for x in d.tolist()]) <= e.get("tol", 0.0)


def test_restated_syrk_gives_what_the_reference_example_expects():
    k = next(c for c in KATS["syrk"] if c["name"] == "sample_dsyrk")
    val = values_of(k["type"], k["val"])
    got = restated_syrk(OPS[k["op"]], k["csc"], k["m"], k["n"], k["base"], np.array(k["ptr"]), np.array(k["ind"]), val)
    assert not takes_dense_row_path(False, N, 4, 3, 7)  # 4 x 3: the A^T * B path, and its order is what the example lists
    check_expected(got, k["expect"], val.dtype)


def test_restated_sypr_gives_what_the_reference_example_expects():
    k = next(c for c in KATS["sypr"] if c["name"] == "sample_zsypr")
    a, b = k["A"], k["B"]
    A = (a["csc"], a["m"], a["n"], a["base"], np.array(a["ptr"]), np.array(a["ind"]), values_of("z", a["val"]))
    B = (b["m"], b["base"], np.array(b["ptr"]), np.array(b["ind"]), values_of("z", b["val"]))
    got, _ = restated_sypr(OPS[k["op"]], A, B, k["fill"] == "lower")
    check_expected(got, k["expect"], np.complex128)


# ---- 1b. the restatement against dense products -------------------------------------------------------------------------------
def to_dense(m, n, base, ptr, ind, val):
    D = np.zeros((m, n), np.result_type(val.dtype, np.float64))
    rows = np.repeat(np.arange(m), np.diff(ptr))
    np.add.at(D, (rows, ind - base), val)
    return D


def check_against_dense(got, exact, scale, chain, dt):
    """the pattern contains the numeric pattern of the upper triangle; every value within (chain + 4) u scale"""
    mc, base, ptr, ind, val = got
    u = float(np.finfo(dt).eps) * (2 if np.dtype(dt).kind == "c" else 1)
    seen = np.zeros((mc, mc), bool)
    for i in range(mc):
        cols = ind[ptr[i] - base:ptr[i + 1] - base] - base
        assert len(set(cols.tolist())) == len(cols) and (cols >= i).all(), "a column twice, or left of the diagonal"
        seen[i, cols] = True
        d = val[ptr[i] - base:ptr[i + 1] - base] - exact[i, cols]
        bound = (chain + 4) * u * scale[i, cols]
        assert (np.abs(d.real) <= bound).all() and (np.abs(d.imag) <= bound).all()
    missing = np.triu(~seen)
    assert (np.abs(exact[missing]) <= (chain + 4) * u * scale[missing]).all(), "an element of the product is not in the pattern"


def random_matrix(seed, m, n, base, dt, lo=0, hi=6):
    ptr, ind, val = random_csr(seed, m, n, lambda rng, i: rng.integers(lo, hi), base=base)
    if np.dtype(dt).kind == "c":
        val = val + 1j * np.random.default_rng(seed + 1).uniform(-1, 1, len(val))
    return ptr, ind, val.astype(dt)


@pytest.mark.parametrize("dt", [np.float64, np.complex128], ids=["d", "z"])
@pytest.mark.parametrize("csc", [False, True], ids=["csr", "csc"])
@pytest.mark.parametrize("shape", [(9, 14), (14, 9), (6, 40)])
def test_restated_syrk_against_dense_products(shape, csc, dt):
    m, n = shape
    cplx = np.dtype(dt).kind == "c"
    for base in (0, 1):
        # the stored arrays: CSR of A, or (csc) col_ptr / row_ind of A = the CSR of A^T
        sm, sn = (n, m) if csc else (m, n)
        ptr, ind, val = random_matrix(7 * m + base, sm, sn, base, dt)
        D = to_dense(sm, sn, base, ptr, ind, val)
        A = D.T if csc else D
        for op in (N, H if cplx else T):
            got = restated_syrk(op, csc, m, n, base, ptr, ind, val)
            left = A if op == N else A.conj().T
            exact, scale = left @ left.conj().T, np.abs(left) @ np.abs(left).T
            chain = np.count_nonzero(left, axis=1).max()
            assert got[0] == left.shape[0] and got[1] == base
            check_against_dense(got, exact, scale, chain, dt)
    assert takes_dense_row_path(False, N, 6, 40, 10) and not takes_dense_row_path(True, T, 6, 40, 10)


def herm(Bd, lower):
    tri = np.tril(Bd) if lower else np.triu(Bd)
    off = np.tril(Bd, -1) if lower else np.triu(Bd, 1)
    return tri + off.conj().T


def symmetric_input(seed, m, base, dt, missing=()):
    """a fully sorted square matrix with entries in both triangles and no entry on the diagonals in `missing`"""
    ptr, ind, val = random_matrix(seed, m, m, 0, dt, 1, 5)
    rows = [dict(zip(ind[ptr[i]:ptr[i + 1]].tolist(), val[ptr[i]:ptr[i + 1]].tolist())) for i in range(m)]
    for i in range(m):
        if i in missing:
            rows[i].pop(i, None)
        else:
            rows[i][i] = dt(1.5 + i / m)  # (a Hermitian matrix has a real diagonal)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ind = np.array([c for r in rows for c in sorted(r)], np.int32)
    val = np.array([r[c] for r in rows for c in sorted(r)], dt)
    return ptr + base, ind + base, val


@pytest.mark.parametrize("dt", [np.float64, np.complex128], ids=["d", "z"])
@pytest.mark.parametrize("csc", [False, True], ids=["csr", "csc"])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
def test_restated_sypr_against_dense_products(lower, csc, dt):
    m, n = 11, 7
    cplx = np.dtype(dt).kind == "c"
    for base in (0, 1):
        sm, sn = (n, m) if csc else (m, n)
        ptr, ind, val = random_matrix(3 * m + base, sm, sn, base, dt)
        D = to_dense(sm, sn, base, ptr, ind, val)
        A = D.T if csc else D
        for op in (N, H if cplx else T):
            k = n if op == N else m  # B is k x k
            bptr, bind, bval = symmetric_input(k + base, k, 1 - base, dt, missing=(1, k - 2))
            Bh = herm(to_dense(k, k, 1 - base, bptr, bind, bval), lower)
            got, Tm = restated_sypr(op, (csc, m, n, base, ptr, ind, val), (k, 1 - base, bptr, bind, bval), lower)
            left = A if op == N else A.conj().T
            exact, scale = left @ Bh @ left.conj().T, np.abs(left) @ np.abs(Bh) @ np.abs(left).T
            chain = np.count_nonzero(left, axis=1).max() + np.count_nonzero(Bh, axis=1).max() + 1  # (+ an inserted diagonal zero)
            assert got[0] == left.shape[0] and got[1] == 0
            check_against_dense(got, exact, scale, chain, dt)


def test_the_walk_order_is_not_ascending_and_completes_rows_that_repeat_a_column():
    # rows {0, 2}, {0}, {0, 1}: column 0's stack holds 2, 1, 0 from the top; row 2 then moves to column 1, row 0 to column 2
    rows = [[(0, 1.0), (2, 2.0)], [(0, 3.0)], [(0, 4.0), (1, 5.0)]]
    assert walk(3, rows) == [[(2, 0), (1, 0), (0, 0)], [(2, 1)], [(0, 1)]]
    # a row that repeats column 1: both entries are visited, and the row still reaches column 3
    rep = [[(0, 1.0), (1, 2.0), (1, 3.0), (3, 4.0)]]
    assert walk(4, rep) == [[(0, 0)], [(0, 1), (0, 2)], [], [(0, 3)]]


def test_first_touch_keeps_a_cancelled_sum_and_the_dense_row_path_drops_it():
    # rows 0 and 1 are orthogonal with two products that cancel exactly: +1 * +1 and +1 * -1
    ptr, ind, val = np.array([0, 2, 4, 5]), np.array([0, 1, 0, 1, 2]), np.array([1.0, 1.0, 1.0, -1.0, 1.0])
    wide = restated_syrk(N, False, 3, 4, 0, ptr, ind, val)  # 3 x 4 with 5 <= 30 entries: dense rows
    assert takes_dense_row_path(False, N, 3, 4, 5)
    assert wide[2].tolist() == [0, 1, 2, 3] and wide[3].tolist() == [0, 1, 2]
    tall = restated_syrk(N, False, 3, 3, 0, ptr, ind, val)  # 3 x 3: A^T * B path, the zero stays
    assert tall[2].tolist() == [0, 2, 3, 4] and tall[3].tolist() == [0, 1, 1, 2] and tall[4].tolist() == [2.0, 0.0, 2.0, 1.0]


# ---- 2. statuses before any device work -----------------------------------------------------------------------------------------
def small(dt, base=0, sort=True):
    """3 x 4: rows {0, 2}, {1}, {0, 3}; unsorted: row 0 stored as {2, 0}"""
    ptr = np.array([0, 2, 3, 5], np.int32) + base
    ind = np.array([0, 2, 1, 0, 3] if sort else [2, 0, 1, 0, 3], np.int32) + base
    return 3, 4, ptr, ind, (np.arange(5) + 1.0).astype(dt)


def square(dt, k, base=0, sort=True):
    """k x k, fully sorted unless asked otherwise: the diagonal and one entry left of it (rows >= 1)"""
    rows = [[0]] + [[i - 1, i] if sort or i != 1 else [i, i - 1] for i in range(1, k)]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32) + base
    ind = np.array([c for r in rows for c in r], np.int32) + base
    return k, k, ptr, ind, np.ones(len(ind), dt)


@pytest.mark.parametrize("t,dt", TYPES, ids=[t for t, _ in TYPES])
def test_syrk_statuses_in_the_reference_order(t, dt):
    cplx = t in "cz"
    A, U = Handle(0, *small(dt)), Handle(0, *small(dt, sort=False))
    csc_ptr, csc_val = np.array([0, 2, 2, 3], np.int32), np.ones(3, dt)
    KU = Handle(0, 4, 3, csc_ptr, np.array([2, 0, 1], np.int32), csc_val, csc=True)  # column 0 stored as rows {2, 0}
    TC, BS = tcsr(dt), bsr(dt)
    assert P.STATUS[L.aoclsparse_syrk(N, None, None)] == "invalid_pointer"  # aoclsparse_syrk.cpp:43
    table = [  # (op, handle, C, expected, line of syrk.hpp)
        (7, A.h, None, "invalid_pointer", 124),
        (7, A.h, "new", "invalid_value", 129),
        (7, TC.h, "new", "invalid_value", 129),
        (N, TC.h, "new", "not_implemented", 133),  # TCSR: a handle without a CSR
        (N, BS.h, "new", "not_implemented", 133),  # BSR
        (T, A.h, "new", "not_implemented" if cplx else "GPU", 140),  # complex + transpose
        (T, U.h, "new", "not_implemented" if cplx else "unsorted_input", 175),
        (H, U.h, "new", "unsorted_input", 175),
        (N, KU.h, "new", "unsorted_input", 175),  # from CSC the effective op is flipped (:166-173)
    ]
    for op, h, C, want, line in table:
        if want == "GPU":
            continue  # (a valid call: tests/test_sy_sparse_gpu.py)
        st, r = syrk(op, h, C)
        assert st == want, (op, line, st)
        assert not r.h, "C must be null after a refused call (:127)"
    # wrong_type cannot be reached through aoclsparse_syrk (it dispatches on A's own type, aoclsparse_syrk.cpp:48-57): the :136 check
    # is kept for the order's sake.  The recorded cases of the reference's unit tests:
    for k in KATS["syrk"]:
        if k["expect"]["status"] == "success" or k["type"] != t:
            continue
        Hk, _ = kat_handle(k["type"], dict(k, ptr=k["ptr"], ind=k["ind"]))
        st, r = syrk(OPS.get(k["op"], k["op"]), Hk.h)
        assert st == k["expect"]["status"] and not r.h, k["name"]


@pytest.mark.parametrize("t,dt", TYPES, ids=[t for t, _ in TYPES])
def test_syrk_empty_quick_return(t, dt):
    """syrk.hpp:206-214: an empty m_C x m_C handle in A's base, every row pointer equal to the base, exportable"""
    cplx = t in "cz"
    for base in (0, 1):
        E = Handle(base, 5, 4, np.full(6, base, np.int32), np.zeros(1, np.int32), np.zeros(1, dt))
        K = Handle(base, 5, 4, np.full(5, base, np.int32), np.zeros(1, np.int32), np.zeros(1, dt), csc=True)
        Z = Handle(base, 0, 4, np.full(1, base, np.int32), np.zeros(1, np.int32), np.zeros(1, dt))
        for h, op, mc in ((E, N, 5), (E, H if cplx else T, 4), (K, N, 5), (K, H, 4), (Z, N, 0), (Z, H, 4)):
            st, r = syrk(op, h.h)
            assert st == "success" and r.h
            x = export(r.h, t)
            assert (x["m"], x["n"], x["nnz"], x["base"]) == (mc, mc, 0, base) and (x["row_ptr"] == base).all()


DESCRS = []  # (a descriptor must outlive the call it is passed to: every one made here is kept)


def sym_descr(t, base=0, fill=P.FILL_LOWER, mtype=None, diag=P.DIAG_NON_UNIT):
    d = P.Descr(base, (P.TYPE_HERMITIAN if t in "cz" else P.TYPE_SYMMETRIC) if mtype is None else mtype, fill, diag)
    DESCRS.append(d)
    return d


@pytest.mark.parametrize("t,dt", TYPES, ids=[t for t, _ in TYPES])
def test_sypr_statuses_in_the_reference_order(t, dt):
    cplx = t in "cz"
    m, n = 3, 4
    A, U = Handle(0, *small(dt)), Handle(0, *small(dt, sort=False))
    B3, B4 = Handle(0, *square(dt, 3)), Handle(0, *square(dt, 4))
    B4one, B4u = Handle(1, *square(dt, 4, base=1)), Handle(0, *square(dt, 4, sort=False))
    Brect = Handle(0, *small(dt))  # 3 x 4
    Bcsc = Handle(0, 4, 4, *square(dt, 4)[2:], csc=True)
    odt = np.float32 if dt != np.float32 else np.float64
    Aother, Bother = Handle(0, *small(odt)), Handle(0, *square(odt, 4))
    KU = Handle(0, 4, 3, np.array([0, 2, 2, 3], np.int32), np.array([2, 0, 1], np.int32), np.ones(3, dt), csc=True)  # 4 x 3
    TC, BS = tcsr(dt), bsr(dt)
    d = sym_descr(t)
    good = dict(op=N, A=A.h, B=B4.h, descr=d.h, request=FULL, C="new")
    opH = H if cplx else T
    table = [  # (changes, expected, line of sypr.hpp unless it says .cpp)
        (dict(A=None, request=7), "invalid_pointer", ".cpp:33"),
        (dict(B=None, op=7), "invalid_pointer", ".cpp:33"),
        (dict(C=None, descr=None), "invalid_pointer", ".cpp:33"),
        (dict(A=Aother.h, request=7, op=7), "wrong_type", ".cpp:37-46"),
        (dict(B=Bother.h, descr=None), "wrong_type", ".cpp:37-46"),
        (dict(request=7, op=7, descr=None), "invalid_value", 548),
        (dict(op=7, descr=None), "invalid_value", 552),
        (dict(descr=None, A=TC.h, B=TC.h), "invalid_pointer", 556),
        (dict(A=TC.h, B=TC.h), "not_implemented", 566),  # TCSR handles: no CSR
        (dict(A=BS.h, B=BS.h), "not_implemented", 566),
        (dict(B=Bcsc.h, descr=sym_descr(t, mtype=P.TYPE_GENERAL).h), "not_implemented", 581),  # B made from CSC arrays
        (dict(op=T, B=B3.h, descr=sym_descr(t, base=1).h), "not_implemented" if cplx else "invalid_value", 587),
        (dict(descr=sym_descr(t, base=1).h, B=Brect.h), "invalid_value", 636),  # the descriptor's base is not B's
        (dict(B=B4one.h, descr=sym_descr(t, base=1, mtype=P.TYPE_GENERAL).h), "invalid_value", 638),
        (dict(descr=sym_descr(t, mtype=P.TYPE_TRIANGULAR, diag=P.DIAG_UNIT).h, B=Brect.h), "invalid_value", 638),
        (dict(descr=sym_descr(t, mtype=P.TYPE_SYMMETRIC if cplx else P.TYPE_HERMITIAN).h), "invalid_value", 638),
        (dict(descr=sym_descr(t, diag=P.DIAG_UNIT).h, B=Brect.h), "not_implemented", 652),
        (dict(B=Brect.h), "invalid_size", 658),  # B is not square
        (dict(B=B3.h), "invalid_size", 674),  # op = none: B must be n x n
        (dict(op=opH, B=B4.h), "invalid_size", 668),  # op = T / H: B must be m x m
        (dict(A=KU.h, B=B4.h), "invalid_size", 674),  # CSC handle, 4 x 3: the caller's dimensions
        (dict(request=FINAL), "invalid_value", 688),  # finalize without a C
        (dict(A=U.h, op=opH, B=B3.h), "unsorted_input", 727),
        (dict(B=B4u.h), "unsorted_input", 727),
        (dict(A=KU.h, B=B3.h), "unsorted_input", 727),  # from CSC, op = none is the effective transpose
    ]
    for kw, want, line in table:
        a = dict(good)
        a.update(kw)
        st, r = sypr(a["op"], a["A"], a["B"], a["descr"], a["request"], a["C"])
        assert st == want, (line, st)
        assert not r.h
    # a C of the wrong size is refused by finalize (:690), and is left as it was
    Z = Handle(0, 0, 4, np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, dt))
    _, small_c = sypr(N, Z.h, B4.h, d.h, COUNT)
    assert small_c.h and export(small_c.h, t)["m"] == 0
    st, same = sypr(N, A.h, B4.h, d.h, FINAL, small_c)
    assert st == "invalid_value" and same.h and export(same.h, t)["m"] == 0
    for k in KATS["sypr"]:
        if k["expect"]["status"] == "success" or k["type"] != t:
            continue
        Ak, _ = kat_handle(k["type"], k["A"])
        Bk, _ = kat_handle(k.get("type_b", k["type"]), dict(k["B"], csc=False))
        dk = sym_descr(t, k["B"]["base"], P.FILL_LOWER if k["fill"] == "lower" else P.FILL_UPPER,
                       P.TYPE_GENERAL if k.get("descr_type") == "general" else None)
        st, r = sypr(OPS[k["op"]], Ak.h, Bk.h, dk.h)
        assert st == k["expect"]["status"] and not r.h, k["name"]


@pytest.mark.parametrize("t,dt", TYPES, ids=[t for t, _ in TYPES])
def test_sypr_empty_quick_return(t, dt):
    """sypr.hpp:695-723: an empty n x n zero-based handle is created only when *C is null; whatever B's and A's bases are"""
    cplx = t in "cz"
    for base in (0, 1):
        E = Handle(base, 3, 4, np.full(4, base, np.int32), np.zeros(1, np.int32), np.zeros(1, dt))  # nnz = 0
        A = Handle(base, *small(dt, base=base))
        B4, B3 = Handle(base, *square(dt, 4, base=base)), Handle(base, *square(dt, 3, base=base))
        B0 = Handle(base, 4, 4, np.full(5, base, np.int32), np.zeros(1, np.int32), np.zeros(1, dt))
        d = sym_descr(t, base)
        for a, op, b, nc in ((E, N, B4, 3), (E, H if cplx else T, B3, 4), (A, N, B0, 3)):
            for request in (FULL, COUNT):
                st, r = sypr(op, a.h, b.h, d.h, request)
                assert st == "success" and r.h
                x = export(r.h, t)
                assert (x["m"], x["n"], x["nnz"], x["base"]) == (nc, nc, 0, 0) and not x["row_ptr"].any()
            st, again = sypr(op, a.h, b.h, d.h, FINAL, r)  # a C is there: nothing is created, nothing changes
            assert st == "success" and again is r and export(r.h, t)["nnz"] == 0
    for k in KATS["sypr"]:
        if k["expect"]["status"] != "success" or k["expect"]["col_ind"] or k["type"] != t:
            continue
        Ak, _ = kat_handle(t, k["A"])
        Bk, _ = kat_handle(t, dict(k["B"], csc=False))
        st, r = sypr(OPS[k["op"]], Ak.h, Bk.h, sym_descr(t, k["B"]["base"]).h)
        x = export(r.h, t)
        assert st == "success" and (x["m"], x["n"], x["nnz"]) == (k["expect"]["m"], k["expect"]["n"], 0), k["name"]
        assert x["row_ptr"].tolist() == k["expect"]["row_ptr"]
