"""aoclsparse_mi355_?ilu0_refactor_device on the GPU: the ILU(0) factor of a handle recomputed in HBM after a value change, on
the schedule the first factorisation kept, by the scan and by the search variant of the row routine.

Every comparison is bit for bit: the factorisation applies, to every position, the reference's fmas in the reference's order
(oracle.dilu0 for double; for float and the complex types, which the oracle does not factorise, a fresh handle created over the
new values).  Matrices are small and diagonally dominant (off-diagonals in +-[0.8, 1.2], diagonal = sum |off-diagonals| + 1), the
new values are the old ones times per-entry factors in [0.8, 1.2]."""
import ctypes
import functools
from ctypes import byref, c_void_p

import numpy as np
import pytest

import oracle
from util import laplace5, pkg

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

P = pkg()
L = P.lib()
NUMERICAL_ERROR = 11
DTYPES = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared systems are read-only)


class Handle(P.Matrix):
    """a handle of any of the four value types over aliased arrays (what P.Matrix's device methods need: h, nnz, letter)"""

    def __init__(self, base, m, rp, ci, v, letter="d"):
        self.row_ptr, self.col_ind = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
        self.val = np.ascontiguousarray(v).astype(DTYPES[letter])
        self.letter, self.double = letter, letter == "d"
        self.m, self.n, self.base, self.nnz = m, m, base, len(self.val)
        self.h = c_void_p()
        self.status = getattr(L, "aoclsparse_create_%scsr" % letter)(byref(self.h), base, m, m, self.nnz, P._ptr(self.row_ptr),
                                                                   P._ptr(self.col_ind), P._ptr(self.val))
        assert self.status == 0
        self.descr = P.Descr(base=base)

    def factor_at(self, address):
        """the nnz factor values behind a pointer the library handed out (a view, not a copy)"""
        real = {"s": ctypes.c_float, "d": ctypes.c_double, "c": ctypes.c_float, "z": ctypes.c_double}[self.letter]
        n = self.nnz * (2 if self.letter in "cz" else 1)
        a = np.ctypeslib.as_array(ctypes.cast(c_void_p(address), ctypes.POINTER(real)), (n,))
        return a.view(DTYPES[self.letter])

    def smoother(self, b):
        """aoclsparse_?ilu_smoother -> (the address it hands out, x)"""
        pv, x = c_void_p(), np.zeros(self.m, DTYPES[self.letter])
        rhs = np.ascontiguousarray(b, DTYPES[self.letter])  # (named: the address alone does not keep a converted copy alive)
        st = getattr(L, "aoclsparse_%silu_smoother" % self.letter)(P.OP_NONE, self.h, self.descr.h, byref(pv), None, P._ptr(x),
                                                                  P._ptr(rhs))
        assert st == 0, P.STATUS.get(st, st)
        return pv.value, x

    def refactor(self):
        st, address = self.ilu0_refactor_device()
        assert st == 0, P.STATUS.get(st, st)
        return address


class ilu_search:
    """with ilu_search(v): ... -- the plan option, read when a handle's ILU schedule is built; -1 (automatic) is restored"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        assert L.aoclsparse_mi355_set_option(P.OPTION_ILU_SEARCH, self.v) == 0

    def __exit__(self, *a):
        assert L.aoclsparse_mi355_set_option(P.OPTION_ILU_SEARCH, -1) == 0


def dominant(m, rp, ci, base, seed, cplx=False):
    """values on the pattern: off-diagonals of modulus in [0.8, 1.2] with a random sign (phase), diagonal = sum of them + 1"""
    rng = np.random.default_rng(seed)
    nnz = len(ci)
    v = rng.uniform(0.8, 1.2, nnz) * (np.exp(2j * np.pi * rng.uniform(0, 1, nnz)) if cplx else rng.choice([-1.0, 1.0], nnz))
    rid = np.repeat(np.arange(m), np.diff(rp))
    dg = (ci - base) == rid
    v[dg] = 0
    v[dg] = np.add.reduceat(np.abs(v), rp[:-1] - base) + 1.0
    return v


def scaled(v, seed):
    return np.ascontiguousarray(v * np.random.default_rng(seed).uniform(0.8, 1.2, len(v)))


def banded(m, hb, base=0, reverse_upper=False):
    rows = []
    for i in range(m):
        lo, up = np.arange(max(0, i - hb), i + 1), np.arange(i + 1, min(m, i + hb + 1))
        rows.append(np.concatenate([lo, up[::-1] if reverse_upper else up]))
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32) + base
    return rp, (np.concatenate(rows) + base).astype(np.int32)


@functools.lru_cache(maxsize=None)
def system(name, base=0):
    """(m, rp, ci, v, v2, b, oracle factor of v, its solve of b, oracle factor of v2, its solve of b), computed once"""
    if name == "laplace":
        m, rp, ci, _ = laplace5(12, base=base)
    else:
        m, hb = {"band10": (96, 10), "band70": (160, 70), "band70rev": (160, 70)}[name]
        rp, ci = banded(m, hb, base, reverse_upper=name.endswith("rev"))
    v = dominant(m, rp, ci, base, 5)
    v2 = scaled(v, 6)
    b = np.random.default_rng(7).uniform(-1, 1, m)
    out = [m, rp, ci, v, v2, b]
    for vals in (v, v2):
        st, lu, dg = oracle.dilu0(m, base, rp, ci, vals.copy())
        assert st == 0
        st, x = oracle.dilu_solve(m, base, dg, lu, rp, ci, b)
        assert st == 0
        out += [lu, x]
    for a in out[1:]:
        a.setflags(write=False)
    return tuple(out)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("base", [0, 1])
def test_refactor_after_update_laplacian_level_launches(base):
    """12 x 12 5-point Laplacian (144 rows, 23 levels, one launch per level).  A value update alone leaves the factor of the old
    values in force (the pinned reference behaviour); the refactorisation replaces it by oracle.dilu0 of the new values, in the
    array whose address was handed out before, without analysing again."""
    m, rp, ci, v, v2, b, lu, x, lu2, x2 = system("laplace", base)
    A = Handle(base, m, rp, ci, v.copy())
    assert L.aoclsparse_set_lu_smoother_hint(A.h, P.OP_NONE, A.descr.h, 10) == 0 and L.aoclsparse_optimize(A.h) == 0
    p0, got = A.smoother(b)
    assert same_bits(A.factor_at(p0), lu) and same_bits(got, x)
    assert A.update_values_device(dev(v2)) == 0
    p1, got = A.smoother(b)
    assert p1 == p0 and same_bits(A.factor_at(p1), lu) and same_bits(got, x), "the old factor stays in force"
    i = A.ilu_info()
    assert (i.factorized, i.levels, i.max_row, i.syncfree, i.search, i.analyses, i.factorizations) == (1, 23, 5, 0, 0, 1, 1)
    assert i.schedule_bytes >= 4 * m
    p2 = A.refactor()
    assert p2 == p0, "the factor's array keeps its address"
    assert same_bits(A.factor_at(p0), lu2), "the pointer handed out before the refactorisation shows the new factor"
    p3, got = A.smoother(b)
    assert p3 == p0 and same_bits(A.factor_at(p3), lu2) and same_bits(got, x2)
    i = A.ilu_info()
    assert (i.factorized, i.levels, i.analyses, i.factorizations) == (1, 23, 1, 2)
    st, none = A.ilu0_refactor_device(want_factor=False)  # precond_csr_val may be null
    assert st == 0 and none is None and same_bits(A.factor_at(p0), lu2) and A.ilu_info().factorizations == 3


@pytest.mark.parametrize("letter", ["d", "s"])
def test_refactor_on_the_syncfree_launch(letter):
    """Banded, m = 96, half-bandwidth 10 (21 entries per row, 96 levels, nnz >= 16 m): the sync-free launch.  Double against the
    oracle; float against a fresh float handle over the new values (the oracle has no float ILU)."""
    m, rp, ci, v, v2, b, lu, x, lu2, x2 = system("band10")
    A = Handle(0, m, rp, ci, v.copy(), letter)
    p0, got = A.smoother(b)
    first = A.factor_at(p0).copy()
    assert A.update_values_device(dev(v2.astype(DTYPES[letter]))) == 0
    p1, again = A.smoother(b)
    assert same_bits(A.factor_at(p1), first) and same_bits(again, got)
    A.refactor()
    i = A.ilu_info()
    auto = 1 if 21 >= P.ILU_SEARCH_MIN else 0  # (the automatic rule: sorted rows, the longest of 21 entries)
    assert (i.levels, i.max_row, i.syncfree, i.search, i.analyses, i.factorizations) == (96, 21, 1, auto, 1, 2)
    p2, got2 = A.smoother(b)
    assert p2 == p0
    if letter == "d":
        assert same_bits(first, lu) and same_bits(got, x)
        assert same_bits(A.factor_at(p0), lu2) and same_bits(got2, x2)
    F = Handle(0, m, rp, ci, v2.copy(), letter)
    pf, xf = F.smoother(b)
    assert same_bits(A.factor_at(p0), F.factor_at(pf)) and same_bits(got2, xf)
    assert not same_bits(A.factor_at(p0), first)


@pytest.mark.parametrize("letter", ["d", "s", "z", "c"])
def test_scan_and_search_give_the_same_bits(letter):
    """Banded, m = 160, half-bandwidth 70: rows of up to 141 entries, upper parts of 70 (two rounds of 64 per k step).  The plan
    option picks the scan (0) or the search (1); both factors are each other's bits, a fresh handle's, and for double the
    oracle's.  Real types take the sync-free launch here, the complex types one launch per level: both kernels, both variants."""
    m, rp, ci, v, v2, b, lu, x, lu2, x2 = system("band70")
    cplx = letter in "cz"
    w = dominant(m, rp, ci, 0, 5, cplx=True) if cplx else v
    w2 = scaled(w, 6)
    facs = []
    for opt in (0, 1):
        with ilu_search(opt):
            A = Handle(0, m, rp, ci, w.copy(), letter)
            A.smoother(b)
        assert A.update_values_device(dev(w2.astype(DTYPES[letter]))) == 0
        p = A.refactor()
        i = A.ilu_info()
        assert (i.search, i.max_row, i.levels, i.syncfree, i.analyses) == (opt, 141, 160, 0 if cplx else 1, 1)
        facs.append((A.factor_at(p).copy(), A.smoother(b)[1]))
    assert same_bits(facs[0][0], facs[1][0]) and same_bits(facs[0][1], facs[1][1])
    F = Handle(0, m, rp, ci, w2.copy(), letter)
    pf, xf = F.smoother(b)
    assert F.ilu_info().search == 1  # (automatic: sorted rows, longest row >= ILU_SEARCH_MIN)
    assert P.ILU_SEARCH_MIN <= 141
    assert same_bits(facs[0][0], F.factor_at(pf)) and same_bits(facs[0][1], xf)
    if letter == "d":
        assert same_bits(facs[0][0], lu2) and same_bits(facs[0][1], x2)


def test_search_is_never_chosen_for_partially_sorted_rows():
    """The same matrix with the upper part of every row reversed: sort class 2 (lower | diagonal | upper groups only).  Option 1
    does not select the search there, and the bits are the oracle's."""
    m, rp, ci, v, v2, b, lu, x, lu2, x2 = system("band70rev")
    with ilu_search(1):
        A = Handle(0, m, rp, ci, v.copy())
        p0, got = A.smoother(b)
        assert A.ilu_info().search == 0
        assert same_bits(A.factor_at(p0), lu) and same_bits(got, x)
        assert A.update_values_device(dev(v2)) == 0
        A.refactor()
    assert A.ilu_info().search == 0
    p, got = A.smoother(b)
    assert same_bits(A.factor_at(p), lu2) and same_bits(got, x2)


def test_refactor_as_the_first_factorisation():
    """No smoother call before it: the refactorisation analyses, factorises and creates the factor handle; the smoother then
    solves with it, and both give what the smoother gives on a fresh handle."""
    m, rp, ci, v, v2, b, lu, x, lu2, x2 = system("band10")
    A = Handle(0, m, rp, ci, v.copy())
    assert A.ilu_info().factorized == 0
    p = A.refactor()
    i = A.ilu_info()
    assert (i.factorized, i.analyses, i.factorizations, i.plans_kept_last) == (1, 1, 1, 0)
    assert same_bits(A.factor_at(p), lu)
    p1, got = A.smoother(b)
    assert p1 == p and same_bits(got, x) and A.ilu_info().factorizations == 1
    F = Handle(0, m, rp, ci, v.copy())
    pf, xf = F.smoother(b)
    assert same_bits(F.factor_at(pf), A.factor_at(p)) and same_bits(xf, got)


@pytest.mark.parametrize("keep", [True, False])
def test_factor_handle_plans_follow_through_their_value_maps(keep):
    """With keep_value_maps(A, 1) set before the first smoother call the factor handle records its plans' maps: the
    refactorisation carries both TRSV plans over (nothing is analysed by it or by the solve after it); without the flag they are
    invalidated and built again.  Same x either way: a fresh handle's."""
    m, rp, ci, v, v2, b, lu, x, lu2, x2 = system("band10")
    A = Handle(0, m, rp, ci, v.copy())
    if keep:
        assert A.keep_value_maps(True) == 0
    A.smoother(b)
    builds = A.ilu_info().factor_plan_builds
    assert builds >= 2
    assert A.revalue_device(dev(v2)) == 0
    p = A.refactor()
    i = A.ilu_info()
    assert i.plans_kept_last == (2 if keep else 0)
    assert i.factor_plan_builds == builds
    _, got = A.smoother(b)
    after = A.ilu_info().factor_plan_builds
    assert after == builds if keep else after >= builds + 2  # (both triangles are analysed again without maps)
    assert same_bits(A.factor_at(p), lu2) and same_bits(got, x2)
    F = Handle(0, m, rp, ci, v2.copy())
    assert same_bits(F.smoother(b)[1], got)


def test_zero_pivot_leaves_the_previous_factor_in_force():
    """The new values have a zero on the diagonal of row 0, which has no lower entries: its pivot stays 0.  numerical_error, and
    the handle is as before: the smoother returns the factor of the old values and its x, no factorisation is counted."""
    m, rp, ci, v, v2, b, lu, x, lu2, x2 = system("band10")
    A = Handle(0, m, rp, ci, v.copy())
    p0, got = A.smoother(b)
    bad = v2.copy()
    assert ci[rp[0]] == 0
    bad[rp[0]] = 0.0
    assert A.update_values_device(dev(bad)) == 0
    before = A.ilu_info()
    st, address = A.ilu0_refactor_device()
    assert st == NUMERICAL_ERROR and address is None
    i = A.ilu_info()
    assert (i.factorized, i.factorizations, i.analyses) == (1, before.factorizations, 1)
    assert i.factor_plan_builds == before.factor_plan_builds
    p1, again = A.smoother(b)
    assert p1 == p0 and same_bits(A.factor_at(p1), lu) and same_bits(again, x) and same_bits(got, x)
    # ... and good values afterwards factorise as ever
    assert A.update_values_device(dev(v2)) == 0
    A.refactor()
    assert same_bits(A.factor_at(p0), lu2) and same_bits(A.smoother(b)[1], x2)


@pytest.mark.parametrize("how", ["order_mat", "invalidate"])
def test_schedule_is_released_with_the_pattern_order(how):
    """aoclsparse_order_mat and aoclsparse_mi355_invalidate release the schedule: the next refactorisation analyses again (and
    makes the factor handle anew); a value update alone does not."""
    m, rp, ci, v, v2, b, lu, x, lu2, x2 = system("laplace")
    A = Handle(0, m, rp, ci, v.copy())
    A.smoother(b)
    assert A.update_values_device(dev(v2)) == 0
    i = A.ilu_info()
    assert (i.analyses, i.levels) == (1, 23) and i.schedule_bytes > 0
    assert (L.aoclsparse_order_mat(A.h) if how == "order_mat" else L.aoclsparse_mi355_invalidate(A.h)) == 0
    i = A.ilu_info()
    assert (i.analyses, i.levels, i.schedule_bytes, i.factorized) == (1, 0, 0, 1)
    p = A.refactor()
    i = A.ilu_info()
    assert (i.analyses, i.levels, i.factorizations) == (2, 23, 2)
    assert same_bits(A.factor_at(p), lu2) and same_bits(A.smoother(b)[1], x2)


def test_gmres_with_ilu0_uses_the_new_factor():
    """GMRES(20) with "ILU0" on the Laplacian with a mild convection term: after update + refactorisation the solver runs as on
    a fresh handle over the new values -- same iteration count, same solution -- and needs at most oracle.dgmres's iterations
    with the ILU(0) of the new values + 2 (the margin of the float stack's comparison: the larger oracle count + the spread of
    the oracle runs + 2; there is one double oracle run, so the spread is 0)."""
    m, rp, ci, _ = laplace5(12)
    rng = np.random.default_rng(9)
    rid = np.repeat(np.arange(m), np.diff(rp))
    v = np.where(ci == rid, 4.0, np.where(ci < rid, -1.0 - 0.3, -1.0 + 0.3))  # upwind / downwind neighbours differ
    v = np.ascontiguousarray(v * rng.uniform(0.9, 1.1, len(v)))
    v2 = scaled(v, 10)
    xe = rng.uniform(-1, 1, m)
    so, b = oracle.dcsrmv(0, 0, 1.0, m, len(v2), v2, ci, rp, xe, 0.0, np.zeros(m))
    assert so == 0
    st, xo, ro = oracle.dgmres(m, 0, rp, ci, v2, b, np.ones(m), 20, 1e-10, 1e-12, 400, 2)
    assert st == 0
    limit = int(ro[30]) + 2

    def solve(H):
        h = c_void_p()
        assert L.aoclsparse_itsol_d_init(byref(h)) == 0
        for k, val in {"iterative method": "GMRES", "gmres preconditioner": "ILU0", "gmres restart iterations": 20,
                       "gmres rel tolerance": 1e-10, "gmres abs tolerance": 1e-12, "gmres iteration limit": 400}.items():
            assert L.aoclsparse_itsol_option_set(h, k.encode(), str(val).encode()) == 0
        xs, rinfo = np.ones(m), np.zeros(100)
        assert L.aoclsparse_itsol_d_solve(h, m, H.h, H.descr.h, P._ptr(b), P._ptr(xs), P._ptr(rinfo), None, None, None) == 0
        L.aoclsparse_itsol_destroy(byref(h))
        return xs, int(rinfo[30])

    A = Handle(0, m, rp, ci, v.copy())
    x_old, it_old = solve(A)  # factorises v (and solves the wrong system for b: only the factor matters here)
    assert A.update_values_device(dev(v2)) == 0
    A.refactor()
    assert A.ilu_info().factorizations == 2
    xa, ita = solve(A)
    F = Handle(0, m, rp, ci, v2.copy())
    xf, itf = solve(F)
    print("gmres ilu0 iterations: refactorised", ita, "fresh", itf, "oracle", int(ro[30]), "limit", limit)
    assert ita == itf and same_bits(xa, xf)
    assert 1 <= ita <= limit
    assert np.max(np.abs(xa - xe)) < 1e-7
