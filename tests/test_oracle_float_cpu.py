"""CPU tier of the single-precision restatements (orc_strsv_lt / _ut, orc_ssymgs, orc_selltmv, orc_ssorv, orc_scg, orc_sgmres,
orc_scsrmm_col / _row).  They are the same template as their double twins (oracle/oracle_tmpl.h; csrmm: the macros DEF_CSRMM_COL /
DEF_CSRMM_ROW of oracle.c), which the reference's golden vectors pin; here:

  * dyadic data -- small integer off-diagonals, power-of-two diagonals, integer right-hand sides -- on which every
    intermediate of the double run is exactly representable in fp32, so the float function must return exactly the double
    result cast to float: a `double` left in the float instantiation, a missing term or a swapped triangle shows;
  * generic data (full mantissas) for the transposed solves against the restated KT kernels of the same precision, which the
    reference's own templates pin (tests/test_oracle_kt.py): the transposed KT solves have no vector arithmetic of their own
    (trsv_kt.cpp:152-295, :385-531), so the two must agree bit for bit;
  * the Krylov solvers by what they promise: the stopping test holds for the true residual, in about as many iterations as in
    double."""
import numpy as np
import pytest

import oracle
from util import kt_lanes, laplace5

KINDS = ("l", "lt", "u", "ut")


def bits32(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def dyadic_system(seed, m, base, band=3):
    """Sorted CSR with a full diagonal: off-diagonals in {-2, -1, 1, 2} on at most `band` neighbours either side, diagonal in
    {1/2, 1, 2} with either sign.  Every division of a solve is a scaling by a power of two."""
    rng = np.random.default_rng(seed)
    rp, ci, v = [0], [], []
    for i in range(m):
        cols = [j for j in range(max(0, i - band), min(m, i + band + 1)) if j == i or rng.random() < 0.5]
        for j in cols:
            ci.append(j)
            v.append(float(rng.choice([0.5, 1.0, 2.0]) * rng.choice([-1.0, 1.0])) if j == i else float(rng.choice([-2, -1, 1, 2])))
        rp.append(len(ci))
    rp, ci, v = np.array(rp, np.int32), np.array(ci, np.int32), np.array(v)
    o = oracle.dcsr_optimize(m, m, len(v), 0, rp, ci, v)
    assert o["status"] == 0 and not o["is_internal"]
    return rp + base, ci + base, v, o["idiag"] + base, o["iurow"] + base


def exactly_the_double_result(xs, xd, what):
    """xs (float run) == xd (double run) cast to float, and the cast loses nothing: the data was dyadic enough"""
    assert xs.dtype == np.float32 and xd.dtype == np.float64
    assert np.array_equal(xd.astype(np.float32).astype(np.float64), xd), ("the double result is not exact in fp32", what)
    assert np.array_equal(bits32(xs), bits32(xd.astype(np.float32))), what


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_strsv_equals_dtrsv_on_dyadic_data(kind, unit, base):
    m = 14
    rp, ci, v, idiag, iurow = dyadic_system(3, m, base)
    rng = np.random.default_rng(5)
    iend = idiag if kind[0] == "l" else iurow
    for incb, incx in ((1, 1), (3, 2)):
        b = rng.integers(-4, 5, m * incb).astype(np.float64)
        x0 = np.full((m - 1) * incx + 1, 7.0)
        sd, xd = oracle.dtrsv(kind, 0.5, m, base, v, ci, rp, iend, b, unit, incb=incb, incx=incx, x0=x0)
        ss, xs = oracle.strsv(kind, 0.5, m, base, v.astype(np.float32), ci, rp, iend, b.astype(np.float32), unit, incb=incb,
                              incx=incx, x0=x0.astype(np.float32))
        assert sd == ss == 0
        exactly_the_double_result(xs, xd, (kind, unit, base, incb, incx))
        assert np.all(xs[1::incx] == 7.0) or incx == 1
        assert np.abs(xd).max() > 8  # the chain did something


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("mtype,fill,trans", [(1, 0, 0), (1, 1, 0), (0, 0, 0), (0, 0, 1), (3, 0, 0), (3, 1, 1)])
def test_ssymgs_equals_dsymgs_on_dyadic_data(mtype, fill, trans, base):
    m = 9
    rp, ci, v, idiag, iurow = dyadic_system(11, m, base, band=2)
    rng = np.random.default_rng(6)
    b, x0 = rng.integers(-3, 4, m).astype(np.float64), rng.integers(-2, 3, m).astype(np.float64)
    sd, xd = oracle.dsymgs(mtype, fill, trans, base, 2.0, m, v, ci, rp, idiag, iurow, b, x0)
    ss, xs = oracle.ssymgs(mtype, fill, trans, base, 2.0, m, v, ci, rp, idiag, iurow, b, x0)
    assert sd == ss == 0
    exactly_the_double_result(xs, xd, (mtype, fill, trans, base))
    # exact arithmetic: the order of a row's terms cannot matter either
    ss, xrev = oracle.ssymgs(mtype, fill, trans, base, 2.0, m, v, ci, rp, idiag, iurow, b, x0, reversed=True)
    assert ss == 0 and np.array_equal(bits32(xrev), bits32(xs))
    assert not np.array_equal(xd, x0)


def test_ssymgs_descriptors_differ_from_each_other():
    """the four compositions are four different sweeps on an unsymmetric matrix (a swapped fill or operation shows)"""
    m = 9
    rp, ci, v, idiag, iurow = dyadic_system(11, m, 0, band=2)
    rng = np.random.default_rng(6)
    b, x0 = rng.integers(-3, 4, m).astype(np.float32), rng.integers(-2, 3, m).astype(np.float32)
    out = [oracle.ssymgs(t, f, tr, 0, 2.0, m, v, ci, rp, idiag, iurow, b, x0)[1] for t, f, tr in ((1, 0, 0), (1, 1, 0), (0, 0, 0), (0, 0, 1))]
    for i in range(4):
        for j in range(i):
            assert not np.array_equal(out[i], out[j]), (i, j)


@pytest.mark.parametrize("base", [0, 1])
def test_selltmv_and_csr2ell_float(base):
    m, n = 37, 29
    rng = np.random.default_rng(8)
    lens = rng.integers(0, 7, m)
    rp = (np.concatenate([[0], np.cumsum(lens)]) + base).astype(np.int32)
    ci = (np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in lens]) + base).astype(np.int32)
    v = rng.integers(-8, 9, len(ci)).astype(np.float32)
    x = rng.integers(-8, 9, n).astype(np.float32)
    for layout in ("ell", "ellt"):
        w, ec, ev = oracle.csr2ell(layout, m, base, rp, ci, v)
        wd, ecd, evd = oracle.csr2ell(layout, m, base, rp, ci, v.astype(np.float64))
        assert ev.dtype == np.float32 and w == wd == lens.max() and np.array_equal(ec, ecd)
        assert np.array_equal(bits32(ev), bits32(evd.astype(np.float32)))
    w, ec, ev = oracle.csr2ell("ellt", m, base, rp, ci, v)
    for alpha, beta in ((1.0, 0.0), (-0.75, 1.0), (2.5, -0.5)):
        y0 = rng.integers(-8, 9, m).astype(np.float32)
        sd, yd = oracle.dellmv("ellt", base, alpha, m, ev, ec, w, x, beta, y0)
        ss, ys = oracle.selltmv(base, alpha, m, ev, ec, w, x, beta, y0 if beta else np.full(m, np.nan, np.float32))
        assert sd == ss == 0
        exactly_the_double_result(ys, yd, (base, alpha, beta))


@pytest.mark.parametrize("base", [0, 1])
def test_ssorv_equals_dsorv_on_dyadic_data(base):
    n = 12
    rp, ci, v, _, _ = dyadic_system(21, n, base)
    rng = np.random.default_rng(9)
    x0, b = rng.integers(-3, 4, n).astype(np.float64), rng.integers(-4, 5, n).astype(np.float64)
    for omega, alpha in ((1.0, 1.0), (0.5, 2.0), (1.5, 0.0)):
        sd, xd = oracle.dsorv(n, base, rp, ci, v, omega, alpha, x0, b)
        ss, xs = oracle.ssorv(n, base, rp, ci, v, omega, alpha, x0, b)
        assert sd == ss == 0
        exactly_the_double_result(xs, xd, (base, omega, alpha))
    # the argument check of the double twin: a row without a diagonal entry
    bad = v.copy()
    bad[ci - base == np.repeat(np.arange(n), np.diff(rp))] = 0.0
    assert oracle.ssorv(n, base, rp, ci, bad, 1.0, 1.0, x0, b)[0] == oracle.dsorv(n, base, rp, ci, bad, 1.0, 1.0, x0, b)[0] == 5


@pytest.mark.skipif(oracle.ktref() is None, reason="oracle/_ref was not built: the KT restatement is pinned on the reference's own templates only there")
@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("kind", ["lt", "ut"])
def test_strsv_transposed_equals_the_kt_kernels_on_generic_data(kind, unit):
    from util import triangular_system
    m = 700
    rp, ci, v = triangular_system(31, m, 4, band=40, dtype=np.float32)
    o = oracle.dcsr_optimize(m, m, len(v), 0, rp, ci, v.astype(np.float64))
    assert not o["is_internal"]
    iend = o["idiag"] if kind[0] == "l" else o["iurow"]
    rng = np.random.default_rng(12)
    for incb, incx in ((1, 1), (2, 3)):
        b = rng.uniform(-1, 1, m * incb).astype(np.float32)
        st, xr = oracle.strsv(kind, 0.75, m, 0, v, ci, rp, iend, b, unit, incb=incb, incx=incx)
        assert st == 0 and np.isfinite(xr).all()
        for kid in (1, 2, 3):
            st, xk = oracle.trsv_kt(kind, kt_lanes(kid, np.float32), 0.75, m, 0, v, ci, rp, iend, b, unit, incb=incb, incx=incx,
                                    dtype=np.float32)
            assert st == 0 and np.array_equal(bits32(xk), bits32(xr)), (kind, unit, kid, incb)
    # and it is a solve: op(T) x = alpha b within the forward-error scale of the chain
    D = np.zeros((m, m))
    for i in range(m):
        D[i, ci[rp[i]:rp[i + 1]]] = v[rp[i]:rp[i + 1]]
    Tm = (np.tril(D) if kind[0] == "l" else np.triu(D)).T
    if unit:
        np.fill_diagonal(Tm, 1.0)
    b = rng.uniform(-1, 1, m).astype(np.float32)
    st, x = oracle.strsv(kind, 0.75, m, 0, v, ci, rp, iend, b, unit)
    res = np.abs(Tm @ x.astype(np.float64) - 0.75 * b.astype(np.float64))
    assert np.all(res <= 64 * np.finfo(np.float32).eps * (np.abs(Tm) @ np.abs(x.astype(np.float64)) + np.abs(b)))


# The Krylov twins.  Iteration margin (section f of the GPU tests uses the same rule): the float solver may take as many
# iterations more than the double one as the two float runs -- dots summed front to back, dots summed pairwise -- differ
# from each other, plus 2.  Measured on laplace5(12), b = A * uniform(-1, 1), rtol 1e-5: CG none 29 / 29 (double 29), CG SymGS
# 11 / 11 (11), GMRES(20) plain 40 / 40 (40), GMRES(20) ILU0 20 / 20 (20): a spread of 0 everywhere, so the margin is 2
# (GMRES counts whole restart cycles of 20: the same number of cycles).
def _krylov_system(g):
    n, rp, ci, v = laplace5(g)
    rng = np.random.default_rng(41)
    xe = rng.uniform(-1, 1, n)
    D = np.zeros((n, n))
    for i in range(n):
        D[i, ci[rp[i]:rp[i + 1]]] = v[rp[i]:rp[i + 1]]
    b = (D @ xe).astype(np.float32)
    o = oracle.dcsr_optimize(n, n, len(v), 0, rp, ci, v)
    return n, rp, ci, v, D, b, o


@pytest.mark.parametrize("precond", [0, 3])
def test_scg_meets_its_stopping_test(precond):
    n, rp, ci, v, D, b, o = _krylov_system(12)
    rtol = 1e-5
    sd, xd, rd = oracle.dcg(n, 0, rp, ci, v, o["idiag"], o["iurow"], b, np.zeros(n), rtol, 0.0, 500, precond)
    runs = {dots: oracle.scg(n, 0, rp, ci, v, o["idiag"], o["iurow"], b, np.zeros(n), rtol, 0.0, 500, precond, dots=dots)
            for dots in ("forward", "pairwise")}
    spread = abs(runs["forward"][2][30] - runs["pairwise"][2][30])
    print("cg precond", precond, "double", rd[30], {k: r[2][30] for k, r in runs.items()})
    for dots, (ss, xs, rs) in runs.items():
        assert sd == ss == 0 and xs.dtype == np.float32 and rs.dtype == np.float32
        true = np.linalg.norm(b.astype(np.float64) - D @ xs.astype(np.float64))
        assert rs[0] <= rtol * rs[1] and true <= rtol * np.linalg.norm(b), (dots, true, rs[0])
        assert abs(rs[1] - np.linalg.norm(b)) <= 1e-5 * np.linalg.norm(b)
        assert 1 <= rs[30] <= rd[30] + spread + 2, (dots, rs[30], rd[30], spread)


@pytest.mark.parametrize("precond", [0, 2])
def test_sgmres_meets_its_stopping_test(precond):
    n, rp, ci, v, D, b, o = _krylov_system(12)
    rtol, restart = 1e-5, 20
    sd, xd, rd = oracle.dgmres(n, 0, rp, ci, v, b, np.ones(n), restart, rtol, 1e-12, 400, precond)
    runs = {dots: oracle.sgmres(n, 0, rp, ci, v, b, np.ones(n), restart, rtol, 1e-12, 400, precond, dots=dots)
            for dots in ("forward", "pairwise")}
    spread = abs(runs["forward"][2][30] - runs["pairwise"][2][30])
    print("gmres precond", precond, "double", rd[30], {k: r[2][30] for k, r in runs.items()})
    for dots, (ss, xs, rs) in runs.items():
        assert sd == ss == 0 and xs.dtype == np.float32
        true = np.linalg.norm(b.astype(np.float64) - D @ xs.astype(np.float64))
        assert true <= rtol * np.linalg.norm(b), (dots, true)
        assert 1 <= rs[30] <= rd[30] + spread + 2, (dots, rs[30], rd[30], spread)


# ---- orc_scsrmm_col / orc_scsrmm_row: the float instantiation of the csrmm macros (DEF_CSRMM_COL / DEF_CSRMM_ROW, oracle.c) -----

def _short_rows(seed, m, k, maxlen, base, values):
    """sorted CSR, rows of 0..maxlen entries (some empty), values drawn by values(rng, count)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, maxlen + 1, m)
    lens[::17] = 0
    rp = (np.concatenate([[0], np.cumsum(lens)]) + base).astype(np.int32)
    ci = (np.concatenate([np.sort(rng.choice(k, q, replace=False)) for q in lens]) + base).astype(np.int32)
    return rp, ci, values(rng, len(ci))


def _dense_operand(rng, order, rows, n, ld, draw, pad):
    """rows x n operand in `order` with leading dimension ld, flat; the padding holds `pad`.  -> (flat, mask of the padding)"""
    buf = np.full((n, ld) if order == "col" else (rows, ld), pad, np.float64)
    used = np.zeros(buf.shape, bool)
    if order == "col":
        used[:, :rows] = True
    else:
        used[:, :n] = True
    buf[used] = draw(rng, int(used.sum()))
    return buf.ravel(), ~used.ravel()


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("order", ["col", "row"])
def test_scsrmm_equals_dcsrmm_on_dyadic_data(order, base):
    """small integers in A, B and C, power-of-two alpha and beta: every intermediate of the double run is exact in fp32"""
    m, k, n = 23, 19, 5
    ints = lambda rng, count: rng.integers(-4, 5, count).astype(np.float64)
    rp, ci, v = _short_rows(13, m, k, 6, base, ints)
    rng = np.random.default_rng(14)
    ldb, ldc = (k + 3, m + 2) if order == "col" else (n + 3, n + 2)
    B, _ = _dense_operand(rng, order, k, n, ldb, ints, 99.0)
    C0, padding = _dense_operand(rng, order, m, n, ldc, ints, 77.0)
    for alpha, beta in ((1.0, 0.0), (0.5, -2.0), (-4.0, 0.25)):
        sd, Cd = oracle.dcsrmm(order, alpha, base, v, ci, rp, m, B, n, ldb, beta, C0, ldc)
        ss, Cs = oracle.scsrmm(order, alpha, base, v.astype(np.float32), ci, rp, m, B.astype(np.float32), n, ldb, beta,
                               C0.astype(np.float32), ldc)
        assert sd == ss == 0
        exactly_the_double_result(Cs[~padding], Cd[~padding], (order, base, alpha, beta))
        assert np.all(Cs[padding] == 77.0) and np.all(Cd[padding] == 77.0)
        assert np.abs(Cd[~padding]).max() > 16  # the chain did something


@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (1.7, -0.3)])
def test_scsrmm_col_equals_the_kt_kernel_below_its_lane_count(alpha, beta):
    """full mantissas, every row shorter than 8 entries: below the lane count csrmm_col_kt is the scalar chain from zero followed
    by fma(beta, C, alpha * cij) (oracle.c DEF_CSRMM_COL_KT, pinned to the reference's templates by tests/test_oracle_kt.py), the
    arithmetic of csrmm_col_major_ref -- so the two restatements, written apart, agree bit for bit"""
    m, k, n = 300, 260, 9
    uni = lambda rng, count: rng.uniform(-1, 1, count).astype(np.float32)
    rp, ci, v = _short_rows(15, m, k, 7, 1, uni)
    assert np.diff(rp).max() == 7 and np.any(np.diff(rp) == 0)
    rng = np.random.default_rng(16)
    ldb, ldc = k + 3, m + 1
    B, C0 = uni(rng, ldb * n), uni(rng, ldc * n)
    ss, Cs = oracle.scsrmm("col", alpha, 1, v, ci, rp, m, B, n, ldb, beta, C0, ldc)
    assert ss == 0 and Cs.dtype == np.float32
    for psz in (8, 16):
        sk, Ck = oracle.scsrmm_kt("col", psz, alpha, 1, v, ci, rp, m, B, n, ldb, beta, C0, ldc)
        assert sk == 0 and np.array_equal(bits32(Ck), bits32(Cs)), psz
    assert not np.array_equal(Cs, C0)


def _stencil_case():
    """the 5-point stencil of tests/test_gpu_scsrmm_kernels.py (its matrix "lap61": laplace5(61), values perturbed with the same
    seed) times eight columns of uniform(-1, 1), the distribution of every operand there"""
    m, rp, ci, v = laplace5(61)
    rng = np.random.default_rng(8)
    v = (v * rng.uniform(0.5, 1.5, len(v))).astype(np.float32)
    n = 8
    B, C0 = rng.uniform(-1, 1, m * n).astype(np.float32), rng.uniform(-1, 1, m * n).astype(np.float32)
    return m, rp, ci, v, n, B, C0


def test_scsrmm_tells_the_fmaf_chain_from_its_neighbours():
    """On the data the GPU tests use a kernel that multiplies and then adds, or one that accumulates in double and rounds once,
    is a different function: measured with NumPy on 200,000 uniform(-1, 1) samples, the first differs from the fmaf chain in
    36 % / 44 % / 56 % of the elements at row lengths 3 / 5 / 12 and the second in 34 % / 44 % / 59 %.  The floor of 20 % sits
    under the smallest of them; it is no tolerance."""
    m, rp, ci, v, n, B, C0 = _stencil_case()
    ss, C = oracle.scsrmm("col", 1.0, 0, v, ci, rp, m, B, n, m, 0.0, C0, m)
    with oracle.contract(False):
        su, Cu = oracle.scsrmm("col", 1.0, 0, v, ci, rp, m, B, n, m, 0.0, C0, m)
    sd, Cd = oracle.dcsrmm("col", 1.0, 0, v, ci, rp, m, B, n, m, 0.0, C0, m)
    assert ss == su == sd == 0
    unfused = np.mean(bits32(Cu) != bits32(C))
    once = np.mean(bits32(Cd.astype(np.float32)) != bits32(C))
    print("differs from the fmaf chain: unfused %.3f, double rounded once %.3f" % (unfused, once))
    assert unfused >= 0.20 and once >= 0.20
    ss, again = oracle.scsrmm("col", 1.0, 0, v, ci, rp, m, B, n, m, 0.0, C0, m)
    assert np.array_equal(bits32(again), bits32(C))  # the switch was restored


@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (1.7, -0.3)])
def test_scsrmm_row_against_col(alpha, beta):
    """two different chains (row: C *= beta, then fma(a b, alpha, C) per entry; col: the dot, then fma(beta, C, alpha dot)): within
    the bound of test_csrmm_random_vs_oracle with the float unit roundoff, (len + 3) u |alpha| sum |a b| + 2 u |beta c|"""
    m, k, n = 200, 170, 7
    uni = lambda rng, count: rng.uniform(-1, 1, count).astype(np.float32)
    rp, ci, v = _short_rows(17, m, k, 13, 1, uni)
    rng = np.random.default_rng(18)
    Bm, Cm = uni(rng, k * n).reshape(k, n), uni(rng, m * n).reshape(m, n)
    ldb, ldc = n + 2, n + 3
    Br, Cr = np.zeros((k, ldb), np.float32), np.full((m, ldc), 5.0, np.float32)
    Br[:, :n], Cr[:, :n] = Bm, Cm
    sr, Crow = oracle.scsrmm("row", alpha, 1, v, ci, rp, m, Br.ravel(), n, ldb, beta, Cr.ravel(), ldc)
    sc, Ccol = oracle.scsrmm("col", alpha, 1, v, ci, rp, m, np.ascontiguousarray(Bm.T).ravel(), n, k, beta,
                             np.ascontiguousarray(Cm.T).ravel(), m)
    assert sr == sc == 0
    Crow = Crow.reshape(m, ldc)
    assert np.all(Crow[:, n:] == 5.0)
    u = float(np.finfo(np.float32).eps)  # (test_csrmm_random_vs_oracle uses finfo(float64).eps)
    scale = np.zeros((m, n))
    for i in range(m):
        s, e = rp[i] - 1, rp[i + 1] - 1
        scale[i] = np.abs(v[s:e]).astype(np.float64) @ np.abs(Bm[ci[s:e] - 1]).astype(np.float64)
    lens = np.diff(rp)[:, None]
    diff = np.abs(Crow[:, :n].astype(np.float64) - Ccol.reshape(n, m).T.astype(np.float64))
    assert np.all(diff <= (lens + 3) * u * scale * abs(alpha) + 2 * u * np.abs(beta * Cm.astype(np.float64)) + 1e-300)
    assert diff.max() > 0  # they are different chains
