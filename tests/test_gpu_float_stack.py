"""The single-precision solver stack on the GPU against the float restatements of the oracle (oracle/oracle_tmpl.h, pinned by
tests/test_oracle_float_cpu.py): transposed strsv under every schedule, strsm, the ssymgs family, sdotmv, ELL-T and the float
converters, itsol_s_*, smv on symmetric / triangular descriptors, ssorv.  Every comparison with a float oracle CHAIN is on the
uint32 view; reductions whose order the library is free to choose, and the Krylov solvers, carry the bound stated at the test."""
import ctypes

import numpy as np
import pytest

import oracle
from util import EPS32, kt_lanes, laplace5, pkg, random_csr, trsv_schedule

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
P = pkg()
L = P.lib()

from test_gpu_trsv_blocks import VARIANTS, mixed, node_mesh  # noqa: E402

F32 = np.float32
TAG32 = np.array([0x7FC0D355], dtype=np.uint32).view(F32)[0]  # the float solves' NOT-READY word (a quiet NaN)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == F32, a.dtype
    return a.view(np.uint32)


def same_bits(got, ref, what):
    g, r = bits(got), bits(ref)
    bad = np.flatnonzero(g != r)
    assert len(bad) == 0, (what, "differing", len(bad), "first", int(bad[0]), float(np.ravel(got)[bad[0]]), float(np.ravel(ref)[bad[0]]))


def same_up_to_nan_payload(got, ref, what):
    """NaN where the chain has NaN (payloads may differ between x86 and gfx950), identical bits elsewhere"""
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), (what, int(gn.sum()), int(rn.sum()))
    same_bits(got[~gn], ref[~rn], what)


@pytest.fixture
def forced_chunks():
    assert L.aoclsparse_mi355_set_option(P.OPTION_TRSV_CHUNKS, 1) == 0
    yield
    assert L.aoclsparse_mi355_set_option(P.OPTION_TRSV_CHUNKS, -1) == 0


def float_mesh(seed, nodes):
    """node_mesh(width 37, mixed dofs, far = 28) cast to float32 + the clean-CSR indices: a block plan, single rows longer
    than one poll batch, halos between chunks"""
    m, rp, ci, v = node_mesh(seed, nodes, 37, mixed(np.random.default_rng(3), nodes), far=28)
    o = oracle.dcsr_optimize(m, m, len(v), 0, rp, ci, v)
    assert not o["is_internal"]
    return m, rp, ci, v.astype(F32), o


# --------------------------------------------------------------------------------------------------
# a. strsv, transposed and not, every schedule
# --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mesh2500():
    m, rp, ci, vf, o = float_mesh(1900, 2500)
    rng = np.random.default_rng(12)
    ref = {}
    for kind, fill, op in VARIANTS:
        for unit in (True, False):
            b = rng.uniform(-1, 1, m).astype(F32)
            st, xr = oracle.strsv(kind, 0.75, m, 0, vf, ci, rp, o["idiag"] if kind[0] == "l" else o["iurow"], b, unit)
            assert st == 0 and np.isfinite(xr).all()
            ref[kind, unit] = (b, xr)
    return m, rp, ci, vf, o, ref


def _solve_all(A, m, ref, sched, want):
    for kind, fill, op in VARIANTS:
        for unit in (True, False):
            d = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=getattr(P, fill), diag=P.DIAG_UNIT if unit else P.DIAG_NON_UNIT)
            b, xr = ref[kind, unit]
            with trsv_schedule(P, sched):
                xd = torch.full((m,), 7.0, dtype=torch.float32, device="cuda")
                assert P.strsv(getattr(P, op), 0.75, A, d, dev(b), xd) == 0, (kind, unit, sched)
                torch.cuda.synchronize()
                info = A.trsv_info(getattr(P, fill), getattr(P, op))
            same_bits(xd.cpu().numpy(), xr, (kind, unit, sched))
            if want is not None:
                assert info.schedule in want, (kind, unit, sched, info.schedule)


@pytest.mark.parametrize("sched", [0, 1, 2, 3, 4, 5, -1])
def test_strsv_every_triangle_every_schedule(mesh2500, sched):
    """L, U, L^T, U^T x unit / non-unit in fp32 under the per-level launches (0), the hybrid (1), the three sync-free kernels
    (2, 3, 4: 4-byte tagged NOT-READY words), the two-level schedule where the plan-time model built its chunk plan (5; it falls
    back to 4 where it did not, so 4 or 5 is reported) and the automatic choice: the serial chain of ref_trsv_* in float bit
    for bit (alpha = 0.75, x prefilled with 7), and the schedule reported is the one asked for."""
    m, rp, ci, vf, o, ref = mesh2500
    A = P.Matrix(0, m, m, rp, ci, vf)
    _solve_all(A, m, ref, sched, None if sched < 0 else ((4, 5) if sched == 5 else (sched,)))
    assert A.trsv_info(P.FILL_LOWER, P.OP_TRANSPOSE).blocks > 0  # the mesh has a block plan


def test_strsv_two_level_schedule_forced(mesh2500, forced_chunks):
    """schedule 5 with the chunk plan built whatever the model says (OPTION_TRSV_CHUNKS = 1): the two-level kernel runs"""
    m, rp, ci, vf, o, ref = mesh2500
    A = P.Matrix(0, m, m, rp, ci, vf)
    _solve_all(A, m, ref, 5, (5,))
    info = A.trsv_info(P.FILL_UPPER, P.OP_TRANSPOSE)
    assert info.chunks >= 2 and info.steps > info.chunks, (info.chunks, info.steps)


def test_strsv_transposed_strided(mesh2500):
    m, rp, ci, vf, o, ref = mesh2500
    A = P.Matrix(0, m, m, rp, ci, vf)
    incb, incx = 3, 2
    rng = np.random.default_rng(9)
    for kind, fill, iend in (("lt", P.FILL_LOWER, o["idiag"]), ("ut", P.FILL_UPPER, o["iurow"])):
        d = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=fill)
        b = rng.uniform(-1, 1, m * incb).astype(F32)
        st, xr = oracle.strsv(kind, 1.5, m, 0, vf, ci, rp, iend, b, False, incb=incb, incx=incx, x0=np.full(m * incx, 7.0, F32))
        assert st == 0
        xh = np.full(m * incx, 7.0, F32)
        assert L.aoclsparse_strsv_strided(P.OP_TRANSPOSE, 1.5, A.h, d.h, P._ptr(b), incb, P._ptr(xh), incx) == 0
        same_bits(xh[::incx], xr[::incx], (kind, "host"))
        assert np.all(xh[1::incx] == 7.0)
        xd = dev(np.full(m * incx, 7.0, F32))
        assert L.aoclsparse_strsv_strided(P.OP_TRANSPOSE, 1.5, A.h, d.h, P._ptr(dev(b)), incb, P._ptr(xd), incx) == 0
        torch.cuda.synchronize()
        same_bits(xd.cpu().numpy(), xh, (kind, "device"))


def test_strsv_transposed_nan_inf_and_tag(mesh2500):
    """NaN, +Inf and the float NOT-READY pattern 0x7FC0D355 in b under op = T: the same propagation as the serial chain, under
    the automatic schedule and the sync-free ones, never a hang or an error"""
    m, rp, ci, vf, o, ref = mesh2500
    A = P.Matrix(0, m, m, rp, ci, vf)
    rng = np.random.default_rng(8)
    for kind, fill, iend in (("lt", P.FILL_LOWER, o["idiag"]), ("ut", P.FILL_UPPER, o["iurow"])):
        d = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=fill)
        b = rng.uniform(-1, 1, m).astype(F32)
        b[[m // 3, m // 2, m // 2 + 40]] = [np.nan, np.inf, TAG32]
        st, xr = oracle.strsv(kind, 1.0, m, 0, vf, ci, rp, iend, b, False)
        assert st == 0 and 2 <= np.isnan(xr).sum() < m
        for sched in (-1, 2, 4):
            with trsv_schedule(P, sched):
                xd = torch.zeros(m, dtype=torch.float32, device="cuda")
                assert P.strsv(P.OP_TRANSPOSE, 1.0, A, d, dev(b), xd) == 0
                torch.cuda.synchronize()
            same_up_to_nan_payload(xd.cpu().numpy(), xr, (kind, sched))
        assert L.aoclsparse_mi355_trsv_status(A.h) == 0


# --------------------------------------------------------------------------------------------------
# b. strsm and strsm_kid
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", [-1, 5])
@pytest.mark.parametrize("order", ["column", "row"])
def test_strsm_every_column_is_the_chain(order, sched):
    """n = 5 right-hand sides, both layouts with padded leading dimensions, L / L^T / U^T / U with unit and non-unit alternating,
    alpha = 0.5: every column equals oracle.strsv of that column, the padding keeps its 7s; kid 3 gives the 512-bit KT order
    (16 float lanes) for L and U."""
    m, rp, ci, vf, o = float_mesh(1500, 1500)
    A = P.Matrix(0, m, m, rp, ci, vf)
    n = 5
    rng = np.random.default_rng(12)
    for kind, fill, op, unit in (("l", P.FILL_LOWER, P.OP_NONE, True), ("lt", P.FILL_LOWER, P.OP_TRANSPOSE, False),
                                 ("ut", P.FILL_UPPER, P.OP_TRANSPOSE, True), ("u", P.FILL_UPPER, P.OP_NONE, False)):
        d = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=fill, diag=P.DIAG_UNIT if unit else P.DIAG_NON_UNIT)
        iend = o["idiag"] if kind[0] == "l" else o["iurow"]
        if order == "column":
            ld, shape, lay = m + 3, (n, m + 3), P.ORDER_COLUMN
            cols, pad_ok = (lambda M, j: M[j, :m]), (lambda M: np.all(M[:, m:] == 7.0))
        else:
            ld, shape, lay = n + 2, (m, n + 2), P.ORDER_ROW
            cols, pad_ok = (lambda M, j: M[:, j]), (lambda M: np.all(M[:, n:] == 7.0))
        Bm = rng.uniform(-1, 1, shape).astype(F32)
        want = [oracle.strsv(kind, 0.5, m, 0, vf, ci, rp, iend, np.ascontiguousarray(cols(Bm, j)), unit) for j in range(n)]
        assert all(st == 0 for st, _ in want)
        with trsv_schedule(P, sched):
            Xh = np.full(shape, 7.0, F32)
            assert L.aoclsparse_strsm(op, 0.5, A.h, d.h, lay, P._ptr(Bm), n, ld, P._ptr(Xh), ld) == 0
            Xd = dev(np.full(shape, 7.0, F32))
            assert L.aoclsparse_strsm(op, 0.5, A.h, d.h, lay, P._ptr(dev(Bm)), n, ld, P._ptr(Xd), ld) == 0
            torch.cuda.synchronize()
        for X, where in ((Xh, "host"), (Xd.cpu().numpy(), "device")):
            assert pad_ok(X), (kind, order, where)
            for j in range(n):
                same_bits(np.ascontiguousarray(cols(X, j)), want[j][1], (kind, order, sched, where, j))
        if op == P.OP_NONE and sched < 0:
            Xk = dev(np.full(shape, 7.0, F32))
            assert L.aoclsparse_strsm_kid(op, 0.5, A.h, d.h, lay, P._ptr(dev(Bm)), n, ld, P._ptr(Xk), ld, 3) == 0
            torch.cuda.synchronize()
            X = Xk.cpu().numpy()
            assert pad_ok(X)
            for j in range(n):
                st, xk = oracle.trsv_kt(kind, kt_lanes(3, F32), 0.5, m, 0, vf, ci, rp, iend, np.ascontiguousarray(cols(Bm, j)), unit,
                                        dtype=F32)
                assert st == 0
                same_bits(np.ascontiguousarray(cols(X, j)), xk, (kind, order, "kid 3", j))


# --------------------------------------------------------------------------------------------------
# c. the ssymgs family
# --------------------------------------------------------------------------------------------------
SYMGS_CASES = [("symmetric-lower", 1, 0, 0), ("symmetric-upper", 1, 1, 0), ("general-N", 0, 0, 0), ("general-T", 0, 0, 1)]


def _symgs_system(base):
    m, rp, ci, v = laplace5(70)
    rng = np.random.default_rng(17)
    v = v.copy()
    v[v < 0] = rng.uniform(-1.0, -0.2, np.count_nonzero(v < 0))  # randomised off-diagonals: the triangles differ
    vf = v.astype(F32)
    o = oracle.dcsr_optimize(m, m, len(v), 0, rp, ci, v)
    assert not o["is_internal"]
    b, x0 = rng.uniform(-1, 1, m).astype(F32), rng.uniform(-1, 1, m).astype(F32)
    return m, rp + base, ci + base, vf, o["idiag"] + base, o["iurow"] + base, b, x0


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("name,mtype,fill,trans", SYMGS_CASES)
def test_ssymgs_sweep_is_the_float_chain(name, mtype, fill, trans, base):
    """One sweep (alpha = 0.9) from a random x0 on laplace5(70) with randomised off-diagonals.  The two solves are serial chains;
    the two triangular products (rows of at most 2 entries here) are not pinned to an order.  Measured on an MI355X against
    oracle.ssymgs, both bases alike: symmetric-upper and general-N -- no transposed product in the composition -- are BIT-EQUAL,
    and are asserted so; symmetric-lower and general-T -- whose products are transposed: the reference sweeps columns and scales
    x by alpha first, the library gathers rows -- differ in 935 / 916 of 4900 entries by at most 0.5 eps32.  For those the bound
    of the double test, |x - x_ref| <= k eps32 max(1, |x_ref|_inf) with its k = 64: the float oracle against itself with every
    product row summed in the opposite order (the spread that would replace 64 if it were larger) differs by at most
    0.5 eps32 (symmetric-lower) and 0.25 eps32 (the other three).
    ssymgs_mv: y is smv of the returned x on the same handle and descriptor, host and device vectors give the same bits, and the
    _kid variants (0, 3) return the plain call's bits (symgs_t ignores kid, as the reference does)."""
    m, rp, ci, vf, idiag, iurow, b, x0 = _symgs_system(base)
    A = P.Matrix(base, m, m, rp, ci, vf)
    d = P.Descr(base=base, mtype=P.TYPE_SYMMETRIC if mtype == 1 else P.TYPE_GENERAL, fill=P.FILL_UPPER if fill else P.FILL_LOWER)
    op = P.OP_TRANSPOSE if trans else P.OP_NONE
    st, xr = oracle.ssymgs(mtype, fill, trans, base, 0.9, m, vf, ci, rp, idiag, iurow, b, x0)
    st2, xrev = oracle.ssymgs(mtype, fill, trans, base, 0.9, m, vf, ci, rp, idiag, iurow, b, x0, reversed=True)
    assert st == st2 == 0
    x = x0.copy()
    assert L.aoclsparse_ssymgs(op, A.h, d.h, 0.9, P._ptr(b), P._ptr(x)) == 0
    print("ssymgs", name, base, "bit-equal", np.array_equal(bits(x), bits(xr)), "max |x - x_ref| / eps32",
          float(np.max(np.abs(x.astype(np.float64) - xr)) / EPS32), "oracle forward vs reversed / eps32",
          float(np.max(np.abs(xrev.astype(np.float64) - xr)) / EPS32))
    if name in ("symmetric-upper", "general-N"):
        same_bits(x, xr, (name, base))
    else:
        spread = float(np.max(np.abs(xrev.astype(np.float64) - xr)))
        k = 64.0
        if spread > k * EPS32 * max(1.0, float(np.abs(xr).max())):
            k = 2.0 * spread / (EPS32 * max(1.0, float(np.abs(xr).max())))
        assert k == 64.0  # the measured spread (0.5 eps32) is far below: the double test's k stands
        assert np.max(np.abs(x.astype(np.float64) - xr)) <= k * EPS32 * max(1.0, float(np.abs(xr).max())), (name, base)
    # device vectors, the _kid variants
    for kid in (None, 0, 3):
        xd, bd = dev(x0), dev(b)
        if kid is None:
            assert L.aoclsparse_ssymgs(op, A.h, d.h, 0.9, P._ptr(bd), P._ptr(xd)) == 0
        else:
            assert L.aoclsparse_ssymgs_kid(op, A.h, d.h, 0.9, P._ptr(bd), P._ptr(xd), kid) == 0
        torch.cuda.synchronize()
        same_bits(xd.cpu().numpy(), x, (name, base, "device", kid))
    # ssymgs_mv and ssymgs_mv_kid: the same x, and y = op(A) x
    xm, ym = x0.copy(), np.full(m, np.nan, F32)
    assert L.aoclsparse_ssymgs_mv(op, A.h, d.h, 0.9, P._ptr(b), P._ptr(xm), P._ptr(ym)) == 0
    same_bits(xm, x, (name, base, "mv x"))
    y = np.full(m, np.nan, F32)
    assert P.smv(op, 1.0, A, d, xm, 0.0, y) == 0
    same_bits(ym, y, (name, base, "mv y"))
    assert np.isfinite(y).all() and np.abs(y).max() > 0.1
    for kid in (None, 0, 3):
        xd, yd = dev(x0), dev(np.full(m, np.nan, F32))
        if kid is None:
            assert L.aoclsparse_ssymgs_mv(op, A.h, d.h, 0.9, P._ptr(dev(b)), P._ptr(xd), P._ptr(yd)) == 0
        else:
            assert L.aoclsparse_ssymgs_mv_kid(op, A.h, d.h, 0.9, P._ptr(dev(b)), P._ptr(xd), P._ptr(yd), kid) == 0
        torch.cuda.synchronize()
        same_bits(xd.cpu().numpy(), x, (name, base, "mv device x", kid))
        same_bits(yd.cpu().numpy(), ym, (name, base, "mv device y", kid))


@pytest.mark.parametrize("base", [0, 1])
def test_ssymgs_triangular_descriptor_is_one_solve(base):
    m, rp, ci, vf, idiag, iurow, b, x0 = _symgs_system(base)
    A = P.Matrix(base, m, m, rp, ci, vf)
    for kind, fill, op, iend in (("l", P.FILL_LOWER, P.OP_NONE, idiag), ("ut", P.FILL_UPPER, P.OP_TRANSPOSE, iurow)):
        d = P.Descr(base=base, mtype=P.TYPE_TRIANGULAR, fill=fill)
        st, xr = oracle.strsv(kind, 1.0, m, base, vf, ci, rp, iend, b, False)
        x = x0.copy()
        assert st == 0 and L.aoclsparse_ssymgs(op, A.h, d.h, 0.9, P._ptr(b), P._ptr(x)) == 0
        same_bits(x, xr, (kind, base))


# --------------------------------------------------------------------------------------------------
# d. sdotmv
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opname", ["n", "t"])
def test_sdotmv(opname):
    """y bit-identical to smv on the same handle; d = x . y over min(m, n) entries within 2 k eps32 sum |x_i y_i| of a float64
    dot of the same y (k terms, any summation tree: the standard bound k eps with a factor 2 as in the double test); host and
    device operands give the same y; a null d is an invalid pointer."""
    m, n = 900, 700
    rp, ci, v = random_csr(171, m, n, lambda r, i: r.integers(0, 12), dtype=F32)
    A, d = P.Matrix(0, m, n, rp, ci, v), P.Descr()
    op = P.OP_NONE if opname == "n" else P.OP_TRANSPOSE
    nx, ny = (n, m) if opname == "n" else (m, n)
    rng = np.random.default_rng(8)
    x, y0 = rng.uniform(-1, 1, nx).astype(F32), rng.uniform(-1, 1, ny).astype(F32)
    yr = y0.copy()
    assert P.smv(op, 1.3, A, d, x, -0.2, yr) == 0
    y, dot = y0.copy(), np.zeros(1, F32)
    assert L.aoclsparse_sdotmv(op, 1.3, A.h, d.h, P._ptr(x), -0.2, P._ptr(y), P._ptr(dot)) == 0
    same_bits(y, yr, opname)
    k = min(m, n)
    ref = float(np.dot(x[:k].astype(np.float64), yr[:k].astype(np.float64)))
    scale = float(np.dot(np.abs(x[:k]).astype(np.float64), np.abs(yr[:k]).astype(np.float64)))
    print("sdotmv", opname, "error / (eps32 * scale)", abs(float(dot[0]) - ref) / (EPS32 * scale))
    assert abs(float(dot[0]) - ref) <= 2 * k * EPS32 * scale
    xd, yd, dd = dev(x), dev(y0), torch.zeros(1, dtype=torch.float32, device="cuda")
    assert L.aoclsparse_sdotmv(op, 1.3, A.h, d.h, P._ptr(xd), -0.2, P._ptr(yd), P._ptr(dd)) == 0
    torch.cuda.synchronize()
    same_bits(yd.cpu().numpy(), yr, (opname, "device"))
    assert abs(dd.item() - ref) <= 2 * k * EPS32 * scale
    assert L.aoclsparse_sdotmv(op, 1.3, A.h, d.h, P._ptr(x), -0.2, P._ptr(y), None) == 2


# --------------------------------------------------------------------------------------------------
# e. ELL-T and the float converters
# --------------------------------------------------------------------------------------------------
def _ell_rows(seed, m, n, maxlen, long_every=0):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, maxlen, m)
    lens[min(5, m - 1)] = 0
    if long_every:
        lens[::long_every] = rng.integers(3 * maxlen, 9 * maxlen, len(lens[::long_every]))
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in lens]).astype(np.int32)
    return rp, ci, rng.uniform(-1, 1, len(ci))


@pytest.mark.parametrize("base", [0, 1])
def test_float_ell_conversions_and_selltmv(base):
    """the matrix of test_ell_family_bit_exact in float32: scsr2ell / scsr2ellt equal the restated conversion cell for cell
    (padding columns included), selltmv equals the float chain bit for bit (beta == 0 must not read y), scsr2ellthyb has the
    structure of dcsr2ellthyb, sellthybmv is not implemented (as in the reference)."""
    m, n = 5000, 4700
    rp, ci, v = _ell_rows(51, m, n, 23, long_every=97)
    rp, ci, vf = rp + base, ci + base, v.astype(F32)
    d = P.Descr(base=base)
    w = ctypes.c_int32(-1)
    assert L.aoclsparse_csr2ell_width(m, len(vf), P._ptr(rp), ctypes.byref(w)) == 0
    conv = {}
    for layout, fn in (("ell", L.aoclsparse_scsr2ell), ("ellt", L.aoclsparse_scsr2ellt)):
        wo, ec, ev = oracle.csr2ell(layout, m, base, rp, ci, vf)
        assert w.value == wo and ev.dtype == F32
        gc, gv = np.full(m * wo, 77, np.int32), np.full(m * wo, 77.0, F32)
        assert fn(m, d.h, P._ptr(rp), P._ptr(ci), P._ptr(vf), P._ptr(gc), P._ptr(gv), wo) == 0
        assert np.array_equal(gc, ec), layout
        same_bits(gv, ev, layout)
        conv[layout] = (wo, gc, gv)
    wo, ec, ev = conv["ellt"]
    rng = np.random.default_rng(52)
    x = rng.uniform(-1, 1, n).astype(F32)
    for alpha, beta in ((1.0, 0.0), (-0.75, 1.0), (2.5, -0.5)):
        y0 = rng.uniform(-1, 1, m).astype(F32) if beta != 0.0 else np.full(m, np.nan, F32)
        a, b = np.array([alpha], F32), np.array([beta], F32)
        st, yr = oracle.selltmv(base, alpha, m, ev, ec, wo, x, beta, y0)
        assert st == 0 and np.isfinite(yr).all()
        y = y0.copy()
        assert L.aoclsparse_selltmv(P.OP_NONE, P._ptr(a), m, n, len(vf), P._ptr(ev), P._ptr(ec), wo, d.h, P._ptr(x), P._ptr(b), P._ptr(y)) == 0
        same_bits(y, yr, (alpha, beta, "host"))
        yd = dev(y0)
        assert L.aoclsparse_selltmv(P.OP_NONE, P._ptr(a), m, n, len(vf), P._ptr(dev(ev)), P._ptr(dev(ec)), wo, d.h, P._ptr(dev(x)), P._ptr(b),
                                    P._ptr(yd)) == 0
        torch.cuda.synchronize()
        same_bits(yd.cpu().numpy(), yr, (alpha, beta, "device"))
    # ELLT-HYB: the float conversion against the double one on the same pattern
    wh, em = ctypes.c_int32(-1), ctypes.c_int32(-1)
    assert L.aoclsparse_csr2ellthyb_width(m, len(vf), P._ptr(rp), ctypes.byref(em), ctypes.byref(wh)) == 0
    out = {}
    for fn, vals, dt in ((L.aoclsparse_dcsr2ellthyb, vf.astype(np.float64), np.float64), (L.aoclsparse_scsr2ellthyb, vf, F32)):
        gc, gv, gm, em2 = np.full(m * wh.value, 77, np.int32), np.full(m * wh.value, 77.0, dt), np.full(m, -5, np.int32), ctypes.c_int32(0)
        assert fn(m, base, ctypes.byref(em2), P._ptr(rp), P._ptr(ci), P._ptr(vals), None, P._ptr(gm), P._ptr(gc), P._ptr(gv), wh.value) == 0
        out[dt] = (em2.value, gm, gc, gv)
    (emd, gmd, gcd, gvd), (ems, gms, gcs, gvs) = out[np.float64], out[F32]
    assert emd == ems == em.value and 0 < m - ems < m and np.array_equal(gmd, gms) and np.array_equal(gcd, gcs)
    same_bits(gvs, gvd.astype(F32), "ellthyb values")
    wo2, emo, mp, hc, hv = oracle.csr2ell("hyb", m, base, rp, ci, vf)
    assert (wo2, emo) == (wh.value, ems) and np.array_equal(gms[: m - emo], mp) and np.array_equal(gcs, hc)
    same_bits(gvs, hv, "ellthyb values against the oracle")
    a, b, y = np.array([1.0], F32), np.array([0.0], F32), np.zeros(m, F32)
    assert L.aoclsparse_sellthybmv(P.OP_NONE, P._ptr(a), m, n, len(vf), P._ptr(gvs), P._ptr(gcs), wh.value, ems, P._ptr(vf), P._ptr(rp),
                                   P._ptr(ci), None, P._ptr(gms), d.h, P._ptr(x), P._ptr(b), P._ptr(y)) == 1  # not_implemented


@pytest.mark.parametrize("base", [0, 1])
def test_float_bsr_and_dia_conversions(base):
    """scsr2bsr (block dimensions 2, 4, 5; both block orders) and scsr2dia copy values: exactly the restated conversion run
    on the same float values"""
    m, n = 1203, 1167
    rp, ci, v = random_csr(95, m, n, lambda r, i: r.integers(0, 9), base=base, sort=False, dtype=F32)
    d = P.Descr(base=base)
    for dim in (2, 4, 5):
        for order, rowmajor in ((P.ORDER_ROW, True), (P.ORDER_COLUMN, False)):
            mb = (m + dim - 1) // dim
            bp, nnzb = np.zeros(mb + 1, np.int32), ctypes.c_int32(-1)
            assert L.aoclsparse_csr2bsr_nnz(m, n, d.h, P._ptr(rp), P._ptr(ci), dim, P._ptr(bp), ctypes.byref(nnzb)) == 0
            obp, obi, obv = oracle.csr2bsr(m, n, base, rp, ci, v, dim, rowmajor)
            assert nnzb.value == len(obi) and np.array_equal(bp, obp)
            bi, bv = np.zeros(nnzb.value, np.int32), np.zeros(nnzb.value * dim * dim, F32)  # (the caller zeroes the blocks: convert.hpp:389-551 writes the stored entries only)
            assert L.aoclsparse_scsr2bsr(m, n, d.h, order, P._ptr(v), P._ptr(rp), P._ptr(ci), dim, P._ptr(bv), P._ptr(bp), P._ptr(bi)) == 0
            assert np.array_equal(bi, obi), (dim, order)
            same_bits(bv, obv.astype(F32), (dim, order))
            assert np.array_equal(obv.astype(F32).astype(np.float64), obv) and np.count_nonzero(bv) == len(v)
    mb, nb = 300, 300  # a band: few diagonals
    rows = [np.arange(max(0, i - 4), min(nb, i + 5)) for i in range(mb)]
    brp = (np.concatenate([[0], np.cumsum([len(r) for r in rows])]) + base).astype(np.int32)
    bci = (np.concatenate(rows) + base).astype(np.int32)
    bv = np.random.default_rng(12).uniform(-1, 1, len(bci)).astype(F32)
    nd = ctypes.c_int32(-1)
    assert L.aoclsparse_csr2dia_ndiag(mb, nb, d.h, len(bv), P._ptr(brp), P._ptr(bci), ctypes.byref(nd)) == 0
    ond, ooff, odv = oracle.csr2dia(mb, nb, base, brp, bci, bv)
    assert nd.value == ond == 9
    off, dv = np.zeros(ond, np.int32), np.zeros(ond * mb, F32)  # (the caller zeroes: convert.hpp:291-387 writes the stored entries only)
    assert L.aoclsparse_scsr2dia(mb, nb, d.h, P._ptr(brp), P._ptr(bci), P._ptr(bv), ond, P._ptr(off), P._ptr(dv)) == 0
    assert np.array_equal(off, ooff)
    same_bits(dv, odv.astype(F32), "dia")


# --------------------------------------------------------------------------------------------------
# f. itsol_s_*
# --------------------------------------------------------------------------------------------------
# Requested relative tolerance: 5e-6.  oracle.scg on this system (laplace5(40), b = A * uniform(-1, 1) rounded to float)
# stagnates at a true relative residual of 4.9e-7 without preconditioner and 1.14e-6 with SymGS (400 iterations at rtol
# 1e-30, forward and pairwise dots alike), so 5e-6 is 4 to 10 times what float reaches here.
ITSOL_RTOL = 5e-6


def _itsol_s(opts):
    h = ctypes.c_void_p()
    assert L.aoclsparse_itsol_s_init(ctypes.byref(h)) == 0
    for k, v in opts.items():
        assert L.aoclsparse_itsol_option_set(h, k.encode(), str(v).encode()) == 0, (k, v)
    return h


@pytest.fixture(scope="module")
def krylov40():
    n, rp, ci, v = laplace5(40)
    rng = np.random.default_rng(71)
    xe = rng.uniform(-1, 1, n)
    D = np.zeros((n, n))
    for i in range(n):
        D[i, ci[rp[i]:rp[i + 1]]] = v[rp[i]:rp[i + 1]]
    b = (D @ xe).astype(F32)
    o = oracle.dcsr_optimize(n, n, len(v), 0, rp, ci, v)
    keep = np.flatnonzero(ci <= np.repeat(np.arange(n), np.diff(rp)))  # the lower triangle, for the symmetric descriptor of CG
    lrp = np.concatenate([[0], np.cumsum(np.bincount(np.repeat(np.arange(n), np.diff(rp))[keep], minlength=n))]).astype(np.int32)
    return dict(n=n, rp=rp, ci=ci, v=v.astype(F32), D=D, b=b, o=o, lrp=lrp, lci=ci[keep].copy(), lv=v[keep].astype(F32))


def _margin(runs):
    """the iteration rule: at most the larger count of the two float oracle runs (forward / pairwise dots) + their spread + 2"""
    counts = [int(r[2][30]) for r in runs]
    assert all(r[0] == 0 for r in runs)
    return max(counts) + (max(counts) - min(counts)) + 2, counts


def _check_solution(K, x, rinfo, limit, what):
    nb = np.linalg.norm(K["b"].astype(np.float64))
    true = np.linalg.norm(K["b"].astype(np.float64) - K["D"] @ x.astype(np.float64))
    print("itsol_s", what, "iterations", rinfo[30], "limit", limit, "true relative residual", true / nb)
    assert true <= ITSOL_RTOL * nb, (what, true / nb)
    assert 1 <= rinfo[30] <= limit, (what, rinfo[30], limit)
    assert 0 <= rinfo[0] <= 1.001 * ITSOL_RTOL * nb and np.all(np.isfinite(rinfo)), (what, rinfo[0])


@pytest.mark.parametrize("pre,code", [("None", 0), ("SymGS", 3)])
def test_itsol_s_cg(krylov40, pre, code):
    """CG in float, no preconditioner and SymGS (the library, like the reference, has no ILU(0) for CG: the option is refused),
    direct interface with host and with device vectors.  Return code 0, the TRUE residual (float64) meets the requested relative
    tolerance, rinfo is populated, and the iteration count is at most that of the float oracle plus the margin: oracle.scg
    with forward and with pairwise dots took 64 / 64 iterations (none) and 23 / 23 (SymGS) -- a spread of 0 -- so at most
    66 and 25."""
    K = krylov40
    n = K["n"]
    A = P.Matrix(0, n, n, K["lrp"], K["lci"], K["lv"])
    d = P.Descr(mtype=P.TYPE_SYMMETRIC, fill=P.FILL_LOWER)
    runs = [oracle.scg(n, 0, K["rp"], K["ci"], K["v"], K["o"]["idiag"], K["o"]["iurow"], K["b"], np.zeros(n), ITSOL_RTOL, 0.0, 500, code, dots=s)
            for s in ("forward", "pairwise")]
    limit, counts = _margin(runs)
    print("oracle.scg", pre, counts)
    h = _itsol_s({"CG Rel Tolerance": ITSOL_RTOL, "CG Abs Tolerance": 0.0, "CG Preconditioner": pre, "CG Iteration Limit": 500})
    x, rinfo = np.zeros(n, F32), np.zeros(100, F32)
    assert L.aoclsparse_itsol_s_solve(h, n, A.h, d.h, P._ptr(K["b"]), P._ptr(x), P._ptr(rinfo), None, None, None) == 0
    _check_solution(K, x, rinfo, limit, ("cg", pre, "host"))
    assert abs(rinfo[1] - np.linalg.norm(K["b"])) <= 1e-5 * np.linalg.norm(K["b"])
    xd, rinfo_d = dev(np.zeros(n, F32)), np.zeros(100, F32)
    assert L.aoclsparse_itsol_s_solve(h, n, A.h, d.h, P._ptr(dev(K["b"])), P._ptr(xd), P._ptr(rinfo_d), None, None, None) == 0
    torch.cuda.synchronize()
    _check_solution(K, xd.cpu().numpy(), rinfo_d, limit, ("cg", pre, "device"))
    # a float handle refuses the double entry point, and CG has no ILU(0)
    xx, rr = np.zeros(n), np.zeros(100)
    assert L.aoclsparse_itsol_d_solve(h, n, A.h, d.h, P._ptr(xx), P._ptr(xx), P._ptr(rr), None, None, None) == 9
    assert L.aoclsparse_itsol_option_set(h, b"CG Preconditioner", b"ILU0") != 0
    L.aoclsparse_itsol_destroy(ctypes.byref(h))


@pytest.mark.parametrize("pre,code", [("None", 0), ("ILU0", 2)])
def test_itsol_s_gmres(krylov40, pre, code):
    """GMRES(20) in float, plain and with ILU(0), direct interface.  oracle.sgmres with forward and with pairwise dots: 180 / 180
    iterations (plain; whole restart cycles are counted) and 40 / 40 (ILU0), a spread of 0: at most 182 and 42."""
    K = krylov40
    n = K["n"]
    A, d = P.Matrix(0, n, n, K["rp"], K["ci"], K["v"]), P.Descr()
    runs = [oracle.sgmres(n, 0, K["rp"], K["ci"], K["v"], K["b"], np.ones(n), 20, ITSOL_RTOL, 1e-30, 1000, code, dots=s) for s in ("forward", "pairwise")]
    limit, counts = _margin(runs)
    print("oracle.sgmres", pre, counts)
    h = _itsol_s({"iterative method": "GMRES", "gmres preconditioner": pre, "gmres restart iterations": 20,
                  "gmres rel tolerance": ITSOL_RTOL, "gmres abs tolerance": 1e-30, "gmres iteration limit": 1000})
    x, rinfo = np.ones(n, F32), np.zeros(100, F32)
    assert L.aoclsparse_itsol_s_solve(h, n, A.h, d.h, P._ptr(K["b"]), P._ptr(x), P._ptr(rinfo), None, None, None) == 0
    _check_solution(K, x, rinfo, limit, ("gmres", pre))
    xx, rr = np.zeros(n), np.zeros(100)
    assert L.aoclsparse_itsol_d_solve(h, n, A.h, d.h, P._ptr(xx), P._ptr(xx), P._ptr(rr), None, None, None) == 9
    L.aoclsparse_itsol_destroy(ctypes.byref(h))


@pytest.mark.parametrize("method,device", [("CG", True), ("CG", False), ("GMRES", False)])
def test_itsol_s_rci_driven_with_smv(krylov40, method, device):
    """Reverse communication in float: the caller computes v = A u with aoclsparse_smv on the workspaces the solver hands out
    (device b: HBM workspaces; host b: pinned host workspaces).  The same checks and the same iteration limits as the direct
    interface (no preconditioner: 66 for CG, 182 for GMRES(20))."""
    K = krylov40
    n = K["n"]
    if method == "CG":
        A, d = P.Matrix(0, n, n, K["lrp"], K["lci"], K["lv"]), P.Descr(mtype=P.TYPE_SYMMETRIC, fill=P.FILL_LOWER)
        runs = [oracle.scg(n, 0, K["rp"], K["ci"], K["v"], K["o"]["idiag"], K["o"]["iurow"], K["b"], np.zeros(n), ITSOL_RTOL, 0.0, 500, 0, dots=s)
                for s in ("forward", "pairwise")]
        h = _itsol_s({"CG Rel Tolerance": ITSOL_RTOL, "CG Abs Tolerance": 0.0, "CG Iteration Limit": 500})
        x0 = np.zeros(n, F32)
    else:
        A, d = P.Matrix(0, n, n, K["rp"], K["ci"], K["v"]), P.Descr()
        runs = [oracle.sgmres(n, 0, K["rp"], K["ci"], K["v"], K["b"], np.ones(n), 20, ITSOL_RTOL, 1e-30, 1000, 0, dots=s) for s in ("forward", "pairwise")]
        h = _itsol_s({"iterative method": "GMRES", "gmres restart iterations": 20, "gmres rel tolerance": ITSOL_RTOL,
                      "gmres abs tolerance": 1e-30, "gmres iteration limit": 1000})
        x0 = np.ones(n, F32)
    limit, counts = _margin(runs)
    rinfo, ircomm = np.zeros(100, F32), ctypes.c_int(1)
    u, w = ctypes.c_void_p(), ctypes.c_void_p()
    bb = dev(K["b"]) if device else K["b"]
    x = dev(x0) if device else x0.copy()
    assert L.aoclsparse_itsol_s_rci_input(h, n, P._ptr(bb)) == 0
    steps = 0
    while ircomm.value != 0 and steps < 3000:
        assert L.aoclsparse_itsol_s_rci_solve(h, ctypes.byref(ircomm), ctypes.byref(u), ctypes.byref(w), P._ptr(x), P._ptr(rinfo)) == 0
        steps += 1
        if ircomm.value == 2:  # aoclsparse_rci_mv
            assert P.smv(P.OP_NONE, 1.0, A, d, u.value, 0.0, w.value) == 0
            if device:
                assert L.aoclsparse_mi355_synchronize() == 0
    assert ircomm.value == 0, steps
    if device:
        torch.cuda.synchronize()
    _check_solution(K, x.cpu().numpy() if device else x, rinfo, limit, ("rci", method, device))
    L.aoclsparse_itsol_destroy(ctypes.byref(h))


# --------------------------------------------------------------------------------------------------
# g. smv on symmetric and triangular descriptors at size
# --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def derived3000():
    m = 3000
    rng = np.random.default_rng(303)
    rows = [rng.permutation(np.unique(np.concatenate([rng.integers(0, m, rng.integers(0, 24)), [i]]))) for i in range(m)]  # unsorted, full diagonal
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    v = rng.uniform(-1, 1, len(ci)).astype(F32)
    D = np.zeros((m, m))
    D[np.repeat(np.arange(m), np.diff(rp)), ci] = v
    x, y0 = rng.uniform(-1, 1, m).astype(F32), rng.uniform(-1, 1, m).astype(F32)
    ops = {}
    for fill in (P.FILL_LOWER, P.FILL_UPPER):
        tri = np.tril(D, -1) if fill == P.FILL_LOWER else np.triu(D, 1)
        for diag in (P.DIAG_NON_UNIT, P.DIAG_UNIT, P.DIAG_ZERO):
            dg = np.diag(np.diag(D)) if diag == P.DIAG_NON_UNIT else (np.eye(m) if diag == P.DIAG_UNIT else 0.0)
            for mtype in (P.TYPE_SYMMETRIC, P.TYPE_TRIANGULAR):
                for op in (P.OP_NONE, P.OP_TRANSPOSE):
                    M = tri + tri.T + dg if mtype == P.TYPE_SYMMETRIC else (tri + dg if op == P.OP_NONE else (tri + dg).T)
                    lens = (M != 0).sum(axis=1)
                    ops[fill, diag, mtype, op] = (M @ x.astype(np.float64), np.abs(M) @ np.abs(x.astype(np.float64)), lens)
    return m, rp, ci, v, x, y0, ops


@pytest.mark.parametrize("hinted", [False, True])
@pytest.mark.parametrize("base", [0, 1])
def test_smv_symmetric_and_triangular_at_size(derived3000, base, hinted):
    """3000 x 3000, unsorted rows of up to 24 entries with a full diagonal; symmetric and triangular descriptors x fill x
    diag in {non_unit, unit, zero} x op in {N, T}, both bases, with and without an mv hint + optimize.  Against a float64 dense
    construction of the operator (which triangle, which diagonal), within the bound of test_symmetric_and_triangular_dmv in
    fp32: |dy| <= (len + 6) eps32 (|alpha| sum |a x| + |beta y|), len = entries of the row of the expanded operator."""
    m, rp, ci, v, x, y0, ops = derived3000
    alpha, beta = 1.7, -0.4
    a32, b32 = float(F32(alpha)), float(F32(beta))
    worst = 0.0
    for (fill, diag, mtype, op), (Mx, Mabs, lens) in ops.items():
        A = P.Matrix(base, m, m, rp + base, ci + base, v)
        d = P.Descr(base=base, mtype=mtype, fill=fill, diag=diag)
        if hinted:
            assert L.aoclsparse_set_mv_hint(A.h, op, d.h, 100) == 0 and L.aoclsparse_optimize(A.h) == 0
        yd = dev(y0)
        assert P.smv(op, alpha, A, d, dev(x), beta, yd) == 0, (fill, diag, mtype, op)
        torch.cuda.synchronize()
        y = yd.cpu().numpy().astype(np.float64)
        bound = (lens + 6) * EPS32 * (abs(a32) * Mabs + np.abs(b32 * y0.astype(np.float64))) + 1e-30
        ratio = float(np.max(np.abs(y - (a32 * Mx + b32 * y0.astype(np.float64))) / bound))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (fill, diag, mtype, op, ratio)
    print("smv derived operators, base", base, "hinted", hinted, "worst error / bound", worst)


# --------------------------------------------------------------------------------------------------
# h. ssorv lives in test_gpu_parity.py::test_sorv_kats_and_bit_exact_sweeps (bit equality with oracle.ssorv, host and device)
# --------------------------------------------------------------------------------------------------
