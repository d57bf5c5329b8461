"""The vector steps of aoclsparse_itsol_{d,s,z,c}_* one by one, through the reverse-communication interface with device
vectors: at every return of rci_solve the vectors that stop exposes are read back and compared with a high-precision
restatement of that one step, started from the library's own previous state (itsol_steps.py holds the restatement, the bound
formulas and their derivation; test_itsol_steps_cpu.py shows that those bounds see a dropped block, trip or element at these
sizes).  The sizes are the smallest at which each path of the reduction kernels is live: one block and its tails (1, 255, 256,
257), more than 256 partials (65 829), the grid-stride trip and the cap of the real kernels (131 877) and of the complex ones
(262 949).  The operator is the test's own: q = A u by torch on the device, in the solver's precision.

Device vectors the test itself holds at once: b, x, the diagonal and two scratch vectors, 21 MB at the largest complex128 size.
"""
import ctypes
from ctypes import c_void_p

import numpy as np
import pytest

import itsol_steps as K
import oracle
from util import pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
P = pkg()
L = P.lib()

NMAX = 262949
TOL = {"d": "1e-14", "z": "1e-14", "s": "1e-7", "c": "1e-7"}  # never met within the few iterations a case runs


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    st, d, cus, name = P.device_info()
    assert st == 0 and cus > 0


_hip = None


def hip_copy(dst, src, nbytes, kind):
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL(P.hip_runtime_path()[1])
        _hip.hipMemcpy.argtypes = [c_void_p, c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert L.aoclsparse_mi355_synchronize() == 0
    assert _hip.hipMemcpy(dst, src, nbytes, kind) == 0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class LibSolver:
    """the library behind the interface itsol_steps.drive_* walks; handles are raw addresses"""

    def __init__(self, prec, n, kind, precond, host_b=False, b=None, x0=None, restart=4, tol=None):
        self.t, self.n, self.prec, self.host_b = K.Ty(prec), n, prec, host_b
        self.diag, self.lo, self.up, self.b, self.x0 = K.system(prec, n, kind)
        if b is not None:
            self.b = b
        if x0 is not None:
            self.x0 = x0
        self.lo_s, self.up_s = (complex(self.lo), complex(self.up)) if self.t.cplx else (float(self.lo), float(self.up))
        self.diag_d = dev(self.diag)
        self.nbytes = n * np.dtype(self.t.dtype).itemsize
        self.h = c_void_p()
        assert self.fn("itsol_?_init")(ctypes.byref(self.h)) == 0
        m = "cg" if kind == "cg" else "gmres"
        opts = [("iterative method", m), (m + " rel tolerance", tol or TOL[prec]), (m + " abs tolerance", "0"),
                (m + " preconditioner", "user" if precond else "none")]
        if kind != "cg":
            opts.append(("gmres restart iterations", str(restart)))
        for k, v in opts:
            assert L.aoclsparse_itsol_option_set(self.h, k.encode(), v.encode()) == 0, (k, v)
        if host_b:
            self.xh = self.x0.copy()
            self.status_input = self.fn("itsol_?_rci_input")(self.h, n, P._ptr(self.b))
            self.xarg = P._ptr(self.xh)
        else:
            self.b_d, self.x_d = dev(self.b), dev(self.x0)
            self.status_input = self.fn("itsol_?_rci_input")(self.h, n, P._ptr(self.b_d))
            self.xarg = P._ptr(self.x_d)
        assert self.status_input == 0
        self.ri = np.zeros(100, self.t.rdtype)
        self.job, self.u, self.v = ctypes.c_int(1), c_void_p(), c_void_p()

    def fn(self, stem):
        return getattr(L, "aoclsparse_" + stem.replace("?", self.prec))

    def close(self):
        L.aoclsparse_itsol_destroy(ctypes.byref(self.h))

    def call(self):
        st = self.fn("itsol_?_rci_solve")(self.h, ctypes.byref(self.job), ctypes.byref(self.u), ctypes.byref(self.v), self.xarg,
                                          P._ptr(self.ri))
        return st, self.job.value, self.u.value, self.v.value

    def read(self, addr):
        out = np.empty(self.n, self.t.dtype)
        if self.host_b:
            ctypes.memmove(out.ctypes.data, addr, self.nbytes)
        else:
            hip_copy(P._ptr(out), c_void_p(addr), self.nbytes, 2)  # device to host
        return out

    def write(self, addr, a):
        a = np.ascontiguousarray(a, self.t.dtype)
        if self.host_b:
            ctypes.memmove(addr, a.ctypes.data, self.nbytes)
        else:
            hip_copy(c_void_p(addr), P._ptr(a), self.nbytes, 1)  # host to device
        return a

    def read_x(self):
        if self.host_b:
            return self.xh.copy()
        assert L.aoclsparse_mi355_synchronize() == 0
        torch.cuda.synchronize()
        return self.x_d.cpu().numpy()

    def rinfo(self):
        return self.ri.copy()

    def _answer(self, u, v, f):
        ut = dev(self.read(u))  # (a host round trip: the arithmetic under test is the library's, not the operator's)
        out = f(ut)
        torch.cuda.synchronize()
        return self.write(v, out.cpu().numpy())

    def apply(self, u, v):
        return self._answer(u, v, lambda ut: K.tri_apply(self.diag_d, self.lo_s, self.up_s, ut))

    def jacobi(self, u, v):
        return self._answer(u, v, lambda ut: ut / self.diag_d)

    def copy(self, u, v):
        self.write(v, self.read(u))

    def base(self, v):
        return v

    def at(self, base, k):
        return base + k * self.nbytes


def show(*a):
    print("itsol_steps", *a)


@pytest.mark.parametrize("precond", [False, True], ids=["none", "user"])
@pytest.mark.parametrize("n", K.SIZES)
@pytest.mark.parametrize("prec", K.PRECS)
def test_cg_steps(prec, n, precond):
    """Six iterations (one at n = 1, where the first step is exact), no preconditioner and a user request served as z = r / diag.
    At every stop: p, q at an mv request, r and the caller's x at the stopping-criterion request, r at a preconditioner request,
    rinfo[RES_NORM], rinfo[RHS_NORM], rinfo[ITER]; r0 = q - b and p1 = -z bit for bit."""
    S = LibSolver(prec, n, "cg", precond)
    ck = K.CgCheck(prec, n, S.b, S.x0, precond)
    try:
        K.drive_cg(S, ck, min(6, n))
    finally:
        S.close()
    show("cg", prec, n, "user" if precond else "none", ck.report())
    assert ck.ok(), ck.report()
    assert {"rinfo[RES_NORM]", "rinfo[RHS_NORM]", "x += alpha p", "r += alpha q"} <= set(ck.ratios)
    assert n == 1 or "p = beta p - z" in ck.ratios


@pytest.mark.parametrize("precond", [False, True], ids=["none", "identity"])
@pytest.mark.parametrize("n", K.SIZES)
@pytest.mark.parametrize("prec", K.PRECS)
def test_gmres_steps(prec, n, precond):
    """GMRES(4), two cycles, no preconditioner and an identity user preconditioner.  The first mv request exposes the base of V
    (ld = n); v0 and then every V[j+1] is checked from the library's own V[0..j] and the w the test wrote, under a bound that has
    to stay below 1e-3 max|v|.  After each cycle the true residual of x (long double) is at most that of the long double
    minimiser over the same basis times a margin, 1 + 4 e + f.  e is measured (itsol_steps.oracle_excess): oracle.dgmres /
    oracle.sgmres run the two cycles on the real system of the same n, and |ratio - 1| of each cycle against the minimiser is
    taken; the complex types use the figures of the real type of their precision.  Measured e, first / second cycle:
      double  n = 255: 1.5e-14 / 2.9e-13   256: 6.3e-15 / 1.5e-12   257: 8.9e-16 / 1.1e-12
              65 829: 1.1e-16 / 1.6e-13   131 877: 2.2e-16 / 2.4e-14   262 949: 0 / 3.3e-14
      float   n = 255: 2.2e-6 / 6.7e-4   256: 4.0e-6 / 1.8e-3   257: 5.8e-6 / 1.2e-3
              65 829: 1.6e-6 / 1.8e-4   131 877: 2.3e-5 / 1.6e-4   262 949: 5.4e-4 / 1.1e-3
    These are signed rounding noise of first order (the oracle's own ratio is below 1 in half of the runs), and a working
    precision GMRES lands anywhere within a few times their spread; f is what no x stored in the working type can resolve, the
    effect on the ratio of rounding the minimiser itself, eps / 2 | |A| |x| | / rho, plus the error of the evaluation
    (itsol_steps.min_residual_ratio)."""
    S = LibSolver(prec, n, "gmres", precond)
    ck = K.GmresCheck(prec, n, S.b)
    ratios = []
    try:
        K.drive_gmres(S, ck, 4, 2, lambda x0, x1, basis: ratios.append(K.min_residual_ratio(S.diag, S.lo, S.up, S.b, x0, x1, basis)))
    finally:
        S.close()
    show("gmres", prec, n, "identity" if precond else "none", ck.report(), "residual over minimiser - 1:", ["%.3e" % (r - 1) for r, f in ratios])
    assert ck.ok(), ck.report()
    if n > 4:
        margins = K.cycle_margins(prec, n, [f for r, f in ratios])
        show("gmres margins - 1:", ["%.3e" % (m - 1) for m in margins])
        assert "v[j+1]" in ck.ratios and len(ratios) == 2
        assert all(r <= m for (r, f), m in zip(ratios, margins)), ([r - 1 for r, f in ratios], [m - 1 for m in margins])


@pytest.mark.parametrize("prec", K.PRECS)
def test_gmres_breakdown_still_corrects_x(prec):
    """An exact preconditioner (z = A^-1 u, by a dense solve on the host) makes the first Arnoldi vector vanish: the solver stops
    after one iteration with success.  The reference leaves x at the initial guess there (itsol_functions.hpp:1121-1135); this
    library applies the correction of the column it has, and x solves the system to the requested tolerance."""
    n, rtol = 257, {"d": 1e-10, "z": 1e-10, "s": 1e-5, "c": 1e-5}[prec]
    S = LibSolver(prec, n, "gmres", True, tol=str(rtol))
    wide = np.complex128 if S.t.cplx else np.float64
    A = (np.diag(S.diag) + np.diag(np.full(n - 1, S.lo), -1) + np.diag(np.full(n - 1, S.up), 1)).astype(wide)
    try:
        st, job, u, v = S.call()
        assert st == 0 and job == K.MV
        S.apply(u, v)
        st, job, u, v = S.call()
        assert st == 0 and job == K.PRECOND
        S.write(v, np.linalg.solve(A, S.read(u).astype(wide)))
        st, job, u, v = S.call()
        assert st == 0 and job == K.MV
        S.apply(u, v)
        st, job, u, v = S.call()
        x, ri = S.read_x(), S.rinfo()
    finally:
        S.close()
    assert st == 0 and job == K.STOP and ri[30] == 1, (st, job, ri[30])
    true, nb = np.linalg.norm(S.b.astype(wide) - A @ x.astype(wide)), np.linalg.norm(S.b.astype(wide))
    show("gmres breakdown", prec, "true relative residual %.3e" % (true / nb), "start %.3e" % (np.linalg.norm(S.b - A @ S.x0) / nb))
    assert true <= rtol * nb, true / nb


def test_route_table():
    """which paths of the reduction kernels each (type, size) of this file takes"""
    for prec in K.PRECS:
        live = set()
        for n in K.SIZES:
            r = K.Ty(prec).route(n)
            show("route", prec, n, "blocks", K.Ty(prec).blocks(n), " ".join(k for k, v in r.items() if v) or "one block")
            live |= {k for k, v in r.items() if v}
        assert live == {"tail", "final2", "stride", "cap"}, (prec, live)


def sentinel_indices(prec):
    cap = K.Ty(prec).cap
    return (0, 255, 256 * 256, 256 * cap, 256 * cap + 255, NMAX - 1)


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("prec", K.PRECS)
def test_cg_sentinels(prec, which):
    """A NaN at one critical index reaches the host through every reduction: in b the first call answers invalid_value, in q
    the call that consumes it answers numerical_error.  Exact, no tolerance: a kernel that skips the index returns success."""
    t, idx = K.Ty(prec), sentinel_indices(prec)[which]
    ones = np.ones(NMAX, t.dtype)
    b = ones.copy()
    b[idx] = np.nan
    S = LibSolver(prec, NMAX, "cg", False, b=b, x0=np.zeros(NMAX, t.dtype))
    try:
        assert S.call()[0] == K.ST_INVALID_VALUE, idx
    finally:
        S.close()
    S = LibSolver(prec, NMAX, "cg", False, b=ones, x0=np.zeros(NMAX, t.dtype))
    try:
        st, job, u, v = S.call()
        assert st == 0 and job == K.MV
        q = np.zeros(NMAX, t.dtype)
        q[idx] = np.nan
        S.write(v, q)
        assert S.call()[0] == K.ST_NUMERICAL, idx
    finally:
        S.close()


@pytest.mark.parametrize("prec,n", [("d", 131877), ("s", 131877), ("z", 262949), ("c", 262949)])
def test_cg_refused_step_changes_no_bit(prec, n):
    """A step the solver refuses leaves x and r as they were.  Real types: q = -p makes p.q negative.  Complex types: p.q is the
    unconjugated sum, -sum p_i^2 is a complex number of full modulus and, as in the reference (utils.hpp:626-638, |p.q| <= 0.02
    eps), not refused; the refusal complex arithmetic has is p.q = 0, so q = 0 there."""
    S = LibSolver(prec, n, "cg", False)
    try:
        st, job, u, v = S.call()
        assert st == 0 and job == K.MV
        S.apply(u, v)
        st, job, r_addr, _ = S.call()
        assert st == 0 and job == K.CRIT
        r0, x0 = S.read(r_addr), S.read_x()
        st, job, u, v = S.call()
        assert st == 0 and job == K.MV
        p = S.read(u)
        assert np.array_equal(p, -r0)
        S.write(v, np.zeros_like(p) if K.Ty(prec).cplx else -p)
        assert S.call()[0] == K.ST_NUMERICAL
        r1, x1 = S.read(r_addr), S.read_x()
    finally:
        S.close()
    rd = K.Ty(prec).rdtype
    assert np.array_equal(r1.view(rd), r0.view(rd)) and np.array_equal(x1.view(rd), x0.view(rd))
    assert np.array_equal(x0, S.x0)


def test_cg_host_b_gives_the_device_bits():
    """b in host memory: pinned workspaces, the same kernels; every vector and every rinfo entry at every stop has the bits of the
    run with b in HBM."""
    n, traces = 65829, []
    for host in (False, True):
        S = LibSolver("d", n, "cg", False, host_b=host)
        tr = []
        try:
            for _ in range(14):
                st, job, u, v = S.call()
                assert st == 0
                tr.append((job, S.read(u), S.read_x(), S.rinfo()))
                if job == K.MV:
                    tr.append((job, S.apply(u, v)))
        finally:
            S.close()
        traces.append(tr)
    assert len(traces[0]) == len(traces[1]) > 14
    for a, c in zip(*traces):
        assert a[0] == c[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], c[1:])), a[0]


# ---- the direct interface at a size where the grid-stride trip and the block cap are live ------------------------------
DIRECT_N = 131877
DIRECT_RTOL = {"d": 1e-9, "s": 5e-6}  # (float stagnates near 1e-7 on a system this well conditioned)


@pytest.fixture(scope="module")
def direct():
    out = {}
    for kind in ("cg", "gmres"):
        diag, lo, up, b, _ = K.system("d", DIRECT_N, kind)
        rp, ci, v = K.tri_csr(diag, lo, up)
        out[kind] = dict(diag=diag, lo=lo, up=up, b=b, rp=rp, ci=ci, v=v, o=oracle.dcsr_optimize(DIRECT_N, DIRECT_N, len(v), 0, rp, ci, v),
                         low=K.tri_csr(diag, lo, up, lower_only=True))
    return out


def _true_residual(c, dt, b, x):
    """|b - A x| in extended precision, A with the values the handle holds (rounded to dt)"""
    ext = np.longdouble
    r = b.astype(ext) - K.tri_apply(c["diag"].astype(dt).astype(ext), ext(dt(c["lo"])), ext(dt(c["up"])), x.astype(ext))
    return float(np.sqrt((r * r).sum()))


def _solve(prec, opts, A, d, b, x0):
    dt = np.float64 if prec == "d" else np.float32
    h = c_void_p()
    assert getattr(L, "aoclsparse_itsol_%s_init" % prec)(ctypes.byref(h)) == 0
    for k, v in opts.items():
        assert L.aoclsparse_itsol_option_set(h, k.encode(), str(v).encode()) == 0, (k, v)
    xd, bd, rinfo = dev(x0.astype(dt)), dev(b.astype(dt)), np.zeros(100, dt)
    st = getattr(L, "aoclsparse_itsol_%s_solve" % prec)(h, len(b), A.h, d.h, P._ptr(bd), P._ptr(xd), P._ptr(rinfo), None, None, None)
    torch.cuda.synchronize()
    L.aoclsparse_itsol_destroy(ctypes.byref(h))
    return st, xd.cpu().numpy(), rinfo


@pytest.mark.parametrize("pre,code", [("None", 0), ("SymGS", 3)])
@pytest.mark.parametrize("prec", ["d", "s"])
def test_direct_cg_at_size(direct, prec, pre, code):
    """aoclsparse_itsol_?_solve, CG, device vectors, lower-stored symmetric CSR handle: the iteration count of oracle.dcg / scg
    within 1, the true residual within the requested tolerance."""
    c, n, dt, rtol = direct["cg"], DIRECT_N, (np.float64 if prec == "d" else np.float32), DIRECT_RTOL[prec]
    o = c["o"]
    b = c["b"].astype(dt)
    if prec == "d":
        so, xo, ro = oracle.dcg(n, 0, o["ptr"], o["ind"], o["val"], o["idiag"], o["iurow"], b, np.zeros(n), rtol, 0.0, 500, code)
    else:
        so, xo, ro = oracle.scg(n, 0, c["rp"], c["ci"], c["v"], o["idiag"], o["iurow"], b, np.zeros(n), rtol, 0.0, 500, code)
    assert so == 0 and ro[30] < 30
    lrp, lci, lv = c["low"]
    A, d = P.Matrix(0, n, n, lrp, lci, lv.astype(dt)), P.Descr(mtype=P.TYPE_SYMMETRIC, fill=P.FILL_LOWER)
    st, x, rinfo = _solve(prec, {"CG Rel Tolerance": rtol, "CG Abs Tolerance": 0.0, "CG Preconditioner": pre, "CG Iteration Limit": 500},
                          A, d, b, np.zeros(n))
    nb = float(np.linalg.norm(b.astype(np.float64)))
    true = _true_residual(c, dt, b, x)
    show("direct cg", prec, pre, "iterations", rinfo[30], "oracle", ro[30], "true relative residual %.3e" % (true / nb))
    assert st == 0
    assert abs(rinfo[30] - ro[30]) <= 1, (rinfo[30], ro[30])
    assert true <= rtol * nb, true / nb


@pytest.mark.parametrize("pre,code", [("None", 0), ("ILU0", 2)])
@pytest.mark.parametrize("prec", ["d", "s"])
def test_direct_gmres_at_size(direct, prec, pre, code):
    """aoclsparse_itsol_?_solve, GMRES(20), device vectors: the iteration count of oracle.dgmres / sgmres within one restart
    cycle, the true residual within the requested tolerance."""
    c, n, dt, rtol = direct["gmres"], DIRECT_N, (np.float64 if prec == "d" else np.float32), DIRECT_RTOL[prec]
    b = c["b"].astype(dt)
    run = oracle.dgmres if prec == "d" else oracle.sgmres
    so, xo, ro = run(n, 0, c["rp"], c["ci"], c["v"], b, np.ones(n), 20, rtol, 1e-30, 400, code)
    assert so == 0
    A, d = P.Matrix(0, n, n, c["rp"], c["ci"], c["v"].astype(dt)), P.Descr()
    st, x, rinfo = _solve(prec, {"iterative method": "GMRES", "gmres preconditioner": pre, "gmres restart iterations": 20,
                                 "gmres rel tolerance": rtol, "gmres abs tolerance": 1e-30, "gmres iteration limit": 400},
                          A, d, b, np.ones(n))
    nb = float(np.linalg.norm(b.astype(np.float64)))
    true = _true_residual(c, dt, b, x)
    show("direct gmres", prec, pre, "iterations", rinfo[30], "oracle", ro[30], "true relative residual %.3e" % (true / nb))
    assert st == 0
    assert abs(rinfo[30] - ro[30]) <= 20, (rinfo[30], ro[30])
    assert true <= rtol * nb, true / nb
