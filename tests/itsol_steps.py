"""The vector steps of the iterative solvers, one by one: a high-precision restatement of each step of CG and of one Arnoldi
step of GMRES, the derived bounds it is compared under, a working-precision model of the library's reverse-communication
interface (with the kernels' two-stage reduction tree) and the defects that model can be given.  Plain numpy; only the
measured margin of the GMRES least-squares check runs the CPU oracle.

A run is a sequence of stops.  `drive_cg` / `drive_gmres` walk a solver that looks like the reverse-communication interface
(`call`, `read`, `write`, `apply`, ...) and feed a checker with what each stop exposes; the GPU test hands them the library,
the CPU test hands them `ModelSolver`, clean or with one defect.

Bounds (eps is the epsilon of the working real type, 2^-52 or 2^-23, i.e. two unit roundoffs):
 * a reduced scalar differs from the exact sum of its terms by at most D * eps * sum|terms|.  d, z: D = n, which holds for
   every summation order.  s, c: n * eps is looser than the effect of a dropped block of 256, so D is the longest chain of
   additions in the kernels' tree: ceil(n / (256 B)) grid-stride trips, 6 shuffle + 2 LDS additions, ceil(B / 256) trips of
   the final kernel and its 6 + 2 again, D = ceil(n / (256 B)) + ceil(B / 256) + 16 with B = min(cap, ceil(n / 256)) blocks.
   cap is RED_BLOCKS = 512 (itsol_kernels.hip:17, applied in red_blocks(), :149-153) for the real types and CDOT_BLOCKS = 1024
   (complex_kernels.hip:239, applied in launch_cdot(), :455) for the complex ones.  Each addition rounds by eps / 2, the
   products by as much once: D * eps is twice the worst case.
 * rel(s) of a scalar formed from reduced scalars is the sum of their relative bounds, D * eps * sum|terms| / |sum terms|
   (the condition ratio is computed here, from the vectors read back), plus eps for each division or square root.
 * a vector s * a + b: |error_i| <= (rel(s) + 2 eps) * (|s| |a_i| + |b_i|); a real fused multiply-add rounds once (eps / 2), a
   complex product and sum by at most (sqrt(5) + 1) / 2 * eps.
 * the Arnoldi vector: the absolute bound of w - sum h_i v_i is sum dh_i |v_i| + 2 eps k (sum |h_i| |v_i| + |w|) for its k
   terms (the bound above applied k times, every intermediate below the sum of moduli); v = w / hh then carries that bound
   over hh plus (rel(hh) + 2 eps) |v|, rel(hh) = D eps / 2 + eps + |bound|_2 / hh.
"""
import numpy as np

MV, PRECOND, CRIT, STOP = 2, 3, 4, 0  # aoclsparse_itsol_rci_job
ST_OK, ST_INVALID_VALUE, ST_NUMERICAL = 0, 5, 11
SIZES = (1, 255, 256, 257, 65829, 131877, 262949)
PRECS = ("d", "s", "z", "c")


class Ty:
    """working and reference types of one precision letter"""

    def __init__(self, prec):
        self.prec = prec
        self.cplx = prec in "zc"
        self.dtype = {"d": np.float64, "s": np.float32, "z": np.complex128, "c": np.complex64}[prec]
        self.rdtype = np.float64 if prec in "dz" else np.float32
        self.ext = {"d": np.longdouble, "s": np.float64, "z": np.clongdouble, "c": np.complex128}[prec]
        self.rext = np.longdouble if prec in "dz" else np.float64
        self.eps = float(np.finfo(self.rdtype).eps)
        self.cap = 1024 if self.cplx else 512

    def blocks(self, n):
        return min(self.cap, max(1, -(-n // 256)))

    def D(self, n):
        if self.prec in "dz":
            return max(n, 1)
        B = self.blocks(n)
        return -(-max(n, 1) // (256 * B)) + -(-B // 256) + 16

    def route(self, n):
        """which paths of the reduction kernels a vector of n elements takes"""
        nb = -(-n // 256)
        return {"tail": n % 256 != 0 and nb > 1, "final2": self.blocks(n) > 256, "stride": n > 256 * self.cap, "cap": nb >= self.cap}


# ---- systems ------------------------------------------------------------------------------------------------------------
def system(prec, n, kind):
    """Tridiagonal, diagonally dominant: diag in [4, 6), off-diagonals (-1, -1) for CG, (-1, -0.5) for GMRES; the complex twins
    multiply by fixed complex numbers (the CG one stays complex symmetric).  Returns diag, lo, up, b, x0 in the working type.
    Condition number below 4 (Gershgorin: [2, 8]), so CG to 1e-9 takes about 20 iterations."""
    t = Ty(prec)
    i = np.arange(n, dtype=np.float64)
    diag = 4.0 + 2.0 * ((i * 0.6180339887498949) % 1.0)
    lo, up = (-1.0, -1.0) if kind == "cg" else (-1.0, -0.5)
    b = np.sin(0.37 * i + 0.2) + 0.5 * np.cos(1.3 * i)
    x0 = 0.1 * np.cos(0.11 * i)
    if t.cplx:
        diag = diag * (1.0 + 0.2j)
        lo, up = lo * (1.0 - 0.3j), up * (1.0 - 0.3j)
        b = b + 1j * (0.7 * np.cos(0.53 * i) - 0.4 * np.sin(0.9 * i + 1.0))
        x0 = x0 + 0.05j * np.sin(0.07 * i)
    return diag.astype(t.dtype), t.dtype(lo), t.dtype(up), b.astype(t.dtype), x0.astype(t.dtype)


def tri_apply(diag, lo, up, u):
    """q = A u in the type of u (numpy arrays or torch tensors alike)"""
    q = diag * u
    q[1:] += lo * u[:-1]
    q[:-1] += up * u[1:]
    return q


def tri_csr(diag, lo, up, lower_only=False):
    n = len(diag)
    rows = np.repeat(np.arange(n), 3)
    cols = rows + np.tile([-1, 0, 1], n)
    vals = np.stack([np.full(n, lo, diag.dtype), diag, np.full(n, up, diag.dtype)], axis=1).ravel()
    ok = (cols >= 0) & (cols < n)
    if lower_only:
        ok &= cols <= rows
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, rows[ok] + 1, 1)
    return np.cumsum(rp).astype(np.int32), cols[ok].astype(np.int32), vals[ok]


# ---- reference pieces ---------------------------------------------------------------------------------------------------
def ratio(err, bound):
    err, bound = np.abs(err).astype(np.float64), np.asarray(bound, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    r = np.where(np.isnan(r), np.inf, r)
    return float(np.max(r)) if r.size else 0.0


def same_bits(a, b):
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))  # (-0 == 0: a sign of zero is no error)


class Ref:
    def __init__(self, prec, n):
        self.t, self.n = Ty(prec), n
        self.Deps = self.t.D(n) * self.t.eps

    def x(self, v):
        return np.asarray(v).astype(self.t.ext)

    def dot(self, a, b, conj=False):
        """exact sum, its absolute bound, its relative bound"""
        terms = (np.conj(a) if conj else a) * b
        s, mod = terms.sum(), np.abs(terms).sum()
        bound = self.Deps * float(mod)
        return s, bound, (bound / float(abs(s)) if abs(s) > 0 else np.inf)

    def norm_ratio(self, got, v):
        ref = float(np.sqrt((np.abs(v) ** 2).sum()))
        return ratio(float(got) - ref, (0.5 * self.Deps + self.t.eps) * ref)

    def axpy_ratio(self, got, s, rel_s, a, b):
        ref = s * a + b
        return ratio(self.x(got) - ref, (rel_s + 2 * self.t.eps) * (abs(s) * np.abs(a) + np.abs(b)))


class CgCheck:
    """Fed with the stops of a CG run; ratios[name] is the largest error / bound of that quantity, exact[name] whether a bit-for-bit
    comparison held at every stop."""

    def __init__(self, prec, n, b, x0, precond):
        self.R, self.t = Ref(prec, n), Ty(prec)
        self.b, self.x0, self.precond = np.array(b), np.array(x0), precond
        self.ratios, self.exact = {}, {}
        self.stage, self.k = "entry", 0
        self.r = self.p = self.q = self.z = self.x = None

    def _r(self, name, v):
        self.ratios[name] = max(self.ratios.get(name, 0.0), v)

    def _e(self, name, ok):
        self.exact[name] = self.exact.get(name, True) and bool(ok)

    def answer(self, v):
        if self.stage == "want_z":
            self.z = self.R.x(v)
        else:
            self.q_work, self.q = np.array(v), self.R.x(v)

    def on_mv(self, p, rinfo):
        if self.stage == "entry":
            self._e("p0 = x0", same_bits(p, self.x0))
            self.stage = "residual"
            return
        R, z = self.R, (self.z if self.precond else self.r)
        rz_new, _, rel_new = R.dot(self.r, z)
        self.k += 1
        self._e("rinfo[ITER]", rinfo[30] == self.k)
        if self.k == 1:  # rz = 1, or (1, 1) for complex, and p = 0: beta * 0 - z
            self._e("p1 = -z", same_bits(p, (-z).astype(self.t.dtype)))
        else:
            beta = rz_new / self.rz
            self._r("p = beta p - z", R.axpy_ratio(p, beta, rel_new + self.rel_rz + self.t.eps, self.p, -z))
        self.rz, self.rel_rz, self.p = rz_new, rel_new, R.x(p)
        self.stage = "want_q"

    def on_precond(self, r):
        self._e("r at the preconditioner request", same_bits(r, self.r_work))
        self.stage = "want_z"

    def on_crit(self, r, x, rinfo):
        R = self.R
        if self.stage == "residual":
            self._e("r0 = q - b", same_bits(r, self.q_work - self.b))
            self._e("x at r0", same_bits(x, self.x0))
            self._r("rinfo[RHS_NORM]", R.norm_ratio(rinfo[1], R.x(self.b)))
            self._e("rinfo[ITER]", rinfo[30] == 0)
            self.x = R.x(x)
        else:
            pq, _, rel_pq = R.dot(self.p, self.q)
            alpha, rel_a = self.rz / pq, self.rel_rz + rel_pq + self.t.eps
            self._r("x += alpha p", R.axpy_ratio(x, alpha, rel_a, self.p, self.x))
            self._r("r += alpha q", R.axpy_ratio(r, alpha, rel_a, self.q, self.r))
            self.x = R.x(x)
        self._r("rinfo[RES_NORM]", R.norm_ratio(rinfo[0], R.x(r)))
        self.r_work, self.r = np.array(r), R.x(r)
        self.stage = "iterate"

    def ok(self):
        return all(self.exact.values()) and all(v <= 1.0 for v in self.ratios.values())

    def report(self):
        return {**{k: round(v, 4) for k, v in self.ratios.items()}, **{k: v for k, v in self.exact.items() if not v}}


class GmresCheck:
    """one restart cycle after another: v0 = (b - A x) / |.|, then each Arnoldi vector from the library's own basis and the w the
    caller wrote"""

    def __init__(self, prec, n, b):
        self.R, self.t, self.b = Ref(prec, n), Ty(prec), Ref(prec, n).x(b)
        self.ratios, self.exact, self.bound_over_v = {}, {}, 0.0
        self.V = []

    def _r(self, name, v):
        self.ratios[name] = max(self.ratios.get(name, 0.0), v)

    def _unit(self, name, got, w, wbound):
        """got against w / |w|, w known to within wbound elementwise"""
        R, eps = self.R, self.t.eps
        hh = float(np.sqrt((np.abs(w) ** 2).sum()))
        rel_hh = 0.5 * R.Deps + eps + float(np.sqrt((wbound.astype(np.float64) ** 2).sum())) / hh
        ref = w / hh
        bound = wbound / hh + (rel_hh + 2 * eps) * np.abs(ref)
        self._r(name, ratio(R.x(got) - ref, bound))
        self.bound_over_v = max(self.bound_over_v, float(np.max(bound)) / float(np.max(np.abs(ref))))

    def on_v0(self, v0, q):
        w = self.b - self.R.x(q)
        self._unit("v0", v0, w, self.t.eps * np.abs(w))
        self.V = [self.R.x(v0)]

    def on_arnoldi(self, w, vnew):
        R, eps, k = self.R, self.t.eps, len(self.V)
        w = R.x(w)
        wn, mod, dh = w.copy(), np.abs(w), 0
        for v in self.V:  # classical Gram-Schmidt: every h_i from the unmodified w
            h, hb, _ = R.dot(v, w, conj=True)
            wn = wn - h * v
            mod = mod + abs(h) * np.abs(v)
            dh = dh + hb * np.abs(v)
        self._unit("v[j+1]", vnew, wn, dh + 2 * eps * k * mod)
        self.V.append(R.x(vnew))

    def ok(self):
        return all(v <= 1.0 for v in self.ratios.values()) and self.bound_over_v < 1e-3

    def report(self):
        return {**{k: round(v, 4) for k, v in self.ratios.items()}, "bound / max|v|": self.bound_over_v}


def min_residual_ratio(diag, lo, up, b, x_start, x_end, basis):
    """|b - A x_end| over rho = the smallest |b - A (x_start + span(basis))|, everything in extended precision, and what such a
    ratio cannot resolve: x_end is stored in the working type, and rounding even the minimiser itself into that type moves it by
    eps / 2 |x|, its residual by up to eps / 2 | |A| |x| |_2 -- first order in the ratio, since the rounding is not in the span
    -- plus the error of this evaluation, 4 n eps(long double).  Returns (ratio, floor)."""
    ext = np.clongdouble if np.iscomplexobj(diag) else np.longdouble
    eps = float(np.finfo(np.asarray(x_end).dtype).eps)
    d, lo, up, b = np.asarray(diag).astype(ext), ext(lo), ext(up), np.asarray(b).astype(ext)
    rmin, Q = b - tri_apply(d, lo, up, np.asarray(x_start).astype(ext)), []
    for v in basis:  # orthonormal basis of A * span(basis), Gram-Schmidt applied twice
        a = tri_apply(d, lo, up, np.asarray(v).astype(ext))
        for _ in range(2):
            for qv in Q:
                a = a - np.vdot(qv, a) * qv
        Q.append(a / np.sqrt((np.abs(a) ** 2).sum()))
    for _ in range(2):
        for qv in Q:
            rmin = rmin - np.vdot(qv, rmin) * qv
    rend = b - tri_apply(d, lo, up, np.asarray(x_end).astype(ext))
    rho = float(np.sqrt((np.abs(rmin) ** 2).sum()))
    ax = tri_apply(np.abs(d), abs(lo), abs(up), np.abs(np.asarray(x_end)).astype(np.longdouble))
    floor = 0.5 * eps * float(np.sqrt((ax ** 2).sum())) / rho + 4 * len(d) * float(np.finfo(np.longdouble).eps)
    return float(np.sqrt((np.abs(rend) ** 2).sum())) / rho, floor


_oracle_excess = {}


def oracle_excess(prec, n, restart=4, cycles=2):
    """The measured part of the margin of the least-squares check: oracle.dgmres (d, z) or oracle.sgmres (s, c; forward and
    pairwise dots, the larger figure) runs one cycle after another on the real system of this n, each from where the last one
    ended, and |ratio - 1| of each cycle against the extended-precision minimiser over the Krylov space of its start is what
    comes back.  The complex types take the figures of the real type of their precision."""
    import oracle

    real = "d" if prec in "dz" else "s"
    if (real, n) not in _oracle_excess:
        diag, lo, up, b, x0 = system(real, n, "gmres")
        rp, ci, v = tri_csr(diag, lo, up)
        worst = [0.0] * cycles
        for dots in (("forward",) if real == "d" else ("forward", "pairwise")):
            x = x0
            for c in range(cycles):
                if real == "d":
                    st, x1, ri = oracle.dgmres(n, 0, rp, ci, v, b, x, restart, 1e-14, 0.0, restart, 0)
                else:
                    st, x1, ri = oracle.sgmres(n, 0, rp, ci, v, b, x, restart, 1e-7, 0.0, restart, 0, dots=dots)
                assert ri[30] == restart, (st, ri[30])
                worst[c] = max(worst[c], abs(min_residual_ratio(diag, lo, up, b, x, x1, krylov_basis(diag, lo, up, b, x, restart))[0] - 1.0))
                x = x1
        _oracle_excess[(real, n)] = worst
    return _oracle_excess[(real, n)]


def cycle_margins(prec, n, floors):
    """1 + 4 * the oracle's measured excess of that cycle + what the ratio cannot resolve (min_residual_ratio)"""
    return [1.0 + 4.0 * e + f for e, f in zip(oracle_excess(prec, n), floors)]


def krylov_basis(diag, lo, up, b, x_start, m):
    """r0, A r0, ..., orthonormalised in extended precision: the space every GMRES(m) cycle from x_start minimises over"""
    ext = np.clongdouble if np.iscomplexobj(diag) else np.longdouble
    d, lo, up = np.asarray(diag).astype(ext), ext(lo), ext(up)
    v = np.asarray(b).astype(ext) - tri_apply(d, lo, up, np.asarray(x_start).astype(ext))
    V = [v / np.sqrt((np.abs(v) ** 2).sum())]
    for _ in range(m - 1):
        a = tri_apply(d, lo, up, V[-1])
        for _ in range(2):
            for qv in V:
                a = a - np.vdot(qv, a) * qv
        V.append(a / np.sqrt((np.abs(a) ** 2).sum()))
    return V


# ---- drivers --------------------------------------------------------------------------------------------------------------
def drive_cg(S, ck, iters):
    """S: .call() -> (status, job, u, v), .read(handle), .read_x(), .rinfo(), .apply(u, v) -> q as written, .jacobi(u, v) -> z"""
    done = 0
    while True:
        st, job, u, v = S.call()
        assert st == ST_OK, st
        if job == MV:
            ck.on_mv(S.read(u), S.rinfo())
            ck.answer(S.apply(u, v))
        elif job == PRECOND:
            ck.on_precond(S.read(u))
            ck.answer(S.jacobi(u, v))
        elif job == CRIT:
            ck.on_crit(S.read(u), S.read_x(), S.rinfo())
            done += 1
            if done > iters:
                return
        elif job == STOP and done == iters:  # (n = 1: the first step is exact, the residual 0 meets any tolerance; u is still r)
            ck.on_crit(S.read(u), S.read_x(), S.rinfo())
            return
        else:
            raise AssertionError("converged before %d iterations: the case checks too little" % iters)


def drive_gmres(S, ck, restart, cycles, on_cycle=None):
    """as drive_cg; S.base(v) turns the v of the first request into the handle of V[0], S.at(base, k) into that of V[k];
    S.copy(u, v) is the identity preconditioner.  on_cycle(x_start, x_end, basis) after every completed cycle.  With n <= restart
    the Krylov space is exhausted inside the first cycle (the next vector is rounding noise over a norm that is zero in exact
    arithmetic): only v0 is checked there."""
    st, job, u, v = S.call()
    assert st == ST_OK and job == MV
    base = S.base(v)
    for _ in range(cycles):
        x_start = S.read_x()
        q = S.apply(u, v)  # V[0] := A x
        j = -1
        while True:
            st, job, u, v = S.call()
            assert st == ST_OK, st
            if job == PRECOND:
                S.copy(u, v)
                continue
            vj = S.read(S.at(base, j + 1))
            if j < 0:
                ck.on_v0(vj, q)
                if S.n <= restart:
                    return
            else:
                ck.on_arnoldi(w, vj)
            j += 1
            if job == CRIT:
                break
            assert job == MV, job
            w = S.apply(u, v)
        assert j == restart, (j, restart)
        if on_cycle:
            on_cycle(x_start, S.read_x(), ck.V[:restart])
        st, job, u, v = S.call()  # the restart: v = A x into V[0] again
        assert st == ST_OK and job == MV, (st, job)


# ---- a working-precision model of the library, and its defects -------------------------------------------------------
DEFECTS = ("tail", "final2", "stride", "last", "conj")


def live(prec, n, defect):
    """does this defect change anything at this size and type"""
    t = Ty(prec)
    return {"tail": n % 256 != 0, "final2": t.blocks(n) > 256, "stride": n > 256 * t.cap, "last": True, "conj": t.cplx}[defect]


class ModelSolver:
    """The two state machines of itsol_api.cpp in the working type on numpy arrays, every reduction through the tree of the
    kernels: thread t of block k takes elements (trip * B + k) * 256 + t, a wavefront halves itself six times, four wavefronts
    meet as (s0 + s1) + (s2 + s3), and one block repeats that over the B partials.  defect: one of DEFECTS, or None."""

    def __init__(self, prec, n, kind, precond, restart=4, defect=None):
        self.t, self.n, self.kind, self.precond, self.m, self.defect = Ty(prec), n, kind, precond, restart, defect
        self.diag, self.lo, self.up, self.b, x0 = system(prec, n, kind)
        self.x = x0.copy()
        self.vec = {}
        self.stage, self.niter, self.j = "entry", 0, 0
        self.ri = np.zeros(100, self.t.rdtype)

    # -- kernels
    def _block(self, a):  # a[..., 256] -> a[...]
        w = a.reshape(a.shape[:-1] + (4, 64))
        for o in (32, 16, 8, 4, 2, 1):
            w = w[..., :o] + w[..., o:2 * o]
        w = w[..., 0]
        return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])

    def _dot(self, a, b, conj=False, alpha_dot=False):
        n, B, dt = self.n, self.t.blocks(self.n), self.t.dtype
        if self.defect == "conj" and alpha_dot:
            conj = True
        terms = ((np.conj(a) if conj else a) * b).astype(dt)
        if self.defect == "tail":
            terms = terms[:n - n % 256]
        if self.defect == "stride":
            terms = terms[:256 * self.t.cap]
        trips = max(1, -(-len(terms) // (256 * B)))
        pad = np.zeros(trips * B * 256, dt)
        pad[:len(terms)] = terms
        pad = pad.reshape(trips, B, 256)
        acc = pad[0].copy()
        for k in range(1, trips):
            acc = acc + pad[k]
        part = self._block(acc)
        if self.defect == "final2":
            part = part[:256]
        k2 = -(-len(part) // 256)
        pad = np.zeros(k2 * 256, dt)
        pad[:len(part)] = part
        pad = pad.reshape(k2, 256)
        acc = pad[0].copy()
        for k in range(1, k2):
            acc = acc + pad[k]
        return self._block(acc)

    def _nrm(self, a):
        return self.t.rdtype(np.sqrt(self._dot(a, a, conj=True).real))

    def _axpy(self, s, a, b):
        out = (self.t.dtype(s) * a + b).astype(self.t.dtype)
        if self.defect == "last":
            out[-1] = b[-1]
        return out

    # -- the interface the drivers use
    def read(self, h):
        return self.vec[h].copy()

    def read_x(self):
        return self.x.copy()

    def rinfo(self):
        return self.ri.copy()

    def apply(self, u, v):
        src = self.x if u == "x" else self.vec[u]
        self.vec[v] = tri_apply(self.diag, self.lo, self.up, src).astype(self.t.dtype)
        return self.vec[v].copy()

    def jacobi(self, u, v):
        self.vec[v] = (self.vec[u] / self.diag).astype(self.t.dtype)
        return self.vec[v].copy()

    def copy(self, u, v):
        self.vec[v] = self.vec[u].copy()

    def base(self, v):
        return v

    def at(self, base, k):
        return ("V", k)

    def call(self):
        return self._cg() if self.kind == "cg" else self._gmres()

    def _cg(self):
        V, ri = self.vec, self.ri
        if self.stage == "entry":
            V["r"], V["p"] = -self.b, self.x.copy()
            ri[1] = self._nrm(self.b)
            self.stage = "residual"
            return ST_OK, MV, "p", "q"
        if self.stage == "residual":
            V["r"] = V["r"] + V["q"]
            ri[0] = self._nrm(V["r"])
            V["p"] = np.zeros_like(V["p"])
            self.rz = self.t.dtype(1 + 1j) if self.t.cplx else self.t.dtype(1)
            self.stage = "precond"
            return ST_OK, CRIT, "r", None
        if self.stage == "precond":
            self.niter += 1
            ri[30] = self.niter
            self.stage = "direction"
            if self.precond:
                return ST_OK, PRECOND, "r", "z"
        if self.stage == "direction":
            z = V["z"] if self.precond else V["r"]
            rz_new = self._dot(V["r"], z)
            beta, self.rz = rz_new / self.rz, rz_new
            V["p"] = self._axpy(beta, V["p"], -z)
            self.stage = "update"
            return ST_OK, MV, "p", "q"
        pq = self._dot(V["p"], V["q"], alpha_dot=True)
        alpha = self.rz / pq
        self.x = self._axpy(alpha, V["p"], self.x)
        V["r"] = self._axpy(alpha, V["q"], V["r"])
        ri[0] = self._nrm(V["r"])
        self.stage = "precond"
        return ST_OK, CRIT, "r", None

    def _gmres(self):
        V, m, dt = self.vec, self.m, self.t.dtype
        src = "Z" if self.precond else "V"
        if self.stage in ("entry", "restart"):
            self.stage = "residual"
            return ST_OK, MV, "x", ("V", 0)
        if self.stage == "residual":
            w = (self.b - V[("V", 0)]).astype(dt)
            V[("V", 0)] = (w * (self.t.rdtype(1) / self._nrm(w))).astype(dt)
            self.j, self.h = 0, np.zeros((m + 1, m), self.t.ext)
            self.g0 = self._nrm(w)
            self.stage = "request_mv"
            if self.precond:
                return ST_OK, PRECOND, ("V", 0), ("Z", 0)
        if self.stage == "request_mv":
            self.stage = "arnoldi"
            return ST_OK, MV, (src, self.j), ("V", self.j + 1)
        if self.stage == "arnoldi":
            j, w = self.j, V[("V", self.j + 1)]
            hs = [self._dot(V[("V", i)], w, conj=True) for i in range(j + 1)]
            for i in range(j + 1):
                self.h[i, j] = hs[i]
            wn = w
            for i in range(j + 1):
                wn = self._axpy(-hs[i], V[("V", i)], wn)
            hh = self._nrm(wn)
            self.h[j + 1, j] = hh
            V[("V", j + 1)] = (wn * (self.t.rdtype(1) / hh)).astype(dt)
            self.j += 1
            if self.j < m:
                self.stage = "request_mv"
                if self.precond:
                    return ST_OK, PRECOND, ("V", self.j), ("Z", self.j)
                return self._gmres()
            # the small least-squares problem (host arithmetic in the library; extended precision here)
            e1 = np.zeros(m + 1, self.t.ext)
            e1[0] = self.g0
            y = np.linalg.lstsq(self.h.astype(np.complex128 if self.t.cplx else np.float64),
                                e1.astype(np.complex128 if self.t.cplx else np.float64), rcond=None)[0]
            for i in range(m):
                self.x = self._axpy(y[i], V[(src, i)], self.x)
            self.stage = "restart"
            return ST_OK, CRIT, None, None
        raise AssertionError(self.stage)
