"""aoclsparse_itsol_{c,z}_*: user callbacks, the statuses of the direct interface and reverse-communication CG on complex
handles -- what test_itsol_callbacks_limits_and_errors and test_itsol_rci_interfaces check for real ones -- on the two
systems of test_complex_itsol_cg_and_gmres."""
import ctypes
from ctypes import c_int32, c_void_p

import numpy as np
import pytest

from util import complex_itsol_systems, pkg

pytestmark = [pytest.mark.gpu, pytest.mark.parametrize("prec", ["z", "c"])]

torch = pytest.importorskip("torch")
P = pkg()
L = P.lib()

PRECOND_T = ctypes.CFUNCTYPE(c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p)
MONIT_T = ctypes.CFUNCTYPE(c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p)
RCI_STOP, RCI_START, RCI_MV = 0, 1, 2


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    st, d, cus, name = P.device_info()
    assert st == 0 and cus > 0


def view(ptr, n, dtype):
    """numpy view of n elements at a raw pointer a callback or the RCI interface handed out"""
    nbytes = n * np.dtype(dtype).itemsize
    return np.frombuffer((ctypes.c_char * nbytes).from_address(ptr), dtype=dtype)


class Case:
    """both systems as handles of one precision, the option sets of the existing test, and a direct-solve shorthand"""

    def __init__(self, prec):
        self.prec = prec
        self.dtype, self.rdtype = (np.complex128, np.float64) if prec == "z" else (np.complex64, np.float32)
        self.n, D, self.gen, S, self.low, self.xs = complex_itsol_systems(self.dtype)  # (the handles alias the CSR arrays)
        self.tol = 1e-9 if prec == "z" else 2e-4
        self.diag = np.diag(S).astype(self.dtype)
        self.A, self.As = c_void_p(), c_void_p()
        for h, (rp, ci, v) in ((self.A, self.gen), (self.As, self.low)):
            assert self.fn("create_?csr")(ctypes.byref(h), 0, self.n, self.n, len(v), P._ptr(rp), P._ptr(ci), P._ptr(v)) == 0
        self.d, self.ds = P.Descr(), P.Descr(mtype=P.TYPE_SYMMETRIC, fill=P.FILL_LOWER)
        self.b, self.bs = (D @ self.xs).astype(self.dtype), (S @ self.xs).astype(self.dtype)
        self.cg_opts = (("cg rel tolerance", str(self.tol)), ("cg abs tolerance", "0"), ("cg iteration limit", "500"))
        self.gmres_opts = (("gmres rel tolerance", str(self.tol)), ("gmres abs tolerance", "0"), ("gmres restart iterations", "15"),
                           ("gmres iteration limit", "300"))
        self.handles = []

    def fn(self, stem):
        return getattr(L, "aoclsparse_" + stem.replace("?", self.prec))

    def handle(self, method, opts=()):
        h = c_void_p()
        assert self.fn("itsol_?_init")(ctypes.byref(h)) == 0
        for k, val in (("iterative method", method),) + tuple(opts):
            assert L.aoclsparse_itsol_option_set(h, k.encode(), val.encode()) == 0
        self.handles.append(h)
        return h

    def solve(self, h, A, d, b, precond=None, monit=None, n=None):
        n = self.n if n is None else n
        x, rinfo = np.zeros(n, self.dtype), np.zeros(100, self.rdtype)
        st = self.fn("itsol_?_solve")(h, n, A, d.h, P._ptr(b), P._ptr(x), P._ptr(rinfo), precond, monit, None)
        return st, x, rinfo

    def close(self):
        for h in self.handles:
            L.aoclsparse_itsol_destroy(ctypes.byref(h))
        L.aoclsparse_destroy(ctypes.byref(self.A)), L.aoclsparse_destroy(ctypes.byref(self.As))


@pytest.fixture
def case(prec):
    c = Case(prec)
    yield c
    c.close()


def jacobi(c, calls):
    def f(flag, nn, u, w, udata):
        calls.append(nn)
        view(w, nn, c.dtype)[:] = view(u, nn, c.dtype) / c.diag
        return 0
    return PRECOND_T(f)


def test_cg_user_preconditioner_and_monitor(case):
    c = case
    pcalls, seen = [], []

    def monit(nn, x, r, rinfo, udata):
        ri = view(rinfo, 100, c.rdtype)
        seen.append((float(np.linalg.norm(view(r, nn, c.dtype).astype(np.complex128))), float(ri[0])))
        return 0

    h = c.handle("cg", c.cg_opts + (("cg preconditioner", "user"),))
    st, x, rinfo = c.solve(h, c.As, c.ds, c.bs, jacobi(c, pcalls), MONIT_T(monit))
    assert st == 0
    assert np.max(np.abs(x - c.xs)) <= 200 * c.tol * np.max(np.abs(c.xs))
    assert len(pcalls) == rinfo[30] and len(seen) >= rinfo[30] and all(nn == c.n for nn in pcalls)
    # the residual handed in is a copy of the vector whose norm was just reduced: only the summation order differs
    rel = 1e-10 if c.prec == "z" else 1e-5
    for rn, r0 in seen:
        assert abs(rn - r0) <= rel * r0, (rn, r0)


def test_direct_interface_statuses(case):
    c = case
    n = c.n
    h = c.handle("cg", c.cg_opts + (("cg preconditioner", "user"),))
    stop = MONIT_T(lambda nn, x, r, ri, u: 1 if view(ri, 100, c.rdtype)[30] >= 1 else 0)  # after the first iteration
    st, x, rinfo = c.solve(h, c.As, c.ds, c.bs, jacobi(c, []), stop)
    assert st == 8 and rinfo[30] == 1  # user_stop
    assert c.solve(h, c.As, c.ds, c.bs)[0] == 2  # "user" without a callback: invalid_pointer
    h = c.handle("cg", (("cg iteration limit", "2"), ("cg abs tolerance", "1e-14"), ("cg rel tolerance", "0")))
    st, x, rinfo = c.solve(h, c.As, c.ds, c.bs)
    assert st == 7 and rinfo[30] == 3  # maxit: the reference stops once niter > maxit
    assert c.solve(h, c.As, c.d, c.bs)[0] == 5  # a general descriptor for CG: invalid_value
    assert c.solve(h, c.As, c.ds, np.zeros(n + 1, c.dtype), n=n + 1)[0] == 3  # invalid_size


def test_gmres_identity_preconditioner_changes_no_bit(case):
    """With a preconditioner Z_j replaces V_j as the mv operand and in the final combination; a callback that copies u
    to v makes Z_j a byte copy of V_j."""
    c = case
    st0, x0, rinfo0 = c.solve(c.handle("gmres", c.gmres_opts), c.A, c.d, c.b)
    calls = []

    def ident(flag, nn, u, w, udata):
        calls.append(nn)
        view(w, nn, c.dtype)[:] = view(u, nn, c.dtype)
        return 0

    h = c.handle("gmres", c.gmres_opts + (("gmres preconditioner", "user"),))
    st1, x1, rinfo1 = c.solve(h, c.A, c.d, c.b, PRECOND_T(ident))
    assert st0 == st1 == 0 and calls
    assert np.max(np.abs(x0 - c.xs)) <= 50 * c.tol * np.max(np.abs(c.xs))
    assert np.array_equal(x1.view(c.rdtype), x0.view(c.rdtype)) and rinfo1[30] == rinfo0[30]


@pytest.mark.parametrize("device", [False, True])
def test_rci_cg_gives_the_direct_solve_bits(case, device):
    """Host b: pinned workspaces the caller reads and writes through numpy views.  Device b: HBM workspaces, the caller's
    mv is aoclsparse_?mv on the pointers handed out."""
    c = case
    n = c.n
    st, xdir, rdir = c.solve(c.handle("cg", c.cg_opts), c.As, c.ds, c.bs)
    assert st == 0
    h = c.handle("cg", c.cg_opts)
    rinfo, job, u, w = np.zeros(100, c.rdtype), ctypes.c_int(RCI_START), c_void_p(), c_void_p()
    one, zero, mv = np.ones(1, c.dtype), np.zeros(1, c.dtype), c.fn("?mv")
    if device:
        bd = torch.from_numpy(c.bs).cuda()
        xd = torch.from_numpy(np.zeros(n, c.dtype)).cuda()
        assert c.fn("itsol_?_rci_input")(h, n, P._ptr(bd)) == 0
        xarg = P._ptr(xd)
    else:
        x = np.zeros(n, c.dtype)
        assert c.fn("itsol_?_rci_input")(h, n, P._ptr(c.bs)) == 0
        xarg = P._ptr(x)
    calls = 0
    while job.value != RCI_STOP and calls < 5000:
        assert c.fn("itsol_?_rci_solve")(h, ctypes.byref(job), ctypes.byref(u), ctypes.byref(w), xarg, P._ptr(rinfo)) == 0
        calls += 1
        if job.value == RCI_MV:
            if device:
                assert mv(P.OP_NONE, P._ptr(one), c.As, c.ds.h, u, P._ptr(zero), w) == 0
            else:
                uu, ww = view(u.value, n, c.dtype).copy(), np.zeros(n, c.dtype)
                assert mv(P.OP_NONE, P._ptr(one), c.As, c.ds.h, P._ptr(uu), P._ptr(zero), P._ptr(ww)) == 0
                view(w.value, n, c.dtype)[:] = ww
    assert job.value == RCI_STOP and calls < 5000
    if device:
        torch.cuda.synchronize()
        x = xd.cpu().numpy()
    assert np.array_equal(x.view(c.rdtype), xdir.view(c.rdtype)) and rinfo[30] == rdir[30]
