"""aoclsparse_itsol_* without a GPU: every answer the solver scaffold gives before the device is touched (handle, option, argument
and value-type checks of the init / option_set / rci_input / rci_solve / solve / destroy entry points), for all four value types."""
import ctypes
from ctypes import byref, c_int, c_void_p

import numpy as np
import pytest

from util import pkg

P = pkg()
L = P.lib()
ST = {v: k for k, v in P.STATUS.items()}
RCI_START, RCI_STOP = 1, 0
DTYPES = {"d": (np.float64, np.float64), "s": (np.float32, np.float32), "c": (np.complex64, np.float32), "z": (np.complex128, np.float64)}
OTHER = {"d": "s", "s": "c", "c": "z", "z": "d"}  # a handle of another value type

pytestmark = pytest.mark.parametrize("t", ["d", "s", "c", "z"])


def fn(t, stem):
    return getattr(L, "aoclsparse_itsol_%s_%s" % (t, stem))


def new_handle(t):
    h = c_void_p()
    assert fn(t, "init")(byref(h)) == 0 and h.value
    return h


def destroy(*handles):
    for h in handles:
        L.aoclsparse_itsol_destroy(byref(h))
        assert h.value is None


def test_init_null(t):
    assert fn(t, "init")(None) == ST["invalid_pointer"]


def test_option_set(t):
    h = new_handle(t)
    opt = L.aoclsparse_itsol_option_set
    assert opt(None, b"cg iteration limit", b"10") == ST["invalid_pointer"]
    assert opt(h, None, b"10") == ST["invalid_pointer"]
    assert opt(h, b"cg iteration limit", None) == ST["invalid_pointer"]
    assert opt(h, b"no such option", b"1") == ST["invalid_value"]
    assert opt(h, b"cg iteration limit", b"0") == ST["invalid_value"]
    assert opt(h, b"cg iteration limit", b"abc") == ST["invalid_value"]
    assert opt(h, b"cg rel tolerance", b"-1") == ST["invalid_value"]
    # names and labels are trimmed, blank-squeezed and lower-cased
    assert opt(h, b"Iterative  Method", b" GM RES ") == ST["success"]
    assert opt(h, b"iterative method", b"bicgstab") == ST["invalid_value"]
    destroy(h)


def test_rci_input(t):
    dtype, _ = DTYPES[t]
    h, other = new_handle(t), new_handle(OTHER[t])
    b = np.ones(4, dtype)
    assert fn(t, "rci_input")(None, 4, P._ptr(b)) == ST["invalid_pointer"]
    assert fn(t, "rci_input")(other, 4, P._ptr(b)) == ST["wrong_type"]
    assert fn(t, "rci_input")(h, -1, P._ptr(b)) == ST["invalid_value"]
    assert fn(t, "rci_input")(h, 4, None) == ST["invalid_pointer"]
    destroy(h, other)


def test_rci_solve(t):
    dtype, rdtype = DTYPES[t]
    h, other = new_handle(t), new_handle(OTHER[t])
    x, rinfo = np.ones(4, dtype), np.zeros(100, rdtype)
    u, v = c_void_p(), c_void_p()
    ok = dict(h=h, job=True, u=byref(u), v=byref(v), x=P._ptr(x), rinfo=P._ptr(rinfo))

    def call(**kw):
        a = {**ok, **kw}
        job = c_int(RCI_START)
        st = fn(t, "rci_solve")(a["h"], byref(job) if a["job"] else None, a["u"], a["v"], a["x"], a["rinfo"])
        return P.STATUS[st], job.value

    assert call(h=None)[0] == "invalid_pointer"
    assert call(h=other)[0] == "wrong_type"
    assert call(job=False)[0] == "invalid_pointer"
    for k in ("u", "v", "x", "rinfo"):
        assert call(**{k: None}) == ("invalid_pointer", RCI_STOP), k
    # rci_input was never called: no right-hand side
    assert call() == ("invalid_pointer", RCI_STOP)
    destroy(h, other)


def test_solve(t):
    dtype, rdtype = DTYPES[t]
    h, other = new_handle(t), new_handle(OTHER[t])
    b, x, rinfo = np.ones(4, dtype), np.ones(4, dtype), np.zeros(100, rdtype)
    ok = dict(h=h, n=4, b=P._ptr(b), x=P._ptr(x), rinfo=P._ptr(rinfo))

    def call(**kw):
        a = {**ok, **kw}
        return P.STATUS[fn(t, "solve")(a["h"], a["n"], None, None, a["b"], a["x"], a["rinfo"], None, None, None)]

    assert call(h=None) == "invalid_pointer"
    assert call(h=other) == "wrong_type"
    assert call(x=None) == "invalid_pointer"
    assert call(rinfo=None) == "invalid_pointer"
    rinfo[:] = 7.0
    assert call(n=-1) == "invalid_value"
    assert np.all(rinfo == 0), "rinfo is zeroed before the size is looked at"
    assert call(b=None) == "invalid_pointer"
    destroy(h, other)


def test_destroy(t):
    L.aoclsparse_itsol_destroy(None)
    h = c_void_p()
    L.aoclsparse_itsol_destroy(byref(h))
    assert h.value is None
    h = new_handle(t)
    destroy(h)
