"""What tests/test_order_device_cpu.py and tests/test_order_device_gpu.py share: the handles aoclsparse_mi355_order_mat_device
answers before it touches the device, and the status it must give for each (aoclsparse_order_mat's order, include/aoclsparse_mi355.h)."""
from ctypes import byref, c_void_p

import numpy as np

from util import pkg

P = pkg()
L = P.lib()

SUCCESS, NOT_IMPLEMENTED, INVALID_POINTER, INVALID_VALUE = 0, 1, 2, 5


class Raw:
    """a handle made by a create call that P.Matrix has no constructor for; keeps the aliased arrays alive"""

    def __init__(self, create, *args):
        self.keep = [a for a in args if isinstance(a, np.ndarray)]
        self.h = c_void_p()
        self.status = getattr(L, create)(byref(self.h), *[P._ptr(a) if isinstance(a, np.ndarray) else a for a in args])

    def __del__(self):
        try:
            if self.h:
                L.aoclsparse_destroy(byref(self.h))
        except Exception:
            pass


def early_cases():
    """[(name, handle object or None, status)]: 3 x 3, the rows [0 1], [1], [0 2] (row 2 is NOT ascending in the CSR-shaped ones)"""
    i32 = lambda *a: np.array(a, np.int32)  # noqa: E731
    v = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    cases = [("null", None, INVALID_POINTER)]
    cases.append(("coo", Raw("aoclsparse_create_dcoo", 0, 3, 3, 5, i32(0, 0, 1, 2, 2), i32(1, 0, 1, 2, 0), v.copy()), NOT_IMPLEMENTED))
    # CSC arrays: a CSR-format handle whose first representation lives in the caller's host arrays
    cases.append(("csc", Raw("aoclsparse_create_dcsc", 0, 3, 3, 5, i32(0, 2, 4, 5), i32(2, 0, 1, 0, 2), v.copy()), NOT_IMPLEMENTED))
    # TCSR: L = the diagonal with (2, 0) in front of it, U = the diagonal with (0, 1) behind it
    cases.append(("tcsr", P.TcsrMatrix(0, 3, i32(0, 1, 2, 4), i32(0, 1, 0, 2), np.array([1.0, 2.0, 5.0, 4.0]),
                                       i32(0, 2, 3, 4), i32(0, 1, 1, 2), np.array([1.0, 3.0, 2.0, 4.0])), NOT_IMPLEMENTED))
    cases.append(("bsr", P.BsrMatrix(0, P.ORDER_ROW, 2, 2, 2, i32(0, 2, 3), i32(1, 0, 1), np.arange(12.0)), NOT_IMPLEMENTED))
    cases.append(("no rows", P.Matrix(0, 0, 3, i32(0), i32(0), np.zeros(1)), SUCCESS))
    cases.append(("no entries", P.Matrix(0, 3, 3, i32(0, 0, 0, 0), i32(0), np.zeros(1)), SUCCESS))
    for name, A, _ in cases:
        assert A is None or A.status == 0, (name, P.STATUS.get(A.status, A.status))
    return cases
