"""aoclsparse_mi355_order_mat_device without a GPU: the symbol, its declaration, the two thresholds, and every status that is
decided before the device is touched, in aoclsparse_order_mat's order (include/aoclsparse_mi355.h: order_mat_device)."""
import os
import re

from order_cases import L, P, early_cases


def _header():
    with open(os.path.join(P.INCLUDE_DIR, "aoclsparse_mi355.h")) as f:
        return f.read()


def test_symbol_is_exported_and_declared():
    assert hasattr(L, "aoclsparse_mi355_order_mat_device")
    assert re.search(r"DLL_PUBLIC\s+aoclsparse_status\s+aoclsparse_mi355_order_mat_device\s*\(\s*aoclsparse_matrix\s+A\s*\)\s*;", _header())
    assert "aoclsparse_mi355_order_mat_device" in P.SIGNATURES
    assert callable(P.Matrix.order_device)


def test_threshold_macros_equal_the_python_constants():
    src = _header()
    for macro, value in (("AOCLSPARSE_MI355_ORDER_SHORT_MAX", P.ORDER_SHORT_MAX), ("AOCLSPARSE_MI355_ORDER_LDS_MAX", P.ORDER_LDS_MAX)):
        m = re.search(r"#define\s+%s\s+(\d+)" % macro, src)
        assert m and int(m.group(1)) == value, macro
    assert 1 < P.ORDER_SHORT_MAX < P.ORDER_LDS_MAX < P.COO_SORT_TILE  # the edge matrix of the GPU test relies on this order


def test_statuses_decided_before_the_device_is_touched():
    """null, the formats that are not CSR, the CSC-created handle and the empty matrices: no GPU is needed for any of them"""
    for name, A, want in early_cases():
        got = L.aoclsparse_mi355_order_mat_device(A.h if A is not None else None)
        assert got == want, (name, P.STATUS.get(got, got), P.STATUS.get(want, want))
        if A is not None and name not in ("csc",):  # the host call agrees wherever it is defined the same way
            assert L.aoclsparse_order_mat(A.h) == want, name
