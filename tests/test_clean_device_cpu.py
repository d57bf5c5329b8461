"""aoclsparse_mi355_clean_csr_device without a GPU: the host route it must equal (csr_optimize, through aoclsparse_optimize without
hints) against a numpy restatement of the clean CSR over every edge matrix of the GPU test; the symbol, its declaration and its
threshold; and every status that is decided before the device is touched (include/aoclsparse_mi355.h: clean_csr_device)."""
import os
import re

import numpy as np
import pytest

from clean_cases import (DTYPES, EDGE_SHAPES, HostMatrix, L, P, SUCCESS, assert_same_clean, early_cases, edge_structure, edge_values,
                         export_clean, small_structures, twin)

STRUCTURES = [(s,) + edge_structure(s) for s in EDGE_SHAPES] + small_structures()


def _header():
    with open(os.path.join(P.INCLUDE_DIR, "aoclsparse_mi355.h")) as f:
        return f.read()


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_route_equals_the_restatement(dtype, base):
    """the yardstick of the GPU test, checked where no GPU is needed: twin() asserts the host route against clean_reference"""
    for name, m, n, rp, ci in STRUCTURES:
        H, got = twin(base, m, n, rp + base, ci + base, edge_values(dtype, len(ci)))
        internal = got[6]
        assert got[0] == (0 if internal else base), name
        if name in ("class 1, full diagonal", "class 2, full diagonal", "m = 0", "n = 0"):
            assert not internal, name
        if name.startswith(("scan", "class 2, diagonals", "one row", "nnz = 0", "tall", "wide")):
            assert internal and len(got[2]) > len(ci), name  # entries were inserted


def test_symbol_is_exported_and_declared():
    assert hasattr(L, "aoclsparse_mi355_clean_csr_device")
    assert re.search(r"DLL_PUBLIC\s+aoclsparse_status\s+aoclsparse_mi355_clean_csr_device\s*\(\s*aoclsparse_matrix\s+A\s*\)\s*;", _header())
    assert "aoclsparse_mi355_clean_csr_device" in P.SIGNATURES
    assert callable(P.Matrix.clean_device)


def test_threshold_macro_equals_the_python_constant():
    m = re.search(r"#define\s+AOCLSPARSE_MI355_CLEAN_ROW_WAVE\s+(\d+)", _header())
    assert m and int(m.group(1)) == P.CLEAN_ROW_WAVE
    assert 1 < P.CLEAN_ROW_WAVE < 2047  # the edge matrix has rows on either side of it


def test_statuses_decided_before_the_device_is_touched():
    for name, A, want in early_cases():
        got = L.aoclsparse_mi355_clean_csr_device(A.h if A is not None else None)
        assert got == want, (name, P.STATUS.get(got, got), P.STATUS.get(want, want))


def test_a_handle_that_has_its_clean_csr_is_left_alone():
    """success at once, whether the clean CSR is the handle's own arrays or a copy, and whether or not a GPU exists"""
    for name, m, n, rp, ci in small_structures():
        H, before = twin(1, m, n, rp + 1, ci + 1, edge_values(np.float64, len(ci)))
        assert H.clean_device() == SUCCESS, name
        assert_same_clean(export_clean(H, np.float64), before, name)


def test_a_valid_handle_answers_what_order_mat_device_answers():
    """after the early statuses comes the runtime's initialisation: without a GPU both calls return its failure, with one both
    succeed; the number is not written down here"""
    name, m, n, rp, ci = small_structures()[7]
    assert name == "one row holds everything"  # (valid and unsorted: neither call has an early answer for it)
    v = edge_values(np.float64, len(ci))
    A, B = HostMatrix(0, m, n, rp, ci, v), HostMatrix(0, m, n, rp, ci, v)
    assert A.status == 0 and B.status == 0
    assert A.clean_device() == B.order_device()
