"""CPU tier of the SELL-64 value tables: the option and the query are part of the C ABI (no device needed)."""
import ctypes
import os
import re
import subprocess

import numpy as np

from util import ROOT, pkg, random_csr

P = pkg()
L = P.lib()


def test_sell_values_option_is_validated():
    assert P.OPTION_SELL_VALUES == 5
    for bad in (-2, 2, 7):
        assert L.aoclsparse_mi355_set_option(P.OPTION_SELL_VALUES, bad) == 5  # invalid_value
    for good in (0, 1, -1):  # (-1, the default, last)
        assert L.aoclsparse_mi355_set_option(P.OPTION_SELL_VALUES, good) == 0
    assert L.aoclsparse_mi355_set_option(6, 0) == 5  # option_count is 6


def test_get_sell_values_is_declared_exported_and_checks_its_arguments():
    src = open(os.path.join(ROOT, "include", "aoclsparse_mi355.h")).read()
    assert re.search(r"DLL_PUBLIC\s+aoclsparse_status\s+aoclsparse_mi355_get_sell_values\s*\(", src)
    assert re.search(r"aoclsparse_mi355_option_sell_values\s*=\s*5", src)
    assert re.search(r"aoclsparse_mi355_option_count\s*=\s*6", src)
    out = subprocess.check_output(["nm", "-D", "--defined-only", P.LIB_PATH], text=True)
    assert "aoclsparse_mi355_get_sell_values" in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    rp, ci, v = random_csr(1, 20, 20, lambda r, i: 3)
    A = P.Matrix(0, 20, 20, rp, ci, v)
    n = ctypes.c_int32(-1)
    assert L.aoclsparse_mi355_get_sell_values(None, P.OP_NONE, ctypes.byref(n)) == 2
    assert L.aoclsparse_mi355_get_sell_values(A.h, P.OP_NONE, None) == 2
    assert A.sell_values() == 0 and A.sell_values(P.OP_TRANSPOSE) == 0  # no SELL-64 copy (nothing on a device yet)
    assert np.array_equal(A.val, v)
