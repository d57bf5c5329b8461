"""CPU tier of the packed SELL-64 table indices: the query is part of the C ABI (no device needed)."""
import ctypes
import os
import re
import subprocess

from util import ROOT, pkg, random_csr

P = pkg()
L = P.lib()


def test_get_sell_packing_is_declared_exported_and_checks_its_arguments():
    src = open(os.path.join(ROOT, "include", "aoclsparse_mi355.h")).read()
    assert re.search(r"DLL_PUBLIC\s+aoclsparse_status\s+aoclsparse_mi355_get_sell_packing\s*\(", src)
    out = subprocess.check_output(["nm", "-D", "--defined-only", P.LIB_PATH], text=True)
    assert "aoclsparse_mi355_get_sell_packing" in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    rp, ci, v = random_csr(1, 20, 20, lambda r, i: 3)
    A = P.Matrix(0, 20, 20, rp, ci, v)
    b, w, u = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    ref = ctypes.byref
    assert L.aoclsparse_mi355_get_sell_packing(None, P.OP_NONE, ref(b), ref(w), ref(u)) == 2  # invalid_pointer
    assert L.aoclsparse_mi355_get_sell_packing(A.h, P.OP_NONE, None, ref(w), ref(u)) == 2
    assert L.aoclsparse_mi355_get_sell_packing(A.h, P.OP_NONE, ref(b), None, ref(u)) == 2
    assert L.aoclsparse_mi355_get_sell_packing(A.h, P.OP_NONE, ref(b), ref(w), None) == 2
    assert (b.value, w.value, u.value) == (-1, -1, -1)  # nothing written on an error
    # no SELL-64 copy (nothing on a device yet): bytes-or-values, no uniform lists
    assert A.sell_packing() == (0, 0, 0) and A.sell_packing(P.OP_TRANSPOSE) == (0, 0, 0)
