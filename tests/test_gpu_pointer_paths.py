"""Every entry point three ways -- host arrays, the same data in device tensors under the automatic pointer mode, and those
tensors under aoclsparse_mi355_set_pointer_mode(device): the three results are bit-identical and meet the family's oracle check;
sentinels in the padding of strided operands and in the gaps of strided vectors survive.  The cases live in
tests/pointer_cases.py (tools/staging_evidence.py hashes the same calls).

Run against the parent build first: every case passes there as it stands and none had to be written around a quirk of the staging
code.  Two oracle checks had to follow what the families' own tests already say: a double-precision row of 32 entries or more is
summed by a wavefront and carries the forward bound instead of bit-exactness (the long row of the 70 x 70 matrix), and row-major
?csrmm is pinned to the reference kernel by the bound of tests/test_gpu_parity.py, column-major bit for bit.  What the parent
refuses is asserted as a refusal (test_level1_refuses_device_indices_with_a_host_vector)."""
import numpy as np
import pytest

from pointer_cases import CASES, NNZ, P, run_case, same_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_device_and_device_mode_agree(name):
    modes = CASES[name][0]
    outs = {}
    for mode in modes:
        out, check = run_case(name, mode)
        check(out)
        outs[mode] = out
    first = outs[modes[0]]
    for mode in modes[1:]:
        assert outs[mode].keys() == first.keys()
        for k in first:
            assert same_bits(first[k], outs[mode][k]), (name, mode, k)


def test_level1_refuses_device_indices_with_a_host_vector():
    """the extent of a host y comes from the indices, which are not inspected on the device: invalid_value, nothing written"""
    import torch
    L = P.lib()
    ix = torch.arange(NNZ, dtype=torch.int32, device="cuda")
    x = torch.ones(NNZ, dtype=torch.float64, device="cuda")
    y = np.arange(NNZ, dtype=np.float64)
    assert P.STATUS[L.aoclsparse_daxpyi(NNZ, 2.0, P._ptr(x), P._ptr(ix), P._ptr(y))] == "invalid_value"
    assert P.STATUS[L.aoclsparse_dsctr(NNZ, P._ptr(x), P._ptr(ix), P._ptr(y))] == "invalid_value"
    assert np.array_equal(y, np.arange(NNZ))
    xg = np.zeros(NNZ)
    assert P.STATUS[L.aoclsparse_dgthr(NNZ, P._ptr(y), P._ptr(xg), P._ptr(ix))] == "invalid_value"
    assert not xg.any()

