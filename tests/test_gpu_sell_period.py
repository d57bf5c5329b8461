"""SELL-64 short rows: the periodic range of the slice records and uniform lists (aoclsparse_mi355_get_sell_period).  On a
stencil the records and lists of one grid line are those of the line before with every column moved by one line; the plan finds
the range and the period, and the short-row kernel reads the FIRST period's records and lists for every slice of the range,
gathering from x + k * stride.

Every case runs double (2 slices per wavefront from 60,000 slices on) and float (4), (alpha, beta) = (1, 0), (1.7, -0.3),
(-0.75, 1.5), two consecutive products per handle (both sweep directions), and compares every result bit for bit with the
sell_values = 0 handle (values in the cells: no records beyond offsets, no range) and with the CPU oracle in the handle's order.
Before a product runs, get_sell_period must report what the construction implies, so no case passes by missing the path."""
import functools

import numpy as np
import pytest

import test_gpu_sell_packed as S
import test_gpu_sell_records as R
import test_gpu_sell_wide as W
from util import pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
P = pkg()
L = P.lib()

DTYPES = S.DTYPES
M1 = R.M1  # 4096 slices: one slice per wavefront
M = W.M  # 61,440 slices: two (double) and four (float) slices per wavefront
NONE = (0, 0, 0, 0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    yield


def up4(s):
    return (s + 3) // 4 * 4


def run(rp, ci, v, n, dtype, expect, off=0, seed=1):
    """expect: the range, or a predicate on it"""
    v = np.ascontiguousarray(v, dtype=dtype)
    x, y0 = R.operands(n, len(rp) - 1, dtype, seed)
    A1, d1 = S.handle(rp, ci, v.copy(), 1, n=n)
    A0, d0 = S.handle(rp, ci, v.copy(), 0, n=n)
    got = A1.sell_period()
    assert expect(got) if callable(expect) else got == expect, got
    assert A0.sell_period() == NONE
    R.products(A1, d1, A0, d0, x, y0, off)
    assert A1.sell_period() == got
    return got


# ---- 5-point stencils ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid(gx, m):
    """the first m rows of a 5-point Laplacian with grid lines of gx rows (the last line may be ragged), natural values"""
    gy = -(-m // gx)
    rp, ci, v = S.laplace5_grid(gx, gy)
    if gx * gy != m:  # cut inside the last line: the rows that lose their south neighbour lose it in the arrays too
        keep = ci[:rp[m]] < m
        lens = np.add.reduceat(keep.astype(np.int64), rp[:m].astype(np.int64))
        rp2 = np.zeros(m + 1, np.int64)
        rp2[1:] = np.cumsum(lens)
        rp, ci, v = rp2.astype(np.int32), ci[:rp[m]][keep], v[:rp[m]][keep]
    return rp, ci, v


def stencil_range(gx, m):
    """what a grid of lines of gx rows implies: the period = the slices after which a line starts at the same lane again, as a
    multiple of 4; the range holds every slice whose rows all have both their north and south neighbours, cut inward to 4
    slices, and no slice that lies in line 0 or in the rows without a south neighbour"""
    period = np.lcm(np.lcm(gx, 64) // 64, 4)
    inner_lo, inner_hi = up4(-(-gx // 64)), (m - gx) // 64 // 4 * 4

    def ok(got):
        lo, hi, p, stride = got
        return (p, stride) == (period, 64 * period) and lo <= inner_lo and hi >= inner_hi and lo >= gx // 64 and hi <= -(-(m - gx) // 64)

    return ok


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("gx, m", [(256, M1), (192, 192 * 1366), (320, 320 * 820), (4096, M1), (192, M), (4096, M)])
def test_grid_lines(gx, m, dtype):
    """periods of 4, 12, 20 and 64 slices (12 and 20: the division by the period is a multiply by a reciprocal, not a shift), at
    one slice per wavefront and at several"""
    rp, ci, v = grid(gx, m)
    got = run(rp, ci, v, m, dtype, stencil_range(gx, m))
    if gx % 64 == 0 and m % gx == 0:  # lines that start at a slice: exactly the lines 1 .. L - 2
        assert got[:2] == (up4(gx // 64), (m - gx) // 64 // 4 * 4)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [M1 + 64 * 40 + 77, M + 3 * 64 + 9])
def test_lines_of_200_rows_and_a_ragged_last_line(m, dtype):
    """a line is 3.125 slices: the pattern repeats after 25 slices, reported as 100; the last line is cut short"""
    rp, ci, v = grid(200, m)
    got = run(rp, ci, v, m, dtype, stencil_range(200, m), seed=2)
    assert got[2:] == (100, 6400)


# ---- boundary-free stencils ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def free(m, drop=()):
    rp, ci = R.shifted_stencil(m, dict(drop))
    return rp, ci, R.by_offset(rp, ci, R.OFFS)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [M1, M])
def test_boundary_free_stencil(m, dtype):
    """every slice is the slice before it moved by 64 columns: the whole matrix is in the range, period 4"""
    rp, ci, v = free(m)
    run(rp, ci, v, m + 16, dtype, (0, m // 64, 4, 256), seed=3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m, s", [(M1, 1001), (M, 20002)])
def test_an_interior_row_loses_a_cell(m, s, dtype):
    """lane 17 of slice s omits cell 2: the slice becomes an exception slice, its record differs, and the range starts behind it"""
    rp, ci, v = free(m, (((s, 17), (2,)),))
    run(rp, ci, v, m + 16, dtype, (up4(s + 1), m // 64, 4, 256), seed=4)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m, s", [(M1, 1001), (M, 20002)])
def test_an_interior_value_differs(m, s, dtype):
    """one cell of lane 5 of slice s holds the table's other value: the slice's rows no longer share a word, its record loses the
    flag, and the range starts behind it"""
    rp, ci, v = free(m)
    v = v.copy()
    e = rp[64 * s + 5] + 1
    v[e] = 1.5 if v[e] == -0.75 else -0.75
    run(rp, ci, v, m + 16, dtype, (up4(s + 1), m // 64, 4, 256), seed=5)


@functools.lru_cache(maxsize=None)
def stacked(m, top):
    """slices [0, top): rows r + OFFS; below: the offsets change with slice % 3 (a period of 12 slices, none of 4)"""
    r = np.arange(m, dtype=np.int64)
    third = (r // 64) % 3
    offs = np.where((r // 64 < top)[:, None], np.array(R.OFFS), np.array(R.OFFS) + third[:, None] * np.array([0, 1, 1, 2]))
    rp = (4 * np.arange(m + 1)).astype(np.int32)
    ci = (r[:, None] + offs).reshape(-1).astype(np.int32)
    return rp, ci, R.by_offset(rp, np.repeat(r, 4).astype(np.int32) + np.tile(np.array(R.OFFS, np.int32), m), R.OFFS)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [M1, M])
def test_two_stencils_stacked(m, dtype):
    """60 % of the slices repeat with period 4, the rest with period 12: ONE range is reported, the rest runs on its own records"""
    top = (m // 64) * 6 // 10 // 12 * 12
    rp, ci, v = stacked(m, top)
    run(rp, ci, v, m + 32, dtype, (0, top, 4, 256), seed=6)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_period_above_the_cap(dtype):
    """grid lines of 4100 slices (the cap is 4096): nothing is reported and the product is right"""
    gx = 64 * 4100
    rp, ci, v = grid(gx, 4 * gx)
    run(rp, ci, v, 4 * gx, dtype, NONE, seed=7)


@pytest.mark.parametrize("dtype", DTYPES)
def test_value_changes_move_the_range(dtype):
    """?set_value on a row of line 5 of the 1024 x 1024 Laplacian: its slice loses its word and the range starts behind it; the
    value comes back through ?update_values and so does the range"""
    gx = 1024
    m = gx * gx
    rp, ci, v = grid(gx, m)
    ra, _ = R.off_pattern_rows(gx)
    dbl = dtype == np.float64
    A1, d1 = S.handle(rp, ci, np.array(v, dtype=dtype), 1)
    A0, d0 = S.handle(rp, ci, np.array(v, dtype=dtype), 0)
    x, y0 = R.operands(m, m, dtype, 8)
    whole = (16, (gx - 1) * 16, 16, 1024)
    assert A1.sell_period() == whole
    R.products(A1, d1, A0, d0, x, y0)
    for A in (A1, A0):
        assert (L.aoclsparse_dset_value if dbl else L.aoclsparse_sset_value)(A.h, ra, ra, -1.0) == 0
    R.products(A1, d1, A0, d0, x, y0)
    assert A1.sell_period() == (up4(ra // 64 + 1), (gx - 1) * 16, 16, 1024) and A1.sell_values() == 2
    v3 = np.array(v, dtype=dtype)
    for A in (A1, A0):
        assert (L.aoclsparse_dupdate_values if dbl else L.aoclsparse_supdate_values)(A.h, len(v3), P._ptr(v3)) == 0
    R.products(A1, d1, A0, d0, x, y0)
    assert A1.sell_period() == whole


@pytest.mark.parametrize("dtype", DTYPES)
def test_unaligned_operands(dtype):
    """x and y allocated exactly, one element into their allocations, guard elements around y: no store lands outside y, and the
    gathers from x + k * stride are the gathers of the slice's own columns"""
    rp, ci, v = grid(4096, M)
    run(rp, ci, v, M, dtype, stencil_range(4096, M), off=1, seed=9)
