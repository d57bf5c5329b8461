"""SELL-64 short rows: stacked periods (aoclsparse_mi355_get_sell_march).  In a periodic range whose first period is made of runs
with their words in the records, one wavefront takes G = 3 consecutive periods of its strip of slices, and where cell q of period
k + 1 is cell a(q) of period k (the alias map: 0x503 on a 5-point stencil whose period is one grid line) it loads that strip of x
once.  The kernel makes no test of its own, so before a product runs every case asserts what the getter must report for its
construction -- no case passes by missing the path -- and then compares, as test_gpu_sell_period does, the three (alpha, beta),
two consecutive products per handle (both sweep directions), bit for bit with the sell_values = 0 handle and the CPU oracle.

Double only: the float kernel (four rows per lane) is not built, and a float handle must report no stacking.  All shapes have
61,440 slices: below 60,000 a wavefront takes one slice and nothing is stacked."""
import functools

import numpy as np
import pytest

import test_gpu_sell_packed as S
import test_gpu_sell_period as T
import test_gpu_sell_records as R
from util import pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
P = pkg()
L = P.lib()

M = T.M  # 61,440 slices
NS = M // 64
NONE = (0, 0, 0, 0)
G = 3  # SELL_MARCH_G
MAP5 = 0x503  # a(0) = 2, a(2) = 4
TWO = (1.5, -0.75, -0.75, 1.5, 1.5, -0.75, 1.5, -0.75)
THREE = (1.5, -0.75, 0.5, 1.5, 1.5, -0.75, 1.5, -0.75)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    yield


def stacked_part(rng, alias=MAP5):
    """the launcher's rule restated: whole groups of G periods, and of them a whole number of workgroups (4 wavefronts of 2
    slices each)"""
    lo, hi, p, _ = rng
    groups = (hi - lo) // p // G if p else 0
    while groups > 0 and (groups * (p // 2)) % 4 != 0:
        groups -= 1
    return (lo, lo + groups * G * p, G, alias) if groups > 0 else NONE


def run(rp, ci, v, n, dtype, period, march, seed=1, off=0):
    """period: the range the construction implies, or a predicate on it; march: the stacked part, or a function of the range"""
    v = np.ascontiguousarray(v, dtype=dtype)
    x, y0 = R.operands(n, len(rp) - 1, dtype, seed)
    A1, d1 = S.handle(rp, ci, v.copy(), 1, n=n)
    A0, d0 = S.handle(rp, ci, v.copy(), 0, n=n)
    rng = A1.sell_period()
    assert period(rng) if callable(period) else rng == period, rng
    want = march(rng) if callable(march) else march
    assert A1.sell_march() == want, (A1.sell_march(), want, rng)
    assert A0.sell_march() == NONE
    R.products(A1, d1, A0, d0, x, y0, off)
    assert A1.sell_march() == want
    return rng, want


# ---- 5-point Laplacians -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gx", [4096, 256])
def test_grid_lines(gx):
    """periods of 64 and 4 slices, one grid line each: the 5-cell map.  958 and 15,358 interior lines: neither is a multiple of
    3, so periods are left over behind the stacked part, and in front of it lies line 0"""
    rp, ci, v = T.grid(gx, M)
    rng, got = run(rp, ci, v, M, np.float64, T.stencil_range(gx, M), stacked_part)
    assert got[2] == G and got[0] == rng[0] and 0 < rng[1] - got[1] and ((rng[1] - rng[0]) // rng[2]) % G != 0


def test_grid_lines_of_192_rows():
    """a period of 12 slices = four lines: no cell of one period is a cell of the next, and a plan without a map is not stacked"""
    rp, ci, v = T.grid(192, M)
    run(rp, ci, v, M, np.float64, T.stencil_range(192, M), NONE, seed=2)


def test_float_is_not_stacked():
    rp, ci, v = T.grid(4096, M)
    run(rp, ci, v, M, np.float32, T.stencil_range(4096, M), NONE, seed=3)


def test_unaligned_operands():
    """x and y one element into their allocations, guard elements around y: the G stores of a wavefront land inside y"""
    rp, ci, v = T.grid(4096, M)
    run(rp, ci, v, M, np.float64, T.stencil_range(4096, M), stacked_part, seed=4, off=1)


# ---- boundary-free stencils -------------------------------------------------------------------------------------------------------
LINE = 256
OFF5 = [0, LINE - 1, LINE, LINE + 1, 2 * LINE]  # the 5-point stencil without its boundary: period 4 slices, one line
OFF7 = [0, 4096 - LINE, 4096 - 1, 4096, 4096 + 1, 4096 + LINE, 8192]  # (-S, -P, -1, 0, 1, P, S) with P = 256, S = 4096


@functools.lru_cache(maxsize=None)
def free(offs, drop=(), tab=TWO):
    every = [np.ones(M, bool) for _ in offs]
    for (s, lane), cells in drop:
        for q in cells:
            every[q][64 * s + lane] = False
    rp, ci, _ = S.stencil(M, list(offs), every)
    return rp, ci, R.by_offset(rp, ci, list(offs), tab), M + offs[-1]


def test_boundary_free_stencil():
    """the whole matrix is the range, 15,360 periods = 5,120 groups of 3: every workgroup is a stacked one"""
    rp, ci, v, n = free(tuple(OFF5))
    run(rp, ci, v, n, np.float64, (0, NS, 4, LINE), (0, NS, G, MAP5), seed=5)


def test_a_table_of_three_values():
    """five cells of two bits do not fit a one-byte word: the records carry no words, the plan has no range, nothing is stacked"""
    rp, ci, v, n = free(tuple(OFF5), (), THREE)
    run(rp, ci, v, n, np.float64, NONE, NONE, seed=11)


def test_exception_lanes_outside_the_stacked_part():
    """lanes 17 and 40 of slice 20,002 omit cells: an exception slice, the range starts behind it at 20,004, and the slices in
    front of it run with the left-over periods in the workgroups that are not stacked"""
    s = 20002
    drop = (((s, 17), (2,)), ((s, 40), (0, 4)))
    rp, ci, v, n = free(tuple(OFF5), drop)
    run(rp, ci, v, n, np.float64, (T.up4(s + 1), NS, 4, LINE), stacked_part, seed=6)


def test_exception_lanes_in_every_period():
    """the same two lanes in the second slice of EVERY period: the records still repeat, the whole matrix is stacked, and every
    wavefront of that strip applies the two masks of its record in each of its three periods"""
    drop = tuple(x for s in range(1, NS, 4) for x in (((s, 17), (2,)), ((s, 40), (0, 4))))
    rp, ci, v, n = free(tuple(OFF5), drop)
    run(rp, ci, v, n, np.float64, (0, NS, 4, LINE), (0, NS, G, MAP5), seed=10)


def test_more_than_two_lanes_dropped():
    """three lanes of a slice omit cells: the slice reads its lists from col, is in no range, and with one such slice in each
    third of the matrix no range holds half of the slices: nothing is stacked"""
    drop = tuple(((s, lane), (1,)) for s in (20001, 41003) for lane in (5, 6, 50))
    rp, ci, v, n = free(tuple(OFF5), drop)
    run(rp, ci, v, n, np.float64, NONE, NONE, seed=7)


def test_seven_offsets():
    """(-S, -P, -1, 0, 1, P, S), period one line of P: the map is a(1) = 3, a(3) = 5, which the kernel is not built for"""
    rp, ci, v, n = free(tuple(OFF7))
    run(rp, ci, v, n, np.float64, (0, NS, 4, LINE), NONE, seed=8)


def test_value_change():
    """dupdate_values gives one row of slices 20,001 and 41,003 another value in one cell: their rows no longer share a word,
    no range holds half of the slices, nothing is stacked, and the product is the oracle's on the new values; the old values
    bring the stacked part back"""
    rp, ci, v, n = free(tuple(OFF5))
    A1, d1 = S.handle(rp, ci, np.array(v, dtype=np.float64), 1, n=n)
    A0, d0 = S.handle(rp, ci, np.array(v, dtype=np.float64), 0, n=n)
    x, y0 = R.operands(n, M, np.float64, 9)
    assert A1.sell_march() == (0, NS, G, MAP5)
    R.products(A1, d1, A0, d0, x, y0)
    v2 = np.array(v, dtype=np.float64)
    for s in (20001, 41003):
        e = rp[64 * s + 5] + 1
        v2[e] = 1.5 if v2[e] == -0.75 else -0.75
    for vals, want in ((v2, NONE), (np.array(v, dtype=np.float64), (0, NS, G, MAP5))):
        for A in (A1, A0):
            assert L.aoclsparse_dupdate_values(A.h, len(vals), P._ptr(vals)) == 0
        R.products(A1, d1, A0, d0, x, y0)
        assert A1.sell_march() == want and A1.sell_values() == 2
