"""SELL-64 short rows, several slices per wavefront (>= 60,000 slices): when the slices of a wavefront's group form a RUN (all
full with one list shifted by one per row, one width, each list the continuation of the one before) a lane owns adjacent rows
and gathers them with one wide load per cell.  Every product is bit-identical to the same matrix built with sell_values = 0
(values in the cells, no uniform lists: the mapping by slice) and to the CPU oracle in the handle's order.

Double handles take that mapping; float handles (4 slices per wavefront) were measured with it, gained nothing and keep the
mapping by slice: for them the same cases check that mapping on the same inputs.

Every case runs double (2 slices per wavefront) and float (4), (alpha, beta) = (1, 0), (1.7, -0.3), (-0.75, 1.5), and two
consecutive products per handle (consecutive products sweep the groups in opposite directions).  Before anything runs on the
GPU, numpy counts from the CSR arrays alone how many groups of each input are runs: no case passes by never meeting one (or,
for the broken runs, by meeting one)."""
import functools

import numpy as np
import pytest

import test_gpu_sell_packed as S
from util import pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
P = pkg()

AB = S.AB
DTYPES = S.DTYPES
SPW_SLICES = 60000  # SELL_SHORT_SPW_SLICES
SPW = {np.float64: 2, np.float32: 4}
M = 64 * 61440  # the smallest round size with several slices per wavefront
GUARD, SENTINEL = 8, 7.0  # elements behind y (a lane's widest store is 4 elements) and what they hold


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    yield


# ---- what the CSR arrays say about slices and groups (numpy only) ------------------------------------------------------------
def row_links(rp, ci):
    """plus1[i]: row i has the length (> 0) of row i - 1 and its columns plus one; same[i]: its length and its columns"""
    rp = rp.astype(np.int64)
    lens = np.diff(rp)
    m = len(lens)
    eq = np.zeros(m, bool)
    eq[1:] = lens[1:] == lens[:-1]
    row = np.repeat(np.arange(m, dtype=np.int64), lens)
    e = np.arange(len(ci), dtype=np.int64)
    d = ci[e].astype(np.int64) - ci[np.where(eq[row], e - lens[row], e)]
    del row, e

    def rows_without(bad):
        c = np.concatenate([[0], np.cumsum(bad)])
        return c[rp[1:]] - c[rp[:-1]] == 0

    return eq & (lens > 0) & rows_without(d != 1), eq & rows_without(d != 0)


def whole_blocks(link, rows):
    """of the blocks of `rows` consecutive rows that lie inside the matrix: those whose rows 1 .. rows - 1 all link to the row before"""
    m = len(link)
    c = np.cumsum(~link)
    r0 = np.arange(0, m - rows + 1, rows)
    return c[r0 + rows - 1] - c[r0] == 0


def census(rp, ci):
    """{slices per wavefront: share of run groups}, and the count of slices with one list (shifted per row or not)"""
    m = len(rp) - 1
    plus1, same = row_links(rp, ci)
    nslices = (m + 63) // 64
    share = {}
    for spw in (2, 4):
        share[spw] = float(whole_blocks(plus1, 64 * spw).sum()) / ((nslices + spw - 1) // spw)
    return share, int((whole_blocks(plus1, 64) | whole_blocks(same, 64)).sum())


def two_values(rp, dtype):
    """a table of two, 1.5 and -0.75, in no regular pattern: every row has its own index bits"""
    lens = np.diff(rp.astype(np.int64))
    i = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    k = np.arange(len(i), dtype=np.int64) - np.repeat(rp[:-1].astype(np.int64), lens)
    h = ((i * 2654435761 + k * 40503 + 12345) >> 9) & 1
    return np.where(h == 1, 1.5, -0.75).astype(dtype)


# ---- matrices (built once, shared by the cases and the two types) ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matrix(name):
    """-> row_ptr, col_ind, columns, natural values or None, census"""
    r = np.arange(M, dtype=np.int64)
    odd = (r // 64) % 2 == 1
    every = np.ones(M, bool)
    n, v = None, None
    if name == "laplace":
        rp, ci, v = S.laplace5_grid(2048, 1920)
    elif name == "ragged":
        rp, ci, v = S.laplace5_grid(2051, 1873)
    elif name == "parity":  # every slice full, one list of 3 shifted per row; the offsets alternate with the slice
        cols = r[:, None] + np.where(odd[:, None], np.array([1, 4, 9]), np.array([0, 3, 7]))
        rp, ci, n = (3 * np.arange(M + 1)).astype(np.int32), cols.reshape(-1).astype(np.int32), M + 16
    elif name == "lastcell":  # the same, but the lists of neighbours continue each other in every cell except the last used one
        cols = r[:, None] + np.where(odd[:, None], np.array([0, 3, 8]), np.array([0, 3, 7]))
        rp, ci, n = (3 * np.arange(M + 1)).astype(np.int32), cols.reshape(-1).astype(np.int32), M + 16
    elif name == "widths":  # r + {0, 1, 2} in even slices, r + {0 .. 4} in odd ones: continuations but for the width
        rp, ci, _ = S.stencil(M, [0, 1, 2, 3, 4], [every, every, every, odd, odd])
        n = M + 16
    elif name == "mixed":  # even slices: one list for all 64 rows (mode 2); odd slices: r + {0, 1, 2, 3} (mode 1)
        _, cb, _ = S.same_list_blocks(M)
        cols = np.where(odd[:, None], r[:, None] + np.arange(4), cb.reshape(M, 4).astype(np.int64))
        rp, ci, n = (4 * np.arange(M + 1)).astype(np.int32), cols.reshape(-1).astype(np.int32), M + 16
    elif name == "diagonal":
        rp, ci, _ = S.banded(M, 0, 0)
    elif name == "tridiagonal":
        rp, ci, _ = S.banded(M, -1, 1)
    elif name == "band8":
        rp, ci, _ = S.banded(M, -4, 3)
    else:
        raise KeyError(name)
    m = len(rp) - 1
    assert (m + 63) // 64 >= SPW_SLICES and np.diff(rp).max() <= S.WMAX
    return rp, ci, (m if n is None else n), v, census(rp, ci)


# ---- products ------------------------------------------------------------------------------------------------------------------
def product(A, d, x, y0, alpha, beta, mode, off):
    """as S.product; x and y start `off` elements into their allocations, and y lies between guard elements (`off` in front,
    GUARD behind) that no store may touch"""
    xb = torch.zeros(len(x) + off, dtype=torch.from_numpy(x).dtype, device="cuda")
    yb = torch.full((off + len(y0) + GUARD,), SENTINEL, dtype=xb.dtype, device="cuda")
    xd, yd = xb[off:], yb[off:off + len(y0)]
    xd.copy_(torch.from_numpy(x)), yd.copy_(torch.from_numpy(y0))
    if off:
        assert xd.data_ptr() % 16 != 0 and yd.data_ptr() % 16 != 0
    with S.sell_values(mode):
        st = (P.dmv if A.val.dtype == np.float64 else P.smv)(P.OP_NONE, alpha, A, d, xd, beta, yd)
    assert st == 0, P.STATUS[st]
    torch.cuda.synchronize()
    assert bool((yb[:off] == SENTINEL).all()) and bool((yb[off + len(y0):] == SENTINEL).all()), "a store outside y"
    return yd.cpu().numpy()


def run_case(name, dtype, values="two", off=0):
    """-> ({slices per wavefront: share of run groups}, the packed handle's (index bits, word bytes, uniform slices))"""
    rp, ci, n, natural, (share, uniform) = matrix(name)
    m = len(rp) - 1
    if values == "natural":
        v = np.ascontiguousarray(natural, dtype=dtype)
    elif values == "two":
        v = two_values(rp, dtype)
    else:
        v = S.table_values(rp, values, dtype)
    ntab = len(np.unique(S.bits(v)))
    rng = np.random.default_rng(len(name) + off)
    x, y0 = rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, m).astype(dtype)
    A1, d1 = S.handle(rp, ci, v, 1, n=n)
    A0, d0 = S.handle(rp, ci, v, 0, n=n)
    assert A1.sell_values() == ntab and A0.sell_values() == 0
    assert A1.spmv_info().kernel in (3, 4) and A0.spmv_info().kernel == A1.spmv_info().kernel
    pb, pw, pu = A1.sell_packing()
    assert (pb, pw) == S.expected_packing(rp, ntab), (pb, pw)
    assert pu == (uniform if pb else 0) and A0.sell_packing() == (0, 0, 0), (pu, uniform)
    for alpha, beta in AB:
        ref = S.cpu_chain(v, ci, rp, x, y0, alpha, beta, None, A1.spmv_info().order)
        for lap in range(2):
            y1 = product(A1, d1, x, y0, alpha, beta, 1, off)
            S.same_bits(y1, product(A0, d0, x, y0, alpha, beta, 0, off), ("option 0", alpha, beta, lap))
            S.same_bits(y1, ref, ("oracle", alpha, beta, lap))
    return share, (pb, pw, pu)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("values", ["natural", "two"])
def test_laplacian(values, dtype):
    """2048 x 1920, 61,440 slices: a grid line is 32 slices, the first and the last of them end at the grid's edge -- 14 groups in
    16 are runs for double, 6 in 8 for float, and the others read the lists in col"""
    share, packing = run_case("laplace", dtype, values)
    assert share[SPW[dtype]] == {2: 14 / 16, 4: 6 / 8}[SPW[dtype]] and packing[:2] == (1, 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_grid(dtype):
    """2051 x 1873: lines end anywhere inside a slice, the bases x + column are odd and even, m is no multiple of 64 (a partial
    last slice, behind a last group that is not whole)"""
    share, packing = run_case("ragged", dtype)
    assert (len(matrix("ragged")[0]) - 1) % 64 != 0 and 0.5 < share[SPW[dtype]] < 1 and packing[:2] == (1, 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["parity", "lastcell", "widths"])
def test_broken_runs(name, dtype):
    """every slice is full with one list shifted per row, and no two neighbours continue each other: the offsets of a 3-cell stencil
    alternate with the slice number (in every cell; or in the last used cell only, the others continuing); or the lists do continue,
    but widths 3 and 5 alternate.  No group is a run."""
    share, packing = run_case(name, dtype)
    assert share == {2: 0.0, 4: 0.0} and packing == (1, 1, M // 64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_modes(dtype):
    """every second slice has one list for all its rows (no shift), the others a shifted stencil: all uniform, no group a run"""
    share, packing = run_case("mixed", dtype)
    assert share == {2: 0.0, 4: 0.0} and packing == (1, 1, M // 64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["diagonal", "band8"])
def test_narrow_and_wide(name, dtype):
    """widths 1 and 8: runs everywhere (but for the band's first and last slice, whose rows are clipped)"""
    share, packing = run_case(name, dtype)
    assert share[SPW[dtype]] > 0.99 and packing[:2] == (1, 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_unaligned_operands(dtype):
    """x and y one element into their allocations: 8 (4) bytes off a 16-byte boundary"""
    share, _ = run_case("laplace", dtype, "two", off=1)
    assert share[SPW[dtype]] > 0.5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ntab", [3, 256])
def test_larger_table_on_the_laplacian(ntab, dtype):
    """3 entries: 2-bit fields, 10 bits, a word of two bytes per row -- such words stay on the mapping by slice; 256 entries:
    40 bits do not fit a word, one byte per cell and no uniform lists.  Both match."""
    _, packing = run_case("laplace", dtype, ntab)
    assert packing[:2] == {3: (2, 2), 256: (0, 0)}[ntab]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,ntab", [("tridiagonal", 3), ("tridiagonal", 4), ("diagonal", 256)])
def test_one_byte_words_of_larger_tables(name, ntab, dtype):
    """a table of more than two entries (read from LDS) whose row still fits one byte: 3 fields of 2 bits, 1 field of 8 -- these
    take the runs (double)"""
    share, packing = run_case(name, dtype, ntab)
    assert share[SPW[dtype]] > 0.99 and packing[:2] == ({3: 2, 4: 2, 256: 8}[ntab], 1)
