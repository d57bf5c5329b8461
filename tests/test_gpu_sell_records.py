"""SELL-64 short rows: what a slice record says beyond offsets, width and mode (aoclsparse_mi355_get_sell_records).  On a copy
with uniform column lists and one-byte packed words, a full slice with one list whose 64 rows share ONE word carries the word in
its record (the kernel then reads no word for it), and a slice that is "one list shifted by lane" in which at most two lanes omit
cells (the first and last slice of a stencil's grid line) is flagged as a shifted slice with exception lanes instead of reading
its columns from the lists.

Every case runs double (2 slices per wavefront from 60,000 slices on) and float (4), (alpha, beta) = (1, 0), (1.7, -0.3),
(-0.75, 1.5), two consecutive products per handle, and compares every result bit for bit with the sell_values = 0 handle (values
in the cells, no records read beyond today's) and with the CPU oracle in the handle's order.  Before anything runs on the GPU,
numpy counts from the CSR arrays alone how many slices must carry a uniform word and how many an exception; get_sell_records
must return exactly those counts, so no case passes by never meeting the path."""
import functools

import numpy as np
import pytest

import test_gpu_sell_packed as S
import test_gpu_sell_wide as W
from util import pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
P = pkg()
L = P.lib()

AB = S.AB
DTYPES = S.DTYPES
M1 = 64 * S.MIN_SLICES  # one slice per wavefront
M = W.M  # several slices per wavefront (61,440 slices)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    yield


# ---- what the CSR arrays say about the records (numpy only) -------------------------------------------------------------------
def census(rp, ci, v, n):
    """-> (slices whose record must hold a uniform word, those among them that must be exception slices), by the documented rule:
    a FULL slice of mode 1 / 2 with one word; or a full slice of another kind, of width >= 1, in which -- B being the columns of
    the lowest lane of full width minus that lane -- every B[q] >= 0 and B[q] + 63 < n, every row's columns are an in-order
    subsequence of B + lane, at most two lanes are shorter than the width, and the rows' table indices at the canonical cell
    positions agree.  (0, 0) when a row's word needs more than one byte."""
    rp64 = rp.astype(np.int64)
    lens = np.diff(rp64)
    m = len(lens)
    ns = m // 64  # full slices
    pat, idx = np.unique(S.bits(np.ascontiguousarray(v, dtype=np.float64)), return_inverse=True)
    pb = next(b for b in (1, 2, 4, 8) if (1 << b) >= len(pat))
    if int(lens.max()) * pb > 8:
        return 0, 0
    row = np.repeat(np.arange(m, dtype=np.int64), lens)
    k = np.arange(len(ci), dtype=np.int64) - rp64[row]
    word = np.bincount(row, weights=(idx.astype(np.int64) << (k * pb)).astype(np.float64), minlength=m).astype(np.int64)
    del row, k
    plus1, same = W.row_links(rp, ci)
    one_list = (W.whole_blocks(plus1, 64) | W.whole_blocks(same, 64))[:ns]
    w2 = word[:64 * ns].reshape(ns, 64)
    uniform = one_list & (w2 == w2[:, :1]).all(axis=1)
    l2 = lens[:64 * ns].reshape(ns, 64)
    width = l2.max(axis=1)
    cand = np.nonzero(~one_list & (width >= 1) & ((l2 < width[:, None]).sum(axis=1) <= 2))[0]
    field = (1 << pb) - 1

    def exception(s):
        r0, w = 64 * int(s), int(width[s])
        ln = l2[s]
        c = int(np.argmax(ln == w))
        b = ci[rp64[r0 + c]:rp64[r0 + c] + w].astype(np.int64) - c
        if b.min() < 0 or b.max() + 63 >= n:
            return False
        full = np.nonzero(ln == w)[0]
        cols = ci[rp64[r0 + full][:, None] + np.arange(w)].astype(np.int64) - full[:, None]
        if not (cols == b).all() or not (word[r0 + full] == word[r0 + c]).all():
            return False
        for lane in np.nonzero(ln < w)[0]:
            own, p = ci[rp64[r0 + lane]:rp64[r0 + lane + 1]].astype(np.int64), 0
            for q in range(w):
                if p < len(own) and own[p] == b[q] + lane:
                    if (word[r0 + lane] >> (p * pb)) & field != (word[r0 + c] >> (q * pb)) & field:
                        return False
                    p += 1
            if p != len(own):
                return False
        return True

    ex = sum(exception(s) for s in cand)
    return int(uniform.sum()) + ex, ex


def positional(rp, tab=(1.5, -0.75, -0.75, 1.5, 1.5, -0.75, 1.5, -0.75)):
    """the value of a cell is a function of its position in the row alone: one word for all rows of one length"""
    rp64 = rp.astype(np.int64)
    lens = np.diff(rp64)
    k = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(rp64[:-1], lens)
    return np.array(tab)[k]


def by_offset(rp, ci, offsets, tab=(1.5, -0.75, -0.75, 1.5, 1.5, -0.75, 1.5, -0.75)):
    """the value of a cell is a function of column - row: rows that omit a cell keep the values of the cells they have"""
    lens = np.diff(rp.astype(np.int64))
    off = ci.astype(np.int64) - np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    return np.array(tab)[np.searchsorted(np.array(offsets), off)]


# ---- products ------------------------------------------------------------------------------------------------------------------
def same_class(got, ref, what):
    """bits where the oracle is finite, NaN / +Inf / -Inf where it is not"""
    fin = np.isfinite(ref)
    assert np.array_equal(S.bits(got[fin]), S.bits(ref[fin])), (what, "finite rows")
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), (what, "class")


def products(A1, d1, A0, d0, x, y0, off=0, finite_rows=None):
    """the three (alpha, beta), two products each: the handle with records against the sell_values = 0 handle and the oracle (on
    the handle's CURRENT values); finite_rows: rows that must come out finite although x holds Inf / NaN"""
    for alpha, beta in AB:
        ref = None
        for lap in range(2):
            y1 = W.product(A1, d1, x, y0, alpha, beta, 1, off)
            if ref is None:  # (after the first product: a rebuilt plan reports its order)
                ref = S.cpu_chain(A1.val, A1.col_ind, A1.row_ptr, x, y0, alpha, beta, None, A1.spmv_info().order)
            y0p = W.product(A0, d0, x, y0, alpha, beta, 0, off)
            if finite_rows is None:
                S.same_bits(y1, y0p, ("option 0", alpha, beta, lap))
                S.same_bits(y1, ref, ("oracle", alpha, beta, lap))
            else:
                assert np.isfinite(y1[finite_rows]).all() and not np.isfinite(y1).all()
                S.same_bits(y1[finite_rows], ref[finite_rows], ("oracle, exception rows", alpha, beta, lap))
                same_class(y1, ref, ("oracle", alpha, beta, lap))
                same_class(y1, y0p, ("option 0", alpha, beta, lap))


def operands(n, m, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, n).astype(dtype), rng.uniform(-1, 1, m).astype(dtype)


def run_case(rp, ci, v, n, dtype, counts, off=0, seed=1):
    """counts: census(rp, ci, v, n), taken before this call"""
    v = np.ascontiguousarray(v, dtype=dtype)
    m = len(rp) - 1
    x, y0 = operands(n, m, dtype, seed)
    A1, d1 = S.handle(rp, ci, v.copy(), 1, n=n)
    A0, d0 = S.handle(rp, ci, v.copy(), 0, n=n)
    assert A1.sell_records() == counts and A0.sell_records() == (0, 0), (A1.sell_records(), counts)
    products(A1, d1, A0, d0, x, y0, off)
    assert A1.sell_records() == counts
    return A1


# ---- matrices (built and counted once, shared by the two types) -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def laplace(gx, gy):
    rp, ci, v = S.laplace5_grid(gx, gy)
    return rp, ci, v, census(rp, ci, v, gx * gy)


@functools.lru_cache(maxsize=None)
def big_laplace(name, values):
    rp, ci, n, natural, _ = W.matrix(name)
    v = natural if values == "natural" else W.two_values(rp, np.float64)
    return rp, ci, n, v, census(rp, ci, v, n)


OFFS = [0, 3, 7, 12]


def shifted_stencil(m, drop):
    """rows r with columns r + OFFS, every slice full and shifted by one per row; drop = {(slice, lane): [cells the row omits]}"""
    every = [np.ones(m, bool) for _ in OFFS]
    for (s, lane), cells in drop.items():
        for q in cells:
            every[q][64 * s + lane] = False
    rp, ci, _ = S.stencil(m, OFFS, every)
    return rp, ci


@functools.lru_cache(maxsize=None)
def limits():
    """slice 10: three short lanes; slice 20: a short row (3 of 4 cells) one of whose columns is off the canonical list; slice 30:
    two short lanes, one of them with two cells -- flagged (the positive control); the rest of the matrix: shifted slices"""
    rp, ci = shifted_stencil(M1, {(10, 5): [1], (10, 9): [2], (10, 20): [0], (20, 33): [3], (30, 0): [1], (30, 63): [0, 3]})
    ci = ci.copy()
    ci[rp[64 * 20 + 33] + 1] += 1  # r + 3 -> r + 4: ascending still, and not in B + lane
    v = by_offset(rp, np.where(np.arange(len(ci)) == rp[64 * 20 + 33] + 1, ci - 1, ci), OFFS)
    return rp, ci, M1 + 16, v, census(rp, ci, v, M1 + 16)


@functools.lru_cache(maxsize=None)
def clipped():
    """columns r, r + 1 with n == m: the last row omits column m, one past the end -- its slice cannot gather there"""
    rp, ci, v = S.banded(M1, 0, 1)
    return rp, ci, M1, v, census(rp, ci, v, M1)


@functools.lru_cache(maxsize=None)
def mixed(name):
    r = np.arange(M, dtype=np.int64)
    odd = (r // 64) % 2 == 1
    if name == "alternate_words":  # runs everywhere; even slices: one word, odd slices: every row its own bits
        rp, ci = shifted_stencil(M, {})
        v = np.where(np.repeat(odd, 4), W.two_values(rp, np.float64), positional(rp))
    else:  # "exception_and_one_list": even slices one list for all 64 rows (mode 2), odd slices r + {0 .. 3}; in every eighth of them lane 7 omits cell 2
        _, cb, _ = S.same_list_blocks(M)
        cols = np.where(odd[:, None], r[:, None] + np.arange(4), cb.reshape(M, 4).astype(np.int64))
        keep = np.ones((M, 4), bool)
        keep[odd & (r % 64 == 7) & ((r // 128) % 8 == 0), 2] = False
        rp = np.zeros(M + 1, np.int64)
        rp[1:] = np.cumsum(keep.sum(axis=1))
        rp, ci = rp.astype(np.int32), cols[keep].astype(np.int32)
        v = np.array([1.5, -0.75, -0.75, 1.5])[np.broadcast_to(np.arange(4), (M, 4))[keep]]
    return rp, ci, M + 16, v, census(rp, ci, v, M + 16)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_laplacian_several_slices_per_wavefront(dtype):
    """2048 x 1920, natural values: every slice but the first and the last has one word; the first and last slice of every grid
    line (but those two, whose canonical list would point outside x) are exception slices"""
    rp, ci, n, v, counts = big_laplace("laplace", "natural")
    assert counts == (61438, 3838)
    run_case(rp, ci, v, n, dtype, counts)


@pytest.mark.parametrize("dtype", DTYPES)
def test_laplacian_one_slice_per_wavefront(dtype):
    rp, ci, v, counts = laplace(1024, 1024)
    assert counts == (16382, 2046)
    run_case(rp, ci, v, 1024 * 1024, dtype, counts, seed=2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_grid(dtype):
    """2051 x 1873: the ends of the grid lines fall inside a slice, two exception lanes per slice (the last point of a line and
    the first of the next); the slices that hold the ends of the first and the last line have more than two short lanes"""
    rp, ci, n, v, counts = big_laplace("ragged", "natural")
    assert counts == (58121 + 1899, 1899)
    run_case(rp, ci, v, n, dtype, counts, seed=3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_with_their_own_bits(dtype):
    """two values in no regular pattern: no slice has one word, nothing is flagged, the rows' words drive the product"""
    rp, ci, n, v, counts = big_laplace("laplace", "two")
    assert counts == (0, 0)
    run_case(rp, ci, v, n, dtype, counts, seed=4)


def off_pattern_rows(gx):
    """(a row of a mode-1 slice, a full-width row of an exception slice) of the gx x gx Laplacian, and their diagonal columns"""
    ra = 5 * gx + 64 * 3 + 10  # line 5, fourth slice of the line
    rb = 9 * gx + 20  # line 9, first slice (its lane 0 omits the west cell)
    return ra, rb


@pytest.mark.parametrize("dtype", DTYPES)
def test_off_pattern_value_at_build_time(dtype):
    """-1 instead of 4 on the diagonal of one row of a mode-1 slice and of one row of an exception slice (the table keeps its two
    entries): both counts drop by exactly those slices"""
    gx = 1024
    rp, ci, v, counts = laplace(gx, gx)
    ra, rb = off_pattern_rows(gx)
    v = v.copy()
    for r in (ra, rb):
        e = rp[r] + int(np.nonzero(ci[rp[r]:rp[r + 1]] == r)[0][0])
        assert v[e] == 4.0
        v[e] = -1.0
    changed = census(rp, ci, v, gx * gx)
    assert changed == (counts[0] - 2, counts[1] - 1)
    run_case(rp, ci, v, gx * gx, dtype, changed, seed=5)


@pytest.mark.parametrize("dtype", DTYPES)
def test_off_pattern_value_after_optimize(dtype):
    """the same through ?set_value and ?update_values: flagged before, dropped after, restored with the value"""
    gx = 1024
    m = gx * gx
    rp, ci, v, counts = laplace(gx, gx)
    ra, rb = off_pattern_rows(gx)
    dbl = dtype == np.float64
    # (a handle aliases its value array and ?set_value writes into it: each handle gets its own copy, the shared one stays)
    A1, d1 = S.handle(rp, ci, np.array(v, dtype=dtype), 1)
    A0, d0 = S.handle(rp, ci, np.array(v, dtype=dtype), 0)
    x, y0 = operands(m, m, dtype, 6)
    assert A1.sell_records() == counts
    products(A1, d1, A0, d0, x, y0)
    # one row of a mode-1 slice, by ?set_value
    for A in (A1, A0):
        assert (L.aoclsparse_dset_value if dbl else L.aoclsparse_sset_value)(A.h, ra, ra, -1.0) == 0
    step1 = census(rp, ci, A1.val, m)
    assert step1 == (counts[0] - 1, counts[1]) and A1.val[rp[ra] + 2] == -1.0
    products(A1, d1, A0, d0, x, y0)
    assert A1.sell_records() == step1 and A1.sell_values() == 2
    # ... and one row of an exception slice, by ?update_values
    v2 = A1.val.copy()
    v2[rp[rb] + 2] = -1.0
    for A in (A1, A0):
        assert (L.aoclsparse_dupdate_values if dbl else L.aoclsparse_supdate_values)(A.h, len(v2), P._ptr(v2)) == 0
    step2 = census(rp, ci, A1.val, m)
    assert step2 == (counts[0] - 2, counts[1] - 1)
    products(A1, d1, A0, d0, x, y0)
    assert A1.sell_records() == step2
    # the values come back: so do the flags
    v3 = np.array(v, dtype=dtype)
    assert census(rp, ci, v3, m) == counts
    for A in (A1, A0):
        assert (L.aoclsparse_dupdate_values if dbl else L.aoclsparse_supdate_values)(A.h, len(v3), P._ptr(v3)) == 0
    products(A1, d1, A0, d0, x, y0)
    assert A1.sell_records() == counts


@pytest.mark.parametrize("dtype", DTYPES)
def test_limits_of_the_exception_rule(dtype):
    """three short lanes: not flagged; a short row off the canonical list: not flagged; two short lanes, one with two cells:
    flagged.  Those two slices have no one list either, so they carry no uniform word."""
    rp, ci, n, v, counts = limits()
    assert counts == (S.MIN_SLICES - 2, 1)
    run_case(rp, ci, v, n, dtype, counts, seed=7)


@pytest.mark.parametrize("dtype", DTYPES)
def test_absent_cell_one_past_the_end(dtype):
    """n == m: the last slice is a shifted list whose last lane omits column m; B + 63 = n is outside x, the slice stays as it is"""
    rp, ci, n, v, counts = clipped()
    assert counts == (S.MIN_SLICES - 1, 0)
    run_case(rp, ci, v, n, dtype, counts, seed=8)


@pytest.mark.parametrize("dtype", DTYPES)
def test_words_of_two_bytes(dtype):
    """4 table entries on 5 cells: 10 bits per row -- no record is annotated"""
    rp, ci, _, _ = laplace(1024, 1024)
    v = S.table_values(rp, 4, dtype)
    counts = census(rp, ci, v, 1024 * 1024)
    assert counts == (0, 0)
    A1 = run_case(rp, ci, v, 1024 * 1024, dtype, counts, seed=9)
    assert A1.sell_packing()[:2] == (2, 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["alternate_words", "exception_and_one_list"])
def test_mixed_groups(name, dtype):
    """in every group of 2 (double) and of 4 (float) slices: slices with and without a uniform word (all runs: the words of the
    others are read, by the mapping of a run for double); exception slices next to mode-2 slices (no runs: the mapping by slice)"""
    rp, ci, n, v, counts = mixed(name)
    assert counts == {"alternate_words": (M // 128, 0), "exception_and_one_list": (M // 64, M // 1024)}[name]
    run_case(rp, ci, v, n, dtype, counts, seed=10)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_nonfinite_x_at_omitted_columns(bad, dtype):
    """x = Inf (NaN) at the west neighbours that the first rows of the even grid lines omit: those rows read none of them and
    come out finite and bit-equal; nothing of an absent cell's gather reaches a chain, not even as 0 x Inf"""
    gx, gy = 2048, 1920
    rp, ci, n, v, counts = big_laplace("laplace", "natural")
    assert counts[1] > 0
    v = np.ascontiguousarray(v, dtype=dtype)
    rows = gx * np.arange(2, gy, 2, dtype=np.int64)  # first rows of lines 2, 4, ...: lane 0 of an exception slice
    x, y0 = operands(n, gx * gy, dtype, 11)
    x[rows - 1] = bad
    for r in rows[:3]:
        assert (r - 1) not in ci[rp[r]:rp[r + 1]] and np.isfinite(x[ci[rp[r]:rp[r + 1]]]).all()
    A1, d1 = S.handle(rp, ci, v.copy(), 1, n=n)
    A0, d0 = S.handle(rp, ci, v.copy(), 0, n=n)
    assert A1.sell_records() == counts
    products(A1, d1, A0, d0, x, y0, finite_rows=rows)


@pytest.mark.parametrize("dtype", DTYPES)
def test_unaligned_operands(dtype):
    """x and y one element into their allocations, guard elements around y: no store lands outside y"""
    rp, ci, n, v, counts = big_laplace("laplace", "natural")
    run_case(rp, ci, v, n, dtype, counts, off=1, seed=12)
