"""CPU tier of the periodic range of a SELL-64 copy's slice records and uniform lists (aoclsparse_mi355_sell_find_period: the
host function that build_sell runs on a copy of the device arrays, here on synthetic ones; no device).

The expected value of every case comes from `brute`, a numpy restatement of the rule (csrc/sell_period.cpp) that tries EVERY
period that is a multiple of 4 in ascending order with one full comparison each, instead of the few candidates the library picks.
A slice is eligible when its mode is 1 or 2 or it carries the exception flag, its width is at least 1 and its first list entry is
a column (>= 0); slice s matches
slice s - p when both are eligible, their wsm words are equal, with the word flag bits 0-7 of cell_lo are equal, with the
exception flag all of cell_lo and bits 0-7 of hi are equal, and below the width every column is the other's + 64 p (-1 equals
-1).  A range [lo, hi): all eligible, [lo + p, hi) all matching, lo / hi cut to multiples of 4, at least two periods and half of
the slices long; the smallest such p <= cap, its range, stride 64 p.  The library compares at most 8 pairs of slices per slice
and reports no range when that does not suffice: the last cases build the shapes that would cost it a pass per period."""
import numpy as np
import pytest

from util import pkg

P = pkg()

UWORD, EXCEPT = 1 << 24, 1 << 25
CAP = 64


def brute(rec, lists, cap):
    rec, lists = np.asarray(rec, np.uint32), np.asarray(lists, np.int64)
    n = len(rec)
    wsm = rec[:, 3].astype(np.int64)
    w, mode = wsm & 0xff, (wsm >> 16) & 0xff
    ex, uw = (wsm & EXCEPT) != 0, (wsm & UWORD) != 0
    el = (ex | (mode == 1) | (mode == 2)) & (w >= 1) & (lists[:, 0] >= 0)
    for p in range(4, min(cap, n // 2) + 1, 4):
        a, b = slice(p, n), slice(0, n - p)
        ok = el[a] & el[b] & (wsm[a] == wsm[b])
        ok &= ~uw[a] | ((rec[a, 0] & 0xff) == (rec[b, 0] & 0xff))
        ok &= ~ex[a] | ((rec[a, 0] == rec[b, 0]) & ((rec[a, 2] & 0xff) == (rec[b, 2] & 0xff)))
        for q in range(8):
            ca, cb = lists[a, q], lists[b, q]
            ok &= (q >= w[a]) | np.where((ca < 0) | (cb < 0), (ca < 0) & (cb < 0), ca == cb + 64 * p)
        best = (0, 0)
        s = 0
        while s < len(ok):  # ok[s]: slice s + p matches slice s
            if not ok[s]:
                s += 1
                continue
            e = s
            while e < len(ok) and ok[e]:
                e += 1
            lo, hi = (s + 3) // 4 * 4, (e + p) // 4 * 4  # the matches [s + p, e + p) give the range [s, e + p)
            if hi - lo >= 2 * p and 2 * (hi - lo) >= n and hi - lo > best[1] - best[0]:
                best = (lo, hi)
            s = e
        if best[1] > best[0]:
            return best + (p, 64 * p)
    return 0, 0, 0, 0


def pattern(n, period, width=5, mode=1, seed=0):
    """n slices repeating `period` distinct slices: mode-1 / 2 records with their word in the record, lists that move by 64 per
    slice plus a per-phase offset (so that no shorter period exists)"""
    rng = np.random.default_rng(seed)
    phase = np.arange(n) % period
    rec = np.zeros((n, 4), np.uint32)
    rec[:, 0] = (0x10 + phase).astype(np.uint32)  # the word (bits 0-7)
    rec[:, 1] = rng.integers(0, 1 << 31, n)  # col_lo: never compared
    rec[:, 2] = rng.integers(0, 1 << 16, n) << 16  # hi bits 16-31: never compared
    rec[:, 3] = width | 1 << 8 | mode << 16 | UWORD
    off = np.sort(rng.choice(np.arange(1, 50), size=(period, width), replace=False if period * width <= 49 else True), axis=1)
    lists = np.full((n, 8), -1, np.int32)
    lists[:, :width] = 1000 + 64 * np.arange(n)[:, None] + off[phase]
    return rec, lists


WORK = 8  # SELL_PERIOD_WORK


def check(rec, lists, cap=CAP, expect=None):
    want = brute(rec, lists, cap)
    if expect is not None:
        assert want == expect, ("the brute-force rule itself", want, expect)
    got, work = P.sell_find_period(rec, lists, cap, work=True)
    assert got == want and 0 <= work <= WORK * len(rec), (got, work)
    return want


def test_one_pattern_repeated():
    rec, lists = pattern(256, 12)
    check(rec, lists, expect=(0, 256, 12, 768))


@pytest.mark.parametrize("period, reported", [(1, 4), (2, 4), (5, 20)])
def test_short_periods_come_out_as_multiples_of_four(period, reported):
    rec, lists = pattern(240, period, seed=period)
    check(rec, lists, expect=(0, 240, reported, 64 * reported))


def test_head_and_tail_that_do_not_repeat():
    rec, lists = pattern(300, 8)
    lists[:21, 0] += 7  # the head: 21 slices, the range starts at the next multiple of 4
    lists[-10:, 1] -= 1
    check(rec, lists, expect=(24, 288, 8, 512))
    rec[:21, 3] = 5 | 64 << 8 | 3 << 16  # ... or a head that is not eligible at all
    check(rec, lists, expect=(24, 288, 8, 512))


@pytest.mark.parametrize("what", ["wsm", "word", "exception_lane", "exception_hi", "column", "unused_entry", "hi_other_bits"])
def test_one_slice_in_the_middle_differs(what):
    """slice 101 of 400 breaks the period of 8 (or, for the fields that do not count, does not): the longer side is the range"""
    rec, lists = pattern(400, 8)
    ex = np.arange(400) % 8 == 3  # exception slices: mode 0 for every other reader, lanes and masks in cell_lo and hi
    rec[ex, 3] = 5 | 2 << 8 | 0 << 16 | UWORD | EXCEPT
    rec[ex, 0] = 0x15 | 0 << 8 | 0x1d << 16 | 0xff << 24
    rec[ex, 2] = (rec[ex, 2] & 0xffff0000) | 0x1f
    s, breaks = 101, True
    if what == "wsm":
        rec[s, 3] = 4 | 1 << 8 | 1 << 16 | UWORD
    elif what == "word":
        rec[s, 0] ^= 0x4
    elif what == "exception_lane":
        s = 99
        rec[s, 0] ^= 63 << 8
    elif what == "exception_hi":
        s = 99
        rec[s, 2] ^= 0x10
    elif what == "column":
        lists[s, 4] += 1
    elif what == "unused_entry":  # beyond the width: not compared
        lists[s, 6], breaks = 12345, False
    else:  # bits 8-31 of hi of a slice without the exception flag, col_lo: not compared
        rec[s, 2] ^= 0xff00
        rec[s, 1] ^= 0xffff
        breaks = False
    assert ex[99] and not ex[101]
    # s does not match s - 8 and s + 8 does not match s: the matches go on from s + 9, the range from s + 1, cut to a multiple of 4
    check(rec, lists, expect=((s + 1 + 3) // 4 * 4, 400, 8, 512) if breaks else (0, 400, 8, 512))


def test_a_period_above_the_cap():
    rec, lists = pattern(400, 68)
    assert brute(rec, lists, 68) == (0, 400, 68, 64 * 68)
    check(rec, lists, cap=68)
    check(rec, lists, cap=64, expect=(0, 0, 0, 0))


def test_a_range_under_half():
    noise = np.cumsum(np.random.default_rng(3).integers(1, 5, 400)).astype(np.int32)  # ascending: no two slices get the same
    rec, lists = pattern(400, 8)
    lists[192:, 2] += noise[192:]  # nothing repeats from slice 192 on
    check(rec, lists, expect=(0, 0, 0, 0))
    rec, lists = pattern(400, 8)
    lists[200:, 2] += noise[200:]  # exactly half is enough ...
    check(rec, lists, expect=(0, 200, 8, 512))
    lists[199, 2] += 1  # ... one slice less is not
    check(rec, lists, expect=(0, 0, 0, 0))


@pytest.mark.parametrize("mode", [0, 3])
def test_a_slice_that_reads_the_lists_in_col(mode):
    """mode 0 / 3 without the exception flag inside an otherwise periodic stretch: not in any range, although it repeats"""
    rec, lists = pattern(400, 8)
    rec[77, 3] = 5 | 3 << 8 | mode << 16
    rec[85, 3] = 5 | 3 << 8 | mode << 16  # (its successor one period on is the same record)
    lists[77], lists[85] = -1, -1
    check(rec, lists, expect=(88, 400, 8, 512))


def test_a_slice_of_width_zero():
    """an empty slice has no first column that would vouch for the moved base of the gathers: not eligible"""
    rec, lists = pattern(400, 8)
    rec[40::8, 3] = 0 | 1 << 8 | 2 << 16
    lists[40::8] = -1
    check(rec, lists, expect=(0, 0, 0, 0))


@pytest.mark.parametrize("n", [253, 254, 255, 257])
def test_slice_counts_that_are_no_multiple_of_four(n):
    rec, lists = pattern(n, 12)
    check(rec, lists, expect=(0, n // 4 * 4, 12, 768))


def test_mode_two_lists_and_minus_one_below_the_width():
    rec, lists = pattern(256, 4, width=3, mode=2)
    lists[:, 1] = -1  # (-1 equals -1)
    check(rec, lists, expect=(0, 256, 4, 256))
    lists[130, 1] = 5
    check(rec, lists, expect=(0, 128, 4, 256))


def test_a_break_in_the_middle_leaves_one_half():
    """slice t breaks the period: the ranges are [0, t) and [t + 1, n) -- disjoint, so at most one of them holds half"""
    rec, lists = pattern(400, 8)
    lists[200, 0] += 1  # [0, 200) and [204, 400): 200 and 196 of 400
    check(rec, lists, expect=(0, 200, 8, 512))
    rec, lists = pattern(404, 8)
    lists[200, 0] += 1  # [0, 200) and [204, 404): the first of two equally long ones
    check(rec, lists, expect=(0, 0, 0, 0))
    rec, lists = pattern(401, 8)
    lists[197, 0] += 1  # [0, 196) and [200, 400)
    check(rec, lists, expect=(0, 0, 0, 0))
    lists[197, 0] -= 1
    lists[195, 0] += 1  # [0, 192) and [196, 400): 204 of 401
    check(rec, lists, expect=(196, 400, 8, 512))


def test_degenerate_sizes():
    rec, lists = pattern(7, 4)
    assert P.sell_find_period(rec, lists, CAP) == (0, 0, 0, 0)
    rec, lists = pattern(8, 4)
    check(rec, lists, expect=(0, 8, 4, 256))
    assert P.sell_find_period(rec, lists, 3) == (0, 0, 0, 0)


def test_random_breaks_agree_with_the_rule():
    rng = np.random.default_rng(5)
    for trial in range(40):
        n, period = int(rng.integers(64, 500)), int(rng.choice([1, 2, 3, 4, 6, 8, 12, 20, 36]))
        rec, lists = pattern(n, period, seed=trial)
        for s in rng.integers(0, n, int(rng.integers(0, 4))):
            lists[s, int(rng.integers(0, 5))] += 1
        check(rec, lists)


def test_a_first_entry_that_is_no_column():
    """-1 in cell 0 below the width: nothing vouches for the moved base of the gathers, the slice is not eligible"""
    rec, lists = pattern(400, 8)
    lists[100, 0] = lists[108, 0] = -1
    check(rec, lists, expect=(112, 400, 8, 512))


def embedded(n, lo, hi, outside):
    """slices [lo, hi) repeat with EVERY period (one record, lists moving by 64 per slice); the others are mode-3 slices
    (`outside` = "lists in col") or eligible slices that repeat with no period ("noise")"""
    rec, lists = pattern(n, 1)
    out = np.ones(n, bool)
    out[lo:hi] = False
    if outside == "lists in col":
        rec[out, 3] = 5 | 64 << 8 | 3 << 16
        lists[out] = -1
    else:
        lists[out, 2] += np.cumsum(np.random.default_rng(9).integers(1, 5, n)).astype(np.int32)[out]
    return rec, lists


@pytest.mark.parametrize("outside", ["lists in col", "noise"])
@pytest.mark.parametrize("lo, hi", [(0.30, 0.70), (0.28, 0.76), (0.40, 0.60)])
def test_a_stencil_embedded_in_other_slices_costs_a_bounded_search(lo, hi, outside):
    """under half of the slices repeat, around the centre, with every period up to the cap: each period passes the local test
    and would fail a full pass.  Nothing is reported, and the comparisons stay within 8 per slice (in slices that read the lists
    in col the search ends before its first comparison)"""
    n = 20000
    rec, lists = embedded(n, int(lo * n), int(hi * n), outside)
    assert brute(rec, lists, 64) == (0, 0, 0, 0)  # (the rule itself, at a cap the restatement can afford)
    got, work = P.sell_find_period(rec, lists, 4096, work=True)
    assert got == (0, 0, 0, 0) and work <= WORK * n
    if outside == "lists in col":
        assert work == 0


def test_a_clean_stencil_is_far_inside_the_bound():
    """40 grid lines of 64 slices, the first and last slice of a line exception slices: the periods 4 .. 60 fail within a line,
    64 gets its pass"""
    n = 64 * 40
    rec, lists = pattern(n, 1)
    ends = (np.arange(n) % 64 == 0) | (np.arange(n) % 64 == 63)
    rec[ends, 3] = 5 | 2 << 8 | UWORD | EXCEPT
    rec[ends, 0] = 0x15 | 0x1d << 16 | 0xff << 24
    rec[ends, 2] |= 0x1f
    rec[:64, 3] = (rec[:64, 3] & ~np.uint32(0xff)) | 4
    rec[-64:, 3] = (rec[-64:, 3] & ~np.uint32(0xff)) | 4
    assert brute(rec, lists, 64) == (64, n - 64, 64, 4096)
    got, work = P.sell_find_period(rec, lists, 4096, work=True)
    assert got == (64, n - 64, 64, 4096) and work <= 2 * n
