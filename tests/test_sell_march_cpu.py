"""The two plan rules behind the stacked periods of the short-row SELL-64 kernel (sell_period.cpp: sell_find_march) and the
launcher's rule on them (internal.hpp: sell_march_rule), on hand-built slice records and uniform lists -- host only -- against a
brute-force restatement.  The kernel that relies on them makes no test of its own."""
import numpy as np
import pytest

from util import pkg

P = pkg()

UWORD, EXCEPT = 1 << 24, 1 << 25
SHIFT, ONE = 1, 2  # slice modes
NONE = (0, 0, 0, 0)
LINE = 256
OFF5 = [0, LINE - 1, LINE, LINE + 1, 2 * LINE]
OFF7 = [0, 4096 - LINE, 4096 - 1, 4096, 4096 + 1, 4096 + LINE, 8192]


def stencil(n, offs, mode=SHIFT, flags=UWORD):
    """n slices of rows r + offs: records (n, 4) {cell_lo, col_lo, hi, wsm}, lists (n, 8)"""
    rec = np.zeros((n, 4), np.uint32)
    rec[:, 3] = len(offs) | 64 << 8 | mode << 16 | flags
    lists = np.full((n, 8), -1, np.int32)
    lists[:, :len(offs)] = 64 * np.arange(n)[:, None] + np.array(offs)[None, :]
    return rec, lists


def brute(rec, lists, rng, word_bytes=1):
    lo, hi, p, stride = rng
    rec, lists = rec.astype(np.int64), lists.astype(np.int64)

    def shifted(s):  # the record's word with the mode of an exception slice read as "shifted"
        w = rec[s, 3]
        return (w & 0xff00ffff) | SHIFT << 16 if w & EXCEPT else w

    stack = word_bytes == 1
    for g in range(lo, lo + p, 4):
        w0 = shifted(g) & 0xff
        for u in range(4):
            e = shifted(g + u)
            stack = stack and (e >> 16) & 0xff == SHIFT and e & 0xff == w0 and w0 >= 1 and bool(rec[g + u, 3] & UWORD)
            stack = stack and all(lists[g + u, q] == lists[g, q] + 64 * u for q in range(w0))
    amap = 0
    for q in range(8):
        for r in range(8):
            if r != q and not (amap >> 4 * q) & 15 and all(
                    q < (rec[s, 3] & 0xff) and r < (rec[s, 3] & 0xff) and lists[s, q] >= 0 and lists[s, r] >= 0
                    and lists[s, r] == lists[s, q] + stride for s in range(lo, lo + p)):
                amap |= (r + 1) << 4 * q
    return int(stack), amap


def check(rec, lists, rng, expect, word_bytes=1):
    got = P.sell_find_march(rec, lists, rng, word_bytes)
    assert got == brute(rec, lists, rng, word_bytes) == expect, (got, expect)


def test_five_and_seven_cell_maps():
    for offs, amap in ((OFF5, 0x503), (OFF7, 0x6040)):
        rec, lists = stencil(64, offs)
        assert P.sell_find_period(rec, lists, 4096) == (0, 64, 4, LINE)
        check(rec, lists, (0, 64, 4, LINE), (1, amap))
    # a period of 16 slices on the same lists: the columns one period on are four lines on, no cell aliases
    rec, lists = stencil(64, OFF5)
    check(rec, lists, (0, 64, 16, 4 * LINE), (1, 0))


def test_only_the_first_period_is_read():
    rec, lists = stencil(64, OFF5)
    rec[40, 3] &= ~np.uint32(UWORD)
    lists[41, 2] += 1
    check(rec, lists, (8, 64, 4, LINE), (1, 0x503))
    check(rec, lists, (40, 64, 4, LINE), (0, 0))  # (in slice 41 cell 2 is neither cell 0 one period on nor cell 4 one back)


@pytest.mark.parametrize("what", ["list off by one", "another width", "no shift", "exception slice", "no word", "two-byte words"])
def test_groups_that_are_not_runs(what):
    rec, lists = stencil(64, OFF5)
    expect, wb = (0, 0x503), 1
    if what == "list off by one":  # slice 2 of the group does not continue slice 0 in cell 1 -- which no map uses
        lists[2, 1] += 1
    elif what == "another width":
        rec[1, 3] = (rec[1, 3] & ~np.uint32(0xff)) | 4
        expect = (0, 0x3)  # (cell 4 is not a cell of slice 1)
    elif what == "no shift":
        rec[3, 3] = (rec[3, 3] & ~np.uint32(0xff0000)) | ONE << 16
    elif what == "exception slice":  # mode 0 with the flag counts as shifted: still a run
        rec[0, 3] = (rec[0, 3] & ~np.uint32(0xff0000)) | EXCEPT
        rec[0, 0] = 7 | 17 << 8 | 0b11011 << 16 | 0xff << 24
        expect = (1, 0x503)
    elif what == "no word":
        rec[2, 3] &= ~np.uint32(UWORD)
    else:
        wb = 2
    check(rec, lists, (0, 64, 4, LINE), expect, wb)


def test_an_unused_entry_never_aliases():
    rec, lists = stencil(64, OFF5)
    lists[:, 4] = -1  # cell 4 is inside the width and holds no column: a(2) is gone, and -1 continues no list
    check(rec, lists, (0, 64, 4, LINE), (0, 0x3))
    rec, lists = stencil(64, OFF5)
    lists[:, 0] = -1
    check(rec, lists, (0, 64, 4, LINE), (0, 0x500))


def test_an_alias_that_fails_in_one_slice():
    rec, lists = stencil(64, OFF5)
    lists[1, 4] += 1  # in every slice of the period but this one, cell 4 is cell 2 one period on
    check(rec, lists, (0, 64, 4, LINE), (0, 0x3))


def test_degenerate_ranges():
    rec, lists = stencil(64, OFF5)
    for rng in (NONE, (0, 64, 6, 384), (2, 64, 4, LINE), (0, 65, 4, LINE), (60, 64, 8, 512)):
        assert P.sell_find_march(rec, lists, rng) == (0, 0)


def stacked_part(rng, g=3, alias=0x503):
    lo, hi, p, _ = rng
    groups = (hi - lo) // p // g
    while groups > 0 and (groups * (p // 2)) % 4 != 0:
        groups -= 1
    return (lo, lo + groups * g * p, g, alias) if groups > 0 else NONE


@pytest.mark.parametrize("rng", [(64, 262080, 64, 4096), (4, 61436, 4, 256), (64, 61376, 64, 4096), (0, 61440, 4, 256), (12, 61428, 12, 768),
                                 (16, 16 + 5 * 4, 4, 256), (16, 16 + 2 * 4, 4, 256), (8, 8 + 3 * 8, 8, 512)])
def test_launcher_rule(rng):
    """whole groups of 3 periods and whole workgroups; what is left over is not stacked"""
    n = 262144
    want = stacked_part(rng)
    assert P.sell_march_rule(n, 5, rng, 1, 0x503) == want
    lo, hi, g, _ = want
    if g:
        assert lo == rng[0] and hi <= rng[1] and (hi - lo) % (3 * rng[2]) == 0 and ((hi - lo) // 3 // 2) % 4 == 0
        assert rng[1] - hi < 3 * rng[2] + 2 * 3 * rng[2]  # at most the left-over periods and one group given up for whole workgroups
    # the same range is not stacked: by a float plan, at one or four slices per wavefront, when it cannot be stacked, with a
    # map the kernel is not built for or at another width
    for args in ((n, 5, rng, 1, 0x503, 4, 2), (n, 5, rng, 1, 0x503, 8, 1), (n, 5, rng, 1, 0x503, 8, 4), (n, 5, rng, 0, 0x503, 8, 2),
                 (n, 5, rng, 1, 0, 8, 2), (n, 7, rng, 1, 0x6040, 8, 2), (n, 6, rng, 1, 0x503, 8, 2)):
        assert P.sell_march_rule(*args) == NONE


def test_a_range_of_fewer_than_three_periods_is_not_stacked():
    assert stacked_part((16, 24, 4, 256)) == NONE and P.sell_march_rule(4096, 5, (16, 24, 4, 256), 1, 0x503) == NONE
