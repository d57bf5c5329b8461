"""CPU tier of the short-row SELL-64 kernel's slice records: mi355_sell_slice_records packs them from host arrays (no device
needed); the words are checked against values computed here."""
import ctypes

import numpy as np

from util import pkg

P = pkg()
L = P.lib()


def records(slice_ptr, leaders, column_entries):
    ns = len(slice_ptr) - 1
    sp = np.ascontiguousarray(slice_ptr, np.int64)
    ld = None if leaders is None else np.ascontiguousarray(leaders, np.int32)
    n = L.mi355_sell_slice_records(ns, P._ptr(sp), P._ptr(ld), column_entries, None)
    assert n > ns  # (padding records behind the last slice)
    out = np.full((n, 4), 0xdeadbeef, np.uint32)
    assert L.mi355_sell_slice_records(ns, P._ptr(sp), P._ptr(ld), column_entries, P._ptr(out)) == n
    return out


def expect(cell, col, w, stride, mode):
    return [cell & 0xffffffff, col & 0xffffffff, ((cell >> 32) & 0xffff) | (((col >> 32) & 0xffff) << 16), w | stride << 8 | mode << 16]


def test_records_of_shared_lists():
    # widths 2, 0, 5, 3, 8; lists per slice 1 (shift = lane), 1 (no shift), 3 (lead[]), 64 (lead[]), 2 (lead[])
    widths = [2, 0, 5, 3, 8]
    nl, mode = [1, 1, 3, 64, 2], [1, 2, 0, 0, 0]
    sp = np.concatenate([[0], np.cumsum(64 * np.array(widths))])
    leaders = [k | m << 8 for k, m in zip(nl, mode)]
    cols = np.concatenate([[0], np.cumsum(np.array(nl) * np.array(widths))])
    got = records(sp, leaders, int(cols[-1]))
    for s in range(5):
        assert got[s].tolist() == expect(int(sp[s]), int(cols[s]), widths[s], nl[s], mode[s]), s
    # padding: empty single-list slices at the end of both arrays, at least 4 waves x 4 slices of them
    assert len(got) - 5 >= 16
    for s in range(5, len(got)):
        assert got[s].tolist() == expect(int(sp[-1]), int(cols[-1]), 0, 1, 2), s


def test_records_without_shared_lists_and_beyond_32_bits():
    # offsets past 2^32 cells (a 5 x 2^32-cell matrix is not built here: the packer only reads the offsets)
    base = (5 << 32) + 0xfffffe80
    widths = [7, 1, 0, 4]
    sp = base + np.concatenate([[0], np.cumsum(64 * np.array(widths, np.int64))])
    got = records(sp, None, int(sp[-1]))
    for s in range(4):
        assert got[s].tolist() == expect(int(sp[s]), int(sp[s]), widths[s], 64, 3), s
    assert got[4].tolist() == expect(int(sp[-1]), int(sp[-1]), 0, 1, 2)
    assert got[1][2] == (6 | 6 << 16) and got[0][2] == (5 | 5 << 16)  # (the carry into the high words)


def test_records_arguments():
    assert L.mi355_sell_slice_records(-1, None, None, 0, None) < 0
    out = np.zeros((20, 4), np.uint32)
    assert L.mi355_sell_slice_records(1, None, None, 0, P._ptr(out)) < 0
    assert L.mi355_sell_slice_records(0, P._ptr(np.zeros(1, np.int64)), None, 0, None) == 16
