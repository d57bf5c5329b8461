"""Conditions on the inputs of tests/test_gpu_spgemm_edges.py, checked with the CPU oracle alone: the operands of
tests/spgemm_edges.py really have the list sizes, bounds, bins, probe chains and chunk-boundary repeats they were built for, so
that the GPU tests cannot pass vacuously.  The capacities are the project's constants (spgemm_kernels.hip: SPG_CAP = 32 / 256 /
2,048 / 8,192; the fill pass has the first three)."""
import functools

import numpy as np

import oracle
import spgemm_edges as E

N_EDGE = 9000  # >= 8,193 + room: the bound cap + 1 of the largest capacity must not be cut by n


@functools.lru_cache(maxsize=None)
def product(kind):
    ops = {"edge": lambda: E.edge_operands(N_EDGE), "capped": E.capped_operands}[kind]()
    (pa, ia, va), (pb, ib, vb) = ops.A, ops.B
    st, pc, ic, vc = oracle.dcsr2m(ops.m, ops.n, 0, pa, ia, va, 0, pb, ib, vb)
    assert st == 0
    return ops, pc, ic, vc


def test_constants_are_the_kernels():
    assert E.CAPS == (32, 256, 2048, 8192)
    assert [E.bin_of(x, False) for x in (0, 32, 33, 256, 257, 2048, 2049, 8192, 8193)] == [0, 0, 1, 1, 2, 2, 3, 3, 4]
    assert [E.bin_of(x, True) for x in (0, 32, 33, 256, 257, 2048, 2049, 8192, 8193)] == [0, 0, 1, 1, 2, 2, 4, 4, 4]
    assert E.heavy_logh(4096) == 13 and E.heavy_logh(4097) == 14 and E.heavy_logh(2049) == 13
    # the hash: top `logh` bits of the low 32 bits of c * 2654435761
    assert int(E.hslot(1, 6)) == (2654435761 >> 26) and int(E.hslot(3, 12)) == ((3 * 2654435761) % 2 ** 32) >> 20


def test_single_row_counts_equal_lens():
    ops, pc, _, _ = product("edge")
    counts = np.diff(pc)
    single = ops.rows("single")
    assert len(single) == ops.k
    for L in E.LENS:
        i = single[ops.row_of_len[L]]
        assert ops.a_rows[i]["b"] == [ops.row_of_len[L]]
        assert counts[i] == L and ops.bounds()[i] == L
    for i in single:  # the variants too: a repeat shortens the list by one
        assert counts[i] == ops.a_rows[i]["count"]
    # ... and {r, r} doubles the bound, not the count
    for i, j in zip(single, ops.rows("double")):
        assert counts[j] == counts[i] and ops.bounds()[j] == min(2 * ops.bounds()[i], ops.n)
    assert (ops.bounds() >= counts).all()
    for want in (32, 33, 256, 257, 2048, 2049, 4096, 4097):
        assert (counts == want).any()


def test_bound_and_count_of_every_built_row():
    for kind in ("edge", "capped"):
        ops, pc, _, _ = product(kind)
        counts, bounds = np.diff(pc), ops.bounds()
        built = [i for i, r in enumerate(ops.a_rows) if "bound" in r]
        assert len(built) >= 7
        for i in built:
            r = ops.a_rows[i]
            assert bounds[i] == r["bound"] and counts[i] == r["count"], (kind, i, r["family"], int(bounds[i]), int(counts[i]))
    ops, _, _, _ = product("edge")
    assert sorted(r["cap"] for r in ops.a_rows if r["family"] == "half") == list(E.CAPS)
    assert sorted(r["cap"] for r in ops.a_rows if r["family"] == "full") == list(E.CAPS[:3])
    assert sorted(r["cap"] for r in ops.a_rows if r["family"] == "over") == sorted(2 * list(E.CAPS))
    assert all(r["count"] <= 32 for r in ops.a_rows if r["family"] == "over")
    # the capped rows: the sum of the touched rows is beyond n, the bound is n, the list is full
    ops, _, _, _ = product("capped")
    assert ops.n == 2048 == E.CAPS[2]
    assert sum(r["uncapped"] > ops.n for r in ops.a_rows) >= 5 and any(r["uncapped"] > E.CAPS[3] for r in ops.a_rows)


def test_count_and_fill_passes_choose_different_bins():
    ops, pc, _, _ = product("edge")
    counts, bounds = np.diff(pc), ops.bounds()
    seen = set()
    for i, r in enumerate(ops.a_rows):
        if r["family"] in ("over", "full"):
            cb, fb = E.bin_of(int(bounds[i]), False), E.bin_of(int(counts[i]), True)
            assert cb == E.CAPS.index(r["cap"]) + 1, (i, r["family"])  # one past the capacity: the next bin (the slab past 8,192)
            assert fb == (0 if r["family"] == "over" else E.CAPS.index(r["cap"])) and fb != cb
            seen.add((cb, fb))
        if r["family"] == "half":
            cb, fb = E.bin_of(int(bounds[i]), False), E.bin_of(int(counts[i]), True)
            assert cb == E.CAPS.index(r["cap"])
            seen.add((cb, fb))
    # bound 33 -> count <= 32, 257 -> ..., 8,193 (slab) -> 32; bound cap + 1 with the list exactly full; 8,192 bin -> slab
    assert {(1, 0), (2, 0), (3, 0), (4, 0), (2, 1), (3, 2), (3, 4)} <= seen
    # the cap by n moves the count pass from the 8,192 bin / the slab into the 2,048 bin
    ops, pc, _, _ = product("capped")
    for i, r in enumerate(ops.a_rows):
        assert E.bin_of(int(ops.bounds()[i]), False) == 2 and E.bin_of(int(np.diff(pc)[i]), True) == 2
    assert {E.bin_of(r["uncapped"], False) for r in ops.a_rows} == {2, 3, 4}


def test_wrap_operands_wrap():
    for logh, entries, n, count_logh in E.WRAP_CASES:
        for desc in (0, entries if logh < 13 else 128):
            ops = E.wrap_operands(logh, entries, n, descending=desc)
            (pa, ia, va), (pb, ib, vb) = ops.A, ops.B
            st, pc, ic, _ = oracle.dcsr2m(ops.m, ops.n, 0, pa, ia, va, 0, pb, ib, vb)
            assert st == 0 and np.diff(pc).tolist() == [entries, 3]
            first_touch = ic[:entries]
            assert np.array_equal(first_touch, ib[:entries])  # one B row, distinct columns: its stored order
            assert entries == (1 << logh) // 2 and (E.hslot(first_touch, logh) >= (1 << logh) - (1 << logh) // 16).all()
            for lh in {logh, count_logh}:
                longest, wrapped = E.probe_sim(first_touch, lh)
                assert wrapped >= 1 and longest >= entries // 2, (logh, lh, desc, longest, wrapped)
            if desc:
                tail = ib[entries - desc:entries]
                assert (np.diff(tail) < 0).all()
            # the table the passes use: the bound and the count are both `entries`
            assert E.bin_of(entries, False) == (3 if logh == 13 else E.CAPS.index(entries))
            assert E.bin_of(entries, True) == (E.HEAVY if logh == 13 else E.CAPS.index(entries))
            assert logh < 13 or E.heavy_logh(entries) == logh
    # probe_sim itself, on a table small enough to do by hand: slots 6, 7 taken, the third key of slot 6 wraps to 0
    keys = [c for c in range(200) if int(E.hslot(c, 3)) == 6][:3]
    assert E.probe_sim(keys, 3) == (2, 1)


def test_boundary_variants_have_their_repeat_or_descent_at_the_boundary():
    ops, _, _, _ = product("edge")
    pb, ib, _ = ops.B
    kinds = set()
    for v in ops.variants:
        c = ib[pb[v["row"]]:pb[v["row"] + 1]]
        at, G = v["at"], v["G"]
        assert len(c) == v["L"]
        d = np.diff(c.astype(np.int64))
        if v["kind"] == "repeat_boundary":
            assert at % G == 0 and c[at] == c[at - 1] and (np.delete(d, at - 1) > 0).all()
        elif v["kind"] == "descent_boundary":
            assert at % G == 0 and c[at] < c[at - 1] and (np.delete(d, at - 1) > 0).all()
            # every chunk of G entries is strictly increasing by itself: only the carried column shows the descent
            assert all((np.diff(c[s:s + G].astype(np.int64)) > 0).all() for s in range(0, len(c), G))
        elif v["kind"] == "repeat_inside":
            assert c[at] == c[at - 1] and all(at % g != 0 for g in E.GROUPS)
        else:
            assert v["kind"] == "repeat_last" and at == len(c) - 1 and c[at] in c[:at]
        kinds.add((v["kind"], v["G"], v["L"]))
    for G in E.GROUPS:
        for kind in ("repeat_boundary", "descent_boundary"):
            assert {L for k, g, L in kinds if k == kind and g == G} >= {L for L in E.VARIANT_LENS if L > G}
    # the boundaries the kernel really puts there: G = 16 serves lists of <= 32, so only a B row of 17 (bound 17) and the row of
    # 2 x 32 columns (fill pass: 32) meet it; G = 64 serves the rows of 65, 128, 129
    assert ("repeat_boundary", 16, 17) in kinds and ("descent_boundary", 16, 64) in kinds
    assert {("descent_boundary", 64, L) for L in (65, 128, 129)} <= kinds
    # rows of A on the chunk width
    assert sorted({r["entries"] for r in ops.a_rows if r["family"] == "arows"}) == list(E.AROW_LENS)
    pa = ops.A[0]
    for i in ops.rows("arows"):
        assert pa[i + 1] - pa[i] == ops.a_rows[i]["entries"] and set(ops.b_len[ops.a_rows[i]["b"]].tolist()) <= {0, 1, 2}


def test_syrk_edge_matrix_has_its_sizes_and_repeats():
    """what test_syrk_upper_on_the_edges needs of its input, without the restatement: row 0 alone holds its 258 columns, so the
    rows of A^T A over them hold 258, 257, ... 1 entries after the cut; every other row is sorted, repeats exactly one column and
    has columns right of it (diagonals for which both repeats lie left of the diagonal)"""
    m, n, ptr, ind, val, repeats = E.syrk_edge_matrix()
    c0 = ind[ptr[0]:ptr[1]]
    assert len(c0) == 258 and (np.diff(c0) > 0).all() and not np.isin(ind[ptr[1]:], c0).any()
    assert {32, 33, 256, 257} <= set(range(1, len(c0) + 1))
    assert [r for r, _ in repeats] == [1, 2, 3, 4]
    for r, col in repeats:
        c = ind[ptr[r]:ptr[r + 1]]
        assert (np.diff(c) >= 0).all() and (np.diff(c) == 0).sum() == 1 and (c == col).sum() == 2 and (c > col).any()
        assert (c != r).all()  # (no diagonal entry at all: a handle refuses one stored twice)
    at = int(np.flatnonzero(np.diff(ind[ptr[2]:ptr[3]]) == 0)[0]) + 1
    assert at == 64  # the repeat of row 2 sits exactly across the boundary of two chunks of 64
