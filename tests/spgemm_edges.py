"""Operands that put spgemm_hash_kernel (aocl-sparse_amd/csrc/spgemm_kernels.hip) on the exact sizes at which it decides: list
lengths on the bin capacities, upper bounds and counts in different bins, probe chains that run over the end of the table, B and A
rows on the chunk width, repeats and descents exactly across a chunk boundary.  Plain numpy, no tests: tests/test_spgemm_edges_cpu.py
checks that the operands have the properties they were built for, tests/test_gpu_spgemm_edges.py runs them.

The kernel's constants are restated here on purpose -- the tests have to aim at them:
  CAPS     list capacity of the bins (SPG_CAP); the fill pass has the first three, its rows above 2,048 go to the global slab;
  a table has twice its capacity in slots; the heavy rows' table is the next power of two >= 2 * list size (spg_product.cpp: bin_rows);
  GROUPS   entries of a B row (and of A's row) taken at a time: 16 in bin 0, 64 elsewhere;
  hslot    (uint32(c) * 2654435761 mod 2^32) >> (32 - logh)."""
import numpy as np

CAPS = (32, 256, 2048, 8192)
HEAVY = len(CAPS)  # the bin of the global slab
GROUPS = (16, 64)
LENS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097)
VARIANT_LENS = (16, 17, 64, 65, 128, 129)
AROW_LENS = (16, 17, 64, 65, 128, 129)
FAMILIES = ("single", "double", "pair", "over", "full", "half", "arows")


def hslot(c, logh):
    """the table slot a column starts its probe at"""
    return ((np.asarray(c).astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - logh)


def bin_of(entries, fill):
    """the bin a list of `entries` columns is served by: the count pass knows four LDS capacities, the fill pass three"""
    for b, cap in enumerate(CAPS[:3] if fill else CAPS):
        if entries <= cap:
            return b
    return HEAVY


def heavy_logh(entries):
    """table of a row of the global slab"""
    logh = 6
    while (1 << logh) < 2 * entries:
        logh += 1
    return logh


def probe_sim(cols_in_first_touch_order, logh):
    """Open addressing with linear probing over 2^logh slots, the columns (distinct) inserted in the given order.
    -> (longest probe: slots passed before the free one, insertions that ran past slot H - 1 and went on at slot 0).
    The next free slot is found through a forwarding table, so a long cluster costs no quadratic walk."""
    H = 1 << logh
    assert len(cols_in_first_touch_order) < H
    nxt = list(range(H))  # nxt[s]: a slot at or after s (cyclically) that may be free; nxt[s] == s: s is free

    def free_from(s):
        path = []
        while nxt[s] != s:
            path.append(s)
            s = nxt[s]
        for p in path:
            nxt[p] = s
        return s

    longest = wrapped = 0
    for h in hslot(cols_in_first_touch_order, logh).tolist():
        s = free_from(h)
        longest = max(longest, (s - h) % H)
        wrapped += s < h
        nxt[s] = (s + 1) % H
    return longest, wrapped


def _csr(rows, values):
    ptr = np.zeros(len(rows) + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    ind = np.concatenate([np.asarray(r, np.int64) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    return ptr, ind, values.uniform(-1, 1, len(ind))


class Operands:
    """A (m x k), B (k x n), zero-based; a_rows[i]: dict(family, b = the B rows the entries of row i point at, and what the row was
    built for: bound / count where that is the point); b_len[r]; row_of_len[L]: the sorted B row of length L;
    variants: dict(row, L, G, kind, at) of the unsorted / repeating B rows."""

    def __init__(self, m, k, n, A, B, a_rows, b_len, row_of_len, variants):
        self.m, self.k, self.n, self.A, self.B = m, k, n, A, B
        self.a_rows, self.b_len, self.row_of_len, self.variants = a_rows, b_len, row_of_len, variants

    def rows(self, family):
        return [i for i, r in enumerate(self.a_rows) if r["family"] == family]

    def bounds(self):
        """min(sum of the touched B rows' lengths, n) per row of A: what spg_bound_kernel computes"""
        pa, ia, _ = self.A
        s = np.zeros(self.m, np.int64)
        np.add.at(s, np.repeat(np.arange(self.m), np.diff(pa)), self.b_len[ia])
        return np.minimum(s, self.n)

    def based(self, base_a, base_b):
        (pa, ia, va), (pb, ib, vb) = self.A, self.B
        return (pa + base_a, ia + base_a, va), (pb + base_b, ib + base_b, vb)


def _variant_rows(rng, n, c_lo):
    """the unsorted / repeating versions of the rows of VARIANT_LENS; every column >= c_lo"""
    out = []

    def fresh(L):
        return np.sort(rng.choice(np.arange(c_lo, n), size=L, replace=False))

    for L in VARIANT_LENS:
        for G in GROUPS:
            if L > G:
                c = fresh(L)
                c[G] = c[G - 1]  # a repeat of the previous column exactly across the chunk boundary
                out.append((c, dict(L=L, G=G, kind="repeat_boundary", at=G)))
                c = fresh(L)
                c[G - 1], c[G] = c[G], c[G - 1]  # both chunks stay strictly increasing: only the carried column shows the descent
                out.append((c, dict(L=L, G=G, kind="descent_boundary", at=G)))
        c = fresh(L)
        c[5] = c[4]  # strictly inside the first chunk of either width
        out.append((c, dict(L=L, G=0, kind="repeat_inside", at=5)))
        c = fresh(L)
        c[L - 1] = c[L - 3]  # the row's last entry repeats an earlier column: in the last, partial chunk wherever there is one
        out.append((c, dict(L=L, G=0, kind="repeat_last", at=L - 1)))
    # 32 columns twice: a list of 32 (fill pass: bin 0, 16 at a time) from a B row of 64, the descent at entry 32 = 2 * 16
    c = fresh(32)
    out.append((np.concatenate([c, c]), dict(L=64, G=16, kind="descent_boundary", at=32)))
    return out


def edge_operands(n, families=FAMILIES, seed=7):
    """B: one sorted row per length of LENS, a row of 1,024 and six short rows (1 or 2 entries), then the variants.  The rows of 32,
    256 and 2,048 entries hold the column of the one-entry row.  A: the families named, each entry of a row pointing at a B row:
      single {r}; double {r, r}; pair {r, r + 1};
      over   bound cap + 1, count <= 32: cap + 1 entries at the one-entry row, and cap / 16 at the 16-entry row plus one at it;
      full   bound cap + 1, count cap: {row of cap entries, the one-entry row};
      half   bound cap, count cap / 2: {r, r} with the row of cap / 2 entries;
      arows  rows of A of exactly 16 .. 129 entries that point at the short rows."""
    assert n >= 2 * max(LENS)
    rng = np.random.default_rng(seed)
    c1 = 3  # the column of the one-entry row; no other random draw takes columns below 8
    cols = np.arange(8, n)
    b_rows, row_of_len = [], {}
    for L in LENS + (1024,):
        if L == 1:
            c = np.array([c1])
        elif L in CAPS[:3]:
            c = np.concatenate([[c1], np.sort(rng.choice(cols, size=L - 1, replace=False))])
        else:
            c = np.sort(rng.choice(cols, size=L, replace=False))
        row_of_len[L] = len(b_rows)
        b_rows.append(c)
    shorts = []
    for L in (1, 2, 2, 1, 2, 2):
        shorts.append(len(b_rows))
        b_rows.append(np.sort(rng.choice(cols[:40], size=L, replace=False)))  # (a narrow range: the A rows below form unions)
    variants = []
    for c, info in _variant_rows(rng, n, 8):
        variants.append(dict(info, row=len(b_rows)))
        b_rows.append(c)
    k = len(b_rows)
    b_len = np.array([len(r) for r in b_rows], np.int64)
    one, sixteen = row_of_len[1], row_of_len[16]

    a_rows = []

    def add(**row):
        # a handle refuses a row that stores its diagonal twice: an empty row of A goes in front of such a row
        while row["b"].count(len(a_rows)) > 1:
            a_rows.append(dict(family="filler", b=[]))
        a_rows.append(row)

    if "single" in families:
        for r in range(k):
            add(family="single", b=[r], count=len(set(b_rows[r].tolist())))
    if "double" in families:
        for r in range(k):
            add(family="double", b=[r, r])
    if "pair" in families:
        for r in range(k - 1):
            add(family="pair", b=[r, r + 1])
    if "over" in families:
        for cap in CAPS:
            add(family="over", b=[one] * (cap + 1), cap=cap, bound=cap + 1, count=1)
            add(family="over", b=[sixteen] * (cap // 16) + [one], cap=cap, bound=cap + 1, count=17)
    if "full" in families:
        for cap in CAPS[:3]:
            add(family="full", b=[row_of_len[cap], one], cap=cap, bound=cap + 1, count=cap)
    if "half" in families:
        for cap in CAPS:
            add(family="half", b=[row_of_len[cap // 2]] * 2, cap=cap, bound=cap, count=cap // 2)
    if "arows" in families:
        for L in AROW_LENS:
            add(family="arows", b=rng.choice(shorts, size=L).tolist(), entries=L)
            add(family="arows", b=rng.choice(shorts + [row_of_len[0]], size=L).tolist(), entries=L)
    m = len(a_rows)
    return Operands(m, k, n, _csr([r["b"] for r in a_rows], rng), _csr(b_rows, rng), a_rows, b_len, row_of_len, variants)


def capped_operands():
    """n = 2,048 and B rows that cover every column: the sum of the touched rows exceeds n, the bound is n exactly and the list is
    exactly full (2,048 of the 2,048 a 4,096-slot table may hold); without the cap the count pass would take the 8,192 bin or the
    global slab."""
    n = 2048
    rng = np.random.default_rng(11)
    every = np.arange(n)
    b_rows = [every[0::2], every[1::2], every, rng.permutation(every)]
    a_rows = [dict(family="capped", b=b, bound=n, count=n, uncapped=sum(len(b_rows[r]) for r in b))
              for b in ([2, 0], [0, 2], [1, 0, 2], [2, 2, 2, 2, 2], [3, 2], [0, 1, 3])]
    a_rows.append(dict(family="capped", b=[2], bound=n, count=n, uncapped=n))  # (bound and count on the capacity without the cap)
    b_len = np.array([len(r) for r in b_rows], np.int64)
    return Operands(len(a_rows), len(b_rows), n, _csr([r["b"] for r in a_rows], rng), _csr(b_rows, rng), a_rows, b_len, {}, [])


# (fill-pass table, list size, n, count-pass table): 32 / 256 / 2,048 fill their LDS table to one half in both passes; 4,096 is a
# row of the global slab in the fill pass (8,192 slots) and of the 8,192 bin (16,384 slots in LDS) in the count pass -- the hash
# takes the TOP bits of the product, so columns at the end of the smaller table are at the end of the larger one too
WRAP_CASES = ((6, 32, 6000, 6), (9, 256, 20000, 9), (12, 2048, 100000, 12), (13, 4096, 100000, 14))


def wrap_operands(logh, entries, n, descending=0, seed=3):
    """One row of C of exactly `entries` columns, all of which start their probe in the last H / 16 slots of a 2^logh table: the
    cluster has to run over the end of the table.  Row 0 of B holds them, ascending; `descending` > 0 stores the last that many
    in descending order (chunks that are not strictly increasing: the serial branch).  Row 1 of A / B is a bystander of three
    entries, so that the product has rows in two bins."""
    H = 1 << logh
    rng = np.random.default_rng(seed)
    every = np.arange(n)
    cand = every[hslot(every, logh) >= H - H // 16]
    assert len(cand) >= entries, "n too small: %d columns hash to the last %d slots" % (len(cand), H // 16)
    c = np.sort(rng.choice(cand, size=entries, replace=False))
    if descending:
        c[entries - descending:] = c[entries - descending:][::-1].copy()
    b_rows = [c, np.sort(rng.choice(every, size=3, replace=False))]
    a_rows = [dict(family="wrap", b=[0], bound=entries, count=entries), dict(family="wrap", b=[1], bound=3, count=3)]
    b_len = np.array([len(r) for r in b_rows], np.int64)
    return Operands(2, 2, n, _csr([r["b"] for r in a_rows], rng), _csr(b_rows, rng), a_rows, b_len, {}, [])


def syrk_edge_matrix(seed=5):
    """5 x 700, rows sorted (a repeated column is sorted input: only a descent is not).  aoclsparse_syrk with op = T builds the
    upper triangle of A^T A: row i of C is the union, over the rows of A that hold column i, of their columns >= i.
      row 0: 258 distinct columns below 300, no other row has them: row c of C holds the entries of row 0 from c on, so every
             size 1 .. 258 occurs, 32 / 33 and 256 / 257 among them, each after a cut left of the diagonal;
      rows 1 .. 4: columns from 300 on, overlapping (unions, several visits per row of C); each repeats one column: at entries
             2 = 1 (left of almost every diagonal of its row), 64 = 63 (across the chunk boundary), 5 = 4, 38 = 37 of 40.
    -> (m, n, ptr, ind, val, repeats = [(row, column)])"""
    rng = np.random.default_rng(seed)
    m, n = 5, 700
    rows = [np.sort(rng.choice(np.arange(10, 300), size=258, replace=False))]
    repeats = []
    for r, (L, at) in enumerate(((70, 2), (140, 64), (70, 5), (40, 38)), start=1):
        c = np.sort(rng.choice(np.arange(300, 500), size=L, replace=False))
        c[at] = c[at - 1]
        repeats.append((r, int(c[at])))
        rows.append(c)
    ptr, ind, val = _csr(rows, rng)
    return m, n, ptr, ind, val, repeats
