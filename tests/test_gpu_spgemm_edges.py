"""spgemm_hash_kernel (aocl-sparse_amd/csrc/spgemm_kernels.hip) at the sizes on which it decides, through aoclsparse_sp2m / ?csr2m /
aoclsparse_syrk: list lengths exactly on the capacities of the bins, rows whose count pass and fill pass run in different bins,
probe chains that wrap round the end of the table, rows of A and B on the chunk width with repeats and descents across the chunk
boundary, the one-entry-at-a-time branch under the upper-triangle cut.  The operands come from tests/spgemm_edges.py;
tests/test_spgemm_edges_cpu.py proves that they have these properties.  Reference: the CPU oracle's two-stage Gustavson
(first-touch column order, first product stored, later ones added with a contracted multiply-add) -- row_ptr, col_ind and the
double values bit for bit; syrk against the restatement of tests/test_sy_sparse_cpu.py."""
import functools
from ctypes import byref

import numpy as np
import pytest

import oracle
import spgemm_edges as E
from test_sy_sparse_cpu import COUNT, FINAL, FULL, Handle, Result, T, export, restated_syrk, syrk
from util import EPS32, EPS64, pkg

pytestmark = pytest.mark.gpu
P = pkg()
L = P.lib()
N_EDGE = 9000
NONE = P.OP_NONE


@functools.lru_cache(maxsize=None)
def edge(families=E.FAMILIES):
    """-> (operands, the oracle's row_ptr, col_ind, val); computed once, read only"""
    return with_oracle(E.edge_operands(N_EDGE, families))


@functools.lru_cache(maxsize=None)
def capped():
    return with_oracle(E.capped_operands())


@functools.lru_cache(maxsize=None)
def wrapped(case, descending):
    logh, entries, n, _ = E.WRAP_CASES[case]
    return with_oracle(E.wrap_operands(logh, entries, n, descending=descending))


def with_oracle(ops, va=None, vb=None):
    (pa, ia, a), (pb, ib, b) = ops.A, ops.B
    st, pc, ic, vc = oracle.dcsr2m(ops.m, ops.n, 0, pa, ia, a if va is None else va, 0, pb, ib, b if vb is None else vb)
    assert st == 0
    for a_ in (pc, ic, vc):
        a_.setflags(write=False)
    return ops, pc, ic, vc


def handles(ops, base_a, base_b, dt=np.float64, va=None, vb=None):
    (pa, ia, a), (pb, ib, b) = ops.based(base_a, base_b)
    A = Handle(base_a, ops.m, ops.k, pa, ia, (a if va is None else va).astype(dt))
    B = Handle(base_b, ops.k, ops.n, pb, ib, (b if vb is None else vb).astype(dt))
    return A, B, P.Descr(base=base_a), P.Descr(base=base_b)


def product(ops, base_a=0, base_b=0, dt=np.float64, two_stage=False, va=None, vb=None, entry=None):
    """C = A * B through aoclsparse_sp2m (or `entry`); a row wrongly declared dead comes back as invalid_value"""
    A, B, da, db = handles(ops, base_a, base_b, dt, va, vb)
    fn = entry or L.aoclsparse_sp2m
    r = Result()
    for request in ((COUNT, FINAL) if two_stage else (FULL,)):
        st = fn(NONE, da.h, A.h, NONE, db.h, B.h, request, byref(r.h))
        assert st == 0, (P.STATUS[st], request)
    return export(r.h, A.t)


def same_bits(x, ref, values=True):
    """the whole result first; on a difference name the first row and what it was built as"""
    ops, pc, ic, vc = ref
    assert (x["m"], x["n"], x["base"]) == (ops.m, ops.n, 0)
    ok = x["nnz"] == len(ic) and np.array_equal(x["row_ptr"], pc) and np.array_equal(x["col_ind"], ic)
    if ok and values:
        ok = np.array_equal(x["val"], vc)
    if ok:
        return
    for i in range(ops.m):
        got = slice(x["row_ptr"][i], x["row_ptr"][i + 1])
        want = slice(pc[i], pc[i + 1])
        same = np.array_equal(x["col_ind"][got], ic[want]) and (not values or np.array_equal(x["val"][got], vc[want]))
        r = ops.a_rows[i]
        assert same, "row %d of C (%s, B rows %s..., %d entries of A): %d columns for %d" % (
            i, r["family"], r["b"][:3], len(r["b"]), got.stop - got.start, want.stop - want.start)
    assert False, "row_ptr differs past the last row"


@pytest.mark.parametrize("base", [0, 1])
def test_list_sizes_on_every_capacity(base):
    """Every family of edge_operands, bases (0, 0) and (1, 1).  Reaches `len + popc(new) > limit` (spgemm_kernels.hip:256) with
    the list landing exactly on limit = H / 2 in every LDS bin (32, 256, 2,048) and in a global-slab table filled to exactly one
    half (4,096 of 8,192: sp2m_api.cpp:157-159), and one past each in the next bin; full computation, then count + finalize."""
    ref = edge()
    counts = np.diff(ref[1])
    for want in (32, 33, 256, 257, 2048, 2049, 4096, 4097):
        assert (counts == want).any()
    same_bits(product(ref[0], base, base), ref)
    same_bits(product(ref[0], base, base, two_stage=True), ref)


def test_count_and_fill_passes_in_different_bins():
    """Rows whose upper bound (spg_bound_kernel, spgemm_kernels.hip:448-463) and exact count fall into different bins
    (spg_bin_dev, :437-445): bound cap + 1 with a list of 1 / 17 / exactly cap entries for all four capacities (8,193: the count
    pass in the global slab, the fill pass in the 32 bin), bound 8,192 with a list of 4,096 (count: LDS, fill: slab); and n = 2,048
    with B rows that cover every column: the bound is cut to n (:462), the count pass then runs in the 2,048 bin with its list
    exactly full where the uncut sum would have taken the 8,192 bin or the slab."""
    ref = edge(("over", "full", "half"))
    assert [len(ref[0].rows(f)) for f in ("over", "full", "half")] == [8, 3, 4]
    same_bits(product(ref[0]), ref)
    same_bits(product(ref[0], two_stage=True), ref)
    ref = capped()
    assert ref[0].n == 2048 and (np.diff(ref[1]) == 2048).all() and (ref[0].bounds() == 2048).all()
    for base in (0, 1):
        same_bits(product(ref[0], base, base), ref)
    same_bits(product(ref[0], two_stage=True), ref)


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("case", range(len(E.WRAP_CASES)), ids=["%d_in_%d" % (c[1], 1 << c[0]) for c in E.WRAP_CASES])
def test_probe_chains_wrap_round_the_table_end(case, descending):
    """All columns of one row of C start their probe in the last H / 16 slots: the chain runs over slot H - 1 and goes on at slot
    0 -- `h = (h + 1) & hmask` in the lookup (:252), the insert (:268) and the serial branch (:309) -- with the table filled to one
    half, slots up to 2,047 in the unsigned-short hpos of the LDS mode, 4,096 entries in a table of the global slab.  Descending:
    the columns arrive in descending order inside the B row, every chunk takes the one-entry-at-a-time branch (for the slab row
    the last 128 only: a serial walk of 4,096 entries through probes of thousands of L2 round trips would run for seconds)."""
    logh, entries, _, _ = E.WRAP_CASES[case]
    desc = 0 if not descending else (entries if logh < 13 else 128)
    ref = wrapped(case, desc)
    assert np.diff(ref[1]).tolist() == [entries, 3]
    same_bits(product(ref[0]), ref)
    same_bits(product(ref[0], 1, 1, two_stage=True), ref)


def test_chunk_boundaries_of_a_and_b_rows():
    """B rows with a repeat / a descent exactly at entry G (the column carried into lane 0 of the next chunk: `carry`, :230-234),
    strictly inside a chunk and in the last partial chunk, alone ({r}), twice ({r, r}: every value a two-term contracted chain)
    and in unions ({r, r + 1}); rows of A of exactly 16 / 17 / 64 / 65 / 128 / 129 entries (my_kb / my_ke / my_va handed round by
    __shfl, :200-219, a second round of A's row from entry G on)."""
    ref = edge(("single", "double", "pair", "arows"))
    ops = ref[0]
    assert len(ops.variants) >= 28 and len(ops.rows("arows")) == 12
    for base_a, base_b in ((0, 0), (1, 0), (0, 1)):
        same_bits(product(ops, base_a, base_b), ref)
    same_bits(product(ops, two_stage=True), ref)


def float_exact(v):
    return v.astype(np.float32).astype(np.float64)


def complex_check(ops, ref, x, dt, eps):
    """structure bit for bit the real product's; values within (2 terms + 8) eps sum|a||b| of scipy's complex128 product"""
    import scipy.sparse as sp
    same_bits(x, ref, values=False)
    (pa, ia, _), (pb, ib, _) = ops.A, ops.B
    va, vb = x["va"], x["vb"]
    A64 = sp.csr_matrix((va.astype(np.complex128), ia.copy(), pa.copy()), shape=(ops.m, ops.k))
    B64 = sp.csr_matrix((vb.astype(np.complex128), ib.copy(), pb.copy()), shape=(ops.k, ops.n))
    R, S = (A64 @ B64).tocsr(), (abs(A64) @ abs(B64)).tocsr()
    rows = np.repeat(np.arange(ops.m), np.diff(x["row_ptr"]))
    want = np.asarray(R[rows, x["col_ind"]]).ravel()
    scale = np.asarray(S[rows, x["col_ind"]]).ravel().real
    terms = int(np.diff(pa).max())
    assert np.all(np.abs(x["val"].astype(np.complex128) - want) <= (2 * terms + 8) * eps * scale + 1e-300)


@pytest.mark.parametrize("t", ["s", "z", "c"])
def test_float_and_complex_on_the_same_edges(t):
    """The list-size families (single, double, pair) and the wrap cases with 4-, 16- and 8-byte values: the cdouble fill of the
    2,048 bin holds 16 + 8 + 8 + 32 KB, the whole 64 KB of static LDS, and is run full here.  float through aoclsparse_scsr2m:
    structure bit for bit the double oracle's (on the same, float-representable inputs), values within the bound of
    test_spgemm_hash_kernel_every_bin_bit_exact (the oracle has no float product); z / c through aoclsparse_sp2m against scipy."""
    cases = [edge(("single", "double", "pair"))] + [wrapped(c, 0) for c in range(len(E.WRAP_CASES))]
    assert (np.diff(cases[3][1]) == 2048).any() and (np.diff(cases[0][1]) == 2048).any()
    rng = np.random.default_rng(17)
    for ops, pc, ic, vc in cases:
        if t == "s":
            va, vb = float_exact(ops.A[2]), float_exact(ops.B[2])
            ref = with_oracle(ops, va, vb)
            x = product(ops, dt=np.float32, va=va, vb=vb, entry=L.aoclsparse_scsr2m)
            same_bits(x, ref, values=False)
            scale = np.abs(ref[3]) + 1e-3
            assert np.all(np.abs(x["val"] - ref[3]) <= 4000 * EPS32 * np.maximum(scale, 1.0))
        else:
            dt, eps = (np.complex128, EPS64) if t == "z" else (np.complex64, EPS32)
            va = (ops.A[2] + 1j * rng.uniform(-1, 1, len(ops.A[2]))).astype(dt)
            vb = (ops.B[2] + 1j * rng.uniform(-1, 1, len(ops.B[2]))).astype(dt)
            x = product(ops, dt=dt, va=va, vb=vb)
            x["va"], x["vb"] = va, vb
            complex_check(ops, (ops, pc, ic, vc), x, dt, eps)


@functools.lru_cache(maxsize=None)
def syrk_case():
    m, n, ptr, ind, val, repeats = E.syrk_edge_matrix()
    ref = restated_syrk(T, False, m, n, 0, ptr, ind, val)
    return (m, n, ptr, ind, val, repeats), ref


def test_syrk_upper_on_the_edges():
    """aoclsparse_syrk, double, op = T: spgemm_hash_kernel with UPPER.  Row c of C = the entries of A's rows that hold c, from c
    on: lists of 32 / 33 and 256 / 257 (and every size between) left after the cut `use = c >= i` (:235), i.e. limit =
    min(H / 2, row_ptr difference) reached with most of the B row passed over.  Rows 1 .. 4 of A repeat a column (sorted input
    still: syrk refuses a descent with unsorted_input, a repeat is the only way into the serial branch here), so for every
    diagonal right of the repeat the chunk is walked one entry at a time and both repeats are skipped by `if(cq < i) continue`
    (:291-293); for the diagonal ON the repeated column they are added twice.  Structure and values bit for bit the restatement."""
    (m, n, ptr, ind, val, repeats), ref = syrk_case()
    mc, _, rp, ci, cv = ref
    sizes = np.diff(rp)
    for want in (32, 33, 256, 257):
        assert (sizes == want).any()
    for r, col in repeats:  # a diagonal right of the repeated column, in the row that repeats it
        c = ind[ptr[r]:ptr[r + 1]]
        assert (c == col).sum() == 2 and (c > col).any() and (np.diff(c) >= 0).all()
    for base in (0, 1):
        Hd = Handle(base, m, n, ptr + base, ind + base, val)
        st, r = syrk(T, Hd.h)
        assert st == "success", st
        x = export(r.h, "d")
        assert (x["m"], x["n"], x["base"], x["nnz"]) == (mc, mc, base, len(ci))
        assert np.array_equal(x["row_ptr"], rp + base) and np.array_equal(x["col_ind"], ci + base)
        assert np.array_equal(x["val"], cv), base
