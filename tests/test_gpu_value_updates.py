"""Every cached copy of a handle's values is dropped when the values change.

A handle keeps many copies of A's values, each built on first use and kept: the device CSR, the SELL-64 copy, the blocked-ELL copy,
the level-ordered TRSV triangles (row, block and chunk plans), the derived symmetric / triangular CSRs, the host transpose, the
clean copy of unsorted arrays, the device diagonal and the multi-device replicas.  Every case here runs one protocol:

  1. build the handle (hints, optimize, forced options as the path needs);
  2. run the operation -- this builds the cached copies -- and compare with the oracle on the OLD values;
  3. record which path ran (spmv_info / trsv_info / the forced schedule);
  4. change the values: (a) ?set_value, (b) ?update_values, (c) both on a handle created from CSC, (d) a write into the aliased
     val array + aoclsparse_mi355_invalidate, (e) aoclsparse_order_mat on an unsorted handle whose plans were built;
  5. run again and compare with the oracle on the NEW values, by the same rule as in 2 (the rule of the path's own test);
  6. the result differs from the one of 2 (the mutation reached the output);
  7. the same path ran (no silent fall-back that would make the case pass trivially).

New values scale every entry by uniform(0.5, 1.5); ?set_value changes the diagonal entry and the first and last off-diagonal entries
of a row the output depends on (one on each side of the diagonal where the row has both: every triangle sees a change)."""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest

import oracle
from util import EPS64, abs_row_sums, laplace5, pkg, random_csr, triangular_system, trsv_schedule

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import standins  # noqa: E402
from test_gpu_trsv_blocks import node_mesh  # noqa: E402

torch = pytest.importorskip("torch")
P = pkg()
L = P.lib()

MUTATIONS = ("set_value", "update", "invalidate")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    yield
    L.aoclsparse_mi355_set_pointer_mode(P.PTR_AUTO)


@contextlib.contextmanager
def options(**kw):
    """process-wide options held for the whole case (analysis AND the rebuild after the update); defaults restored"""
    codes = {"spmv_kernel": (P.OPTION_SPMV_KERNEL, 0), "sell": (P.OPTION_SELL, -1), "strict": (P.OPTION_SPMV_STRICT, 0),
             "chunks": (P.OPTION_TRSV_CHUNKS, -1)}
    env = kw.pop("bell_xcd_chunk", None)
    old = os.environ.pop("AOCLSPARSE_MI355_BELL_XCD_CHUNK", None)
    if env is not None:
        os.environ["AOCLSPARSE_MI355_BELL_XCD_CHUNK"] = str(env)
    try:
        for k, v in kw.items():
            assert L.aoclsparse_mi355_set_option(codes[k][0], v) == 0
        yield
    finally:
        for k in kw:
            assert L.aoclsparse_mi355_set_option(codes[k][0], codes[k][1]) == 0
        os.environ.pop("AOCLSPARSE_MI355_BELL_XCD_CHUNK", None)
        if old is not None:
            os.environ["AOCLSPARSE_MI355_BELL_XCD_CHUNK"] = old


def scaled(v, seed):
    return np.ascontiguousarray(v * np.random.default_rng(seed).uniform(0.5, 1.5, len(v)).astype(v.dtype))


def mutate(how, A, row, seed=99):
    """change A's values by `how`; -> the values the handle holds now (in the order of its own CSR arrays)"""
    cplx = np.iscomplexobj(A.val)
    if how == "update":
        v2 = scaled(A.val, seed)
        fn = L.aoclsparse_zupdate_values if cplx else L.aoclsparse_dupdate_values if A.double else L.aoclsparse_supdate_values
        assert fn(A.h, len(v2), P._ptr(v2)) == 0
        assert np.array_equal(A.val, v2)
    elif how == "invalidate":
        A.val[:] = scaled(A.val, seed)
        assert L.aoclsparse_mi355_invalidate(A.h) == 0
    else:  # the diagonal entry of `row` (else its first entry) and its first and last off-diagonal entries
        b = A.base

        def entries(r):
            lo, hi = int(A.row_ptr[r]) - b, int(A.row_ptr[r + 1]) - b
            cols = A.col_ind[lo:hi] - b
            return lo, hi, cols, bool(np.any(cols < r)), bool(np.any(cols > r)), bool(np.any(cols == r))

        # from `row` on: the first row with its diagonal and entries on both sides of it (else with two entries at least)
        cand = [r for r in range(row, A.m) if all(entries(r)[3:])] or [r for r in range(row, A.m) if len(entries(r)[2]) >= 2]
        assert cand, "no row from %d on has two entries" % row
        row = cand[0]
        lo, hi, cols = entries(row)[:3]
        diag = [p for p in range(lo, hi) if cols[p - lo] == row] or [lo]
        off = [p for p in range(lo, hi) if p != diag[0]]
        fn = L.aoclsparse_zset_value if cplx else L.aoclsparse_dset_value if A.double else L.aoclsparse_sset_value
        for p, f in ((diag[0], 1.375), (off[0], -0.625), (off[-1], 0.8125)):
            nv = A.val[p] * f + (0.25 if A.val[p] == 0 else 0.0)
            assert fn(A.h, row + b, int(A.col_ind[p]), P.CDouble(nv.real, nv.imag) if cplx else float(nv)) == 0
            assert A.val[p] == A.val.dtype.type(nv)
    return A.val.copy()


def protocol(how, A, run, expect, close, path, row=None):
    """steps 2-7 of the module docstring; `expect(vals)` -> the oracle's result on those values of A's arrays"""
    got0 = np.array(run(), copy=True)
    close(got0, expect(A.val.copy()), "old values")
    p0 = path()
    vals = mutate(how, A, row)
    got1 = np.array(run(), copy=True)
    close(got1, expect(vals), "new values (%s)" % how)
    assert not np.array_equal(got0, got1), "the mutation did not reach the output"
    assert path() == p0, ("another path ran after the update", p0, path())


def exact(got, ref, what):
    assert np.array_equal(np.asarray(got), np.asarray(ref)), (what, int(np.sum(np.asarray(got) != np.asarray(ref))))


def within(bound):
    def close(got, ref, what):
        b = bound() if callable(bound) else bound
        assert np.all(np.abs(got - ref) <= b), (what, float(np.max(np.abs(got - ref) / b)))
    return close


def dense(m, n, rp, ci, v, base=0):
    D = np.zeros((m, n))
    rows = np.repeat(np.arange(m), np.diff(rp.astype(np.int64)))
    np.add.at(D, (rows, ci.astype(np.int64) - base), v.astype(np.float64))
    return D


def spmv_path(A, op=P.OP_NONE):
    i = A.spmv_info(op)
    return (i.kernel, i.order, i.mm_groups, i.mm_window_rows, i.mm_bell_width, i.mm_bell_xcd_chunk)


# --------------------------------------------------------------------------------------------------
# SpMV (?mv)
# --------------------------------------------------------------------------------------------------
def _dmv_runner(A, d, x, y0, alpha, beta, op=P.OP_NONE):
    def run():
        yd = dev(y0)
        assert P.dmv(op, alpha, A, d, dev(x), beta, yd) == 0
        torch.cuda.synchronize()
        return yd.cpu().numpy()
    return run


def _general(seed, m, n, rowlen):
    """random rows, mv hint + optimize"""
    rp, ci, v = random_csr(seed, m, n, rowlen)
    A = P.Matrix(0, m, n, rp, ci, v)
    d = P.Descr()
    assert L.aoclsparse_set_mv_hint(A.h, P.OP_NONE, d.h, 100) == 0 and L.aoclsparse_optimize(A.h) == 0
    return A, d


def _spmv_case(name):
    """-> (A, descr, options to hold, spmv_info kernel, alpha, beta, comparison rule)"""
    rng = np.random.default_rng(len(name))
    if name in ("adaptive", "adaptive_strict"):
        opts = dict(spmv_kernel=1, sell=0, **({"strict": 1} if name == "adaptive_strict" else {}))
        m = 6000
        with options(**opts):
            A, d = _general(3, m, m, lambda r, i: r.integers(1, 30))
        return A, d, opts, 1, 1.3, -0.4, "exact"
    if name == "adaptive_long":  # rows above the tree threshold, no strict mode: the rule of test_mix_full_size_dmv_after_optimize
        opts = dict(spmv_kernel=1, sell=0)
        m = 4000
        with options(**opts):
            # (nnz <= 10 m: the scalar order, whose rows from tree_min on are reduced by a tree)
            A, d = _general(4, m, m, lambda r, i: 300 + i % 50 if i % 97 == 5 else r.integers(1, 8))
        return A, d, opts, 1, 1.0, 0.0, "tree"
    if name == "merge":
        opts = dict(spmv_kernel=2, sell=0)
        m = 30000
        with options(**opts):
            A, d = _general(77, m, m, lambda r, i: 9000 if i in (3, 14000, 29990) else r.integers(1, 8))
        return A, d, opts, 2, 1.0, 0.0, "bound"
    if name == "sell":
        A, d = _general(5, 20000, 20000, lambda r, i: r.integers(9, 13))
        return A, d, {}, 3, 1.3, -0.4, "exact"
    if name == "sell_shared":
        m, rp, ci, v = laplace5(300)
        A = P.Matrix(0, m, m, rp, ci, v * rng.uniform(0.5, 1.5, len(v)))
        d = P.Descr()
        assert L.aoclsparse_set_mv_hint(A.h, P.OP_NONE, d.h, 100) == 0 and L.aoclsparse_optimize(A.h) == 0
        return A, d, {}, 4, 1.3, -0.4, "exact"
    if name == "sell_promoted":  # no hint, no optimize: the SELL copy arrives at the 8th product
        m, rp, ci, v = laplace5(300)
        A = P.Matrix(0, m, m, rp, ci, v * rng.uniform(0.5, 1.5, len(v)))
        return A, P.Descr(), {}, 4, 1.0, 0.0, "promote"
    if name in ("kid1", "kid3"):
        nodes = 1200
        m, rp, ci, v = node_mesh(71, nodes, 31, np.full(nodes, 5), keep=1.0)
        A = P.Matrix(0, m, m, rp, ci, v)
        d = P.Descr()
        assert L.aoclsparse_set_mv_hint_kid(A.h, P.OP_NONE, d.h, 100, int(name[-1])) == 0 and L.aoclsparse_optimize(A.h) == 0
        return A, d, {}, 4, -1.3, 0.7, "lane4" if name == "kid1" else "lane8"
    raise KeyError(name)


SPMV_GENERAL = ["adaptive", "adaptive_strict", "adaptive_long", "merge", "sell", "sell_shared", "sell_promoted", "kid1", "kid3"]


@pytest.mark.parametrize("how", MUTATIONS)
@pytest.mark.parametrize("name", SPMV_GENERAL)
def test_dmv_general_paths(name, how):
    """?mv with a general descriptor on every kernel: CSR-Adaptive (rows shorter than tree_min and strict mode bit for bit; longer
    rows within (2 ceil(log2 len) + 4 + len/256) eps sum|a x|, the rule of test_mix_full_size_dmv_after_optimize), merge-path (the
    bound of test_merge_path_launch_replayed_from_a_hip_graph_with_a_new_x_every_time), SELL-64 with and without shared column
    lists, a SELL copy promoted on an un-hinted handle, and the 4- / 8-lane summation orders of kid 1 / 3 (bit for bit against the
    oracle's lane order)"""
    A, d, opts, want, alpha, beta, rule = _spmv_case(name)
    m = A.m
    rng = np.random.default_rng(7)
    x, y0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)
    run = _dmv_runner(A, d, x, y0, alpha, beta)

    def expect(vals):
        if rule in ("lane4", "lane8"):
            so, yr = oracle.dcsrmv_order(rule, 0, alpha, m, vals, A.col_ind, A.row_ptr, x, beta, y0)
        else:
            so, yr = oracle.dcsrmv(-1, 0, alpha, m, len(vals), vals, A.col_ind, A.row_ptr, x, beta, y0)
        assert so == 0
        return yr

    close = exact
    if rule == "bound":
        close = within(lambda: (np.diff(A.row_ptr) + 24) * EPS64 * abs_row_sums(A.row_ptr, A.col_ind, A.val, x) + 1e-300)
    if rule == "tree":
        def close(got, ref, what):
            lens = np.diff(A.row_ptr)
            tree_min = A.spmv_info().tree_min
            assert tree_min == 32, (what, tree_min)
            short = lens < tree_min
            assert np.array_equal(got[short], ref[short]), (what, int(np.sum(got[short] != ref[short])))
            bound = (2 * np.ceil(np.log2(np.maximum(lens, 2))) + 4 + lens / 256.0) * EPS64 * abs(alpha) \
                * abs_row_sums(A.row_ptr, A.col_ind, A.val, x) + 2 * EPS64 * np.abs(beta * y0)
            assert np.all(np.abs(got - ref)[~short] <= bound[~short]), (what, float(np.max((np.abs(got - ref) / (bound + 1e-300))[~short])))
            assert np.any(~short)
    with options(**opts):
        if rule == "promote":
            for _ in range(8):
                run()
        protocol(how, A, run, expect, close, lambda: spmv_path(A), row=m // 2)
        assert A.spmv_info().kernel == want, (name, A.spmv_info().kernel)


@pytest.mark.parametrize("how", MUTATIONS)
def test_dmv_transposed_within_bound(how):
    """op = T (the handle's transpose and its device copy): the componentwise bound of test_transposed_spmv_within_bound"""
    m, n = 4000, 3000
    rp, ci, v = random_csr(41, m, n, lambda r, i: r.integers(1, 30))
    A = P.Matrix(0, m, n, rp, ci, v)
    d = P.Descr()
    assert L.aoclsparse_set_mv_hint(A.h, P.OP_TRANSPOSE, d.h, 5) == 0 and L.aoclsparse_optimize(A.h) == 0
    x = np.random.default_rng(3).uniform(-1, 1, m)
    y0 = np.random.default_rng(4).uniform(-1, 1, n)
    run = _dmv_runner(A, d, x, y0, 5.1, 3.2, op=P.OP_TRANSPOSE)

    def expect(vals):
        so, yr = oracle.dcsrmvt(0, 5.1, m, n, vals, ci, rp, x, 3.2, y0)
        assert so == 0
        return yr

    def bound():
        st, cp, ri, cv = oracle.dcsr2csc(m, n, len(A.val), 0, 0, rp, ci, A.val)
        return (np.diff(cp) + 4) * EPS64 * abs_row_sums(cp, ri, cv, x) * 5.1 + 2 * EPS64 * np.abs(3.2 * y0) + 1e-300

    protocol(how, A, run, expect, within(bound), lambda: spmv_path(A, P.OP_TRANSPOSE), row=5)


def _special_dmv(A, mtype, fill, diag, op, how, row):
    """symmetric / triangular descriptor (the derived general CSR) against the oracle's serial kernels within the bound of
    test_symmetric_and_triangular_dmv.  (No counter reports the plans of the derived matrix: step 7 compares only what spmv_info
    says of the handle's own plans.)"""
    m = A.m
    d = P.Descr(mtype=mtype, fill=fill, diag=diag)
    rng = np.random.default_rng(9)
    x, y0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)
    alpha, beta = 1.7, -0.4
    run = _dmv_runner(A, d, x, y0, alpha, beta, op=op)
    held = {}

    def expect(vals):
        o = oracle.dcsr_optimize(m, m, len(vals), 0, A.row_ptr, A.col_ind, vals)
        if mtype == P.TYPE_SYMMETRIC:
            so, yo = oracle.dcsrmv_special("symm", o["base"], alpha, m, m, diag, fill, o["val"], o["ind"], o["ptr"], o["idiag"],
                                           o["iurow"], x, beta, y0)
        else:
            so, yo = oracle.dcsrmv_special("tri" if op == P.OP_NONE else "tri_t", o["base"], alpha, m, m, diag, fill, o["val"],
                                           o["ind"], o["ptr"], o["idiag"], o["iurow"], x, beta, y0)
        assert so == 0
        D = dense(m, m, o["ptr"], o["ind"], o["val"], o["base"])
        tri = np.tril(D, -1) if fill == P.FILL_LOWER else np.triu(D, 1)
        dg = np.diag(np.diag(D)) if diag == P.DIAG_NON_UNIT else (np.eye(m) if diag == P.DIAG_UNIT else 0.0)
        M = tri + tri.T + dg if mtype == P.TYPE_SYMMETRIC else (tri + dg if op == P.OP_NONE else (tri + dg).T)
        held["M"] = M
        return yo

    def close(got, ref, what):
        M = held["M"]
        bound = ((M != 0).sum(axis=1) + 6) * EPS64 * (abs(alpha) * (np.abs(M) @ np.abs(x)) + np.abs(beta * y0)) + 1e-300
        assert np.all(np.abs(got - ref) <= bound), (what, float(np.max(np.abs(got - ref) / bound)))

    protocol(how, A, run, expect, close, lambda: spmv_path(A, op), row=row)


@pytest.mark.parametrize("how", MUTATIONS)
@pytest.mark.parametrize("mtype,op", [(P.TYPE_SYMMETRIC, P.OP_NONE), (P.TYPE_TRIANGULAR, P.OP_NONE), (P.TYPE_TRIANGULAR, P.OP_TRANSPOSE)])
@pytest.mark.parametrize("sort", [True, False])
def test_dmv_symmetric_and_triangular(sort, mtype, op, how):
    """the derived CSRs of a symmetric / triangular descriptor are built from the clean CSR; with unsorted rows that is the
    handle's own clean COPY -- both have to follow the new values"""
    m = 1500
    rp, ci, v = triangular_system(101, m, 6)
    if not sort:  # every row reversed: the clean copy is made
        for i in range(m):
            ci[rp[i]:rp[i + 1]] = ci[rp[i]:rp[i + 1]][::-1].copy()
            v[rp[i]:rp[i + 1]] = v[rp[i]:rp[i + 1]][::-1].copy()
    A = P.Matrix(0, m, m, rp, ci, v)
    _special_dmv(A, mtype, P.FILL_LOWER, P.DIAG_NON_UNIT, op, how, row=m // 3)


@pytest.mark.parametrize("how", MUTATIONS)
def test_smv_float_sell(how):
    """float ?mv on a SELL-64 copy: the 8-lane order bit for bit (test_float_smv_bit_exact)"""
    m = 12000
    rp, ci, v = random_csr(31, m, m, lambda r, i: r.integers(8, 12), dtype=np.float32)
    A = P.Matrix(0, m, m, rp, ci, v)
    d = P.Descr()
    assert L.aoclsparse_set_mv_hint(A.h, P.OP_NONE, d.h, 100) == 0 and L.aoclsparse_optimize(A.h) == 0
    assert A.spmv_info().kernel in (3, 4)
    x = np.random.default_rng(1).uniform(-1, 1, m).astype(np.float32)
    y0 = np.random.default_rng(2).uniform(-1, 1, m).astype(np.float32)

    def run():
        yd = dev(y0)
        assert P.smv(P.OP_NONE, 1.5, A, d, dev(x), 0.25, yd) == 0
        torch.cuda.synchronize()
        return yd.cpu().numpy()

    def expect(vals):
        so, yr = oracle.scsrmv("lane8", 0, 1.5, m, vals, ci, rp, x, 0.25, y0)
        assert so == 0
        return yr

    protocol(how, A, run, expect, exact, lambda: spmv_path(A), row=77)


@pytest.mark.parametrize("how", MUTATIONS)
def test_ddotmv(how):
    """?dotmv: y bit for bit, the dot product within the bound of test_ddotmv"""
    m, rp, ci, v = laplace5(60)
    A = P.Matrix(0, m, m, rp, ci, v * np.random.default_rng(2).uniform(0.5, 1.5, len(v)))
    d = P.Descr()
    rng = np.random.default_rng(3)
    x, y0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)

    def run():
        yd, dd = dev(y0), torch.zeros(1, dtype=torch.float64, device="cuda")
        assert L.aoclsparse_ddotmv(P.OP_NONE, 1.3, A.h, d.h, P._ptr(dev(x)), -0.2, P._ptr(yd), P._ptr(dd)) == 0
        torch.cuda.synchronize()
        return np.concatenate([yd.cpu().numpy(), dd.cpu().numpy()])

    def expect(vals):
        so, yr = oracle.dcsrmv(-1, 0, 1.3, m, len(vals), vals, ci, rp, x, -0.2, y0)
        return np.concatenate([yr, [float(np.dot(x.astype(np.longdouble), yr.astype(np.longdouble)))]])

    def close(got, ref, what):
        exact(got[:m], ref[:m], what)
        assert abs(got[m] - ref[m]) <= 2 * m * EPS64 * float(np.dot(np.abs(x), np.abs(ref[:m]))), what

    protocol(how, A, run, expect, close, lambda: spmv_path(A), row=m // 2)


# --------------------------------------------------------------------------------------------------
# csrmm (?csrmm)
# --------------------------------------------------------------------------------------------------
def _csrmm_col_ref(vals, A, alpha, beta, B, C0, n, order):
    """oracle.dcsrmm's bits; a row-major product through the column-major oracle of the transposed operands"""
    m, k = A.m, A.n
    if order == P.ORDER_COLUMN:
        so, Cr = oracle.dcsrmm("col", alpha, A.base, vals, A.col_ind, A.row_ptr, m, B, n, k, beta, C0, m)
        assert so == 0
        return Cr
    so, Cr = oracle.dcsrmm("col", alpha, A.base, vals, A.col_ind, A.row_ptr, m, np.ascontiguousarray(B.reshape(k, n).T).ravel(), n,
                           k, beta, np.ascontiguousarray(C0.reshape(m, n).T).ravel(), m)
    assert so == 0
    return np.ascontiguousarray(Cr.reshape(n, m).T).ravel()


def mm_path(A):
    """spmv_path + the csrmm plans the exported state announces: row runs, row pairs, LDS window, line blocks of the narrow kernel
    (aoclsparse_mi355_mm_state_export scalars S_RUNS, S_PAIRS, S_WIN, S_SLAB_NBLOCKS)"""
    st, state, _ = A.mm_state_export()
    assert st == 0
    s = list(state.scalars)
    return spmv_path(A) + (s[13], s[18], s[21], s[30])


def _csrmm_case(name):
    """-> (A, order, n, options, predicate on mm_path)"""
    if name in ("default_row", "default_col"):
        m, k = 3000, 2500
        rp, ci, v = random_csr(81, m, k, lambda r, i: r.integers(1, 14))
        A = P.Matrix(0, m, k, rp, ci, v)
        return A, P.ORDER_ROW if name == "default_row" else P.ORDER_COLUMN, 24, {}, None
    if name == "row_groups":
        m, rp, ci, v = standins.flan_like(nx=12, ny=12, nz=12)
        return P.Matrix(0, m, m, rp, ci, v), P.ORDER_ROW, 64, {}, lambda p: p[2] > 0
    if name in ("row_runs", "line_blocks", "col_pairs", "col_window"):
        m, rp, ci, v = laplace5({"col_window": 200, "col_pairs": 61}.get(name, 300))  # (61: test_csrmm_column_major_row_pairs_bit_exact)
        v = v * np.random.default_rng(8).uniform(0.5, 1.5, len(v))
        n = {"row_runs": 128, "line_blocks": 40, "col_pairs": 7, "col_window": 16}[name]
        order = P.ORDER_ROW if name.startswith(("row", "line")) else P.ORDER_COLUMN
        want = {"row_runs": lambda p: p[6] == 1, "line_blocks": lambda p: p[9] > 0, "col_pairs": lambda p: p[7] == 1,
                "col_window": lambda p: p[3] > 0 and p[8] == 1}[name]
        return P.Matrix(0, m, m, rp, ci, v), order, n, {}, want
    if name in ("bell_row", "bell_col"):
        m, rp, ci, v = standins.block_dense(12, 16, 16, seed=5)
        return (P.Matrix(0, m, m, rp, ci, v), P.ORDER_ROW if name == "bell_row" else P.ORDER_COLUMN, 64, dict(bell_xcd_chunk=3),
                lambda p: p[4] > 0 and p[5] == 3)
    raise KeyError(name)


CSRMM = ["default_row", "default_col", "row_groups", "row_runs", "line_blocks", "col_pairs", "col_window", "bell_row", "bell_col"]


@pytest.mark.parametrize("how", MUTATIONS)
@pytest.mark.parametrize("name", CSRMM)
def test_dcsrmm_paths(name, how):
    """?csrmm on device operands, every plan of an mm-hinted handle: row groups, row runs, the narrow kernel's line blocks, the
    column-major row pairs and LDS window, the blocked-ELL MFMA copy (both layouts, forced XCD chunk): oracle.dcsrmm's bits.  The
    default kernels on a random matrix: column-major bit for bit, row-major within the bound of test_csrmm_random_vs_oracle."""
    A, order, n, opts, want = _csrmm_case(name)
    m, k = A.m, A.n
    d = P.Descr()
    rng = np.random.default_rng(17)
    B, C0 = rng.uniform(-1, 1, k * n), rng.uniform(-1, 1, m * n)
    alpha, beta = 1.25, -0.5
    with options(**opts):
        assert L.aoclsparse_set_mm_hint(A.h, P.OP_NONE, d.h, 10) == 0 and L.aoclsparse_optimize(A.h) == 0

        def run():
            Cd = dev(C0)
            assert P.dcsrmm(P.OP_NONE, alpha, A, d, order, dev(B), n, k if order == P.ORDER_COLUMN else n, beta, Cd,
                            m if order == P.ORDER_COLUMN else n) == 0
            torch.cuda.synchronize()
            return Cd.cpu().numpy()

        close = exact
        if name == "default_row":
            def close(got, ref, what):
                Bm = B.reshape(k, n)
                scale = np.zeros((m, n))
                for i in range(m):
                    lo, hi = A.row_ptr[i], A.row_ptr[i + 1]
                    scale[i] = np.abs(A.val[lo:hi]) @ np.abs(Bm[A.col_ind[lo:hi]])
                lens = np.diff(A.row_ptr)[:, None]
                bound = (lens + 3) * EPS64 * scale * abs(alpha) + 2 * EPS64 * np.abs(beta * C0.reshape(m, n)) + 1e-300
                assert np.all(np.abs(got.reshape(m, n) - ref.reshape(m, n)) <= bound), what

        protocol(how, A, run, lambda vals: _csrmm_col_ref(vals, A, alpha, beta, B, C0, n, order), close, lambda: mm_path(A),
                 row=m // 2)
        if want is not None:  # (the default kernels of a random matrix have no plan to name)
            assert want(mm_path(A)), (name, mm_path(A))


@pytest.mark.parametrize("how", MUTATIONS)
def test_dcsrmm_transposed_and_symmetric(how):
    """op = T (through the handle's transpose): oracle.dcsrmm's bits on the CSC arrays; a symmetric descriptor (the derived
    expansion) within the bound of test_symmetric_csrmm.  (The plans of the derived matrix are not reported by any counter: step 7
    compares only what spmv_info says of the handle's own plans.)"""
    m, k, n = 1200, 1000, 12
    rp, ci, v = random_csr(132, m, k, lambda r, i: r.integers(1, 12))
    A = P.Matrix(0, m, k, rp, ci, v)
    d = P.Descr()
    rng = np.random.default_rng(3)
    B, Ct = rng.uniform(-1, 1, m * n), rng.uniform(-1, 1, k * n)

    def run_t():
        Ch = Ct.copy()
        assert P.dcsrmm(P.OP_TRANSPOSE, 2.0, A, d, P.ORDER_ROW, B, n, n, 0.5, Ch, n) == 0
        return Ch

    def expect_t(vals):
        st, cp, ri, cv = oracle.dcsr2csc(m, k, len(vals), 0, 0, rp, ci, vals)
        so, Cref = oracle.dcsrmm("col", 2.0, 0, cv, ri, cp, k, np.ascontiguousarray(B.reshape(m, n).T).ravel(), n, m, 0.5,
                                 np.ascontiguousarray(Ct.reshape(k, n).T).ravel(), k)
        return np.ascontiguousarray(Cref.reshape(n, k).T).ravel()

    protocol(how, A, run_t, expect_t, exact, lambda: spmv_path(A, P.OP_TRANSPOSE), row=m // 2)

    ms = 800
    rps, cis, vs = triangular_system(131, ms, 5)
    S = P.Matrix(0, ms, ms, rps, cis, vs)
    ds = P.Descr(mtype=P.TYPE_SYMMETRIC, fill=P.FILL_UPPER)
    Bs, Cs = rng.uniform(-1, 1, ms * n), rng.uniform(-1, 1, ms * n)
    held = {}

    def run_s():
        C = Cs.copy()
        assert P.dcsrmm(P.OP_NONE, 2.0, S, ds, P.ORDER_ROW, Bs, n, n, 0.5, C, n) == 0
        return C

    def expect_s(vals):
        o = oracle.dcsr_optimize(ms, ms, len(vals), 0, rps, cis, vals)
        D = dense(ms, ms, o["ptr"], o["ind"], o["val"])
        M = np.triu(D, 1) + np.triu(D, 1).T + np.diag(np.diag(D))
        held["scale"] = 2.0 * (np.abs(M) @ np.abs(Bs.reshape(ms, n))) + np.abs(0.5 * Cs.reshape(ms, n))
        return (2.0 * (M @ Bs.reshape(ms, n)) + 0.5 * Cs.reshape(ms, n)).ravel()

    def close_s(got, ref, what):
        assert np.all(np.abs(got - ref) <= 40 * EPS64 * held["scale"].ravel() + 1e-300), what

    protocol(how, S, run_s, expect_s, close_s, lambda: spmv_path(S), row=ms // 2)


@pytest.mark.parametrize("how", ["update", "invalidate"])
def test_dcsrmm_multi_against_the_oracle(how):
    """aoclsparse_mi355_dcsrmm_multi over three slots of device 0 (replicas cloned from the primary): after the update every slot's
    slab is oracle.dcsrmm's bits on the NEW values -- not only equal to the single-call product of the same library"""
    st, dev0, _, _ = P.device_info()
    assert st == 0
    m, rp, ci, v = standins.block_dense(12, 16, 16, seed=5)
    A = P.Matrix(0, m, m, rp, ci, v)
    d = P.Descr()
    n = 192
    rng = np.random.default_rng(77)
    B, C0 = rng.uniform(-1, 1, m * n), rng.uniform(-1, 1, m * n)
    with options(bell_xcd_chunk=3):
        assert L.aoclsparse_set_mm_hint(A.h, P.OP_NONE, d.h, 10) == 0 and L.aoclsparse_optimize(A.h) == 0

        def run():
            C = C0.copy()
            assert P.dcsrmm_multi(P.OP_NONE, 1.25, A, d, P.ORDER_ROW, B, n, n, -0.5, C, n, [dev0] * 3) == 0
            return C

        protocol(how, A, run, lambda vals: _csrmm_col_ref(vals, A, 1.25, -0.5, B, C0, n, P.ORDER_ROW), exact,
                 lambda: (spmv_path(A), L.aoclsparse_mi355_replicas_cloned(A.h)), row=m // 2)


# --------------------------------------------------------------------------------------------------
# TRSV / TRSM
# --------------------------------------------------------------------------------------------------
KIND = {(P.FILL_LOWER, P.OP_NONE): "l", (P.FILL_UPPER, P.OP_NONE): "u", (P.FILL_LOWER, P.OP_TRANSPOSE): "lt",
        (P.FILL_UPPER, P.OP_TRANSPOSE): "ut"}


def _trsv_expect(A, fill, op, unit, alpha, b, kid):
    def expect(vals):
        m = A.m
        o = oracle.dcsr_optimize(m, m, len(vals), A.base, A.row_ptr, A.col_ind, vals)
        assert o["status"] == 0
        ilend = o["idiag"] if fill == P.FILL_LOWER else o["iurow"]
        kind = KIND[(fill, op)]
        if kid == 3:
            st, x = oracle.trsv_kt(kind, 8, alpha, m, o["base"], o["val"], o["ind"], o["ptr"], ilend, b, unit)
        else:
            st, x = oracle.dtrsv(kind, alpha, m, o["base"], o["val"], o["ind"], o["ptr"], ilend, b, unit)
        assert st == 0
        return x
    return expect


def _trsv_run(A, d, op, alpha, b, kid):
    def run():
        xd = torch.full((A.m,), 7.0, dtype=torch.float64, device="cuda")
        assert P.dtrsv(op, alpha, A, d, dev(b), xd, kid=kid) == 0
        torch.cuda.synchronize()
        return xd.cpu().numpy()
    return run


def _trsv_path(A, fill, op, sched):
    i = A.trsv_info(fill, op)
    return (sched, i.levels, i.blocks, i.chunks)


@pytest.mark.parametrize("how", MUTATIONS)
@pytest.mark.parametrize("sched", [0, 1, 2, 3, 4])
def test_trsv_schedules(sched, how):
    """every forced schedule, L and U, N and T, unit and non-unit, kid 0 and 3: the serial chain on the NEW values bit for bit
    (the level-ordered triangles, the block plan and the device diagonal are rebuilt)"""
    m = 3000
    rp, ci, v = triangular_system(7 + sched, m, 4, band=60)
    b = np.random.default_rng(11).uniform(-1, 1, m)
    with trsv_schedule(P, sched):
        for fill, op in KIND:
            for unit in (False, True):
                for kid in (0, 3):
                    A = P.Matrix(0, m, m, rp, ci, v.copy())  # (a fresh handle: repeated scalings would compound)
                    d = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=fill, diag=P.DIAG_UNIT if unit else P.DIAG_NON_UNIT)
                    protocol(how, A, _trsv_run(A, d, op, 0.75, b, kid), _trsv_expect(A, fill, op, unit, 0.75, b, kid), exact,
                             lambda: _trsv_path(A, fill, op, sched), row=m // 2)


@pytest.fixture
def forced_chunks():
    assert L.aoclsparse_mi355_set_option(P.OPTION_TRSV_CHUNKS, 1) == 0
    yield
    assert L.aoclsparse_mi355_set_option(P.OPTION_TRSV_CHUNKS, -1) == 0


@pytest.mark.parametrize("how", MUTATIONS)
def test_trsv_two_level_schedule(forced_chunks, how):
    """schedule 5 (chunks of blocks, values staged per step) on the mesh factor of test_two_level_trsv_after_update_values"""
    nodes = 3000
    m, rp, ci, v = node_mesh(5, nodes, 40, np.full(nodes, 5))
    A = P.Matrix(0, m, m, rp, ci, v)
    b = np.random.default_rng(3).uniform(-1, 1, m)
    for fill, op in ((P.FILL_LOWER, P.OP_NONE), (P.FILL_UPPER, P.OP_TRANSPOSE)):
        d = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=fill)
        with trsv_schedule(P, 5):
            protocol(how, A, _trsv_run(A, d, op, 1.0, b, None), _trsv_expect(A, fill, op, False, 1.0, b, 0), exact,
                     lambda: _trsv_path(A, fill, op, 5), row=m // 2)
            assert A.trsv_info(fill, op).chunks >= 2


def _unclean(seed, m, missing):
    """a triangular system whose row m/2 is unsorted (and, if `missing`, whose row m/3 lacks its diagonal entry): the handle
    solves on a clean COPY of its arrays"""
    rp, ci, v = triangular_system(seed, m, 4, band=40)
    r = m // 2
    ci[rp[r]:rp[r + 1]] = ci[rp[r]:rp[r + 1]][::-1].copy()
    v[rp[r]:rp[r + 1]] = v[rp[r]:rp[r + 1]][::-1].copy()
    if not missing:
        return rp, ci, v
    q = m // 3
    keep = np.ones(len(ci), bool)
    keep[rp[q] + int(np.nonzero(ci[rp[q]:rp[q + 1]] == q)[0][0])] = False
    counts = np.add.reduceat(keep.astype(int), rp[:-1])
    rp2 = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return rp2, ci[keep].copy(), v[keep].copy()


@pytest.mark.parametrize("how", MUTATIONS)
@pytest.mark.parametrize("missing", [False, True])
def test_trsv_on_the_clean_copy(missing, how):
    """an unsorted row (non-unit solves: the device diagonal comes from the clean copy too) and, in addition, a missing diagonal
    entry (unit solves: a non-unit one is refused, as in the reference): the TRSV plans are built from the handle's clean copy,
    which must follow the new values"""
    m = 2000
    rp, ci, v = _unclean(21, m, missing)
    b = np.random.default_rng(5).uniform(-1, 1, m)
    for fill, op in ((P.FILL_LOWER, P.OP_NONE), (P.FILL_UPPER, P.OP_NONE), (P.FILL_LOWER, P.OP_TRANSPOSE)):
        A = P.Matrix(0, m, m, rp, ci, v.copy())
        d = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=fill, diag=P.DIAG_UNIT if missing else P.DIAG_NON_UNIT)
        protocol(how, A, _trsv_run(A, d, op, 1.0, b, None), _trsv_expect(A, fill, op, missing, 1.0, b, 0), exact,
                 lambda: _trsv_path(A, fill, op, -1), row=m // 2)
        assert A.export_diag()["is_internal"]


@pytest.mark.parametrize("how", MUTATIONS)
def test_dtrsm(how):
    """?trsm, four right-hand sides (column-major): every column the serial chain on the new values"""
    m, k = 2000, 4
    rp, ci, v = triangular_system(33, m, 4, band=50)
    A = P.Matrix(0, m, m, rp, ci, v)
    d = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=P.FILL_LOWER)
    Bm = np.random.default_rng(6).uniform(-1, 1, m * k)

    def run():
        X = np.zeros(m * k)
        assert L.aoclsparse_dtrsm(P.OP_NONE, 1.5, A.h, d.h, P.ORDER_COLUMN, P._ptr(Bm), k, m, P._ptr(X), m) == 0
        return X

    def expect(vals):
        return np.concatenate([_trsv_expect(A, P.FILL_LOWER, P.OP_NONE, False, 1.5, Bm[j * m:(j + 1) * m], 0)(vals) for j in range(k)])

    protocol(how, A, run, expect, exact, lambda: _trsv_path(A, P.FILL_LOWER, P.OP_NONE, -1), row=m // 2)


# --------------------------------------------------------------------------------------------------
# solvers
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", MUTATIONS)
def test_dsymgs_and_dsorv(how):
    """?symgs (triangular solves + the device diagonal) and ?sorv (the device CSR) against the oracle, bit for bit"""
    m = 1500
    rp, ci, v = triangular_system(44, m, 4, band=30)
    A = P.Matrix(0, m, m, rp, ci, v)
    d = P.Descr()
    rng = np.random.default_rng(8)
    b, x0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)

    def run_gs():
        x = x0.copy()
        assert L.aoclsparse_dsymgs(P.OP_NONE, A.h, d.h, 1.0, P._ptr(b), P._ptr(x)) == 0
        return x

    def expect_gs(vals):
        o = oracle.dcsr_optimize(m, m, len(vals), 0, rp, ci, vals)
        st, x = oracle.dsymgs(P.TYPE_GENERAL, P.FILL_LOWER, 0, o["base"], 1.0, m, o["val"], o["ind"], o["ptr"], o["idiag"],
                              o["iurow"], b, x0)
        assert st == 0
        return x

    protocol(how, A, run_gs, expect_gs, exact, lambda: _trsv_path(A, P.FILL_LOWER, P.OP_NONE, -1), row=m // 2)

    def run_sor():
        x = x0.copy()
        assert L.aoclsparse_dsorv(0, d.h, A.h, 0.7, 1.0, P._ptr(x), P._ptr(b)) == 0
        return x

    def expect_sor(vals):
        st, x = oracle.dsorv(m, 0, rp, ci, vals, 0.7, 1.0, x0, b)
        assert st == 0
        return x

    protocol(how, A, run_sor, expect_sor, exact, lambda: None, row=m // 3)


def _itsol(opts):
    h = ctypes.c_void_p()
    assert L.aoclsparse_itsol_d_init(ctypes.byref(h)) == 0
    for k, v in opts.items():
        assert L.aoclsparse_itsol_option_set(h, k.encode(), str(v).encode()) == 0, (k, v)
    return h


@pytest.mark.parametrize("how", MUTATIONS)
@pytest.mark.parametrize("pre,code", [("None", 0), ("SymGS", 3)])
def test_itsol_cg(pre, code, how):
    """CG (lower-stored symmetric descriptor; SymGS scales by the device diagonal) against oracle.dcg on the new values: the same
    iteration count (+-1: different dot-product trees) and the solution within 1e-6 (test_itsol_cg_laplacian_matches_restated_solver).
    The Laplacian carries 16 on its diagonal so that the scaled matrix stays diagonally dominant, hence SPD."""
    g = 40
    n, rp, ci, v = laplace5(g)
    v = np.where(v > 0, 16.0, v)
    keep = ci <= np.repeat(np.arange(n), np.diff(rp))
    lrp = np.concatenate([[0], np.cumsum(np.add.reduceat(keep.astype(int), rp[:-1]))]).astype(np.int32)
    A = P.Matrix(0, n, n, lrp, ci[keep].copy(), v[keep].copy())
    d = P.Descr(mtype=P.TYPE_SYMMETRIC, fill=P.FILL_LOWER)
    b = np.random.default_rng(71).uniform(-1, 1, n)
    held = {}

    def full(vals):
        Dl = dense(n, n, A.row_ptr, A.col_ind, vals)
        return Dl + np.tril(Dl, -1).T

    def run():
        h = _itsol({"CG Rel Tolerance": 1e-9, "CG Abs Tolerance": 0.0, "CG Preconditioner": pre, "CG Iteration Limit": 500})
        try:
            xd, rinfo = dev(np.zeros(n)), np.zeros(100)
            assert L.aoclsparse_itsol_d_solve(h, n, A.h, d.h, P._ptr(dev(b)), P._ptr(xd), P._ptr(rinfo), None, None, None) == 0
            held["iters"] = rinfo[30]
            return xd.cpu().numpy()
        finally:
            L.aoclsparse_itsol_destroy(ctypes.byref(h))

    def expect(vals):
        M = full(vals)
        r, c = np.nonzero(M)
        fp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int32)
        fi, fv = c.astype(np.int32), M[r, c]
        o = oracle.dcsr_optimize(n, n, len(fv), 0, fp, fi, fv)
        st, xo, ro = oracle.dcg(n, 0, o["ptr"], o["ind"], o["val"], o["idiag"], o["iurow"], b, np.zeros(n), 1e-9, 0.0, 500, code)
        assert st == 0
        held["ref_iters"] = ro[30]
        return xo

    def close(got, ref, what):
        assert abs(held["iters"] - held["ref_iters"]) <= 1, (what, held["iters"], held["ref_iters"])
        assert np.max(np.abs(got - ref)) < 1e-6, what

    protocol(how, A, run, expect, close, lambda: None, row=n // 2)


# --------------------------------------------------------------------------------------------------
# other ways in: CSC handles, aoclsparse_order_mat
# --------------------------------------------------------------------------------------------------
class CscMatrix(P.Matrix):
    """a handle created with aoclsparse_create_dcsc; `val` is the caller's CSC value array (what ?update_values writes)"""

    def __init__(self, m, n, rp, ci, v):
        st, cp, ri, cv = oracle.dcsr2csc(m, n, len(v), 0, 0, rp, ci, v)
        assert st == 0
        self.csc_ptr, self.csc_ind, self.val = cp.astype(np.int32), ri.astype(np.int32), np.ascontiguousarray(cv)
        self.row_ptr, self.col_ind = rp, ci  # the CSR the handle converts to (rows sorted)
        self.double, self.m, self.n, self.nnz, self.base = True, m, n, len(v), 0
        self.h = ctypes.c_void_p()
        self.status = L.aoclsparse_create_dcsc(ctypes.byref(self.h), 0, m, n, len(v), P._ptr(self.csc_ptr), P._ptr(self.csc_ind),
                                               P._ptr(self.val))
        assert self.status == 0

    def csr_vals(self, cvals):
        st, rp, ci, v = oracle.dcsr2csc(self.n, self.m, len(cvals), 0, 0, self.csc_ptr, self.csc_ind, cvals)
        assert st == 0 and np.array_equal(rp, self.row_ptr) and np.array_equal(ci, self.col_ind)
        return v


def _csc_mutate(how, A, row):
    if how == "update":
        v2 = scaled(A.val, 5)
        assert L.aoclsparse_dupdate_values(A.h, len(v2), P._ptr(v2)) == 0
        assert np.array_equal(A.val, v2)
    elif how == "invalidate":  # a write into the caller's CSC values, then aoclsparse_mi355_invalidate
        A.val[:] = scaled(A.val, 6)
        assert L.aoclsparse_mi355_invalidate(A.h) == 0
    else:  # set_value: one diagonal and one off-diagonal entry of `row`
        lo, hi = A.row_ptr[row], A.row_ptr[row + 1]
        old = A.csr_vals(A.val)
        for j, f in ((row, 1.375), (int(A.col_ind[hi - 1]) if A.col_ind[hi - 1] != row else int(A.col_ind[lo]), -0.625)):
            p = lo + int(np.nonzero(A.col_ind[lo:hi] == j)[0][0])
            assert L.aoclsparse_dset_value(A.h, row, j, float(old[p]) * f) == 0
    return A.csr_vals(A.val)


@pytest.mark.parametrize("how", MUTATIONS)
def test_csc_handle(how):
    """(c) a handle created from CSC: dmv N and T, non-unit trsv, csrmm and symmetric dmv on the new values -- after ?set_value,
    ?update_values, and a write into the caller's CSC value array followed by aoclsparse_mi355_invalidate (which refreshes the
    handle's own CSR from the CSC arrays first)"""
    m = 1500
    rp, ci, v = triangular_system(61, m, 5)
    A = CscMatrix(m, m, rp, ci, v)
    rng = np.random.default_rng(4)
    x, y0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)
    d = P.Descr()
    dt = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=P.FILL_LOWER)
    ds = P.Descr(mtype=P.TYPE_SYMMETRIC, fill=P.FILL_LOWER)
    n = 8
    B, C0 = rng.uniform(-1, 1, m * n), rng.uniform(-1, 1, m * n)

    def run():
        out = [_dmv_runner(A, d, x, y0, 1.3, -0.4)(), _dmv_runner(A, d, x, y0, 1.3, -0.4, op=P.OP_TRANSPOSE)(),
               _trsv_run(A, dt, P.OP_NONE, 1.0, x, None)(), _dmv_runner(A, ds, x, y0, 1.3, -0.4)()]
        Cd = dev(C0)
        assert P.dcsrmm(P.OP_NONE, 1.25, A, d, P.ORDER_COLUMN, dev(B), n, m, -0.5, Cd, m) == 0
        torch.cuda.synchronize()
        return out + [Cd.cpu().numpy()]

    def expect(vals):
        y = oracle.dcsrmv(-1, 0, 1.3, m, len(vals), vals, ci, rp, x, -0.4, y0)[1]
        yt = oracle.dcsrmvt(0, 1.3, m, m, vals, ci, rp, x, -0.4, y0)[1]
        xs = _trsv_expect(A, P.FILL_LOWER, P.OP_NONE, False, 1.0, x, 0)(vals)
        o = oracle.dcsr_optimize(m, m, len(vals), 0, rp, ci, vals)
        ys = oracle.dcsrmv_special("symm", o["base"], 1.3, m, m, 0, P.FILL_LOWER, o["val"], o["ind"], o["ptr"], o["idiag"],
                                   o["iurow"], x, -0.4, y0)[1]
        D = dense(m, m, rp, ci, vals)
        M = np.tril(D, -1) + np.tril(D, -1).T + np.diag(np.diag(D))
        return [y, yt, xs, ys, _csrmm_col_ref(vals, A, 1.25, -0.5, B, C0, n, P.ORDER_COLUMN), M, vals]

    got0 = run()
    ref0 = expect(A.csr_vals(A.val))
    vals = _csc_mutate(how, A, m // 2)
    got1 = run()
    ref1 = expect(vals)
    for got, ref in ((got0, ref0), (got1, ref1)):
        exact(got[0], ref[0], "dmv N")
        st, cp, ri, cv = oracle.dcsr2csc(m, m, len(v), 0, 0, rp, ci, ref[6])
        assert np.all(np.abs(got[1] - ref[1]) <= (np.diff(cp) + 4) * EPS64 * abs_row_sums(cp, ri, cv, x) * 1.3
                      + 2 * EPS64 * np.abs(0.4 * y0) + 1e-300), "dmv T"
        exact(got[2], ref[2], "trsv")
        M = ref[5]
        bound = ((M != 0).sum(axis=1) + 6) * EPS64 * (1.3 * (np.abs(M) @ np.abs(x)) + np.abs(0.4 * y0)) + 1e-300
        assert np.all(np.abs(got[3] - ref[3]) <= bound), "symmetric dmv"
        exact(got[4], ref[4], "csrmm")
    for a, b in zip(got0, got1):
        assert not np.array_equal(a, b), "the mutation did not reach the output"


def test_order_mat_after_the_plans_were_built():
    """(e) aoclsparse_order_mat sorts the caller's (unsorted) arrays in place after every plan was built from them: dmv N and T,
    non-unit trsv, csrmm and symmetric dmv then run on the sorted arrays -- same matrix, so the same oracle results, and the
    handle no longer needs its clean copy"""
    m = 1500
    rp, ci, v = triangular_system(62, m, 5)
    rng = np.random.default_rng(9)
    for i in range(m):  # every row permuted
        p = rng.permutation(rp[i + 1] - rp[i]) + rp[i]
        ci[rp[i]:rp[i + 1]], v[rp[i]:rp[i + 1]] = ci[p].copy(), v[p].copy()
    A = P.Matrix(0, m, m, rp, ci, v)
    x, y0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)
    d, dt = P.Descr(), P.Descr(mtype=P.TYPE_TRIANGULAR, fill=P.FILL_LOWER)
    ds = P.Descr(mtype=P.TYPE_SYMMETRIC, fill=P.FILL_LOWER)
    n = 8
    B, C0 = rng.uniform(-1, 1, m * n), rng.uniform(-1, 1, m * n)

    def run():
        Cd = dev(C0)
        assert P.dcsrmm(P.OP_NONE, 1.25, A, d, P.ORDER_COLUMN, dev(B), n, m, -0.5, Cd, m) == 0
        torch.cuda.synchronize()
        return [_dmv_runner(A, d, x, y0, 1.3, -0.4)(), _trsv_run(A, dt, P.OP_NONE, 1.0, x, None)(),
                _dmv_runner(A, ds, x, y0, 1.3, -0.4)(), Cd.cpu().numpy(), _dmv_runner(A, d, x, y0, 1.3, -0.4, op=P.OP_TRANSPOSE)()]

    def check(got):
        exact(got[0], oracle.dcsrmv(-1, 0, 1.3, m, len(A.val), A.val, A.col_ind, A.row_ptr, x, -0.4, y0)[1], "dmv")
        exact(got[1], _trsv_expect(A, P.FILL_LOWER, P.OP_NONE, False, 1.0, x, 0)(A.val), "trsv")
        o = oracle.dcsr_optimize(m, m, len(A.val), 0, A.row_ptr, A.col_ind, A.val)
        ys = oracle.dcsrmv_special("symm", o["base"], 1.3, m, m, 0, P.FILL_LOWER, o["val"], o["ind"], o["ptr"], o["idiag"],
                                   o["iurow"], x, -0.4, y0)[1]
        D = dense(m, m, A.row_ptr, A.col_ind, A.val)
        M = np.tril(D, -1) + np.tril(D, -1).T + np.diag(np.diag(D))
        bound = ((M != 0).sum(axis=1) + 6) * EPS64 * (1.3 * (np.abs(M) @ np.abs(x)) + np.abs(0.4 * y0)) + 1e-300
        assert np.all(np.abs(got[2] - ys) <= bound), "symmetric dmv"
        exact(got[3], _csrmm_col_ref(A.val, A, 1.25, -0.5, B, C0, n, P.ORDER_COLUMN), "csrmm")
        # op = T within the bound of test_transposed_spmv_within_bound
        so, yt = oracle.dcsrmvt(0, 1.3, m, m, A.val, A.col_ind, A.row_ptr, x, -0.4, y0)
        st, cp, ri, cv = oracle.dcsr2csc(m, m, len(A.val), 0, 0, A.row_ptr, A.col_ind, A.val)
        assert so == 0 and st == 0
        assert np.all(np.abs(got[4] - yt) <= (np.diff(cp) + 4) * EPS64 * abs_row_sums(cp, ri, cv, x) * 1.3
                      + 2 * EPS64 * np.abs(0.4 * y0) + 1e-300), "dmv T"

    check(run())
    assert A.export_diag()["is_internal"]
    assert L.aoclsparse_order_mat(A.h) == 0
    assert all(np.all(np.diff(A.col_ind[rp[i]:rp[i + 1]]) > 0) for i in range(m))
    check(run())
    assert not A.export_diag()["is_internal"]


@pytest.mark.parametrize("how", ["update", "invalidate"])
def test_order_mat_then_update(how):
    """(e) then (b) / (d): order_mat on an unsorted handle with built plans, then new values -- dmv and non-unit trsv"""
    m = 1500
    rp, ci, v = triangular_system(63, m, 5)
    for i in range(0, m, 3):
        ci[rp[i]:rp[i + 1]], v[rp[i]:rp[i + 1]] = ci[rp[i]:rp[i + 1]][::-1].copy(), v[rp[i]:rp[i + 1]][::-1].copy()
    A = P.Matrix(0, m, m, rp, ci, v)
    x = np.random.default_rng(2).uniform(-1, 1, m)
    dt = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=P.FILL_LOWER)
    _trsv_run(A, dt, P.OP_NONE, 1.0, x, None)()
    assert L.aoclsparse_order_mat(A.h) == 0
    protocol(how, A, _trsv_run(A, dt, P.OP_NONE, 1.0, x, None), _trsv_expect(A, P.FILL_LOWER, P.OP_NONE, False, 1.0, x, 0), exact,
             lambda: _trsv_path(A, P.FILL_LOWER, P.OP_NONE, -1), row=m // 2)


# --------------------------------------------------------------------------------------------------
# sp2m and ILU(0)
# --------------------------------------------------------------------------------------------------
def _export_csr(h):
    base, m, n, nnz = ctypes.c_int(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    rp, ci, v = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert L.aoclsparse_export_dcsr(h, ctypes.byref(base), ctypes.byref(m), ctypes.byref(n), ctypes.byref(nnz), ctypes.byref(rp),
                                    ctypes.byref(ci), ctypes.byref(v)) == 0
    k = max(nnz.value, 1)
    return (np.ctypeslib.as_array(ctypes.cast(rp, ctypes.POINTER(ctypes.c_int32)), (m.value + 1,)).copy(),
            np.ctypeslib.as_array(ctypes.cast(ci, ctypes.POINTER(ctypes.c_int32)), (k,))[: nnz.value].copy(),
            np.ctypeslib.as_array(ctypes.cast(v, ctypes.POINTER(ctypes.c_double)), (k,))[: nnz.value].copy())


@pytest.mark.parametrize("how", MUTATIONS)
@pytest.mark.parametrize("op", [P.OP_NONE, P.OP_TRANSPOSE])
def test_sp2m_after_updating_a(op, how):
    """sp2m (full stage) with op N / T on A after A's values changed: structure and values bit for bit (dcsr2m / csr2csc + csr2m)"""
    m = 2000
    pa, ia, va = random_csr(55, m, m, lambda r, i: r.integers(1, 8))
    for i in range(m):  # every row holds its diagonal (?set_value changes it)
        if i not in ia[pa[i]:pa[i + 1]]:
            ia[pa[i]] = i
        ia[pa[i]:pa[i + 1]] = np.sort(ia[pa[i]:pa[i + 1]])
    pb, ib, vb = random_csr(56, m, m, lambda r, i: r.integers(1, 8))
    A, B = P.Matrix(0, m, m, pa, ia, va), P.Matrix(0, m, m, pb, ib, vb)
    d = P.Descr()

    def run():
        C = ctypes.c_void_p()
        assert L.aoclsparse_sp2m(op, d.h, A.h, P.OP_NONE, d.h, B.h, P.STAGE_FULL, ctypes.byref(C)) == 0
        try:
            return np.concatenate([a.astype(np.float64) for a in _export_csr(C)])
        finally:
            assert L.aoclsparse_destroy(ctypes.byref(C)) == 0

    def expect(vals):
        if op == P.OP_NONE:
            so, pc, ic, vc = oracle.dcsr2m(m, m, 0, pa, ia, vals, 0, pb, ib, vb)
        else:
            st, cp, ri, cv = oracle.dcsr2csc(m, m, len(vals), 0, 0, pa, ia, vals)
            so, pc, ic, vc = oracle.dcsr2m(m, m, 0, cp, ri.astype(np.int32), cv, 0, pb, ib, vb)
        assert so == 0
        return np.concatenate([pc.astype(np.float64), ic.astype(np.float64), vc])

    protocol(how, A, run, expect, exact, lambda: None, row=m // 2)


def test_ilu0_factor_is_kept_across_value_updates():
    """Pinned reference semantics: the ILU(0) factor is computed ONCE, from the values seen at the first factorisation, and later
    value updates do not change it (analysis/aoclsparse_analysis.cpp: the factorisation runs only while the handle is not yet
    factorised; solvers/aoclsparse_ilu0.hpp).  After ?update_values the smoother still returns the factor of the OLD values
    (oracle.dilu0 of them) and solves with it -- do not 'fix' this away from the reference."""
    g = 30
    m, rp, ci, v = laplace5(g)
    v = np.ascontiguousarray(v * np.random.default_rng(72).uniform(0.8, 1.2, len(v)))
    A = P.Matrix(0, m, m, rp, ci, v)
    d = P.Descr()
    assert L.aoclsparse_set_lu_smoother_hint(A.h, P.OP_NONE, d.h, 10) == 0 and L.aoclsparse_optimize(A.h) == 0
    st, lu, diag = oracle.dilu0(m, 0, rp, ci, v.copy())
    assert st == 0
    b = np.random.default_rng(3).uniform(-1, 1, m)
    st, xr = oracle.dilu_solve(m, 0, diag, lu, rp, ci, b)
    assert st == 0
    pv = ctypes.c_void_p()
    for rnd in range(2):
        if rnd == 1:
            v2 = scaled(v, 11)
            assert L.aoclsparse_dupdate_values(A.h, len(v2), P._ptr(v2)) == 0
            assert not np.array_equal(oracle.dilu0(m, 0, rp, ci, v2)[1], lu)  # (a refactorisation WOULD differ)
        x = np.zeros(m)
        assert L.aoclsparse_dilu_smoother(P.OP_NONE, A.h, d.h, ctypes.byref(pv), None, P._ptr(x), P._ptr(b)) == 0
        fac = np.ctypeslib.as_array(ctypes.cast(pv, ctypes.POINTER(ctypes.c_double)), (len(v),))
        assert np.array_equal(fac, lu), rnd
        assert np.array_equal(x, xr), rnd


# --------------------------------------------------------------------------------------------------
# complex handles: the Hermitian expansion (zmv) and the conjugate-transposed TRSV plans (ztrsv, op = H)
# --------------------------------------------------------------------------------------------------
class ZMatrix(P.Matrix):
    """a double-complex handle over aliased arrays (what `mutate` needs: row_ptr, col_ind, val, base, m, h)"""

    def __init__(self, m, rp, ci, v):
        self.row_ptr, self.col_ind = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
        self.val = np.ascontiguousarray(v, np.complex128)
        self.m, self.n, self.base, self.double = m, m, 0, True
        self.h = ctypes.c_void_p()
        assert L.aoclsparse_create_zcsr(ctypes.byref(self.h), 0, m, m, len(self.val), P._ptr(self.row_ptr), P._ptr(self.col_ind),
                                        P._ptr(self.val)) == 0
        self.status, self.nnz = 0, len(self.val)


def _complex_system(seed, m):
    """a diagonally dominant square system with complex off-diagonal entries and a real diagonal (as a Hermitian matrix has)"""
    rp, ci, v = triangular_system(seed, m, 5, band=50)
    rows = np.repeat(np.arange(m), np.diff(rp))
    im = np.random.default_rng(seed + 1).uniform(-0.5, 0.5, len(v)) * (ci != rows)
    return rp, ci, v + 1j * im


@pytest.mark.parametrize("how", MUTATIONS)
@pytest.mark.parametrize("op", ["n", "h"])
def test_zmv_hermitian(op, how):
    """aoclsparse_zmv with a Hermitian descriptor (lower triangle; the derived expansion, conjugated for op = H) against oracle.zmv
    within (2 max len + 16) eps of the restated operator, the rule of test_complex_mv_every_descriptor_and_operation.  (No counter
    reports the plans of the derived matrix: step 7 compares only what spmv_info says of the handle's own plans.)"""
    m = 1200
    rp, ci, v = _complex_system(71, m)
    A = ZMatrix(m, rp, ci, v)
    d = P.Descr(mtype=P.TYPE_HERMITIAN, fill=P.FILL_LOWER)
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, m) + 1j * rng.uniform(-1, 1, m)
    y0 = rng.uniform(-1, 1, m) + 1j * rng.uniform(-1, 1, m)
    alpha, beta = np.array([0.7 - 0.4j]), np.array([-0.3 + 0.2j])
    opc = P.OP_NONE if op == "n" else P.OP_CONJ_TRANSPOSE
    held = {}

    def run():
        yd = dev(y0)
        assert L.aoclsparse_zmv(opc, P._ptr(alpha), A.h, d.h, P._ptr(dev(x)), P._ptr(beta), P._ptr(yd)) == 0
        torch.cuda.synchronize()
        return yd.cpu().numpy()

    def expect(vals):
        yr, held["scale"] = oracle.zmv(op, "hermitian", "lower", "non_unit", 0, alpha[0], m, m, rp, ci, vals, x, beta[0], y0)
        return yr

    def close(got, ref, what):
        bound = (2 * np.diff(rp).max() + 16) * EPS64 * (held["scale"] + 1e-30)
        assert np.all(np.abs(got - ref) <= bound), (what, float(np.max(np.abs(got - ref) / bound)))

    protocol(how, A, run, expect, close, lambda: spmv_path(A, opc), row=m // 2)


@pytest.mark.parametrize("how", MUTATIONS)
@pytest.mark.parametrize("fill", [P.FILL_LOWER, P.FILL_UPPER])
def test_ztrsv_conjugate_transposed(fill, how):
    """aoclsparse_ztrsv with op = H (the only user of the conjugated TRSV plans) and op = N, non-unit: x within 64 eps max|x| of a
    dense solve of the NEW triangle, the rule of the complex trsv test in test_gpu_parity.py"""
    m = 1500
    rp, ci, v = _complex_system(81 + fill, m)
    A = ZMatrix(m, rp, ci, v)
    dt = P.Descr(mtype=P.TYPE_TRIANGULAR, fill=fill)
    b = np.random.default_rng(5).uniform(-1, 1, m) + 1j * np.random.default_rng(6).uniform(-1, 1, m)
    for op in (P.OP_CONJ_TRANSPOSE, P.OP_NONE):
        def run():
            x = np.zeros(m, np.complex128)
            assert L.aoclsparse_ztrsv(op, P.CDouble(0.5, 0.5), A.h, dt.h, P._ptr(b), P._ptr(x)) == 0
            return x

        def expect(vals):
            D = np.zeros((m, m), np.complex128)
            np.add.at(D, (np.repeat(np.arange(m), np.diff(rp)), ci), vals)
            T = np.tril(D) if fill == P.FILL_LOWER else np.triu(D)
            return np.linalg.solve(T.conj().T if op == P.OP_CONJ_TRANSPOSE else T, (0.5 + 0.5j) * b)

        def close(got, ref, what):
            assert np.max(np.abs(got - ref)) <= 64 * EPS64 * max(1.0, np.max(np.abs(ref))), what

        def path():
            info = A.trsv_info(fill, op)
            assert info.levels > 0, "the solve did not run on this handle's plan for the operation"
            return (info.levels, info.blocks, info.chunks)

        protocol(how, A, run, expect, close, path, row=m // 2)


# --------------------------------------------------------------------------------------------------
# exported csrmm state: made after an update, and an update on the adopted handle itself
# --------------------------------------------------------------------------------------------------
def _adopt(A):
    """aoclsparse_mi355_mm_state_export -> device copies of the buffers (what a receiving rank holds) -> adopt; the adopted handle
    owns its arrays: the returned Matrix aliases them (row_ptr, col_ind, val are views, so a write into val reaches the handle)"""
    from aocl_sparse_amd.sharded import _DeviceView
    st, state, ptrs = A.mm_state_export()
    assert st == 0
    held = [torch.as_tensor(_DeviceView(p, n), device="cuda").clone() if n else None for p, n in zip(ptrs, list(state.bytes))]
    torch.cuda.synchronize()
    st, R = P.Matrix.mm_state_adopt(state, [t.data_ptr() if t is not None else None for t in held])
    assert st == 0
    del held
    base, m, n, nnz = ctypes.c_int(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    rp, ci, v = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert L.aoclsparse_export_dcsr(R.h, ctypes.byref(base), ctypes.byref(m), ctypes.byref(n), ctypes.byref(nnz), ctypes.byref(rp),
                                    ctypes.byref(ci), ctypes.byref(v)) == 0
    R.row_ptr = np.ctypeslib.as_array(ctypes.cast(rp, ctypes.POINTER(ctypes.c_int32)), (m.value + 1,))
    R.col_ind = np.ctypeslib.as_array(ctypes.cast(ci, ctypes.POINTER(ctypes.c_int32)), (nnz.value,))
    R.val = np.ctypeslib.as_array(ctypes.cast(v, ctypes.POINTER(ctypes.c_double)), (nnz.value,))
    return R


MM_STATE = [("block_dense", P.ORDER_ROW, 64), ("laplace", P.ORDER_COLUMN, 16), ("laplace", P.ORDER_ROW, 40)]


def _mm_state_handle(which):
    if which == "block_dense":
        m, rp, ci, v = standins.block_dense(5, 4, 4, seed=3)  # blocked-ELL copy
    else:
        m, rp, ci, v = laplace5(140)  # LDS window (column-major), line blocks (narrow row-major)
        v = v * np.random.default_rng(8).uniform(0.5, 1.5, len(v))
    A = P.Matrix(0, m, m, rp, ci, v)
    d = P.Descr()
    assert L.aoclsparse_set_mm_hint(A.h, P.OP_NONE, d.h, 10) == 0 and L.aoclsparse_optimize(A.h) == 0
    return A, d


def _mm_runner(H, d, order, n, B, C0):
    def run():
        Cd = dev(C0)
        ld = H.m if order == P.ORDER_COLUMN else n
        assert P.dcsrmm(P.OP_NONE, 1.25, H, d, order, dev(B), n, ld, -0.5, Cd, ld) == 0
        torch.cuda.synchronize()
        return Cd.cpu().numpy()
    return run


@pytest.mark.parametrize("how", MUTATIONS)
@pytest.mark.parametrize("which,order,n", MM_STATE)
def test_mm_state_exported_after_an_update(which, order, n, how):
    """the state exported AFTER a value change carries the new values: the adopted handle's product is oracle.dcsrmm's bits on
    them, on the exporter's plans (blocked ELL / LDS window / line blocks)"""
    A, d = _mm_state_handle(which)
    m = A.m
    rng = np.random.default_rng(21)
    B, C0 = rng.uniform(-1, 1, m * n), rng.uniform(-1, 1, m * n)
    run = _mm_runner(A, d, order, n, B, C0)
    got0 = run()
    exact(got0, _csrmm_col_ref(A.val.copy(), A, 1.25, -0.5, B, C0, n, order), "exporter, old values")
    p0 = mm_path(A)
    vals = mutate(how, A, m // 2)
    R = _adopt(A)  # (no product of A in between: the export itself has to rebuild what the update dropped)
    assert np.array_equal(R.val, vals)
    got1 = _mm_runner(R, d, order, n, B, C0)()
    exact(got1, _csrmm_col_ref(vals, A, 1.25, -0.5, B, C0, n, order), "adopted, new values (%s)" % how)
    assert not np.array_equal(got0, got1), "the mutation did not reach the output"
    assert mm_path(R) == p0 == mm_path(A), ("another path", p0, mm_path(R), mm_path(A))


@pytest.mark.parametrize("how", MUTATIONS)
@pytest.mark.parametrize("which,order,n", MM_STATE)
def test_update_on_the_adopted_handle(which, order, n, how):
    """a value change on the ADOPTED handle (its plans came from outside, its analysis flags say 'done'): its next product is
    oracle.dcsrmm's bits on the new values, on the same plans"""
    A, d = _mm_state_handle(which)
    R = _adopt(A)
    rng = np.random.default_rng(22)
    B, C0 = rng.uniform(-1, 1, R.m * n), rng.uniform(-1, 1, R.m * n)
    protocol(how, R, _mm_runner(R, d, order, n, B, C0), lambda vals: _csrmm_col_ref(vals, R, 1.25, -0.5, B, C0, n, order), exact,
             lambda: mm_path(R), row=R.m // 2)
