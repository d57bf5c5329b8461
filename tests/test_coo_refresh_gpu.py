"""New values for a CSR handle that kept the map of its triplet sort: aoclsparse_mi355_create_?csr_from_coo_device with
aoclsparse_mi355_coo_keep_map, aoclsparse_mi355_?refresh_values_from_coo_device, aoclsparse_mi355_get_coo_map_info
(device_handle_api.cpp, coo_sort_kernels.hip) and Matrix.refresh_from_coo_device / Matrix.coo_map_info.

The yardstick throughout is a FRESH creation: after refresh(v2) the handle's host view (aoclsparse_export_?csr) and its resident
arrays (export_csr_device, copied back) must equal -- integers exactly, values bitwise -- those of a new handle created WITHOUT the
flag from (row, col, v2).  That creation is pinned against the host route and against sum_reference by
tests/test_coo_device_gpu.py, whose helpers are used here.

T = P.COO_SORT_TILE; the `keep` kernel takes 8 x 256 = 2048 entries per workgroup, the `sum` kernel 256 runs, and a run of more than
64 entries is walked by a wavefront: the sizes below lie around all of these."""
import numpy as np
import pytest

import oracle
import test_coo_device_gpu as C
from util import pkg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
P = pkg()
L = P.lib()
T = P.COO_SORT_TILE

SUCCESS, INVALID_POINTER, INVALID_SIZE, INVALID_VALUE, WRONG_TYPE = 0, 2, 3, 5, 9
KEEP, SUM, MAP = P.COO_KEEP, P.COO_SUM, P.COO_KEEP_MAP
DTYPES = [np.float32, np.float64, np.complex64, np.complex128]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    yield
    L.aoclsparse_mi355_set_pointer_mode(P.PTR_AUTO)


def refreshable(base, m, n, row, col, val, mode, nnz=None):
    D = C.device_route(base, m, n, row, col, val, mode | MAP, nnz=nnz)
    assert D.status == 0, P.STATUS.get(D.status)
    return D


def refresh(D, v2, length=None, letter=None):
    """?refresh_values_from_coo_device with a device copy of v2 (which is wiped afterwards: the handle keeps nothing of it)"""
    t = C.dev_arr(v2)
    torch.cuda.synchronize()
    fn = getattr(L, "aoclsparse_mi355_%srefresh_values_from_coo_device" % (letter or D.letter))
    st = fn(D.h, len(v2) if length is None else length, P._ptr(t))
    t.zero_()
    torch.cuda.synchronize()
    return st


def arrays(D, dtype):
    return C.handle_arrays(D, np.dtype(dtype))


def same(a, b):
    return a[0] == b[0] and all(C.same_bits(np.asarray(x), np.asarray(y)) for x, y in zip(a[1:], b[1:]))


def assert_like_fresh(D, base, m, n, row, col, v2, mode):
    """the refreshed handle against a new one created without the flag from (row, col, v2) -> the arrays"""
    F = C.device_route(base, m, n, row, col, v2, mode)
    assert F.status == 0, P.STATUS.get(F.status)
    got, want = arrays(D, v2.dtype), arrays(F, v2.dtype)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert C.same_bits(got[3], want[3]), "the refreshed values are not a fresh creation's"
    return got


def with_repeats(row, col, val, every=10, off_diagonal_only=False):
    """every `every`-th coordinate once more, with another value, at the end (off_diagonal_only: `keep` refuses a second
    diagonal entry in a row)"""
    rep = np.arange(0, len(val), every)
    if off_diagonal_only:
        rep = rep[row[rep] != col[rep]]
    return np.concatenate([row, row[rep]]), np.concatenate([col, col[rep]]), np.concatenate([val, (0.25 * val[rep]).astype(val.dtype)])


def other_values(seed, like):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, len(like))
    if like.dtype.kind == "c":
        v = v + 1j * rng.uniform(-1, 1, len(like))
    return v.astype(like.dtype)


# --------------------------------------------------------------------------------------------------
# keep mode: the gather
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nnz", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, T - 1, T, T + 1, 3 * T + 17])
def test_keep_entry_counts(nnz):
    """around the wavefront, the 256 lanes of a workgroup, the 2048 entries a workgroup of the gather takes, and the sort's tile"""
    m, n = 300, 280
    row, col, val = C.random_triplets(nnz, m, n, nnz)
    D = refreshable(0, m, n, row, col, val, KEEP)
    before = arrays(D, np.float64)
    v2 = other_values(nnz + 1, val)
    assert refresh(D, v2) == SUCCESS
    assert D.spmv_info().device_resident == 1
    after = assert_like_fresh(D, 0, m, n, row, col, v2, KEEP)
    assert np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2])  # row_ptr and col_ind untouched
    assert after[0] == nnz
    if nnz:
        # what `keep` means: every entry holds the value of the triplet it came from
        order = np.argsort(row, kind="stable")
        assert C.same_bits(after[3], v2[order])


# --------------------------------------------------------------------------------------------------
# sum mode: the run chain
# --------------------------------------------------------------------------------------------------
def _run_length_input():
    """the input of test_sum_run_lengths_and_runs_across_tile_boundaries (tests/test_coo_device_gpu.py): runs of 1, 2, 63, 64, 65
    and 300 equal coordinates in rows of their own, the other sorted runs across every tile boundary"""
    m, n = 40, 40
    rng = np.random.default_rng(11)
    row, col = rng.integers(0, m - 8, 3 * T + 17), rng.integers(0, n, 3 * T + 17)
    extra_r, extra_c = [], []
    for k, length in enumerate((1, 2, 63, 64, 65, 300)):
        extra_r += [m - 8 + k] * length
        extra_c += [3 * k] * length
    row, col = np.concatenate([row, extra_r]), np.concatenate([col, extra_c])
    p = rng.permutation(len(row))
    row, col = row[p].astype(np.int32), col[p].astype(np.int32)
    val = rng.uniform(-1, 1, len(row)) * 10.0 ** rng.integers(-8, 8, len(row))
    order = np.lexsort((col, row))
    assert any((row[order][b - 1], col[order][b - 1]) == (row[order][b], col[order][b]) for b in (T, 2 * T, 3 * T))
    return m, n, row, col, val


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_sum_run_lengths_and_runs_across_tile_boundaries(dtype):
    m, n, row, col, val = _run_length_input()
    val = val.astype(dtype)
    D = refreshable(0, m, n, row, col, val, SUM)
    before = arrays(D, dtype)
    assert np.diff(before[1])[m - 8:m - 2].tolist() == [1] * 6
    rng = np.random.default_rng(12)
    v2 = (rng.uniform(-1, 1, len(row)) * 10.0 ** rng.integers(-8, 9, len(row))).astype(dtype)  # magnitudes 1e-8 .. 1e8
    assert refresh(D, v2) == SUCCESS
    assert D.spmv_info().device_resident == 1
    after = assert_like_fresh(D, 0, m, n, row, col, v2, SUM)
    rp, ci, v = C.sum_reference(0, m, row, col, v2)
    assert np.array_equal(after[1], rp) and np.array_equal(after[2], ci)
    assert C.same_bits(after[3], v), "a run was not added left to right in triplet order"
    assert np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2])
    assert not C.same_bits(after[3], before[3])


@pytest.mark.parametrize("dtype", DTYPES)
def test_sum_the_chain_order_matters(dtype):
    """the construction of the creation's test of the same name; the chain values are planted by the REFRESH"""
    run = C._chain(dtype)
    chain = run[0]
    for x in run[1:]:
        chain = chain + x
    srt = np.sort(run)
    sorted_sum = srt[0]
    for x in srt[1:]:
        sorted_sum = sorted_sum + x
    assert chain != sorted_sum and chain != np.sum(srt) and chain == np.asarray(1.0 + (1.0j if run.dtype.kind == "c" else 0)).astype(dtype)
    m, n = 70, 60
    row, col, val = C.random_triplets(8, m, n, T + 300, dtype=np.float64)
    val = val.astype(dtype) if run.dtype.kind != "c" else (val + 1j * val[::-1]).astype(dtype)
    far, close = (5, 700, T - 1, T + 250), (62, 63, 64, 65)
    for p in far:
        row[p], col[p] = 33, 44
    for p in close:
        row[p], col[p] = 34, 2
    clash = ((row == 33) & (col == 44)) | ((row == 34) & (col == 2))
    clash[list(far + close)] = False
    col[clash] += 1  # nothing else lands on the two coordinates
    D = refreshable(0, m, n, row, col, val, SUM)  # (created from the random values: no chain there yet)
    v2 = other_values(9, val)
    for k in range(4):
        v2[far[k]] = v2[close[k]] = run[k]
    assert refresh(D, v2) == SUCCESS
    _, rp, ci, v = assert_like_fresh(D, 0, m, n, row, col, v2, SUM)
    ref = C.sum_reference(0, m, row, col, v2)
    assert C.same_bits(v, ref[2])
    for r, c in ((33, 44), (34, 2)):
        seg = slice(rp[r], rp[r + 1])
        assert v[seg][ci[seg] == c][0] == chain


@pytest.mark.parametrize("mode", [KEEP, SUM])
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_all_four_value_types_both_bases_both_modes(dtype, base, mode):
    m, n = 400, 380
    row, col, val = C.shuffled(31, m, n, lambda r, i: 6, base=base, dtype=dtype)
    row, col, val = with_repeats(row, col, val, off_diagonal_only=(mode == KEEP))
    D = refreshable(base, m, n, row, col, val, mode)
    assert D.letter == C.LETTER[np.dtype(dtype)]
    info = D.coo_map_info()
    assert (info.kept, info.mode, info.triplets, info.entries) == (1, mode, len(val), D.nnz)
    assert (D.nnz < len(val)) == (mode == SUM)
    v2 = other_values(32, val)
    assert refresh(D, v2) == SUCCESS
    assert D.spmv_info().device_resident == 1
    after = assert_like_fresh(D, base, m, n, row, col, v2, mode)
    if mode == SUM:
        assert C.same_bits(after[3], C.sum_reference(base, m, row, col, v2)[2])


# --------------------------------------------------------------------------------------------------
# the flag at creation, determinism
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [KEEP, SUM])
def test_the_flag_is_inert_at_creation(mode):
    m, n = 900, 800
    row, col, val = C.random_triplets(6, m, n, 3 * T + 17)
    plain = C.device_route(0, m, n, row, col, val, mode)
    D = C.device_route(0, m, n, row, col, val, mode | MAP)
    assert plain.status == 0 and D.status == 0, (P.STATUS.get(plain.status), P.STATUS.get(D.status))
    assert D.nnz == plain.nnz and D.spmv_info().device_resident == 1
    assert same(arrays(D, np.float64), arrays(plain, np.float64))
    assert C.probe(D) == C.probe(plain)
    assert plain.coo_map_info().kept == 0 and D.coo_map_info().kept == 1


@pytest.mark.parametrize("mode", [KEEP, SUM])
def test_refresh_is_deterministic_and_reproduces_the_creation(mode):
    m, n = 900, 800
    row, col, val = C.random_triplets(6, m, n, 3 * T + 17)
    D = refreshable(0, m, n, row, col, val, mode)
    created = arrays(D, np.float64)
    v2 = other_values(7, val)
    assert refresh(D, v2) == SUCCESS
    first = arrays(D, np.float64)
    assert not C.same_bits(first[3], created[3])
    assert refresh(D, v2) == SUCCESS
    assert same(arrays(D, np.float64), first)  # two refreshes with one v2
    assert refresh(D, val) == SUCCESS
    assert same(arrays(D, np.float64), created)  # the creation's own values give the creation's bytes


# --------------------------------------------------------------------------------------------------
# derived state
# --------------------------------------------------------------------------------------------------
def _transposed(m, n, rp, ci, v):
    """the CSR arrays of A^T (zero-based), columns of a row in ascending order"""
    rows = np.repeat(np.arange(m), np.diff(rp))
    order = np.lexsort((rows, ci))
    tp = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=n))]).astype(np.int32)
    return tp, rows[order].astype(np.int32), v[order]


def _assembled():
    m, n = 1500, 1400
    row, col, val = C.random_triplets(12, m, n, 2 * T + 5, diag_free=False)
    row[1::10], col[1::10] = row[0::10][:len(row[1::10])], col[0::10][:len(col[1::10])]  # every tenth one repeated
    return m, n, row, col, val


def test_derived_state_is_dropped_dmv_and_transposed_dmv():
    m, n, row, col, val = _assembled()
    D = refreshable(0, m, n, row, col, val, SUM)
    nnz, rp, ci, v = arrays(D, np.float64)
    assert nnz < len(val)
    rng = np.random.default_rng(13)
    x, y0, xt, yt0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), rng.uniform(-1, 1, n)
    d = P.Descr(base=0)

    def dmv_t():
        yd = C.dev(yt0)
        assert P.dmv(P.OP_TRANSPOSE, 1.3, D, d, C.dev(xt), -0.4, yd) == 0
        torch.cuda.synchronize()
        return yd.cpu().numpy()

    assert L.aoclsparse_set_mv_hint(D.h, P.OP_NONE, d.h, 10) == 0
    assert L.aoclsparse_optimize(D.h) == 0
    so, yr = oracle.dcsrmv(-1, 0, 1.3, m, nnz, v, ci, rp, x, -0.4, y0)
    y1 = C.run_dmv(D, x, y0)
    assert so == 0 and np.all(np.abs(y1 - yr) <= C.dmv_bound(0, rp, ci, v, x, y0))
    yt1 = dmv_t()
    v2 = other_values(14, val)
    assert refresh(D, v2) == SUCCESS
    assert D.spmv_info().device_resident == 1
    nnz2, rp2, ci2, w = assert_like_fresh(D, 0, m, n, row, col, v2, SUM)
    assert nnz2 == nnz and np.array_equal(rp2, rp) and np.array_equal(ci2, ci)
    so, yr2 = oracle.dcsrmv(-1, 0, 1.3, m, nnz, w, ci, rp, x, -0.4, y0)
    y2 = C.run_dmv(D, x, y0)
    assert so == 0 and np.all(np.abs(y2 - yr2) <= C.dmv_bound(0, rp, ci, w, x, y0)), "a copy of the old values was used"
    assert not np.array_equal(y2, y1) and np.linalg.norm(y2 - y1) > 1e-3
    tp, ti, tv = _transposed(m, n, rp, ci, w)
    so, ytr = oracle.dcsrmv(-1, 0, 1.3, n, nnz, tv, ti, tp, xt, -0.4, yt0)
    yt2 = dmv_t()
    assert so == 0 and np.all(np.abs(yt2 - ytr) <= C.dmv_bound(0, tp, ti, tv, xt, yt0)), "the transpose holds old values"
    assert not np.array_equal(yt2, yt1)


def test_derived_state_is_dropped_dcsrmm():
    m, n, row, col, val = _assembled()
    k = 4
    D = refreshable(0, m, n, row, col, val, SUM)
    nnz, rp, ci, v = arrays(D, np.float64)
    rng = np.random.default_rng(15)
    B, C0 = rng.uniform(-1, 1, (k, n)), rng.uniform(-1, 1, (k, m))  # column j of the column-major operands is row j here
    d = P.Descr(base=0)

    def mm():
        cd = C.dev(C0)
        assert P.dcsrmm(P.OP_NONE, 1.3, D, d, P.ORDER_COLUMN, C.dev(B), k, n, -0.4, cd, m) == 0
        torch.cuda.synchronize()
        return cd.cpu().numpy()

    def check(out, vals):
        for j in range(k):
            so, yr = oracle.dcsrmv(-1, 0, 1.3, m, nnz, vals, ci, rp, B[j], -0.4, C0[j])
            assert so == 0 and np.all(np.abs(out[j] - yr) <= C.dmv_bound(0, rp, ci, vals, B[j], C0[j])), j

    assert L.aoclsparse_optimize(D.h) == 0
    c1 = mm()
    check(c1, v)
    v2 = other_values(16, val)
    assert refresh(D, v2) == SUCCESS
    w = C.sum_reference(0, m, row, col, v2)[2]
    c2 = mm()
    check(c2, w)
    assert not np.array_equal(c2, c1)


# --------------------------------------------------------------------------------------------------
# statuses
# --------------------------------------------------------------------------------------------------
def test_statuses():
    m, n = 200, 190
    row, col, val = C.random_triplets(17, m, n, 900)
    row, col, val = with_repeats(row, col, val)
    # created without the flag: no map
    plain = C.device_route(0, m, n, row, col, val, SUM)
    assert plain.status == 0 and refresh(plain, val) == INVALID_VALUE
    D = refreshable(0, m, n, row, col, val, SUM)
    assert D.nnz != len(val)
    created = arrays(D, np.float64)
    # the handle's nnz is not the triplet count
    assert refresh(D, val[:D.nnz]) == INVALID_SIZE
    assert refresh(D, val, length=len(val) + 1) == INVALID_SIZE
    # a float handle through the double entry point, and the other way round
    F = refreshable(0, m, n, row, col, val.astype(np.float32), SUM)
    assert refresh(F, val, letter="d") == WRONG_TYPE
    assert refresh(D, val.astype(np.float32), letter="s") == WRONG_TYPE
    # a host array in automatic pointer mode: refused, and nothing was written
    L.aoclsparse_mi355_set_pointer_mode(P.PTR_AUTO)
    host = np.ascontiguousarray(other_values(18, val))
    assert L.aoclsparse_mi355_drefresh_values_from_coo_device(D.h, len(host), P._ptr(host)) == INVALID_POINTER
    assert same(arrays(D, np.float64), created)
    assert D.spmv_info().device_resident == 1
    # the size comes before the type
    assert refresh(F, val[:5], letter="d") == INVALID_SIZE


@pytest.mark.parametrize("mode", [KEEP, SUM])
def test_no_triplets(mode):
    one = np.zeros(1, np.int32)
    D = refreshable(0, 5, 5, one, one, np.zeros(1), mode, nnz=0)
    info = D.coo_map_info()
    assert (info.kept, info.mode, info.triplets, info.entries) == (1, mode, 0, 0)
    assert refresh(D, np.zeros(1), length=0) == SUCCESS
    nnz, rp, ci, v = arrays(D, np.float64)
    assert nnz == 0 and np.array_equal(rp, np.zeros(6, np.int32))
    assert refresh(D, np.zeros(1), length=1) == INVALID_SIZE
    assert L.aoclsparse_mi355_drefresh_values_from_coo_device(D.h, 0, None) == INVALID_POINTER


# --------------------------------------------------------------------------------------------------
# the map's lifetime
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [KEEP, SUM])
def test_the_map_survives_value_changes(mode):
    m, n = 200, 190
    row, col, val = C.random_triplets(19, m, n, T + 40)
    D = refreshable(0, m, n, row, col, val, mode)
    nnz, rp, ci, v = arrays(D, np.float64)
    # ?set_value: the mirror is dropped, the map is not
    assert L.aoclsparse_dset_value(D.h, int(row[0]), int(col[0]), 123.0) == 0
    assert D.coo_map_info().kept == 1
    v2 = other_values(20, val)
    assert refresh(D, v2) == SUCCESS
    assert_like_fresh(D, 0, m, n, row, col, v2, mode)
    # ?update_values_device
    t = C.dev(np.full(nnz, 7.0))
    torch.cuda.synchronize()
    assert D.update_values_device(t) == 0
    assert np.all(arrays(D, np.float64)[3] == 7.0) and D.coo_map_info().kept == 1
    v3 = other_values(21, val)
    assert refresh(D, v3) == SUCCESS
    assert D.spmv_info().device_resident == 1
    assert_like_fresh(D, 0, m, n, row, col, v3, mode)
    # aoclsparse_optimize and aoclsparse_mi355_invalidate
    assert L.aoclsparse_optimize(D.h) == 0 and L.aoclsparse_mi355_invalidate(D.h) == 0
    assert D.coo_map_info().kept == 1
    assert refresh(D, v2) == SUCCESS
    assert_like_fresh(D, 0, m, n, row, col, v2, mode)


def test_order_mat_drops_the_map():
    m, n = 200, 190
    row, col, val = C.random_triplets(22, m, n, 900)
    D = refreshable(0, m, n, row, col, val, KEEP)
    _, rp, ci, v = arrays(D, np.float64)
    assert any(np.any(np.diff(ci[rp[i]:rp[i + 1]]) < 0) for i in range(m)), "the rows are unsorted: order_mat moves entries"
    assert D.coo_map_info().kept == 1
    assert L.aoclsparse_order_mat(D.h) == 0
    info = D.coo_map_info()
    assert (info.kept, info.mode, info.triplets, info.entries, info.map_bytes) == (0, 0, 0, 0, 0)
    assert refresh(D, val) == INVALID_VALUE
    _, rp2, ci2, v2 = arrays(D, np.float64)
    assert all(np.all(np.diff(ci2[rp2[i]:rp2[i + 1]]) >= 0) for i in range(m))


# --------------------------------------------------------------------------------------------------
# introspection
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [KEEP, SUM])
def test_coo_map_info(mode):
    m, n = 300, 280
    row, col, val = C.random_triplets(23, m, n, T + 77)
    row, col, val = with_repeats(row, col, val, off_diagonal_only=(mode == KEEP))
    D = refreshable(0, m, n, row, col, val, mode)
    info = D.coo_map_info()
    triplets, entries = len(val), D.nnz
    assert entries == (triplets if mode == KEEP else len(set(zip(row.tolist(), col.tolist()))))
    assert (info.kept, info.mode, info.triplets, info.entries) == (1, mode, triplets, entries)
    assert info.map_bytes >= 4 * triplets
    if mode == SUM:
        assert info.map_bytes >= 4 * (triplets + entries + 1)
    assert info.map_bytes <= 4 * (triplets + entries + 1) + 4096
    plain = C.device_route(0, m, n, row, col, val, mode)
    pi = plain.coo_map_info()
    assert (pi.kept, pi.mode, pi.triplets, pi.entries, pi.map_bytes) == (0, 0, 0, 0, 0)


# --------------------------------------------------------------------------------------------------
# Python layer
# --------------------------------------------------------------------------------------------------
def test_from_torch_coo_refreshable():
    m, n = 300, 260
    row, col, val = C.random_triplets(14, m, n, T + 77, diag_free=False)
    idx = torch.from_numpy(np.stack([row, col]).astype(np.int64))
    t = torch.sparse_coo_tensor(idx, torch.from_numpy(val), size=(m, n)).cuda()
    v2 = other_values(24, val)
    t2 = torch.sparse_coo_tensor(idx, torch.from_numpy(v2), size=(m, n)).cuda()
    assert not t.is_coalesced()
    A = P.Matrix.from_torch_coo(t, refreshable=True)
    assert A.status == 0 and A.nnz < len(val) and A.coo_map_info().kept == 1 and A.coo_map_info().mode == SUM
    torch.cuda.synchronize()
    assert A.refresh_from_coo_device(t2._values()) == SUCCESS
    B = P.Matrix.from_torch_coo(t2)
    assert B.status == 0 and B.coo_map_info().kept == 0
    assert same(arrays(A, np.float64), arrays(B, np.float64))
    assert A.spmv_info().device_resident == 1
    # keep mode through from_coo_device
    colk = np.where(col == row, (col + 1) % n, col).astype(np.int32)  # (`keep` refuses a second diagonal entry in a row)
    tr, tc, tv, tv2 = C.dev(row), C.dev(colk), C.dev(val), C.dev(v2)
    torch.cuda.synchronize()
    K = P.Matrix.from_coo_device(0, m, n, len(val), tr, tc, tv, duplicates=KEEP, refreshable=True)
    assert K.status == 0 and K.coo_map_info().mode == KEEP and K.refresh_from_coo_device(tv2) == SUCCESS
    assert_like_fresh(K, 0, m, n, row, colk, v2, KEEP)
