"""GPU tier: aoclsparse_mi355_sp2m_numeric_device (include/aoclsparse_mi355.h) -- the values of C = op(A) * op(B) again, from the
values the operands hold now, on the structure C has; and the plan the handle keeps for it (get_sp2m_plan_info).

Every case follows the TWIN protocol of tests/test_revalue_device_gpu.py: (1) C = sp2m(full computation) on the old values is
right; (2) the operands get new, independently drawn values, once by aoclsparse_?update_values on the host and once by
?revalue_device in HBM; (3) the numeric call; (4) export(C) is bit for bit -- row_ptr, col_ind, val -- what a fresh full
computation on fresh handles over the new values gives (all four value types: both kernels do the same arithmetic in the same
order), double also against oracle.dcsr2m; (5) C differs from (1); (6) a second numeric call with the first values restores the
bits of (1); (7) plan_builds == 1 and numeric_runs == 2.  The operands of the kernel's deciding sizes are those of
tests/spgemm_edges.py, at the sizes tests/test_gpu_spgemm_edges.py uses."""
import ctypes
from ctypes import byref, c_void_p

import numpy as np
import pytest

import oracle
import spgemm_edges as E
from test_gpu_spgemm_edges import capped, edge, handles, wrapped
from test_sy_sparse_cpu import FINAL, FULL, H, N, T, Handle, Result, export
from util import pkg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
P = pkg()
L = P.lib()
INVALID_VALUE = 5
assert P.STATUS[INVALID_VALUE] == "invalid_value"
LETTER = {np.dtype(np.float32): "s", np.dtype(np.float64): "d", np.dtype(np.complex64): "c", np.dtype(np.complex128): "z"}
DTYPES = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}
numeric = L.aoclsparse_mi355_sp2m_numeric_device


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    yield
    L.aoclsparse_mi355_set_pointer_mode(P.PTR_AUTO)


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def same_csr(x, y, what):
    """two exports, bit for bit"""
    assert (x["base"], x["m"], x["n"], x["nnz"]) == (y["base"], y["m"], y["n"], y["nnz"]), what
    for k in ("row_ptr", "col_ind", "val"):
        assert x[k].dtype == y[k].dtype and np.array_equal(bits(x[k]), bits(y[k])), (
            what, k, int(np.sum(bits(x[k]) != bits(y[k]))) if x[k].shape == y[k].shape else "shape")


def plan_info(h):
    info = P.Sp2mPlanInfo(struct_size=ctypes.sizeof(P.Sp2mPlanInfo))
    assert L.aoclsparse_mi355_get_sp2m_plan_info(h, byref(info)) == 0
    return info


def full(A, da, B, db, opa=N, opb=N, request=FULL, into=None):
    r = into or Result()
    st = L.aoclsparse_sp2m(opa, da.h, A.h, opb, db.h, B.h, request, byref(r.h))
    assert st == 0, P.STATUS[st]
    return r


def full_export(A, da, B, db, t, **kw):
    """the export of one full computation (the result handle lives until its arrays are copied)"""
    r = full(A, da, B, db, **kw)
    return export(r.h, t)


def give(Hd, v, route):
    """new values into a host-created handle: aoclsparse_?update_values, or ?revalue_device from HBM"""
    v = np.ascontiguousarray(v, dtype=Hd.val.dtype)
    if route == "host":
        st = getattr(L, "aoclsparse_%supdate_values" % Hd.t)(Hd.h, len(v), P._ptr(v))
    else:
        st = getattr(L, "aoclsparse_mi355_%srevalue_device" % Hd.t)(Hd.h, len(v), P._ptr(dev(v)))
    assert st == 0, (route, P.STATUS[st])


def draw(rng, n, dt):
    """independent values in [-1, 1) (complex: both parts), exactly representable in dt"""
    v = rng.uniform(-1, 1, n)
    if np.dtype(dt).kind == "c":
        v = v + 1j * rng.uniform(-1, 1, n)
    return v.astype(dt)


def twin_protocol(ops, dt, base_a=0, base_b=0, ref=None, seed=29):
    """ops: spgemm_edges.Operands; ref = (ops, pc, ic, vc): the double oracle on ops' own values.  -> the plan info after it all"""
    t = LETTER[np.dtype(dt)]
    rng = np.random.default_rng(seed)
    va0, vb0 = ops.A[2].astype(dt), ops.B[2].astype(dt)
    va1, vb1 = draw(rng, len(va0), dt), draw(rng, len(vb0), dt)
    # the twin: a fresh full computation on fresh handles with the new values (once, shared by both routes)
    At, Bt, dat, dbt = handles(ops, base_a, base_b, dt, va1, vb1)
    fresh = full_export(At, dat, Bt, dbt, t)
    info = None
    for route in ("host", "device"):
        A, B, da, db = handles(ops, base_a, base_b, dt, va0.copy(), vb0.copy())
        C = full(A, da, B, db)
        x0 = export(C.h, t)
        if ref is not None:  # (1)
            assert np.array_equal(x0["row_ptr"], ref[1]) and np.array_equal(x0["col_ind"], ref[2])
            if t == "d":
                assert np.array_equal(bits(x0["val"]), bits(ref[3])), "old values against the oracle"
        give(A, va1, route), give(B, vb1, route)  # (2)
        st = numeric(N, da.h, A.h, N, db.h, B.h, C.h)  # (3)
        assert st == 0, (route, P.STATUS[st])
        x1 = export(C.h, t)
        same_csr(x1, fresh, (route, "new values against the twin"))  # (4)
        if t == "d":
            st, pc, ic, vc = oracle.dcsr2m(ops.m, ops.n, 0, ops.A[0], ops.A[1], va1, 0, ops.B[0], ops.B[1], vb1)
            assert st == 0 and np.array_equal(x1["row_ptr"], pc) and np.array_equal(x1["col_ind"], ic)
            assert np.array_equal(bits(x1["val"]), bits(vc)), (route, "new values against the oracle")
        assert not np.array_equal(bits(x1["val"]), bits(x0["val"])), "the new values did not reach C"  # (5)
        give(A, va0, route), give(B, vb0, route)
        st = numeric(N, da.h, A.h, N, db.h, B.h, C.h)  # (6)
        assert st == 0, (route, P.STATUS[st])
        same_csr(export(C.h, t), x0, (route, "the first values again"))
        info = plan_info(C.h)  # (7)
        assert (info.kept, info.plan_builds, info.numeric_runs, info.refused) == (1, 1, 2, 0), route
        assert sum(info.rows_in_bin) == ops.m and info.rows_in_bin[3] == 0 and info.heavy_rows == info.rows_in_bin[4]
        assert info.plan_bytes > 0
    return info


# ---- 1. every size on which the kernel decides ------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 1])
def test_every_list_size_double(base):
    """all families of edge_operands(9000): lists of 32 / 33 / 256 / 257 / 2,048 / 2,049 / 4,096 / 4,097, rows of A and B on the
    chunk widths, repeats and descents across the chunk boundary (the serial branch); every bin populated, rows in the slab"""
    ref = edge()
    counts = np.diff(ref[1])
    for want in (32, 33, 256, 257, 2048, 2049, 4096, 4097):
        assert (counts == want).any()
    info = twin_protocol(ref[0], np.float64, base, base, ref)
    assert all(info.rows_in_bin[b] > 0 for b in (0, 1, 2, 4))
    assert info.heavy_rows == int((counts > 2048).sum()) and info.rows_in_bin[0] == int((counts <= 32).sum())


def test_capped_rows_double():
    """n = 2,048 and every list exactly full: 2,048 of the 2,048 a 4,096-slot table may hold; one bin holds every row (no order)"""
    ref = capped()
    info = twin_protocol(ref[0], np.float64, ref=ref)
    assert list(info.rows_in_bin) == [0, 0, ref[0].m, 0, 0]


@pytest.mark.parametrize("t", ["d", "s", "c", "z"])
@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("case", range(len(E.WRAP_CASES)), ids=["%d_in_%d" % (c[1], 1 << c[0]) for c in E.WRAP_CASES])
def test_probe_chains_wrap_round_the_table_end(case, descending, t):
    """every column of one row of C starts its probe in the last H / 16 slots: the inserts of phase 1 and the lookups of phase 2
    run over the end of the table, in LDS and in the slab; descending: the serial branch (the slab row: its last 128 entries)"""
    logh, entries, _, _ = E.WRAP_CASES[case]
    desc = 0 if not descending else (entries if logh < 13 else 128)
    ref = wrapped(case, desc)
    assert np.diff(ref[1]).tolist() == [entries, 3]
    info = twin_protocol(ref[0], DTYPES[t], ref=ref)
    assert info.heavy_rows == (1 if entries > 2048 else 0)


@pytest.mark.parametrize("t", ["s", "c", "z"])
def test_float_and_complex_on_the_same_edges(t):
    """the single, pair and arows families with 4-, 8- and 16-byte values (the cdouble accumulators of the 2,048 bin fill 32 KB)"""
    ref = edge(("single", "pair", "arows"))
    assert (np.diff(ref[1]) == 2048).any() and (np.diff(ref[1]) == 4097).any()
    twin_protocol(ref[0], DTYPES[t], ref=ref)


# ---- 2. signed zero -----------------------------------------------------------------------------------------------------------------
def tiny(rows, dt=np.float64):
    """dense rows -> a 0-based handle that stores every entry, zeros included"""
    a = np.array(rows, dt)
    m, n = a.shape
    return Handle(0, m, n, np.arange(m + 1, dtype=np.int32) * n, np.tile(np.arange(n, dtype=np.int32), m), a.ravel().copy())


@pytest.mark.parametrize("route", ["host", "device"])
def test_a_lone_negative_zero_product_stays_negative_zero(route):
    """A = diag(-1, 1), B = [[0, 2], [3, 0]] with the zeros stored: C(0, 0) = -1 * 0.0 is -0.0 as the reference has it (the first
    product is STORED; an accumulator that starts at +0.0 and adds would give +0.0).  Second pair: the slot's first product is
    -0.0 and a second one follows, -0.0 + (1 * -0.0) = -0.0, and with +0.0 as the second it is +0.0."""
    d = P.Descr()
    NEG, POS = np.array([-0.0]).view(np.uint64)[0], np.uint64(0)
    for a_rows, b_new, want in (([[-1.0, 0.0], [0.0, 1.0]], [[0.0, 2.0], [3.0, 0.0]], NEG),
                                ([[-1.0, 1.0], [2.0, 3.0]], [[0.0, 5.0], [-0.0, 7.0]], NEG),
                                ([[-1.0, 1.0], [2.0, 3.0]], [[0.0, 5.0], [0.0, 7.0]], POS)):
        if a_rows[0][1] == 0.0:  # diag(-1, 1): only the diagonal is stored
            A = Handle(0, 2, 2, np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.array([-1.0, 1.0]))
        else:
            A = tiny(a_rows)
        B = tiny([[1.5, 2.5], [3.5, 4.5]])
        C = full(A, d, B, d)
        give(B, np.array(b_new).ravel(), route)
        assert numeric(N, d.h, A.h, N, d.h, B.h, C.h) == 0
        x = export(C.h, "d")
        Bt = tiny(b_new)
        same_csr(x, full_export(A, d, Bt, d, "d"), "the twin")
        assert x["col_ind"][0] == 0 and x["val"][0:1].view(np.uint64)[0] == want, (b_new, x["val"])


# ---- 3. one transposed operand, chained (Galerkin) ------------------------------------------------------------------------------
def stencil5(nx, ny):
    """5-point stencil on ny lines of nx points, rows ascending -> (m, row_ptr, col_ind, position of each entry in its stencil)"""
    m = nx * ny
    r = np.arange(m)
    i, j = r // nx, r % nx
    cols = np.stack([r - nx, r - 1, r, r + 1, r + nx], axis=1)
    ok = np.stack([i > 0, j > 0, np.ones(m, bool), j < nx - 1, i < ny - 1], axis=1)
    rp = np.zeros(m + 1, np.int32)
    rp[1:] = np.cumsum(ok.sum(axis=1))
    return m, rp, cols[ok].astype(np.int32), np.broadcast_to(np.arange(5), cols.shape)[ok]


def prolongation(rng, m, n, dt):
    """m x n, 1 .. 4 entries per row in drawn (not ascending) order; every column used"""
    rows = [rng.choice(n, size=rng.integers(1, 5), replace=False) for _ in range(m)]
    for c in range(n):
        if c not in rows[c]:
            rows[c][0] = c
    rp = np.zeros(m + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    return rp, np.concatenate(rows).astype(np.int32), draw(rng, int(rp[-1]), dt)


@pytest.mark.parametrize("t, op", [("d", T), ("z", T), ("z", H)], ids=["double-T", "cdouble-T", "cdouble-H"])
@pytest.mark.parametrize("route", ["host", "device"])
def test_galerkin_chain_with_a_transposed_operand(t, op, route):
    """C1 = A P and C = op(P) C1 by full computations; A gets new values; numeric on C1, then numeric on C with B = C1, a result
    handle whose mirror followed the numeric call.  Bit for bit the twin's chain."""
    dt = DTYPES[t]
    rng = np.random.default_rng(31)
    m, rp, ci, _ = stencil5(6, 10)
    assert m == 60
    prp, pci, pv = prolongation(rng, 60, 24, dt)
    assert np.diff(prp).max() <= 4
    va0, va1 = draw(rng, len(ci), dt), draw(rng, len(ci), dt)
    d = P.Descr()

    def chain(va):
        A, Pm = Handle(0, m, m, rp, ci, va.copy()), Handle(0, 60, 24, prp, pci, pv.copy())
        C1 = full(A, d, Pm, d)
        return A, Pm, C1, full(Pm, d, C1, d, opa=op)

    A, Pm, C1, C = chain(va0)
    x0, y0 = export(C1.h, t), export(C.h, t)
    assert (y0["m"], y0["n"]) == (24, 24) and (x0["m"], x0["n"]) == (60, 24)
    _, _, C1t, Ct = twin = chain(va1)
    give(A, va1, route)
    assert numeric(N, d.h, A.h, N, d.h, Pm.h, C1.h) == 0
    assert numeric(op, d.h, Pm.h, N, d.h, C1.h, C.h) == 0
    same_csr(export(C1.h, t), export(C1t.h, t), "A P against the twin")
    y1 = export(C.h, t)
    same_csr(y1, export(Ct.h, t), "op(P) (A P) against the twin")
    assert not np.array_equal(bits(y1["val"]), bits(y0["val"]))
    give(A, va0, route)
    assert numeric(N, d.h, A.h, N, d.h, Pm.h, C1.h) == 0 and numeric(op, d.h, Pm.h, N, d.h, C1.h, C.h) == 0
    same_csr(export(C1.h, t), x0, "A P, the first values again")
    same_csr(export(C.h, t), y0, "the chain, the first values again")
    for h in (C1.h, C.h):
        i = plan_info(h)
        assert (i.kept, i.plan_builds, i.numeric_runs, i.refused) == (1, 1, 2, 0)
    del twin


# ---- 4. what C keeps ------------------------------------------------------------------------------------------------------------
def square_of_stencil(seed):
    """A = the 5-point stencil of a 24 x 24 grid with values that do not repeat (4 (1 + e) on the diagonal, -(1 + e) off it)"""
    m, rp, ci, k = stencil5(24, 24)
    e = np.random.default_rng(seed).uniform(0.0, 0.25, len(ci))
    v = np.where(k == 2, 4.0, -1.0) * (1.0 + e)
    assert len(np.unique(v)) == len(v)
    return m, rp, ci, v


def solves_and_product(Cm, b, x):
    """one dtrsv lower, one upper-transposed and one dmv with the handle -> three host vectors"""
    out = []
    for fill, op in ((P.FILL_LOWER, P.OP_NONE), (P.FILL_UPPER, P.OP_TRANSPOSE)):
        dd = P.Descr(base=Cm.base, mtype=P.TYPE_TRIANGULAR, fill=fill)
        xd = torch.zeros(Cm.m, dtype=torch.float64, device="cuda")
        st = P.dtrsv(op, 1.0, Cm, dd, dev(b), xd)
        assert st == 0, P.STATUS[st]
        torch.cuda.synchronize()
        out.append(xd.cpu().numpy())
    yd = torch.zeros(Cm.m, dtype=torch.float64, device="cuda")
    st = P.dmv(P.OP_NONE, 1.0, Cm, P.Descr(base=Cm.base), dev(x), 0.0, yd)
    assert st == 0, P.STATUS[st]
    torch.cuda.synchronize()
    return out + [yd.cpu().numpy()]


def prepared(Cm):
    """the flag, the clean CSR built in HBM, an mv hint and optimize: the handle then holds maps, plans and a SELL-64 copy"""
    assert Cm.keep_value_maps() == 0
    assert Cm.clean_device() == 0
    d = P.Descr(base=Cm.base)
    assert L.aoclsparse_set_mv_hint(Cm.h, P.OP_NONE, d.h, 100) == 0 and L.aoclsparse_optimize(Cm.h) == 0
    return Cm


def counters(Cm):
    i, k = Cm.value_map_info(), Cm.sell_keep_info()
    return i.plan_builds, i.clean_builds, k.structure_builds


def test_what_c_keeps_through_the_numeric_call():
    """C = A A for the stencil of a 24 x 24 grid: 576 rows (nine SELL-64 slices), a full diagonal, rows in first-touch order (not
    ascending: the clean CSR is a copy with a map).  C is a device handle with keep_value_maps over the product's exported arrays;
    after the numeric call nothing was analysed again and both solves and the product are the twin's bit for bit.  Control: a
    result handle taken through sp2m(stage_finalize) instead analyses everything again."""
    m, rp, ci, v0 = square_of_stencil(41)
    _, _, _, v1 = square_of_stencil(42)
    d = P.Descr()
    rng = np.random.default_rng(43)
    b, x = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m)

    def product_of(v):
        A = Handle(0, m, m, rp, ci, v.copy())
        return A, full_export(A, d, A, d, "d")

    def device_handle(e):
        Cm = P.Matrix.from_device(0, m, m, e["nnz"], dev(e["row_ptr"]), dev(e["col_ind"]), dev(e["val"]))
        assert Cm.status == 0
        return prepared(Cm)

    A, e0 = product_of(v0)
    assert e0["m"] == 576
    first_row = e0["col_ind"][e0["row_ptr"][1]:e0["row_ptr"][2]]
    assert (np.diff(first_row) < 0).any(), "first-touch order is not ascending here"
    Cm = device_handle(e0)
    old = solves_and_product(Cm, b, x)
    c0 = counters(Cm)
    assert c0[0] >= 2 and c0[1] >= 1 and c0[2] == 1, c0
    give(A, v1, "device")
    assert numeric(N, d.h, A.h, N, d.h, A.h, Cm.h) == 0
    new = solves_and_product(Cm, b, x)
    assert counters(Cm) == c0, ("something was analysed again", c0, counters(Cm))
    _, e1 = product_of(v1)
    twin = solves_and_product(device_handle(e1), b, x)
    for got, want, was in zip(new, twin, old):
        assert np.array_equal(bits(got), bits(want)) and not np.array_equal(bits(got), bits(was))
    i = plan_info(Cm.h)
    assert (i.kept, i.plan_builds, i.numeric_runs) == (1, 1, 1) and i.rows_in_bin[0] == 576
    # control: the same on a result handle, with sp2m(stage_finalize) in place of the numeric call
    A2 = Handle(0, m, m, rp, ci, v0.copy())
    r = full(A2, d, A2, d)
    Cr = prepared(P.Matrix.from_handle(r.h))
    r.h = c_void_p()  # (the wrapper owns the handle now)
    old_r = solves_and_product(Cr, b, x)
    for got, want in zip(old_r, old):
        assert np.array_equal(bits(got), bits(want))
    k0 = counters(Cr)
    give(A2, v1, "device")
    st = L.aoclsparse_sp2m(N, d.h, A2.h, N, d.h, A2.h, FINAL, byref(Cr.h))
    assert st == 0, P.STATUS[st]
    new_r = solves_and_product(Cr, b, x)
    for got, want in zip(new_r, twin):
        assert np.array_equal(bits(got), bits(want))
    k1 = counters(Cr)
    assert k1[0] > k0[0] and k1[1] > k0[1] and k1[2] > k0[2], (k0, k1)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def fetch(addr, count, dtype):
    """count elements at a device address -> numpy, by a plain ctypes hipMemcpy"""
    out = np.zeros(max(count, 1), dtype)
    hip = ctypes.CDLL(P.hip_runtime_path()[1])
    hip.hipMemcpy.argtypes = [c_void_p, c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip.hipMemcpy(P._ptr(out), c_void_p(addr), count * out.itemsize, 2) == 0  # hipMemcpyDeviceToHost
    return out[:count]


def device_bits(h, t, nnz, m):
    """the three arrays of aoclsparse_mi355_export_csr_device, copied to the host"""
    base, mm, nn, nz = ctypes.c_int(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    rp, ci, v = c_void_p(), c_void_p(), c_void_p()
    st = L.aoclsparse_mi355_export_csr_device(h, byref(base), byref(mm), byref(nn), byref(nz), byref(rp), byref(ci), byref(v))
    assert st == 0 and (mm.value, nz.value) == (m, nnz), P.STATUS.get(st, st)
    return [fetch(rp.value, m + 1, np.int32), fetch(ci.value, nnz, np.int32), fetch(v.value, nnz, DTYPES[t])]


def refusal_operands():
    """A 6 x 5 (row 2 unsorted: columns 3, 1), B 5 x 8; every row of C has a first-touch order of its own"""
    pa = np.array([0, 2, 4, 6, 8, 9, 11], np.int32)
    ia = np.array([0, 1, 1, 2, 3, 1, 0, 4, 2, 3, 4], np.int32)
    pb = np.array([0, 2, 4, 6, 8, 10], np.int32)
    ib = np.array([0, 1, 1, 2, 5, 3, 4, 2, 6, 7], np.int32)
    rng = np.random.default_rng(51)
    return (pa, ia, draw(rng, len(ia), np.float64)), (pb, ib, draw(rng, len(ib), np.float64))


@pytest.mark.parametrize("how", ["a column outside C's row", "a slot without a product", "another first-touch order",
                                 "a column twice in C's row"])
def test_refusals_leave_everything_as_it_was(how):
    (pa, ia, va), (pb, ib, vb) = refusal_operands()
    d = P.Descr()
    A, B = Handle(0, 6, 5, pa, ia, va.copy()), Handle(0, 5, 8, pb, ib, vb.copy())
    st, pc, ic, vc = oracle.dcsr2m(6, 8, 0, pa, ia, va, 0, pb, ib, vb)
    assert st == 0
    C, Abad, Bbad = None, A, B
    if how == "a column outside C's row":
        ib2 = ib.copy()
        ib2[4] = 7  # row 2 of B: columns {5, 3} -> {7, 3}; same dimensions and nnz
        Bbad = Handle(0, 5, 8, pb, ib2, vb.copy())
        st2, pc2, ic2, _ = oracle.dcsr2m(6, 8, 0, pa, ia, va, 0, pb, ib2, vb)
        assert st2 == 0 and np.array_equal(pc2, pc) and not np.array_equal(ic2, ic)
    elif how == "a slot without a product":
        ib2 = ib.copy()
        ib2[9] = 6  # row 4 of B: {6, 7} -> {6, 6}: rows 3 and 5 of C meet no new column, and their last slot (7) gets nothing
        Bbad = Handle(0, 5, 8, pb, ib2, vb.copy())
        _, pc2, ic2, _ = oracle.dcsr2m(6, 8, 0, pa, ia, va, 0, pb, ib2, vb)
        for i in range(6):  # every row of the other product is the head of C's row: nothing is out of place, two slots stay empty
            assert np.array_equal(ic2[pc2[i]:pc2[i + 1]], ic[pc[i]:pc[i] + pc2[i + 1] - pc2[i]])
        assert (np.diff(pc) - np.diff(pc2)).tolist() == [0, 0, 0, 1, 0, 1]
    elif how == "another first-touch order":
        ia2, va2 = ia.copy(), va.copy()
        ia2[4], ia2[5], va2[4], va2[5] = ia[5], ia[4], va[5], va[4]  # row 2 of A: (3, 1) -> (1, 3)
        Abad = Handle(0, 6, 5, pa, ia2, va2)
        _, pc2, ic2, _ = oracle.dcsr2m(6, 8, 0, pa, ia2, va2, 0, pb, ib, vb)
        assert np.array_equal(pc2, pc) and not np.array_equal(ic2, ic), "the order really differs"
        assert all(set(ic2[pc[i]:pc[i + 1]]) == set(ic[pc[i]:pc[i + 1]]) for i in range(6)), "... and the column sets are the same"
    else:
        ic_bad = ic.copy()
        assert ic[pc[3]:pc[4]].tolist() == [0, 1, 6, 7]
        ic_bad[pc[3] + 3] = 6  # row 3 lists column 6 twice (not its diagonal: a handle may hold that)
        C = Handle(0, 6, 8, pc, ic_bad, np.full(len(vc), 7.0))  # (other values: a refused call must leave them)
    if C is None:
        C = full(A, d, B, d)
    if how != "a column twice in C's row":  # (a good call first: the plan exists, and a refusal must leave it alone)
        assert numeric(N, d.h, A.h, N, d.h, B.h, C.h) == 0
    before = export(C.h, "d")
    i0 = plan_info(C.h)
    assert i0.refused == 0
    before_dev = device_bits(C.h, "d", before["nnz"], 6)
    st = numeric(N, d.h, Abad.h, N, d.h, Bbad.h, C.h)
    assert st == INVALID_VALUE, P.STATUS[st]
    same_csr(export(C.h, "d"), before, "the host view after a refused call")
    for got, was in zip(device_bits(C.h, "d", before["nnz"], 6), before_dev):
        assert np.array_equal(bits(got), bits(was)), "the mirror after a refused call"
    i1 = plan_info(C.h)
    assert (i1.refused, i1.numeric_runs, i1.plan_builds, i1.kept) == (1, i0.numeric_runs, i0.plan_builds, i0.kept)
    # ... and a valid call on the same C succeeds
    if how == "a column twice in C's row":
        # (no operands have this structure: the caller repairs its own col_ind, says so, and the same handle is then accepted)
        C.ind[pc[3] + 3] = 7
        assert np.array_equal(C.ind, ic) and L.aoclsparse_mi355_invalidate(C.h) == 0
        assert numeric(N, d.h, A.h, N, d.h, B.h, C.h) == 0
        assert np.array_equal(bits(C.val), bits(vc)) and np.array_equal(C.ind, ic)
        i2 = plan_info(C.h)
        assert (i2.kept, i2.plan_builds, i2.numeric_runs, i2.refused) == (1, 1, 1, 1)
        return
    v2 = draw(np.random.default_rng(52), len(va), np.float64)
    give(A, v2, "host")
    assert numeric(N, d.h, A.h, N, d.h, B.h, C.h) == 0
    _, pc3, ic3, vc3 = oracle.dcsr2m(6, 8, 0, pa, ia, v2, 0, pb, ib, vb)
    x = export(C.h, "d")
    assert np.array_equal(x["col_ind"], ic3) and np.array_equal(bits(x["val"]), bits(vc3))
    assert plan_info(C.h).numeric_runs == i0.numeric_runs + 1 and plan_info(C.h).refused == 1


# ---- 6. release of the plan --------------------------------------------------------------------------------------------------------
def test_the_plan_is_released_with_the_order_and_kept_through_value_changes():
    (pa, ia, va), (pb, ib, vb) = refusal_operands()
    d = P.Descr()
    A, B = Handle(0, 6, 5, pa, ia, va.copy()), Handle(0, 5, 8, pb, ib, vb.copy())

    def started():
        C = full(A, d, B, d)
        x = export(C.h, "d")
        assert any((np.diff(x["col_ind"][x["row_ptr"][i]:x["row_ptr"][i + 1]]) < 0).any() for i in range(6)), "a row not ascending"
        assert numeric(N, d.h, A.h, N, d.h, B.h, C.h) == 0
        i = plan_info(C.h)
        assert (i.kept, i.plan_builds, i.numeric_runs) == (1, 1, 1) and i.rows_in_bin[0] == 6
        return C, x

    # aoclsparse_order_mat: the plan goes, and C's structure is no longer the product's
    C, x = started()
    assert L.aoclsparse_order_mat(C.h) == 0
    assert plan_info(C.h).kept == 0
    assert numeric(N, d.h, A.h, N, d.h, B.h, C.h) == INVALID_VALUE
    i = plan_info(C.h)
    assert (i.kept, i.plan_builds, i.numeric_runs, i.refused) == (0, 1, 1, 1), "a plan built by a refused call is not kept"
    # sp2m(stage_finalize) into C: the plan goes (aoclsparse_mi355_invalidate), and the next numeric call builds it again
    C, x = started()
    full(A, d, B, d, request=FINAL, into=C)
    assert plan_info(C.h).kept == 0
    assert numeric(N, d.h, A.h, N, d.h, B.h, C.h) == 0
    i = plan_info(C.h)
    assert (i.kept, i.plan_builds, i.numeric_runs) == (1, 2, 2)
    same_csr(export(C.h, "d"), x, "the same product")
    # aoclsparse_?update_values on C itself: a value change, the plan stays
    junk = np.zeros(x["nnz"])
    assert L.aoclsparse_dupdate_values(C.h, len(junk), P._ptr(junk)) == 0
    assert plan_info(C.h).kept == 1
    assert numeric(N, d.h, A.h, N, d.h, B.h, C.h) == 0
    i = plan_info(C.h)
    assert (i.kept, i.plan_builds, i.numeric_runs) == (1, 2, 3)
    same_csr(export(C.h, "d"), x, "the product again over the junk")


@pytest.mark.parametrize("base", [0, 1])
def test_a_handle_created_over_the_products_arrays_in_either_base(base):
    """C is no result handle: created over arrays that hold the product's structure (in base 0 or 1) and other values; its mirror
    is uploaded by the call.  The caller's arrays receive the values; row_ptr and col_ind are not written."""
    (pa, ia, va), (pb, ib, vb) = refusal_operands()
    d = P.Descr()
    A, B = Handle(0, 6, 5, pa, ia, va.copy()), Handle(0, 5, 8, pb, ib, vb.copy())
    st, pc, ic, vc = oracle.dcsr2m(6, 8, 0, pa, ia, va, 0, pb, ib, vb)
    assert st == 0
    C = Handle(base, 6, 8, pc + base, ic + base, np.full(len(vc), 7.0))
    assert numeric(N, d.h, A.h, N, d.h, B.h, C.h) == 0
    assert np.array_equal(bits(C.val), bits(vc)) and np.array_equal(C.ptr, pc + base) and np.array_equal(C.ind, ic + base)
    x = export(C.h, "d")
    assert x["base"] == base and np.array_equal(bits(x["val"]), bits(vc))
    got = device_bits(C.h, "d", len(vc), 6)
    assert np.array_equal(got[0], pc + base) and np.array_equal(got[1], ic + base) and np.array_equal(bits(got[2]), bits(vc))
