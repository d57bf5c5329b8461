// trsv_plan.cpp -- the analysis behind aoclsparse_?trsv / ?trsm: the triangle one (fill, op) variant walks, its level sets, the
// blocked (supernodal) plan with its slices, the two-level chunk plan and the plan-time model that chooses between them.
//
// Runs once per (fill, op) at aoclsparse_optimize after aoclsparse_set_sv_hint, or lazily on the first solve (ensure_trsv),
// mirroring the reference's lazy aoclsparse_csr_csc_optimize (level2/aoclsparse_trsv.cpp:128).  The checks, the schedule choice
// and the C entry points are in trsv_api.cpp, the kernels in trsv_kernels.hip.
#include "trsv_schedule.hpp"

#include <initializer_list>
#include <system_error>
#include <thread>
#include <tuple>

#include <cstdlib>

#include <algorithm>
#include <cstring>
#include <type_traits>

namespace mi355
{

// Host view of the strict triangle one (fill, op) variant walks: row i depends on the rows listed in
// [ptr[i], ptr[i+1]) of ind (0-based), val in the order the reference's chain applies them.
// nnz-sized scratch that every element of is written before it is read: NOT zero-filled (a std::vector of 25 M entries costs
// ~30 ms of single-threaded zeroing and page faults per array; here the first touch happens in the parallel fill loops)
template <typename U>
struct RawArray
{
    std::unique_ptr<U[]> p;
    size_t               n = 0;
    RawArray()             = default;
    explicit RawArray(size_t count) { resize(count); }
    void resize(size_t count)
    {
        p.reset(new U[count]); // default-initialised: no fill for arithmetic types
        n = count;
    }
    U       *data() { return p.get(); }
    const U *data() const { return p.get(); }
    U       *begin() { return p.get(); }
    const U *begin() const { return p.get(); }
    U       *end() { return p.get() + n; }
    const U *end() const { return p.get() + n; }
    size_t   size() const { return n; }
    U       &operator[](size_t i) { return p[i]; }
    const U &operator[](size_t i) const { return p[i]; }
};

// Hundreds of MB of analysis scratch take tens of ms to give back to the kernel (munmap of page-faulted memory): the 25 M-entry
// shell-like factor spent 40 of its 95 ms of block-plan time in destructors.  The arrays are moved into a box that a detached
// thread deletes, off the caller's critical path (if no thread can be started they are freed here, as before).
template <typename... Ts>
static void free_later(Ts &&...xs)
{
    auto *box = new(std::nothrow) std::tuple<std::decay_t<Ts>...>(std::move(xs)...);
    if(!box)
        return; // (the arguments are destroyed by their owners)
    try
    {
        std::thread([box] { delete box; }).detach();
    }
    catch(const std::system_error &)
    {
        delete box;
    }
}

template <typename T>
struct Triangle
{
    std::vector<aoclsparse_int> ptr;
    RawArray<aoclsparse_int>    ind;
    RawArray<T>                 val;
    // value map (only for a handle that keeps them, else empty): src[q] = the 0-based position of val[q] in the clean value array
    RawArray<aoclsparse_int>    src;
    bool                        descending = false; // solve order m-1..0 (dependencies point to larger rows)
    aoclsparse_int len(aoclsparse_int i) const { return ptr[i + 1] - ptr[i]; }
    aoclsparse_int row_at(aoclsparse_int k, aoclsparse_int m) const { return descending ? m - 1 - k : k; } // k-th row in solve order
};

// MAPS: also t.src (decided at compile time: the loops without it are the ones they were)
template <typename T, bool MAPS>
static void build_triangle(const HostCsr &c, bool upper, bool transposed, bool conj, Triangle<T> &t)
{
    const aoclsparse_int  m = c.m, b = c.base;
    const aoclsparse_int *s = upper ? c.iurow : c.ptr; // strict triangle of row i: [s[i], e[i]) in base b
    const aoclsparse_int *e = upper ? c.ptr + 1 : c.idiag;
    const T              *v = static_cast<const T *>(c.val);
    t.ptr.assign((size_t)m + 1, 0);
    if(!transposed)
    {
        // L: rows ascending, entries left to right (ref_trsv_l); U: rows descending (ref_trsv_u)
        for(aoclsparse_int i = 0; i < m; i++)
            t.ptr[i + 1] = t.ptr[i] + (e[i] - s[i]);
        t.ind.resize((size_t)std::max(t.ptr[m], 1));
        t.val.resize((size_t)std::max(t.ptr[m], 1));
        if constexpr(MAPS)
            t.src.resize((size_t)std::max(t.ptr[m], 1));
        parallel_for(m, 1 << 16, [&](long long i0, long long i1) {
            for(aoclsparse_int i = (aoclsparse_int)i0; i < (aoclsparse_int)i1; i++)
                for(aoclsparse_int p = s[i] - b, q = t.ptr[i]; p < e[i] - b; p++, q++)
                {
                    t.ind[q] = c.ind[p] - b;
                    t.val[q] = v[p];
                    if constexpr(MAPS)
                        t.src[q] = p;
                }
        });
        t.descending = upper;
        return;
    }
    // transposed solves are column sweeps (ref_trsv_lth / _uth): x_c receives a_ic * x_i from every
    // stored (i, c).  Row form on the transposed triangle: row c lists the i's.  L^T: sweep i = m-1..0,
    // so x_c is updated in DESCENDING i; U^T: i = 0..m-1, ascending.
    for(aoclsparse_int i = 0; i < m; i++)
        for(aoclsparse_int p = s[i] - b; p < e[i] - b; p++)
            t.ptr[c.ind[p] - b + 1]++;
    for(aoclsparse_int j = 0; j < m; j++)
        t.ptr[j + 1] += t.ptr[j];
    t.ind.resize((size_t)std::max(t.ptr[m], 1));
    t.val.resize((size_t)std::max(t.ptr[m], 1));
    if constexpr(MAPS)
        t.src.resize((size_t)std::max(t.ptr[m], 1));
    std::vector<aoclsparse_int> next(t.ptr.begin(), t.ptr.end() - 1);
    const bool                  desc_fill = !upper; // L^T: fill from the largest source row down
    for(aoclsparse_int ii = 0; ii < m; ii++)
    {
        const aoclsparse_int i = desc_fill ? m - 1 - ii : ii;
        for(aoclsparse_int p = s[i] - b; p < e[i] - b; p++)
        {
            const aoclsparse_int q = next[c.ind[p] - b]++;
            t.ind[q]               = i;
            t.val[q]               = v[p];
            if constexpr(MAPS)
                t.src[q] = p;
        }
    }
    t.descending = !upper; // L^T is upper triangular: x_c needs x_i, i > c
    if(conj) // op = H: the column sweep applies conj(a_ic) (ref_trsv_lth / _uth with the conjugating accessor)
        for(auto &a : t.val)
            a = conj_of(a);
}

using Ints = std::vector<aoclsparse_int>;

// The triangle re-laid out in a given order of its rows (position k holds row rowmap[k], pos[] is the inverse): entries in
// chain order, dependencies rewritten as POSITIONS in that order.
template <typename T>
struct Layout
{
    Ints                     pptr;
    RawArray<aoclsparse_int> pind;
    RawArray<T>              pval;
    RawArray<aoclsparse_int> psrc; // t.src in the same order (empty when the triangle has none)
};
template <typename T>
static void layout_triangle(const Triangle<T> &t, const Ints &rowmap, const Ints &pos, Layout<T> &L)
{
    const aoclsparse_int m = (aoclsparse_int)rowmap.size();
    L.pptr.assign((size_t)m + 1, 0);
    L.pind.resize(t.ind.size());
    L.pval.resize(t.val.size());
    for(aoclsparse_int k = 0; k < m; k++)
        L.pptr[k + 1] = L.pptr[k] + t.len(rowmap[k]);
    if(t.src.size()) // the value map in a pass of its own: the loop below is the one it was
    {
        L.psrc.resize(t.src.size());
        parallel_for(m, 1 << 16, [&](long long k0, long long k1) {
            for(aoclsparse_int k = (aoclsparse_int)k0; k < (aoclsparse_int)k1; k++)
                std::copy(t.src.begin() + t.ptr[rowmap[k]], t.src.begin() + t.ptr[rowmap[k] + 1], L.psrc.begin() + L.pptr[k]);
        });
    }
    parallel_for(m, 1 << 16, [&](long long k0, long long k1) {
        for(aoclsparse_int k = (aoclsparse_int)k0; k < (aoclsparse_int)k1; k++)
        {
            const aoclsparse_int i = rowmap[k], len = t.len(i);
            for(aoclsparse_int j = 0; j < len; j++)
                L.pind[L.pptr[k] + j] = pos[t.ind[t.ptr[i] + j]];
            std::copy(t.val.begin() + t.ptr[i], t.val.begin() + t.ptr[i + 1], L.pval.begin() + L.pptr[k]);
        }
    });
}

// host arrays to device buffers, in order; stops at the first failure
struct Upload
{
    DeviceBuffer &to;
    const void   *from;
    size_t        bytes;
};
static aoclsparse_status upload_all(hipStream_t st, std::initializer_list<Upload> list)
{
    for(const Upload &u : list)
    {
        const aoclsparse_status rc = u.to.upload(u.from, u.bytes, st);
        if(rc != aoclsparse_status_success)
            return rc;
    }
    return aoclsparse_status_success;
}
static Upload ints(DeviceBuffer &to, const Ints &v, size_t count)
{
    return {to, v.data(), sizeof(aoclsparse_int) * count};
}
static Upload ints(DeviceBuffer &to, const Ints &v)
{
    return ints(to, v, v.size());
}

// level[i] = 1 + max level of the rows row i depends on; rows bucketed by level (counting sort,
// ascending row index inside a level); then the triangle is re-laid out in that order and the hybrid
// schedule (runs of narrow levels vs. wide levels) is derived.
template <typename T>
static aoclsparse_status build_levels(aoclsparse_int m, const Triangle<T> &t, TrsvPlan &plan, bool do_layout)
{
    LapTimer       lt;
    Ints           level((size_t)m, 0);
    aoclsparse_int nlev = 0;
    for(aoclsparse_int k = 0; k < m; k++)
    {
        const aoclsparse_int i  = t.row_at(k, m);
        aoclsparse_int       lv = 0;
        for(aoclsparse_int p = t.ptr[i]; p < t.ptr[i + 1]; p++)
            lv = std::max(lv, level[t.ind[p]] + 1);
        level[i] = lv;
        nlev     = std::max(nlev, lv + 1);
    }
    plan.level_ptr.assign((size_t)nlev + 1, 0);
    for(aoclsparse_int i = 0; i < m; i++)
        plan.level_ptr[level[i] + 1]++;
    plan.max_width = 0;
    for(aoclsparse_int l = 0; l < nlev; l++)
    {
        plan.max_width = std::max(plan.max_width, plan.level_ptr[l + 1]);
        plan.level_ptr[l + 1] += plan.level_ptr[l];
    }
    Ints next(plan.level_ptr.begin(), plan.level_ptr.end() - 1);
    Ints rowmap((size_t)m);
    for(aoclsparse_int i = 0; i < m; i++)
        rowmap[next[level[i]]++] = i;
    plan.nlevels = nlev;
    plan.nnz_tri = t.ptr[m];

    lt.lap("levels: level pass + buckets");
    if(!do_layout)
        return aoclsparse_status_success;
    // level-ordered copy of the triangle; dependencies are rewritten as POSITIONS in that order
    Ints pos((size_t)m);
    for(aoclsparse_int k = 0; k < m; k++)
        pos[rowmap[k]] = k;
    Layout<T> L;
    layout_triangle(t, rowmap, pos, L);
    lt.lap("levels: layout");
    // level slices (<= 64 positions, inside one level) for the slice-per-wavefront sync-free kernel
    Ints slices;
    slices.reserve((size_t)m / 48 + (size_t)nlev + 2);
    for(aoclsparse_int l = 0; l < nlev; l++)
        for(aoclsparse_int k = plan.level_ptr[l]; k < plan.level_ptr[l + 1]; k += 64)
            slices.push_back(k);
    slices.push_back(m);
    plan.nslices = (aoclsparse_int)slices.size() - 1;
    // hybrid schedule
    plan.segments.clear();
    plan.launches = 0;
    for(aoclsparse_int l = 0; l < nlev;)
    {
        const bool     narrow = plan.level_ptr[l + 1] - plan.level_ptr[l] <= TRSV_NARROW;
        aoclsparse_int e      = l + 1;
        while(e < nlev && ((plan.level_ptr[e + 1] - plan.level_ptr[e] <= TRSV_NARROW) == narrow))
            e++;
        // a lone narrow level between wide ones is cheaper as an ordinary launch
        plan.segments.push_back({l, e, narrow && e - l > 1});
        plan.launches += (narrow && e - l > 1) ? 1 : e - l;
        l = e;
    }
    lt.lap("levels: slices + segments");
    aoclsparse_status rc = upload_all(Runtime::get().stream(),
                                            {ints(plan.rowmap, rowmap, (size_t)m), ints(plan.levels, plan.level_ptr, (size_t)nlev + 1),
                                             ints(plan.pptr, L.pptr, (size_t)m + 1), {plan.pind, L.pind.data(), sizeof(aoclsparse_int) * L.pind.size()},
                                             {plan.pval, L.pval.data(), sizeof(T) * L.pval.size()}, ints(plan.slices, slices)});
    plan.psrc.release(); // (never a leftover of an earlier layout)
    if(rc == aoclsparse_status_success && L.psrc.size())
        rc = plan.psrc.upload(L.psrc.data(), sizeof(aoclsparse_int) * L.psrc.size(), Runtime::get().stream());
    lt.lap("levels: upload");
    plan.rows_valid = rc == aoclsparse_status_success;
    free_later(std::move(L.pind), std::move(L.pval), std::move(L.psrc), std::move(rowmap), std::move(pos), std::move(L.pptr),
               std::move(level));
    return rc;
}

// ---- the blocked (supernodal) plan, stage by stage: see TrsvBlockPlan and trsv_block_kernel -------------------------------------
// A row joins the block of the row its chain applies last
// (round 4: wherever that row is numbered; rounds 2-3: only the predecessor in solve order) when its dependency list -- in the order the reference's chain applies it
// -- is exactly the predecessor's list with the predecessor itself
//   * appended at the END  (L, L^T, U^T: the chain runs over the far rows first, the nearest last), or
//   * put at the FRONT     (U: ref_trsv_u walks the row left to right, so the row solved last comes first);
// the block stays within TRSV_BLK_ROWS rows, TRSV_BLK_EXT external dependencies and TRSV_BLK_NV entries.  One triangle
// uses one of the two forms (whichever groups more rows).  Built only when it pays: >= 1.6 rows per block on average.

// does `row` (lj entries) chain onto `prev` (lq entries)?  front = the predecessor is the FIRST entry
template <typename T>
static bool chains(const Triangle<T> &t, aoclsparse_int row, aoclsparse_int prev, bool front)
{
    const aoclsparse_int  lq = t.len(prev), lj = t.len(row);
    const aoclsparse_int *a = &t.ind[t.ptr[row]], *q = &t.ind[t.ptr[prev]];
    if(lj != lq + 1 || a[front ? 0 : lq] != prev)
        return false;
    return lq == 0 || std::memcmp(a + (front ? 1 : 0), q, sizeof(aoclsparse_int) * (size_t)lq) == 0;
}

// One grouping = blocks (bptr / brows), their levels, the widest block and the most external dependencies a multi-row
// block has.
struct Grouping
{
    Ints           bptr, brows, blev;
    aoclsparse_int nlev = 0;
    int            max_rows = 1, max_ext = 0;
    bool           front = false;
    aoclsparse_int nb() const { return (aoclsparse_int)bptr.size() - 1; }
    aoclsparse_int rows(aoclsparse_int bq) const { return bptr[bq + 1] - bptr[bq]; }
    aoclsparse_int first_row(aoclsparse_int bq) const { return brows[bptr[bq]]; } // the row of the block that is solved first
    Ints           block_of(aoclsparse_int m) const // block (natural index) of every row
    {
        Ints bof((size_t)m);
        for(aoclsparse_int bq = 0; bq < nb(); bq++)
            for(aoclsparse_int k = bptr[bq]; k < bptr[bq + 1]; k++)
                bof[brows[k]] = bq;
        return bof;
    }
};

// 1. blocks = CHAINS of the dependency structure (round 4; rounds 2-3 took ranges of the solve order, which only finds the
// chains of a matrix whose chained rows are numbered consecutively -- the dofs of a mesh node in natural order -- and lost
// them all on a renumbered mesh: 7,315 row levels at 0.62 us instead of ~1,100 block levels).  Row j can continue row p's
// block when p is the dependency its chain applies LAST (or FIRST, form `front`) and the rest of its list is exactly p's
// list: then everything j waits for outside the block, p's block has already waited for.  Every row has at most one
// follower (the first candidate in solve order).  A block's first row is solved before every other row of it, and the
// blocks' dependencies point to blocks with an earlier first row only: numbered by first row they are in topological order.
// The kernel is compiled for blocks of up to 5 rows (every value in registers across the wait) and up to TRSV_BLK_ROWS
// (row by row, values in LDS): when only a few chains run longer than 5 rows they are cut at 5, so that one long chain does
// not put the whole solve on the slower shape.
// ext_cap: a block is only grown from a first row with at most that many entries.
template <typename T>
static void group_chains(aoclsparse_int m, const Triangle<T> &t, int ext_cap, Grouping &G)
{
    Ints              follower((size_t)m), bptr, brows;
    std::vector<char> taken((size_t)m);
    for(int form = 0; form < 2; form++)
    {
        const bool front = form == 1;
        std::fill(follower.begin(), follower.end(), (aoclsparse_int)-1);
        for(aoclsparse_int k = 0; k < m; k++)
        {
            const aoclsparse_int j = t.row_at(k, m), lj = t.len(j);
            if(lj == 0)
                continue;
            const aoclsparse_int pr = t.ind[t.ptr[j] + (front ? 0 : lj - 1)];
            if(follower[pr] < 0 && chains(t, j, pr, front))
                follower[pr] = j;
        }
        for(int cap : {TRSV_BLK_ROWS, 5})
        {
            bptr.clear(), brows.clear();
            bptr.reserve((size_t)m / 2 + 2), brows.reserve((size_t)m);
            std::fill(taken.begin(), taken.end(), 0);
            aoclsparse_int longer = 0;
            for(aoclsparse_int k = 0; k < m; k++)
            {
                aoclsparse_int j = t.row_at(k, m);
                if(taken[j])
                    continue;
                bptr.push_back((aoclsparse_int)brows.size());
                brows.push_back(j), taken[j] = 1;
                const aoclsparse_int n0 = t.len(j);
                aoclsparse_int       rows = 1, total = n0;
                if(n0 <= ext_cap)
                    while(rows < cap)
                    {
                        const aoclsparse_int f = follower[j];
                        if(f < 0 || taken[f] || total + t.len(f) > TRSV_BLK_NV)
                            break;
                        brows.push_back(f), taken[f] = 1;
                        total += t.len(f), rows++, j = f;
                    }
                longer += (rows > 5);
            }
            if(longer == 0 || longer * 10 >= (aoclsparse_int)bptr.size())
                break; // nothing to cut, or long chains are the rule: keep them
        }
        bptr.push_back((aoclsparse_int)brows.size());
        if(G.bptr.empty() || bptr.size() < G.bptr.size())
            G.bptr = bptr, G.brows = brows, G.front = front;
        if((G.bptr.size() - 1) * 16 <= (size_t)m * 10)
            break; // this form already groups the rows
    }
    const aoclsparse_int nb = G.nb();
    G.max_rows = 1, G.max_ext = 0;
    for(aoclsparse_int bq = 0; bq < nb; bq++)
    {
        const int rows = G.rows(bq);
        G.max_rows     = std::max(G.max_rows, rows);
        // a single row longer than the cap is served by the kernel's tail loop: it does not widen the unrolled part
        if(rows > 1 || t.len(G.first_row(bq)) <= ext_cap)
            G.max_ext = std::max(G.max_ext, std::min<int>(t.len(G.first_row(bq)), ext_cap));
    }
    // block levels (a block's external dependencies are those of its first-solved row; blocks are numbered by first row in
    // solve order, so every dependency's block is already levelled)
    const Ints bof = G.block_of(m);
    G.blev.assign((size_t)nb, 0);
    G.nlev = 0;
    for(aoclsparse_int bq = 0; bq < nb; bq++)
    {
        const aoclsparse_int r  = G.first_row(bq);
        aoclsparse_int       lv = 0;
        for(aoclsparse_int p = t.ptr[r]; p < t.ptr[r + 1]; p++)
            lv = std::max(lv, G.blev[bof[t.ind[p]]] + 1);
        G.blev[bq] = lv;
        G.nlev     = std::max(G.nlev, lv + 1);
    }
}

// 2. the blocks in level order: lptr (first block of every level), order (natural index of the k-th block), bfirst (first
// position of the k-th block) and the positions of the rows (in solve order inside a block)
struct BlockOrder
{
    Ints lptr, order, bfirst, rowmap, pos;
};
template <typename T>
static void order_blocks(aoclsparse_int m, const Triangle<T> &t, const Grouping &G, BlockOrder &O)
{
    const Ints          &bptr = G.bptr, &brows = G.brows, &blev = G.blev;
    const aoclsparse_int nb = G.nb(), nlev = G.nlev;
    // blocks in level order (stable)
    Ints &lptr = O.lptr, &order = O.order;
    lptr.assign((size_t)nlev + 1, 0);
    for(aoclsparse_int bq = 0; bq < nb; bq++)
        lptr[blev[bq] + 1]++;
    for(aoclsparse_int l = 0; l < nlev; l++)
        lptr[l + 1] += lptr[l];
    order.resize((size_t)nb);
    Ints next(lptr.begin(), lptr.end() - 1);
    for(aoclsparse_int bq = 0; bq < nb; bq++)
        order[next[blev[bq]]++] = bq;
    // ... and inside a level, by the place of a block's LAST dependency in the level below (stable: the natural order where that says
    // nothing -- a mesh numbered line by line is left as it is).  Neighbours in a slice then wait for the same producer slices: fan-in of a
    // slice 15.7 -> 13.5 on the unstructured shell-like factor, L 3.15 -> 3.00 ms, U 3.25 -> 3.06 (profiles/r6/trsv_chunk_experiments.txt
    // v17; the first, the mean or two levels of dependencies as the key: the same within 1 %).  Positions change, chains do not: same bits.
    {
        const Ints bofx = G.block_of(m);
        Ints       rank((size_t)nb, 0);
        for(aoclsparse_int k = lptr[0]; k < lptr[1]; k++)
            rank[order[k]] = k - lptr[0];
        std::vector<std::pair<aoclsparse_int, aoclsparse_int>> keyed;
        for(aoclsparse_int l = 1; l < nlev; l++)
        {
            keyed.clear();
            for(aoclsparse_int k = lptr[l]; k < lptr[l + 1]; k++)
            {
                const aoclsparse_int bq = order[k], r = G.first_row(bq);
                aoclsparse_int       key = -1;
                for(aoclsparse_int p = t.ptr[r]; p < t.ptr[r + 1]; p++)
                {
                    const aoclsparse_int d = bofx[t.ind[p]];
                    if(blev[d] == l - 1)
                        key = std::max(key, rank[d]);
                }
                keyed.push_back({key, bq});
            }
            std::stable_sort(keyed.begin(), keyed.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
            for(size_t i = 0; i < keyed.size(); i++)
                order[lptr[l] + (aoclsparse_int)i] = keyed[i].second, rank[keyed[i].second] = (aoclsparse_int)i;
        }
    }
    O.bfirst.assign((size_t)nb + 1, 0), O.rowmap.resize((size_t)m), O.pos.resize((size_t)m);
    for(aoclsparse_int k = 0; k < nb; k++)
    {
        const aoclsparse_int bq = order[k];
        O.bfirst[k + 1]         = O.bfirst[k] + (bptr[bq + 1] - bptr[bq]);
        for(aoclsparse_int kk = bptr[bq], q = O.bfirst[k]; kk < bptr[bq + 1]; kk++, q++)
            O.rowmap[q] = brows[kk], O.pos[brows[kk]] = q;
    }
}

// 4. slices of <= 64 (or 32) blocks inside one block level: the first block of every slice and nb; followed by each slice's
// block level, and the first slice of each level (nlev + 1 entries): the kernel's gate counts finished slices per level.
// Returns the fan-in of a slice of 64 blocks in fan_in.
static Ints slice_blocks(aoclsparse_int m, const Grouping &G, const BlockOrder &O, const Ints &pptr, const RawArray<aoclsparse_int> &pind,
                         double &fan_in)
{
    const Ints          &lptr = O.lptr, &bfirst = O.bfirst;
    const aoclsparse_int nb = G.nb(), nlev = G.nlev;
    Ints                 slices;
    // How many blocks share a wavefront.  A slice starts when the LAST dependency of its 64 blocks is in; when those dependencies come from
    // many producer slices (an irregular numbering: 15.7 on average on the unstructured shell-like factor, 3.6 on the structured one --
    // there a slice waits for the slices at the same place one and two levels down), narrower slices wait for less: slices of 32 blocks
    // 3.42 -> 3.14 ms on the unstructured factor (48: 3.30, 40: 3.22, 24: 3.16, 16: 3.41), and 1.86 -> 2.19 on the structured one, whose
    // slices are full either way (profiles/r6/trsv_chunk_experiments.txt).  Fan-in above 8: 32 blocks per slice.
    int SW = 64;
    {
        Ints blk_of_pos((size_t)m), slice_of_blk((size_t)nb), seen;
        for(aoclsparse_int k = 0; k < nb; k++)
            for(aoclsparse_int q = bfirst[k]; q < bfirst[k + 1]; q++)
                blk_of_pos[q] = k;
        aoclsparse_int ns = 0;
        for(aoclsparse_int l = 0; l < nlev; l++)
            for(aoclsparse_int k = lptr[l]; k < lptr[l + 1]; k += 64, ns++)
                for(aoclsparse_int kk = k; kk < std::min<aoclsparse_int>(k + 64, lptr[l + 1]); kk++)
                    slice_of_blk[kk] = ns;
        long long fan = 0;
        for(aoclsparse_int l = 0; l < nlev; l++)
            for(aoclsparse_int k = lptr[l]; k < lptr[l + 1]; k += 64)
            {
                seen.clear();
                for(aoclsparse_int kk = k; kk < std::min<aoclsparse_int>(k + 64, lptr[l + 1]); kk++)
                    for(aoclsparse_int p = pptr[bfirst[kk]]; p < pptr[bfirst[kk] + 1]; p++)
                        seen.push_back(slice_of_blk[blk_of_pos[pind[p]]]);
                std::sort(seen.begin(), seen.end());
                fan += std::unique(seen.begin(), seen.end()) - seen.begin();
            }
        fan_in = ns > 0 ? (double)fan / (double)ns : 0.0;
        if(fan_in > 8.0)
            SW = 32;
    }
    for(aoclsparse_int l = 0; l < nlev; l++)
        for(aoclsparse_int k = lptr[l]; k < lptr[l + 1]; k += SW)
            slices.push_back(k);
    slices.push_back(nb);
    const size_t ns = slices.size() - 1;
    for(size_t q = 0; q < ns; q++)
        slices.push_back(G.blev[O.order[slices[q]]]);
    aoclsparse_int first = 0;
    for(aoclsparse_int l = 0; l < nlev; l++)
    {
        slices.push_back(first);
        first += (lptr[l + 1] - lptr[l] + SW - 1) / SW;
    }
    slices.push_back(first);
    return slices;
}

// ---- 5. the two-level schedule (TrsvChunkPlan): chunks of consecutive blocks in natural order, each walked in block-level order
constexpr int TRSV_CHUNK_NBS = 64 / TRSV_CHUNK_LANES; // blocks per step
constexpr int TRSV_CHUNK_NCW = TRSV_CHUNK_WAVES - 1; // wavefronts that take steps (the last one fetches the halo)

// the chunk plan on the host (the layout of the device arrays: TrsvChunkPlan in internal.hpp)
struct Chunks
{
    bool           fits = true; // false: a block does not fit a chunk of its own
    Ints           kof, chunk_of, bof2; // per natural block: index in block-level order, chunk; bof2: natural block index of a row
    Ints           cfirst; // first block (natural index) of every chunk
    Ints           stamp; // per row: scratch of the halo counts
    Ints           steps, cptr, crows, hptr, hcount, hind, slot_of;
    Ints           eptr, cind;
    aoclsparse_int maxslots = 0;
    aoclsparse_int nch() const { return (aoclsparse_int)cfirst.size() - 1; }
};

// chunks of consecutive blocks: at most `cap` rows, and rows + halo (the rows of EARLIER chunks it depends on) within slots_max
template <typename T>
static void cut_chunks(aoclsparse_int m, const Triangle<T> &t, const Grouping &G, const BlockOrder &O, aoclsparse_int cap,
                       aoclsparse_int slots_max, Chunks &C)
{
    const aoclsparse_int nb = G.nb();
    C.kof.resize((size_t)nb), C.chunk_of.resize((size_t)nb);
    for(aoclsparse_int k = 0; k < nb; k++)
        C.kof[O.order[k]] = k;
    C.bof2 = G.block_of(m);
    C.stamp.assign((size_t)m, -1); // row counted in the halo of chunk stamp[row]
    aoclsparse_int rows = 0, halo = 0, c = 0, bq0 = 0;
    C.cfirst.push_back(0);
    for(aoclsparse_int bq = 0; bq < nb && C.fits; bq++)
    {
        const aoclsparse_int r = G.rows(bq), first = G.first_row(bq);
        for(;;)
        {
            aoclsparse_int add = 0;
            for(aoclsparse_int p = t.ptr[first]; p < t.ptr[first + 1]; p++)
                if(C.bof2[t.ind[p]] < bq0 && C.stamp[t.ind[p]] != c)
                    C.stamp[t.ind[p]] = c, add++;
            if(rows + r <= cap && rows + r + halo + add <= slots_max)
            {
                rows += r, halo += add;
                break;
            }
            if(rows == 0) // a block that does not fit a chunk of its own (a row with ~15,000 dependencies)
            {
                C.fits = false;
                break;
            }
            C.cfirst.push_back(bq), c++, bq0 = bq, rows = 0, halo = 0; // close the chunk in front of this block; count again
        }
        C.chunk_of[bq] = c;
    }
    C.cfirst.push_back(nb);
}

// the steps of every chunk (8 words each), the LDS slot of every position and the halos in the order of first use
template <typename T>
static void chunk_steps(aoclsparse_int m, const Triangle<T> &t, const Grouping &G, const BlockOrder &O, Chunks &C)
{
    const Ints          &bfirst = O.bfirst, &blev = G.blev, &order = O.order;
    const aoclsparse_int nch = C.nch();
    C.cptr.assign((size_t)nch + 1, 0), C.crows.assign((size_t)nch, 0), C.hptr.assign((size_t)nch + 1, 0), C.hcount.assign((size_t)nch, 0);
    C.slot_of.resize((size_t)m);
    Ints                                                   &steps = C.steps, ks;
    std::vector<std::pair<aoclsparse_int, aoclsparse_int>> hl; // (first step that needs it, position)
    steps.reserve((size_t)G.nb());
    for(aoclsparse_int c = 0; c < nch && C.fits; c++)
    {
        ks.clear();
        for(aoclsparse_int bq = C.cfirst[c]; bq < C.cfirst[c + 1]; bq++)
            ks.push_back(C.kof[bq]);
        std::sort(ks.begin(), ks.end()); // = (block level, natural index): the level order is stable
        aoclsparse_int slot = 0;
        hl.clear();
        for(size_t i = 0; i < ks.size();)
        {
            size_t               j  = i + 1;
            const aoclsparse_int lv = blev[order[ks[i]]];
            while(j < ks.size() && j - i < (size_t)TRSV_CHUNK_NBS && ks[j] == ks[j - 1] + 1 && blev[order[ks[j]]] == lv)
                j++;
            // header of the step, 8 words: first block (index in block-level order), position of its first row, LDS slot of
            // that row, rows of the (<= 8) blocks as nibbles; rows in front of block j as bytes (2 words), rows of the step, blocks
            unsigned cw = 0, pre[2] = {0, 0};
            int      rows_before = 0;
            const aoclsparse_int sidx = (aoclsparse_int)(steps.size() / 8);
            for(size_t q = i; q < j; q++)
            {
                const int rws = bfirst[ks[q] + 1] - bfirst[ks[q]];
                cw |= (unsigned)rws << (4 * (q - i));
                pre[(q - i) / 4] |= (unsigned)rows_before << (8 * ((q - i) % 4));
                rows_before += rws;
                const aoclsparse_int first = O.rowmap[bfirst[ks[q]]];
                for(aoclsparse_int p = t.ptr[first]; p < t.ptr[first + 1]; p++)
                    if(C.chunk_of[C.bof2[t.ind[p]]] != c && C.stamp[t.ind[p]] != -2 - c) // the halo: first use decides the order
                        C.stamp[t.ind[p]] = -2 - c, hl.emplace_back(sidx, O.pos[t.ind[p]]);
            }
            steps.push_back(ks[i]), steps.push_back(bfirst[ks[i]]), steps.push_back(slot), steps.push_back((aoclsparse_int)cw);
            steps.push_back((aoclsparse_int)pre[0]), steps.push_back((aoclsparse_int)pre[1]), steps.push_back(rows_before);
            steps.push_back((aoclsparse_int)(j - i));
            for(aoclsparse_int q = bfirst[ks[i]]; q < bfirst[ks[j - 1] + 1]; q++)
                C.slot_of[q] = slot++;
            i = j;
        }
        std::sort(hl.begin(), hl.end());
        for(size_t i = 0; i < hl.size(); i++)
            C.hind.push_back(hl[i].second);
        C.hcount[c] = (aoclsparse_int)hl.size();
        while(C.hind.size() % 4)
            C.hind.push_back(0); // (the fetching wavefront reads four positions per lane with one load)
        C.crows[c]    = slot;
        C.hptr[c + 1] = (aoclsparse_int)C.hind.size();
        C.maxslots    = std::max<aoclsparse_int>(C.maxslots, slot + (aoclsparse_int)hl.size());
        C.cptr[c + 1] = (aoclsparse_int)(steps.size() / 8);
    }
}

// external dependency lists (those of a block's first-solved row), indexed like bfirst; every entry an LDS slot of the
// block's chunk.  hslot[] of a position is valid for ONE chunk at a time, so the lists are written chunk by chunk.
template <typename T>
static void chunk_dependency_lists(aoclsparse_int m, const Triangle<T> &t, const Grouping &G, const BlockOrder &O, Chunks &C)
{
    const aoclsparse_int nb = G.nb();
    C.eptr.assign((size_t)nb + 1, 0);
    for(aoclsparse_int k = 0; k < nb; k++)
        C.eptr[k + 1] = C.eptr[k] + t.len(O.rowmap[O.bfirst[k]]);
    C.cind.assign((size_t)C.eptr[nb] + 256, 0); // (padded: the kernel reads whole rounds of 64 words)
    Ints hslot((size_t)(C.fits ? m : 0));
    for(aoclsparse_int c = 0; c < C.nch() && C.fits; c++)
    {
        for(aoclsparse_int i = C.hptr[c]; i < C.hptr[c] + C.hcount[c]; i++)
            hslot[C.hind[i]] = C.crows[c] + (i - C.hptr[c]);
        for(aoclsparse_int bq = C.cfirst[c]; bq < C.cfirst[c + 1]; bq++)
        {
            const aoclsparse_int k = C.kof[bq], r = O.rowmap[O.bfirst[k]];
            for(aoclsparse_int jj = 0; jj < t.len(r); jj++)
            {
                const aoclsparse_int dep = t.ind[t.ptr[r] + jj];
                C.cind[C.eptr[k] + jj]   = C.chunk_of[C.bof2[dep]] == c ? C.slot_of[O.pos[dep]] : hslot[O.pos[dep]];
            }
        }
    }
}

// 6. plan-time model of both schedules (costs in us from the traces: profiles/r5/trsv_experiments.txt, profiles/r6/): a step
// = the later of {its wavefront free + the latency of its values, its last dependency + the hand-off} + the work
// (round 6, profiles/r6/trsv_chunk_trace*.txt: a hand-off through LDS 0.45, solving a step 0.4, a wavefront's loads for a step
// 1.7, a value of another chunk 2.5 us after it was produced)
// (FRONT: the rows of a block are phases one after the other, ~0.08 us each on top)
struct ChunkModel
{
    double model_us, model_block_us; // the two-level schedule (0 where it cannot be built) / the lane-per-block one
};
template <typename T>
static ChunkModel model_chunks(const Triangle<T> &t, const Grouping &G, const BlockOrder &O, const Chunks &C, double slice_fan_in)
{
    const int    max_rows = G.max_rows, max_ext = G.max_ext;
    const double work = G.front ? 0.4 + 0.08 * max_rows : 0.4, local = 0.45, remote = 2.5, vals = 1.7;
    double       total = 0.0;
    if(C.fits)
    {
        std::vector<double> fin((size_t)G.nb(), 0.0);
        for(aoclsparse_int c = 0; c < C.nch(); c++)
        {
            double wfree[TRSV_CHUNK_NCW] = {0};
            for(aoclsparse_int sidx = C.cptr[c]; sidx < C.cptr[c + 1]; sidx++)
            {
                const int            w    = (int)((sidx - C.cptr[c]) % TRSV_CHUNK_NCW);
                double               when = wfree[w] + vals;
                const aoclsparse_int kf = C.steps[8 * (size_t)sidx], kn = kf + C.steps[8 * (size_t)sidx + 7];
                for(aoclsparse_int k = kf; k < kn; k++)
                {
                    const aoclsparse_int r = O.rowmap[O.bfirst[k]];
                    for(aoclsparse_int jj = t.ptr[r]; jj < t.ptr[r + 1]; jj++)
                    {
                        const aoclsparse_int d = C.bof2[t.ind[jj]];
                        when = std::max(when, fin[d] + (C.chunk_of[d] == c ? local : remote));
                    }
                }
                const double f = when + work;
                for(aoclsparse_int k = kf; k < kn; k++)
                    fin[O.order[k]] = f;
                wfree[w] = f;
                total    = std::max(total, f);
            }
        }
    }
    // (the lane-per-block schedule, measured per block level: 1.69 us with every block in registers, 2.51 us with the larger shape)
    return {total, (double)G.nlev * (max_rows <= 5 ? (max_ext <= 16 ? 1.7 : (max_ext <= 20 ? (slice_fan_in > 8.0 ? 2.15 : 2.35) : 2.55)) : 2.55)};
}

// chunk cutting, steps / halo, dependency lists, the model and -- where the model (or the trsv_chunks option) says so -- the upload
template <typename T>
static aoclsparse_status build_chunk_plan(aoclsparse_int m, const Triangle<T> &t, const Grouping &G, const BlockOrder &O,
                                          TrsvBlockPlan &bp, hipStream_t st, LapTimer &lt)
{
    TrsvChunkPlan &cp = bp.chunk;
    // rows per chunk: as many as the LDS holds next to the chunk's halo (the rows of EARLIER chunks it depends on, copied into
    // LDS by the fetching wavefront), but at least ~32 chunks on large triangles (a chunk streams its part of the matrix with
    // one workgroup)
    // (the kernel is compiled for four shapes; the larger ones leave less LDS for the chunk's words: trsv_chunk_slots)
    const aoclsparse_int slots_max = trsv_chunk_slots(trsv_chunk_bs(G.max_rows), trsv_chunk_ext(G.max_ext));
    static const char   *cap_env   = getenv("AOCLSPARSE_MI355_TRSV_CHUNK_ROWS"); // (diagnostics: rows per chunk)
    const aoclsparse_int cap       = cap_env ? std::min<aoclsparse_int>(slots_max, std::max(64, atoi(cap_env)))
                                             : std::min<aoclsparse_int>(slots_max, std::max<aoclsparse_int>(2048, m / 32));
    Chunks C;
    cut_chunks(m, t, G, O, cap, slots_max, C);
    chunk_steps(m, t, G, O, C);
    chunk_dependency_lists(m, t, G, O, C);
    const ChunkModel model = model_chunks(t, G, O, C, bp.slice_fan_in);
    cp.model_us = model.model_us, cp.model_block_us = model.model_block_us;
    lt.lap("chunks: steps + dependency lists + model");
    // aoclsparse_mi355_set_option(trsv_chunks, ...): -1 the model decides (default), 0 never, 1 whenever the plan can be built
    const int want = plan_option(aoclsparse_mi355_option_trsv_chunks);
    if(!C.fits || want == 0 || !(cp.model_us < 0.9 * cp.model_block_us || want == 1))
        return aoclsparse_status_success;
    // cptr: first step of every chunk (nch + 1), rows of every chunk (nch), first halo entry of every chunk (nch, each a
    // multiple of 4), halo entries of every chunk (nch)
    Ints cp2(C.cptr);
    cp2.insert(cp2.end(), C.crows.begin(), C.crows.end());
    cp2.insert(cp2.end(), C.hptr.begin(), C.hptr.end() - 1);
    cp2.insert(cp2.end(), C.hcount.begin(), C.hcount.end());
    C.hind.resize(C.hind.size() + 256 * 4, 0); // (a round reads 256 positions whatever is left of the list)
    aoclsparse_status rc = upload_all(st, {ints(cp.steps, C.steps), ints(cp.cptr, cp2), ints(cp.eptr, C.eptr), ints(cp.cind, C.cind),
                                           ints(cp.hind, C.hind)});
    if(rc == aoclsparse_status_success)
        rc = hipStreamSynchronize(st) == hipSuccess ? rc : aoclsparse_status_internal_error; // (the host vectors die here)
    if(rc == aoclsparse_status_success)
    {
        cp.nchunks = C.nch(), cp.nsteps = (aoclsparse_int)(C.steps.size() / 8), cp.max_rows = C.maxslots;
        cp.valid = true;
    }
    lt.lap("chunks: upload");
    return rc;
}

template <typename T>
static aoclsparse_status build_blocked(aoclsparse_int m, const Triangle<T> &t, TrsvBlockPlan &bp)
{
    bp.tried = true;
    bp.chunk.valid = bp.chunk.tried = false; // (rebuilt below where it applies: never a leftover of an earlier plan)
    if(m < 2)
        return aoclsparse_status_success;
    LapTimer lt;
    Grouping G;
    group_chains(m, t, TRSV_BLK_EXT, G);
    lt.lap("blocks: chains + levels");
    // (Growing blocks only from rows of <= 16 entries -- so that every block fits the in-register shape of the kernel -- was tried
    // on the unstructured shell-like factor, 45 % of whose rows have 16-24 entries: 534,653 blocks in 3,061 levels instead of
    // 359,873 in 1,784; not a trade.)
    const aoclsparse_int nb = G.nb();
    if((long long)nb * 16 > (long long)m * 10)
        return aoclsparse_status_success; // fewer than 1.6 rows per block: the row-level schedules are as good
    BlockOrder O;
    order_blocks(m, t, G, O);
    // 3. the triangle in that order (entries in chain order), dependencies as positions
    Layout<T> L;
    layout_triangle(t, O.rowmap, O.pos, L);
    lt.lap("blocks: order + layout");
    const Ints  slices = slice_blocks(m, G, O, L.pptr, L.pind, bp.slice_fan_in);
    hipStream_t st     = Runtime::get().stream();
    aoclsparse_status rc = upload_all(st, {ints(bp.rowmap, O.rowmap, (size_t)m), ints(bp.pptr, L.pptr, (size_t)m + 1),
                                           {bp.pind, L.pind.data(), sizeof(aoclsparse_int) * L.pind.size()},
                                           {bp.pval, L.pval.data(), sizeof(T) * L.pval.size()}, ints(bp.bfirst, O.bfirst), ints(bp.slices, slices)});
    bp.psrc.release(); // (never a leftover of an earlier layout)
    if(rc == aoclsparse_status_success && L.psrc.size())
        rc = bp.psrc.upload(L.psrc.data(), sizeof(aoclsparse_int) * L.psrc.size(), st);
    if(rc != aoclsparse_status_success)
        return rc;
    lt.lap("blocks: upload");
    bp.nblocks = nb, bp.nslices = (aoclsparse_int)(slices.size() - 2 - (size_t)G.nlev) / 2, bp.nlevels = G.nlev;
    bp.max_rows = G.max_rows, bp.max_ext = G.max_ext;
    bp.front = G.front;
    bp.valid = true;
    // only for shapes the chunk kernel is compiled for
    bp.chunk.tried = true;
    if(G.max_rows <= TRSV_CHUNK_LANES && G.max_ext <= TRSV_BLK_EXT && nb >= 64)
        (void)build_chunk_plan(m, t, G, O, bp, st, lt); // (a chunk plan that could not be uploaded leaves the block plan to serve)
    free_later(std::move(L.pind), std::move(L.pval), std::move(L.psrc), std::move(O.rowmap), std::move(O.pos), std::move(L.pptr),
               std::move(G.brows));
    return aoclsparse_status_success;
}

template <typename T>
static aoclsparse_status build_plan_t(const HostCsr &c, bool upper, bool transposed, bool conj, TrsvPlan &plan, bool need_rows,
                                      bool maps)
{
    Triangle<T> t;
    {
        PhaseTimer pt("trsv plan: triangle");
        if(maps)
            build_triangle<T, true>(c, upper, transposed, conj, t);
        else
            build_triangle<T, false>(c, upper, transposed, conj, t);
    }
    plan.conj = conj; // (what aoclsparse_mi355_?revalue_device applies to the values it gathers through the maps)
    aoclsparse_status st = aoclsparse_status_success;
    constexpr bool    real = std::is_floating_point<T>::value;
    if(!plan.valid)
    {
        // levels first (cheap; every schedule choice needs nlevels), then the block plan, then -- only if asked for, or if
        // the triangle has no blocks -- the level-ordered row layout.  On the 25 M-entry shell-like factor the row layout is
        // ~75 ms of page-faulting, filling, uploading and freeing 300 MB that the automatic schedule (blocks) never reads.
        {
            PhaseTimer pt("trsv plan: level pass");
            st = build_levels<T>(c.m, t, plan, false);
        }
        if constexpr(real)
            if(st == aoclsparse_status_success && !plan.blk.tried)
            {
                PhaseTimer pt("trsv plan: blocks + layout + upload");
                st = build_blocked<T>(c.m, t, plan.blk);
            }
    }
    if(st == aoclsparse_status_success && !plan.rows_valid && (need_rows || !real || !plan.blk.valid))
    {
        PhaseTimer pt("trsv plan: levels + layout + upload");
        st = build_levels<T>(c.m, t, plan, true);
    }
    free_later(std::move(t.ptr), std::move(t.ind), std::move(t.val), std::move(t.src));
    return st;
}

aoclsparse_status ensure_trsv(aoclsparse_matrix A, bool upper, bool transposed, bool conj, bool need_rows)
{
    conj = conj && transposed && is_complex_type(A->val_type);
    aoclsparse_status st;
    {
        PhaseTimer pt("trsv plan: csr_optimize (if needed)");
        st = csr_optimize(A);
    }
    if(st != aoclsparse_status_success)
        return st;
    TrsvPlan &plan = A->trsv_plan[trsv_plan_index(upper, transposed, conj)];
    {
        std::shared_lock<std::shared_mutex> r(A->guard);
        if(plan.valid && (plan.rows_valid || !need_rows))
            return aoclsparse_status_success;
    }
    std::unique_lock<std::shared_mutex> w(A->guard);
    if(plan.valid && (plan.rows_valid || !need_rows))
        return aoclsparse_status_success;
    const HostCsr       &c  = *A->opt;
    const size_t         vs = val_size(A->val_type);
    const aoclsparse_int m  = c.m;
    Runtime             &rt = Runtime::get();
    try
    {
        if(!A->dev_diag.ptr)
        {
            // diagonal values (only read for non-unit solves, which require a full diagonal)
            std::vector<char> dv(vs * (size_t)std::max(m, 1), 0);
            for(aoclsparse_int i = 0; i < std::min(c.m, c.n); i++)
                if(c.iurow[i] == c.idiag[i] + 1)
                    std::memcpy(&dv[vs * (size_t)i],
                                static_cast<const char *>(c.val) + vs * (size_t)(c.idiag[i] - c.base), vs);
            st = A->dev_diag.upload(dv.data(), vs * (size_t)m, rt.stream());
            if(st != aoclsparse_status_success)
                return st;
        }
        if(A->keep_maps && !A->diag_src.ptr)
        {
            // the diagonal's value map: the clean position gathered above, -1 where the row has no diagonal entry
            std::vector<int> ds((size_t)std::max(m, 1), -1);
            for(aoclsparse_int i = 0; i < std::min(c.m, c.n); i++)
                if(c.iurow[i] == c.idiag[i] + 1)
                    ds[(size_t)i] = c.idiag[i] - c.base;
            st = A->diag_src.upload(ds.data(), sizeof(int) * (size_t)std::max(m, 1), rt.stream());
            if(st != aoclsparse_status_success)
                return st;
        }
        st = dispatch_value_type(A->val_type, [&](auto tag) {
            return build_plan_t<decltype(tag)>(c, upper, transposed, conj, plan, need_rows, A->keep_maps);
        });
        if(st != aoclsparse_status_success)
            return st;
        plan.valid = true;
        A->plan_builds++; // a plan was built or extended (an observer: aoclsparse_mi355_get_value_map_info)
    }
    catch(const std::bad_alloc &)
    {
        return aoclsparse_status_memory_error;
    }
    return aoclsparse_status_success;
}

} // namespace mi355
