// spmv_plan.cpp -- the CSR side of the SpMV plans: device mirror, CSR-Adaptive row blocks, merge-path tiling, ensure_spmv.
#include "internal.hpp"

#include <algorithm>
#include <cstdlib>
#include <vector>

using namespace mi355;

namespace mi355
{

// ---- device mirrors ---------------------------------------------------------------------------------
aoclsparse_status upload_csr(const HostCsr &h, size_t vsize, DeviceCsr &d)
{
    Runtime          &rt = Runtime::get();
    const aoclsparse_int nnz = h.ptr[h.m] - h.base;
    aoclsparse_status st = d.ptr.upload(h.ptr, sizeof(aoclsparse_int) * (size_t)(h.m + 1), rt.stream());
    if(st == aoclsparse_status_success)
        st = d.ind.upload(h.ind, sizeof(aoclsparse_int) * (size_t)nnz, rt.stream());
    if(st == aoclsparse_status_success)
        st = d.val.upload(h.val, vsize * (size_t)nnz, rt.stream());
    if(st != aoclsparse_status_success)
        return st;
    d.m = h.m, d.n = h.n, d.nnz = nnz, d.base = h.base;
    d.valid = true;
    return aoclsparse_status_success;
}

static aoclsparse_int choose_tile(aoclsparse_int /*m*/, aoclsparse_int nnz, size_t vsize)
{
    // float, large: 2048 entries per block (the LDS footprint of 1024 doubles; a float load instruction moves half the bytes, so a
    // block needs twice the entries in flight: raw scsrmv on the 4096^2 Laplacian 0.216 / 0.202 / 0.182 ms at 512 / 1024 / 2048,
    // double 0.267 / 0.261 / 0.284 on the same box -- profiles/r4/float_headline.txt)
    if(vsize == 4 && (long long)nnz >= 1024LL * 256 * 16)
        return 2048;
    // 1024: 18 KiB of LDS per workgroup -> 8 workgroups (32 wavefronts) per CU hide the
    // load -> gather -> reduce latency chain better than 4 fatter ones (0.257 vs 0.290 ms on the 4096^2
    // Laplacian).  A matrix too small to give every CU ~16 such blocks gets 512-entry tiles and 128-lane
    // workgroups instead (web-like stand-in: 0.039 vs 0.056 ms).  profiles/r1, DESIGN.md 5.1.
    // (the XCD-contiguous block order -- bit 0 of the tile word, which the kernel still decodes -- measured slower than launch
    // order on the Laplacian and 6 % faster at most on the graph stand-ins: profiles/r3/irregular_locality_pmc.txt; the round 1-3
    // switches that forced a tile size or that order are gone, the losing sides are recorded under profiles/)
    // (diagnostics, counter passes of round 6: AOCLSPARSE_MI355_SPMV_XCD_ORDER=1 sets that bit; profiles/r6/csrmv_xcd_order_pmc.txt)
    static const bool xcd_order = getenv("AOCLSPARSE_MI355_SPMV_XCD_ORDER") && getenv("AOCLSPARSE_MI355_SPMV_XCD_ORDER")[0] == '1';
    return ((long long)nnz < 1024LL * 256 * 16 ? 512 : 1024) | (xcd_order ? 1 : 0);
}

// CSR-Adaptive row blocks (host, O(rows)) of the row range [r0, r1): consecutive rows are packed into a block while their
// non-zeros fit one LDS tile and the row count stays <= spmv_maxrows(tile); a row longer than a tile gets a block of its own
// (counted in lr; mx = the longest row seen).  An entry = {first row, first non-zero (0-based)}, appended to `out`; the caller
// closes the last block with the terminal entry.
static void plan_rows_range(aoclsparse_int r0, aoclsparse_int r1, aoclsparse_index_base base, aoclsparse_int tile,
                            const aoclsparse_int *row_ptr, std::vector<aoclsparse_int> &out, aoclsparse_int &lr,
                            aoclsparse_int &mx)
{
    aoclsparse_int i = r0;
    while(i < r1)
    {
        const aoclsparse_int start = row_ptr[i] - base;
        aoclsparse_int       j     = i;
        while(j < r1 && j - i < spmv_maxrows(tile) && (row_ptr[j + 1] - base) - start <= tile)
            j++;
        if(j == i) // single row longer than a tile
        {
            j = i + 1;
            lr++;
        }
        for(aoclsparse_int r = i; r < j; r++)
            mx = std::max(mx, row_ptr[r + 1] - row_ptr[r]);
        out.push_back(i);
        out.push_back(start);
        i = j;
    }
}

aoclsparse_status build_spmv_plan(aoclsparse_int m, aoclsparse_int nnz, aoclsparse_index_base base,
                                  const aoclsparse_int *row_ptr_host, SpmvPlan &plan, size_t vsize)
{
    try
    {
        // Big matrices: the greedy packing runs on 16 fixed row chunks in parallel (the chunking does not depend on
        // the thread count, so the plan is reproducible; a chunk edge merely ends a block early).  The one-shot raw
        // aoclsparse_?csrmv on host arrays builds a plan per call: a sequential pass over 16.8 M rows into a zeroed
        // 2(m+2)-int buffer cost ~50 ms there, more than sending the matrix over PCIe (profiles/r2/h2d_probe.jsonl).
        plan.tile                 = choose_tile(m, nnz, vsize);
        const aoclsparse_int tile = plan.tile & ~1;
        const int            nchunks = m >= (1 << 20) ? 16 : 1;
        std::vector<std::vector<aoclsparse_int>> part(nchunks);
        std::vector<aoclsparse_int>              lrs(nchunks, 0), mxs(nchunks, 0);
        auto work = [&](int c) {
            const aoclsparse_int r0 = (aoclsparse_int)((long long)m * c / nchunks);
            const aoclsparse_int r1 = (aoclsparse_int)((long long)m * (c + 1) / nchunks);
            part[c].reserve((size_t)(r1 - r0) / 64 + 16);
            plan_rows_range(r0, r1, base, tile, row_ptr_host, part[c], lrs[c], mxs[c]);
        };
        // parallel_for (internal.hpp) carries a worker's exception (bad_alloc inside reserve / push_back) to this thread and
        // runs a chunk inline when a thread cannot be started, so nothing can reach std::terminate below the C ABI
        // (ADVICE r2); the 16 chunks are fixed, so the plan does not depend on how many threads took them.
        mi355::parallel_for(nchunks, 1, [&](long long c0, long long c1) {
            for(long long c = c0; c < c1; c++)
                work((int)c);
        });
        std::vector<aoclsparse_int> blk;
        size_t                      total = 2;
        for(auto &p : part)
            total += p.size();
        blk.reserve(total);
        plan.long_rows = 0, plan.max_row_nnz = 0;
        for(int c = 0; c < nchunks; c++)
        {
            blk.insert(blk.end(), part[c].begin(), part[c].end());
            plan.long_rows += lrs[c];
            plan.max_row_nnz = std::max(plan.max_row_nnz, mxs[c]);
        }
        plan.nblocks = (aoclsparse_int)(blk.size() / 2);
        blk.push_back(m);
        blk.push_back(row_ptr_host[m] - base);
        aoclsparse_status st = plan.rowblocks.upload(
            blk.data(), sizeof(aoclsparse_int) * 2 * (size_t)(plan.nblocks + 1), Runtime::get().stream());
        if(st != aoclsparse_status_success)
            return st;
        // Heavy blocks first.  A row is ONE lane's serial chain (scalar order), so a block that holds a row of a few
        // hundred entries -- or is a single row longer than a tile -- runs 2-4 x as long as the others; workgroups start
        // over 2.5-4.5 us (circuit-like: 1,900 of them), and a heavy block started last is the kernel's tail
        // (tools/spmv_trace.py).  Same blocks, same rows, same chains: only the workgroup that takes them changes.
        plan.heavy_first = false;
        if(plan.nblocks >= 512 && plan.max_row_nnz >= 64)
        {
            const aoclsparse_int        nb = plan.nblocks;
            std::vector<aoclsparse_int> weight((size_t)nb), order((size_t)nb);
            aoclsparse_int              heavy = 0;
            for(aoclsparse_int b = 0; b < nb; b++)
            {
                aoclsparse_int w = 0;
                for(aoclsparse_int r = blk[2 * b]; r < blk[2 * b + 2]; r++)
                    w = std::max(w, row_ptr_host[r + 1] - row_ptr_host[r]);
                weight[b] = w >= 64 ? w : 0;
                heavy += w >= 64;
                order[b] = b;
            }
            if(heavy > 0) // (circuit-like: most blocks hold a row >= 64; the 300-entry ones still have to go first)
            {
                std::stable_sort(order.begin(), order.end(), [&](aoclsparse_int a, aoclsparse_int c) { return weight[a] > weight[c]; });
                // (Tried: the heaviest eighth on the XCD a lone launch reaches first -- workgroup i runs on XCD i % 8 and a
                // synchronous launch reaches the XCDs staggered by up to 4.5 us, tools/spmv_trace.py -- the traced span fell
                // 13.8 -> 11.0 us, but back-to-back calls got SLOWER (14.8 vs 13.6 us, web-like 37 vs 28 us): in a stream of
                // launches the stagger is not there and one XCD ends up with all the long chains.)
                std::vector<aoclsparse_int> b4(4 * (size_t)nb);
                for(aoclsparse_int k = 0; k < nb; k++)
                {
                    const aoclsparse_int b = order[k];
                    b4[4 * k] = blk[2 * b], b4[4 * k + 1] = blk[2 * b + 1];
                    b4[4 * k + 2] = blk[2 * b + 2] - blk[2 * b], b4[4 * k + 3] = blk[2 * b + 3] - blk[2 * b + 1];
                }
                st = plan.rowblocks4.upload(b4.data(), sizeof(aoclsparse_int) * b4.size(), Runtime::get().stream());
                if(st != aoclsparse_status_success)
                    return st;
                plan.heavy_first = true;
            }
        }
        plan.valid = true;
    }
    catch(const std::bad_alloc &)
    {
        return aoclsparse_status_memory_error;
    }
    catch(const std::exception &)
    {
        return aoclsparse_status_internal_error;
    }
    return aoclsparse_status_success;
}

constexpr int MERGE_AUTO_TILES = 16; // auto: merge-path once the longest row spans this many LDS tiles (32 until round 5)
// 0 auto, 1 CSR-Adaptive always, 2 merge-path whenever it can serve the request
// (read at plan-build time, i.e. once per handle and operator)
static int spmv_kernel_choice()
{
    return plan_option(aoclsparse_mi355_option_spmv_kernel);
}

aoclsparse_status build_merge_plan(aoclsparse_int m, aoclsparse_int nnz, aoclsparse_index_base base,
                                   const aoclsparse_int *ptr, size_t vsize, SpmvPlan &plan)
{
    MergePlan &mp = plan.merge;
    if(mp.valid || mp.tried)
        return aoclsparse_status_success;
    mp.tried = true;
    const int choice = spmv_kernel_choice();
    if(m <= 0 || nnz <= 0)
        return aoclsparse_status_success;
    // Automatic choice (aoclsparse_optimize / first product, from the row-length statistics of the row-block plan):
    // the row-block kernel gives a row longer than one LDS tile to ONE workgroup, which walks it tile by tile --
    // fine for rows of a few tiles (web-like: longest row 2,908 = 6 tiles; merge-path loses there, 29.8 vs 25.0 us,
    // and on circuit-like, 8.8 vs 7.3 us), a serial tail once a row spans tens of tiles.  Merge-path cuts such rows
    // into 1,024-item pieces spread over the chip, so it is selected when the longest row exceeds MERGE_AUTO_TILES tiles.
    // Round 5 (one launch, wavefront trees for the pieces; tools/exp_arrow.py, profiles/r5/merge_vs_adaptive.jsonl; adaptive /
    // merge, us): 1 row of 300 k 125 / 9.8; 4 x 250 k 114 / 12.4; 16 x 64 k 48 / 14.4; 64 x 16 k 24.9 / 16.9; 256 x 4 k
    // 15.6 / 18.8; 1,024 x 1 k 15.5 / 19.1 -- the crossover lies between rows of 8 and 32 tiles.
    constexpr int auto_tiles = MERGE_AUTO_TILES;
    const bool auto_pick = choice == 0 && auto_tiles > 0 && plan.long_rows > 0
                           && (long long)plan.max_row_nnz >= (long long)auto_tiles * (plan.tile & ~1);
    if(choice != 2 && !auto_pick)
        return aoclsparse_status_success;
    const long long             items  = (long long)m + nnz;
    const aoclsparse_int        ntiles = (aoclsparse_int)((items + MP_ITEMS - 1) / MP_ITEMS);
    std::vector<aoclsparse_int> st;
    try
    {
        st.resize(2 * ((size_t)ntiles + 1));
    }
    catch(const std::bad_alloc &)
    {
        return aoclsparse_status_memory_error;
    }
    for(aoclsparse_int w = 0; w <= ntiles; w++)
    {
        // merge-path search on diagonal d: the largest i with (row end i-1) <= (d - i) consumed non-zeros
        const long long d  = std::min<long long>((long long)w * MP_ITEMS, items);
        long long       lo = std::max<long long>(0, d - nnz), hi = std::min<long long>(d, m);
        while(lo < hi)
        {
            const long long mid = (lo + hi) / 2;
            if((long long)(ptr[mid + 1] - base) <= d - mid - 1)
                lo = mid + 1;
            else
                hi = mid;
        }
        st[2 * (size_t)w]     = (aoclsparse_int)lo;
        st[2 * (size_t)w + 1] = (aoclsparse_int)(d - lo);
    }
    // first[w]: tile w holds the END of a row that started in an earlier tile -> the first tile with a (non-empty) head piece of
    // that row; -1 otherwise.  Tile v's head piece belongs to the row its successor starts in (st[2(v+1)]), and is non-empty
    // when the tile ends past that row's first entry.  Each tile is visited by at most one row's walk: O(ntiles).
    std::vector<aoclsparse_int> first;
    try
    {
        first.assign(2 * (size_t)ntiles, -1);
    }
    catch(const std::bad_alloc &)
    {
        return aoclsparse_status_memory_error;
    }
    for(aoclsparse_int w = 1; w < ntiles; w++)
    {
        const aoclsparse_int i0 = st[2 * (size_t)w], j0 = st[2 * (size_t)w + 1];
        if(st[2 * (size_t)w + 2] == i0 || i0 >= m) // no row ends in this tile
            continue;
        const aoclsparse_int rowstart = ptr[i0] - base;
        if(rowstart >= j0) // row i0 starts here
            continue;
        aoclsparse_int f = w - 1;
        while(f > 0 && st[2 * (size_t)f] == i0 && st[2 * (size_t)f + 1] > rowstart)
            f--;
        first[w] = f;
    }
    // endt[v] (stored behind first[]): the tile in which the row of tile v's head piece ends -- the inverse of first[]
    for(aoclsparse_int w = 1; w < ntiles; w++)
        for(aoclsparse_int v = first[w]; v >= 0 && v < w; v++)
            first[(size_t)ntiles + v] = w;
    // (the kernel decides "tile v has a head piece" from row_ptr: every such tile must know its end tile)
    for(aoclsparse_int v = 0; v < ntiles; v++)
    {
        const aoclsparse_int i1 = st[2 * (size_t)v + 2], j0 = st[2 * (size_t)v + 1], j1 = st[2 * (size_t)v + 3];
        const bool           has_head = i1 < m && std::max<aoclsparse_int>(ptr[i1] - base, j0) < j1;
        if(has_head != (first[(size_t)ntiles + v] >= 0))
            return aoclsparse_status_success; // (never seen) leave the matrix to the row-block kernel
    }
    (void)vsize;
    Runtime          &rt = Runtime::get();
    aoclsparse_status s1 = mp.starts.upload(st.data(), sizeof(aoclsparse_int) * st.size(), rt.stream());
    if(s1 == aoclsparse_status_success)
        s1 = mp.first.upload(first.data(), sizeof(aoclsparse_int) * first.size(), rt.stream());
    if(s1 != aoclsparse_status_success)
        return s1;
    MI355_HIP_TRY(hipStreamSynchronize(rt.stream())); // (uploads read the host vectors until the stream has run them)
    {
        std::lock_guard<std::mutex> g(mp.launch_lock);
        mp.sets.clear(); // piece sets are made by the first launch on each stream (spmv_api.cpp)
    }
    mp.ntiles = ntiles;
    mp.valid  = true;
    return aoclsparse_status_success;
}

// the value size build_spmv_plan sizes its row blocks by: a float handle plans 2,048-entry blocks for its products with vectors --
// unless it carries an mm hint: csrmm_tile_kernel walks the same blocks, and the 32-column float slab of the 1000^2 Laplacian
// measured 0.094-0.096 ms over 1,024-entry blocks against 0.101 over 2,048 (tools/history/exp_float_slab.py)
static size_t plan_value_size(const _aoclsparse_matrix &A)
{
    if(A.val_type != aoclsparse_smat)
        return 8;
    for(const Hint &h : A.hints)
        if(h.act == action_mm)
            return 8;
    return 4;
}

aoclsparse_status ensure_spmv(aoclsparse_matrix A, bool transposed, DeviceCsr *&dcsr, SpmvPlan *&plan)
{
    dcsr = transposed ? &A->dev_trans : &A->dev_user;
    plan = transposed ? &A->plan_trans : &A->plan_user;
    {
        std::shared_lock<std::shared_mutex> r(A->guard);
        if(dcsr->valid && plan->valid)
            return aoclsparse_status_success;
    }
    if(transposed)
    {
        aoclsparse_status st = build_transpose(A);
        if(st != aoclsparse_status_success)
            return st;
    }
    std::unique_lock<std::shared_mutex> w(A->guard);
    const HostCsr                      &h = transposed ? *A->trans : A->user;
    if(!dcsr->valid)
    {
        aoclsparse_status st = upload_csr(h, val_size(A->val_type), *dcsr);
        if(st != aoclsparse_status_success)
            return st;
    }
    if(!plan->valid)
    {
        aoclsparse_status st = build_spmv_plan(h.m, h.ptr[h.m] - h.base, h.base, h.ptr, *plan, plan_value_size(*A));
        if(st != aoclsparse_status_success)
            return st;
    }
    if(!is_complex_type(A->val_type))
    {
        aoclsparse_status st = build_merge_plan(h.m, h.ptr[h.m] - h.base, h.base, h.ptr, val_size(A->val_type), *plan);
        if(st != aoclsparse_status_success)
            return st;
    }
    return aoclsparse_status_success;
}

} // namespace mi355

extern "C" {

aoclsparse_int mi355_csrmv_plan_bound(aoclsparse_int m, aoclsparse_int /*nnz*/)
{
    return 2 * (m + 2);
}

aoclsparse_int mi355_csrmv_plan_host(aoclsparse_int m, aoclsparse_int base, aoclsparse_int tile,
                                     const aoclsparse_int *row_ptr_host, aoclsparse_int *blocks_host)
{
    if(m < 0 || !row_ptr_host || !blocks_host || (base != 0 && base != 1) || (tile != 512 && tile != 1024 && tile != 2048))
        return -1;
    // the planner of build_spmv_plan on the single range [0, m) (whatever m is: only build_spmv_plan cuts chunks), then the
    // terminal entry; blocks_host holds mi355_csrmv_plan_bound entries, and a plan of m rows has at most m blocks
    std::vector<aoclsparse_int> blk;
    aoclsparse_int              lr = 0, mx = 0;
    try
    {
        plan_rows_range(0, m, (aoclsparse_index_base)base, tile, row_ptr_host, blk, lr, mx);
    }
    catch(const std::bad_alloc &)
    {
        return -1;
    }
    std::copy(blk.begin(), blk.end(), blocks_host);
    blocks_host[blk.size()]     = m;
    blocks_host[blk.size() + 1] = row_ptr_host[m] - base;
    return (aoclsparse_int)(blk.size() / 2);
}

} // extern "C"
