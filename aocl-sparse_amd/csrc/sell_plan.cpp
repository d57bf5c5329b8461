// sell_plan.cpp -- the SELL-64 plan: structure stage, values stage, and what the C ABI reports of a plan.
#include "internal.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace mi355;

namespace mi355
{

void sell_pack_descriptors(aoclsparse_int nslices, const long long *slice_ptr, const aoclsparse_int *leaders, long long ccells,
                           SellSliceDesc *out)
{
    auto pack = [](long long cell, long long col, int w, int stride, int mode) {
        SellSliceDesc d;
        d.cell_lo = (uint32_t)cell, d.col_lo = (uint32_t)col;
        d.hi      = (uint32_t)((cell >> 32) & 0xffff) | (uint32_t)((col >> 32) & 0xffff) << 16;
        d.wsm     = (uint32_t)w | (uint32_t)stride << 8 | (uint32_t)mode << 16;
        return d;
    };
    long long c0 = 0;
    for(aoclsparse_int s = 0; s < nslices; s++)
    {
        const int w = (int)((slice_ptr[s + 1] - slice_ptr[s]) >> 6);
        if(leaders)
        {
            const int nl = leaders[s] & 0xff;
            out[s]       = pack(slice_ptr[s], c0, w, nl, leaders[s] >> 8);
            c0 += (long long)nl * w;
        }
        else
            out[s] = pack(slice_ptr[s], slice_ptr[s], w, 64, SELL_DESC_MODE_OWN);
    }
    // past the end: empty slices on the padding cells (one list, no shift: nothing but the padding is read)
    for(int k = 0; k < SELL_DESC_PAD; k++)
        out[nslices + k] = pack(slice_ptr[nslices], ccells, 0, 1, SELL_DESC_MODE_ONE);
}

// ---- build_sell = the STRUCTURE stage, then the VALUES stage ------------------------------------------------------------------
// Structure: what row_ptr, col_idx, the sizes and aoclsparse_mi355_option_sell decide (SellStructure lists it).  Values: the
// table and the cell encoding chosen from it, the cells, ucol and the uniform lists, the device flags of the records, the periodic
// range and the stacking facts.  A first build interleaves the two where today's order of allocations asks for it (the table pass
// sits between the shared lists and the column arrays: where the later arrays lie in HBM moves the products by 2 - 3 %); a handle
// whose structure aoclsparse_mi355_?revalue_device kept (SellPlan::stale) runs sell_values_kept alone.
namespace
{

// the encoding the values stage chooses from the table pass
struct SellEncoding
{
    int           ntab = 0, pbits = 0, pbytes = 0;
    unsigned char tab[sizeof(double) * SELL_VTAB_MAX];
};

// Value table: at most SELL_VTAB_MAX distinct bit patterns (a constant-coefficient stencil holds two) -> one byte per cell instead
// of 4 / 8 (sell_build_kernels.hip).  Real types only; the same size gate as the shared lists (a matrix that lives in the caches gains
// nothing); aoclsparse_mi355_set_option(sell_values, 0 / 1): never / whatever the size.  One pass over the device values.
// With slice records the indices of a row are packed into ONE word where they fit: fields of 1 / 2 / 4 / 8 bits (the smallest that
// holds ntab - 1), cell q at bit q * bits, in the smallest word of 1 / 2 / 4 bytes that holds the widest slice.
aoclsparse_status sell_choose_encoding(const DeviceCsr &d, size_t vsize, bool complex_values, const SellPlan &sp, SellEncoding &enc)
{
    const int vmode = plan_option(aoclsparse_mi355_option_sell_values); // -1 automatic (default), 0 never, 1 whatever the size
    if(complex_values || (vsize != sizeof(double) && vsize != sizeof(float)) || vmode == 0 || !(vmode == 1 || d.nnz >= (1 << 17)))
        return aoclsparse_status_success;
    int ntab = 0;
    MI355_TRY(sell_value_table(Runtime::get().stream(), vsize, d.nnz, d.val.ptr, enc.tab, &ntab));
    if(ntab > 0)
    {
        int bits = 1;
        while((1 << bits) < ntab)
            bits *= 2;
        const int wbits = (int)sp.st.wmax * bits;
        enc.ntab        = ntab;
        if(sp.st.records && wbits <= 32)
            enc.pbits = bits, enc.pbytes = wbits <= 8 ? 1 : (wbits <= 16 ? 2 : 4);
    }
    if(PhaseTimer::on())
        std::fprintf(stderr, "[mi355 timing] sell: %d distinct value patterns%s\n", ntab, ntab ? "" : " (more than 256, or none)");
    return aoclsparse_status_success;
}

// the table and the cell array of enc: vtab + pidx ((nslices + SELL_DESC_PAD) x 64 words, addressed by row number alone) or vidx
// (one byte per cell), or val; what another encoding held is released.  With the SELL_CELL_PAD cells after the last: value 0 /
// index 0 -- what the short-row kernel reads for a slice of width 0 -- and the words of the padding slices (the rows behind m in
// the last slice are the fill kernel's).
aoclsparse_status sell_alloc_cells(SellPlan &sp, const SellEncoding &enc, size_t vsize)
{
    Runtime     &rt = Runtime::get();
    const size_t nslices = (size_t)sp.st.nslices, cells = (size_t)sp.st.cells;
    sp.vals.ntab = sp.vals.pbits = sp.vals.pbytes = 0;
    if(enc.ntab > 0)
    {
        MI355_TRY(sp.vals.vtab.upload(enc.tab, vsize * (size_t)SELL_VTAB_MAX, rt.stream()));
        if(enc.pbits)
        {
            MI355_TRY(sp.vals.pidx.alloc((nslices + SELL_DESC_PAD) * 64 * (size_t)enc.pbytes));
            sp.vals.vidx.release();
        }
        else
        {
            MI355_TRY(sp.vals.vidx.alloc(cells + SELL_CELL_PAD));
            sp.vals.pidx.release();
        }
        sp.vals.ntab = enc.ntab, sp.vals.pbits = enc.pbits, sp.vals.pbytes = enc.pbytes;
        sp.vals.val.release();
        if(sp.vals.pbits)
            MI355_HIP_TRY(hipMemsetAsync(sp.vals.pidx.as<unsigned char>() + nslices * 64 * (size_t)sp.vals.pbytes, 0,
                                         (size_t)SELL_DESC_PAD * 64 * (size_t)sp.vals.pbytes, rt.stream()));
        else
            MI355_HIP_TRY(hipMemsetAsync(sp.vals.vidx.as<unsigned char>() + cells, 0, SELL_CELL_PAD, rt.stream()));
        return aoclsparse_status_success;
    }
    sp.vals.vtab.release(), sp.vals.vidx.release(), sp.vals.pidx.release();
    MI355_TRY(sp.vals.val.alloc(vsize * (cells + SELL_CELL_PAD)));
    MI355_HIP_TRY(hipMemsetAsync(sp.vals.val.as<unsigned char>() + vsize * cells, 0, vsize * SELL_CELL_PAD, rt.stream()));
    return aoclsparse_status_success;
}

// bytes of the uniform lists (SELL_SHORT_WMAX columns per slice, the padding slices included)
size_t sell_ucol_bytes(aoclsparse_int nslices)
{
    return sizeof(aoclsparse_int) * SELL_SHORT_WMAX * ((size_t)nslices + SELL_DESC_PAD);
}

// The periodic range of the records and lists as the device now holds them (flags, words and canonical lists included: they
// depend on the values).  A stencil's records repeat from grid line to grid line, and the short-row kernel then reads one
// period's for the whole range (sell_period.cpp).  On a host copy: the pristine records stay; a copy that cannot be made keeps no range.
aoclsparse_status sell_search_range(SellPlan &sp, size_t vsize)
{
    Runtime                    &rt      = Runtime::get();
    const aoclsparse_int        nslices = sp.st.nslices;
    PhaseTimer                  pt("sell: periodic range of the records");
    std::vector<aoclsparse_int> uh;
    std::vector<SellSliceDesc>  desc;
    sp.vals.no_range();
    try
    {
        uh.resize((size_t)nslices * SELL_SHORT_WMAX);
        desc.resize((size_t)nslices);
    }
    catch(const std::bad_alloc &)
    {
        return aoclsparse_status_success;
    }
    if(uh.empty())
        return aoclsparse_status_success;
    MI355_HIP_TRY(hipMemcpyAsync(desc.data(), sp.st.desc.ptr, sizeof(SellSliceDesc) * (size_t)nslices, hipMemcpyDeviceToHost, rt.stream()));
    MI355_HIP_TRY(hipMemcpyAsync(uh.data(), sp.vals.ucol.ptr, sizeof(aoclsparse_int) * uh.size(), hipMemcpyDeviceToHost, rt.stream()));
    MI355_HIP_TRY(hipStreamSynchronize(rt.stream()));
    aoclsparse_int pr[4];
    sell_find_period(desc.data(), uh.data(), nslices, SELL_PERIOD_CAP, pr);
    if(sell_period_usable(nslices, pr[0], pr[1], pr[2], pr[3], vsize))
    {
        sp.vals.pslo = (int)pr[0], sp.vals.pshi = (int)pr[1], sp.vals.pper = (int)pr[2], sp.vals.pstride = (int)pr[3];
        // whether the range can be stacked, and its alias map: one pass over the first period (<= SELL_PERIOD_CAP slices)
        PhaseTimer     mt("sell: stacking and alias map of the period");
        aoclsparse_int mr[2];
        sell_find_march(desc.data(), uh.data(), nslices, pr, sp.vals.pbytes, mr);
        sp.vals.mstack = (int)mr[0], sp.vals.malias = (unsigned)mr[1];
    }
    return aoclsparse_status_success;
}

// Where a values stage writes what is not a cell (the cells are the view's).
struct SellFillTarget
{
    SellSliceDesc  *desc   = nullptr; // the records that get sell_records_kernel's flags
    aoclsparse_int *ucol   = nullptr; // the uniform lists; nullptr: the plan has none
    unsigned       *counts = nullptr; // two device words for the records kernel's counters; nullptr: that kernel is not to run
    aoclsparse_int *col = nullptr, *rowlen = nullptr; // the structure the same pass writes (a first build); nullptr: it is kept
    hipEvent_t      fill_begin = nullptr, fill_end = nullptr; // recorded around the fill launch where set
};

// THE VALUES STAGE'S DEVICE WORK, of a first build and on a kept structure, enqueued on s: the lists preset to -1 (a slice of mode
// 1 / 2 -- full, one leader -- has ONE list, which the fill kernel writes and the short-row kernel reads with a scalar load; every
// other entry stays -1), the fill pass, and behind it the records kernel, which reads the words and lists that pass wrote.
aoclsparse_status sell_enqueue_values(hipStream_t s, const DeviceCsr &d, size_t vsize, const SellView &view, const SellFillTarget &t)
{
    if(t.ucol)
        MI355_HIP_TRY(hipMemsetAsync(t.ucol, 0xff, sell_ucol_bytes(view.nslices), s));
    if(t.fill_begin)
        MI355_HIP_TRY(hipEventRecord(t.fill_begin, s));
    MI355_TRY(launch_sell_fill(s, d, vsize, view, const_cast<void *>(view.cells), t.col, t.rowlen, t.ucol));
    if(t.fill_end)
        MI355_HIP_TRY(hipEventRecord(t.fill_end, s));
    if(t.counts)
        MI355_TRY(launch_sell_records(s, d, view, t.desc, t.ucol, t.counts));
    return aoclsparse_status_success;
}

// ... and its end: the first nwords of counts (if that kernel ran) come back into rc, the stream is drained, and the plan records
// what the stage counted
aoclsparse_status sell_collect_values(hipStream_t s, SellPlan &sp, const unsigned *counts, int nwords, unsigned *rc)
{
    if(counts)
        MI355_HIP_TRY(hipMemcpyAsync(rc, counts, nwords * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    MI355_HIP_TRY(hipStreamSynchronize(s));
    sp.vals.uniform       = sp.vals.ucol.ptr ? sp.st.nuniform : 0;
    sp.vals.uniform_words = (aoclsparse_int)rc[0], sp.vals.exceptions = (aoclsparse_int)rc[1];
    return aoclsparse_status_success;
}

void swap_buffers(DeviceBuffer &a, DeviceBuffer &b)
{
    DeviceBuffer t;
    t.adopt(a), a.adopt(b), b.adopt(t);
}

// The values stage on a kept structure: table pass, cells of the chosen encoding (buffers of another encoding class are released
// and allocated as a first build would), the value-only fill, and -- on a copy with uniform lists and one-byte words -- the
// records kernel on the SPARE set of records and lists (records copied from the pristine ones, lists preset to -1), a compare
// kernel against the current set, and the host search only when the two differ or the class changed.  The spare set becomes the
// current one either way.  Values scaled by a positive factor keep the order of their bit patterns, hence every index, word, flag
// and list: the range is then carried over and nothing but three words comes back to the host.
aoclsparse_status sell_values_kept(const DeviceCsr &d, size_t vsize, SpmvPlan &plan, bool complex_values)
{
    SellPlan            &sp      = plan.sell;
    Runtime             &rt      = Runtime::get();
    hipStream_t          s       = rt.stream();
    const aoclsparse_int nslices = sp.st.nslices;
    PhaseTimer           pt("sell: values (structure kept)");
    SellEncoding         enc;
    LapTimer             lt; // (host clock; the laps end where the stage waits for the stream anyway)
    MI355_TRY(sell_choose_encoding(d, vsize, complex_values, sp, enc));
    lt.lap("sell kept: table pass");
    const bool had_ucol = sp.vals.ucol.ptr != nullptr, want_ucol = sp.st.records && sp.st.shared && enc.pbits > 0;
    const bool flagged  = had_ucol && sp.vals.ntab > 0 && sp.vals.pbytes == 1; // the current records may carry device flags
    const bool same     = (sp.vals.ntab > 0) == (enc.ntab > 0) && (sp.vals.ntab > 0 ? sp.vals.pbits : 0) == enc.pbits
                      && (sp.vals.ntab > 0 ? sp.vals.pbytes : 0) == enc.pbytes && had_ucol == want_ucol;
    const bool compare  = same && flagged; // (same class, so the new set has flags too)
    if(!same) // another encoding class: as after any other value change, and no current set to compare with
        sp.vals.reset(), sp.st.ucol_spare.release();
    MI355_TRY(sell_alloc_cells(sp, enc, vsize));
    lt.lap("sell kept: table + cell buffers");
    SellSliceDesc  *desc_t = sp.st.desc.as<SellSliceDesc>();
    aoclsparse_int *ucol_t = nullptr;
    const size_t    dbytes = sizeof(SellSliceDesc) * ((size_t)nslices + SELL_DESC_PAD), ubytes = sell_ucol_bytes(nslices);
    if(flagged) // the records kernel starts from the pristine records
    {
        if(sp.st.desc0.size() != (size_t)nslices + SELL_DESC_PAD)
            return aoclsparse_status_internal_error;
        if(!sp.st.desc0_dev.ptr)
            MI355_TRY(sp.st.desc0_dev.upload(sp.st.desc0.data(), dbytes, s));
        if(compare)
        {
            MI355_TRY(sp.st.desc_spare.alloc(dbytes));
            MI355_TRY(sp.st.ucol_spare.alloc(ubytes + 2 * sizeof(unsigned)));
            desc_t = sp.st.desc_spare.as<SellSliceDesc>(), ucol_t = sp.st.ucol_spare.as<aoclsparse_int>();
        }
        MI355_HIP_TRY(hipMemcpyAsync(desc_t, sp.st.desc0_dev.ptr, dbytes, hipMemcpyDeviceToDevice, s));
    }
    if(want_ucol && !compare)
    {
        MI355_TRY(sp.vals.ucol.alloc(ubytes + 2 * sizeof(unsigned)));
        ucol_t = sp.vals.ucol.as<aoclsparse_int>();
    }
    const bool     timed = PhaseTimer::on();
    hipEvent_t     ev[2] = {nullptr, nullptr};
    if(timed)
        for(hipEvent_t &e : ev)
            if(hipEventCreate(&e) != hipSuccess)
                e = nullptr;
    struct EventGuard
    {
        hipEvent_t *ev;
        ~EventGuard()
        {
            for(int i = 0; i < 2; i++)
                if(ev[i])
                    (void)hipEventDestroy(ev[i]);
        }
    } eg{ev};
    SellFillTarget t;
    t.desc = desc_t, t.ucol = ucol_t, t.fill_begin = ev[0], t.fill_end = ev[1];
    if(ucol_t && enc.pbytes == 1) // (the records kernel will run)
    {
        MI355_TRY(sp.st.kwords.alloc(4 * sizeof(unsigned)));
        t.counts = sp.st.kwords.as<unsigned>();
    }
    const bool flags = t.counts != nullptr;
    unsigned   rc[3] = {0, 0, 1}; // flags set, exceptions, verdict (1: the sets differ)
    MI355_TRY(sell_enqueue_values(s, d, vsize, sp.view(d.m, plan.max_row_nnz), t));
    if(flags && compare)
        MI355_TRY(launch_sell_compare(s, nslices, desc_t, sp.st.desc.as<SellSliceDesc>(), ucol_t, sp.vals.ucol.as<aoclsparse_int>(), t.counts + 2));
    MI355_TRY(sell_collect_values(s, sp, t.counts, compare ? 3 : 2, rc));
    lt.lap("sell kept: refill, flags, compare");
    if(ev[0] && ev[1])
    {
        float ms = 0.0f;
        if(hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess)
            std::fprintf(stderr, "[mi355 timing]     %-30s %8.3f ms\n", "sell: refill kernel events", ms);
    }
    if(compare) // the new set is the current one from here on
        swap_buffers(sp.st.desc, sp.st.desc_spare), swap_buffers(sp.vals.ucol, sp.st.ucol_spare);
    const bool carried = compare && rc[2] == 0;
    if(!carried && flags) // (without flags there is no range: the plan had none, or the class changed and took it along)
        MI355_TRY(sell_search_range(sp, vsize));
    if(timed)
        std::fprintf(stderr, "[mi355 timing] sell: values stage, periodic range %s\n",
                     carried ? "carried over (search skipped)" : (flags ? "searched" : "not applicable"));
    sp.count.searches_skipped += carried;
    sp.count.last_route = carried ? 3 : 2;
    return aoclsparse_status_success;
}

} // namespace

aoclsparse_status build_sell(const aoclsparse_int *row_ptr_host, const DeviceCsr &d, size_t vsize, SpmvPlan &plan, bool complex_values)
{
    SellPlan &sp = plan.sell;
    if(sp.valid || sp.tried)
        return aoclsparse_status_success;
    sp.tried = true;
    const int mode = plan_option(aoclsparse_mi355_option_sell); // -1 automatic (default), 0 never, 1 whatever the padding
    // a structure kept through ?revalue_device: the values stage alone, if it was built under this option value from this CSR
    if(sp.stale && sp.st.built && mode == sp.st.mode && mode != 0 && d.valid && d.m == sp.st.m && d.nnz == sp.st.nnz && d.m > 0 && d.nnz > 0)
    {
        sp.stale                   = false;
        const aoclsparse_status st = sell_values_kept(d, vsize, plan, complex_values);
        if(st != aoclsparse_status_success) // as a failed first build: tried, not valid; nothing of the structure is trusted again
        {
            sp.drop_structure();
            return st;
        }
        sp.count.value_fills++;
        sp.valid = sp.wanted = true;
        return aoclsparse_status_success;
    }
    sp.drop_structure();
    sp.vals.reset(); // (a copy built before a value change may have had a table: it goes with the values)
    sp.st.desc.release(); // (uploaded anew below, or gone with the records)
    if(mode == 0 || d.m <= 0 || d.nnz <= 0 || !d.valid)
        return aoclsparse_status_success;
    // -- structure: slice widths, padding verdict, shared lists
    LapTimer               lt;
    const aoclsparse_int   m = d.m, nslices = (m + 63) / 64;
    std::vector<long long> sptr;
    try
    {
        sptr.resize((size_t)nslices + 1);
    }
    catch(const std::bad_alloc &)
    {
        return aoclsparse_status_memory_error;
    }
    // PACK 4 (four consecutive cells of a row adjacent, width rounded up to a multiple of 4) for long rows:
    // contiguous 2 KB wavefront loads; PACK 1 otherwise (a 5-wide slice must not be padded to 8)
    // (complex values: PACK 1 only -- their kernels are the scalar-chain ones)
    const int pack = (!complex_values && (long long)d.nnz >= 16LL * m) ? 4 : 1;
    sptr[0] = 0;
    aoclsparse_int wmax = 0; // widest slice
    for(aoclsparse_int s = 0; s < nslices; s++)
    {
        aoclsparse_int w = 0;
        for(aoclsparse_int i = s * 64; i < std::min<aoclsparse_int>(m, s * 64 + 64); i++)
            w = std::max(w, row_ptr_host[i + 1] - row_ptr_host[i]);
        w           = (w + pack - 1) / pack * pack;
        wmax        = std::max(wmax, w);
        sptr[s + 1] = sptr[s] + 64LL * w;
    }
    const long long cells = sptr[nslices];
    // slice records for the short-row kernel (sell_kernels.hip), where it can serve this copy
    const bool records = pack == 1 && wmax >= 1 && wmax <= SELL_SHORT_WMAX && nslices >= SELL_SHORT_MIN_SLICES;
    // Padding budget: 1.35 cells per non-zero.  Round 1 set 1.15 from the two kernels' rates then (0.78 vs 0.66 of peak); the SELL
    // kernel has gained since.  Round-3 measurement on the unstructured flan-like variant (padding 1.21: tools/history/exp_r3_sellpad.sh,
    // profiles/r3/sell_padding_budget.txt): SELL-64 0.259 ms vs CSR-Adaptive 0.352 ms, i.e. break-even near 1.21 * 0.352 / 0.259 =
    // 1.64 cells per non-zero; 1.35 keeps a margin for matrices with shorter rows.
    if(mode != 1 && (double)cells > 1.35 * (double)d.nnz + 64.0)
        return aoclsparse_status_success;
    sp.st.nslices = nslices, sp.st.cells = cells, sp.st.pack = pack;
    sp.st.wmax = wmax, sp.st.records = records, sp.st.nuniform = 0;
    Runtime          &rt = Runtime::get();
    aoclsparse_status st = sp.st.slice_ptr.upload(sptr.data(), sizeof(long long) * sptr.size(), rt.stream());
    // Shared column lists: rows that repeat the list of the row before them -- as it is (the dofs of a mesh node) or
    // shifted by one (the rows of a stencil) -- keep ONE copy per slice.  Leaders are found on the device (one compare
    // pass over the CSR arrays); used when the column stream shrinks to <= 70 %.
    sp.st.shared = false, sp.st.ccells = cells;
    std::vector<long long>      cptr;
    std::vector<aoclsparse_int> nlh; // leaders | mode << 8 of every slice
    // (not for matrices that live in the caches anyway: the leader / shift words are one more dependent load, and the 10k x 10k
    // Laplacian of BASELINE configs[0] -- 50 k non-zeros, launch-bound -- ran at 5.4 instead of 4.6 us per call with them)
    if(st == aoclsparse_status_success && d.nnz >= (1 << 17))
    {
        DeviceBuffer nl;
        st = sp.st.lead.alloc(sizeof(unsigned short) * (size_t)m);
        if(st == aoclsparse_status_success)
            st = nl.alloc(sizeof(aoclsparse_int) * (size_t)nslices);
        if(st == aoclsparse_status_success)
            st = launch_sell_leaders(rt.stream(), m, d.base, d.ptr.as<aoclsparse_int>(), d.ind.as<aoclsparse_int>(), nslices,
                                     sp.st.lead.as<unsigned short>(), nl.as<aoclsparse_int>());
        if(st != aoclsparse_status_success)
            return st;
        nlh.resize((size_t)nslices);
        MI355_HIP_TRY(hipMemcpyAsync(nlh.data(), nl.ptr, sizeof(aoclsparse_int) * (size_t)nslices, hipMemcpyDeviceToHost, rt.stream()));
        MI355_HIP_TRY(hipStreamSynchronize(rt.stream()));
        cptr.resize((size_t)nslices + 1);
        cptr[0] = 0;
        for(aoclsparse_int s = 0; s < nslices; s++)
            cptr[s + 1] = cptr[s] + (long long)(nlh[s] & 0xff) * ((sptr[s + 1] - sptr[s]) >> 6);
        const long long ctotal = cptr[nslices];
        if(PhaseTimer::on())
            std::fprintf(stderr, "[mi355 timing] sell: %lld cells, %lld column cells with shared lists (%d slices)\n", cells, ctotal, (int)nslices);
        if((double)ctotal <= 0.7 * (double)cells)
        {
            for(aoclsparse_int s = 0; s < nslices; s++) // the slice's mode rides in the top byte
                cptr[s] |= (long long)(nlh[s] >> 8) << SELL_CPTR_MODE_SHIFT;
            sp.st.shared = true, sp.st.ccells = ctotal;
            st        = sp.st.cptr.upload(cptr.data(), sizeof(long long) * cptr.size(), rt.stream());
        }
        else
            sp.st.lead.release();
    }
    if(st != aoclsparse_status_success)
        return st;
    // -- values: the table pass and the cells of the encoding it chooses (here, between the shared lists and the column arrays:
    // the order of a build's allocations is part of the plan)
    SellEncoding enc;
    MI355_TRY(sell_choose_encoding(d, vsize, complex_values, sp, enc));
    MI355_TRY(sell_alloc_cells(sp, enc, vsize));
    // -- structure: the column arrays (SELL_CELL_PAD column entries after the last: -1) and the pristine records
    MI355_TRY(sp.st.col.alloc(sizeof(aoclsparse_int) * ((size_t)sp.st.ccells + SELL_CELL_PAD)));
    MI355_TRY(sp.st.rowlen.alloc(sizeof(aoclsparse_int) * (size_t)m));
    MI355_HIP_TRY(hipMemsetAsync(sp.st.col.as<aoclsparse_int>() + sp.st.ccells, 0xff, sizeof(aoclsparse_int) * SELL_CELL_PAD, rt.stream()));
    std::vector<SellSliceDesc> &desc = sp.st.desc0;
    if(records)
    {
        try
        {
            desc.resize((size_t)nslices + SELL_DESC_PAD);
        }
        catch(const std::bad_alloc &)
        {
            return aoclsparse_status_memory_error;
        }
        sell_pack_descriptors(nslices, sptr.data(), sp.st.shared ? nlh.data() : nullptr, sp.st.ccells, desc.data());
        st = sp.st.desc.upload(desc.data(), sizeof(SellSliceDesc) * desc.size(), rt.stream());
        if(st != aoclsparse_status_success)
            return st;
        if(sp.st.shared)
            for(aoclsparse_int s = 0; s < nslices; s++)
                sp.st.nuniform += (nlh[s] >> 8) == SELL_DESC_MODE_LANE_SHIFT || (nlh[s] >> 8) == SELL_DESC_MODE_ONE;
    }
    sp.st.built = true, sp.st.mode = mode, sp.st.m = d.m, sp.st.nnz = d.nnz;
    sp.count.structure_builds++;
    lt.lap("sell: structure (with the table pass)");
    // -- values: uniform lists, cells, device flags, periodic range
    SellFillTarget t;
    t.desc = sp.st.desc.as<SellSliceDesc>(), t.col = sp.st.col.as<aoclsparse_int>(), t.rowlen = sp.st.rowlen.as<aoclsparse_int>();
    // uniform lists only next to packed words: with values or one-byte indices in the cells the lists gained nothing for double and
    // lost 4 - 6 % for float (profiles/r10/spw_sweep.txt, "ucol with values"), so those plans keep the kernels they had.
    if(records && sp.st.shared && sp.vals.pbits)
    {
        // (+ two words behind the lists: the counters of sell_records_kernel, so that the plan makes no allocation of its own
        // for them -- where later arrays lie in HBM moves the other SELL products by 2 - 3 %)
        MI355_TRY(sp.vals.ucol.alloc(sell_ucol_bytes(nslices) + 2 * sizeof(unsigned)));
        t.ucol = sp.vals.ucol.as<aoclsparse_int>();
        if(sp.vals.pbytes == 1)
            t.counts = reinterpret_cast<unsigned *>(t.ucol + SELL_SHORT_WMAX * ((size_t)nslices + SELL_DESC_PAD));
    }
    unsigned rc[2] = {0, 0};
    MI355_TRY(sell_enqueue_values(rt.stream(), d, vsize, sp.view(m, plan.max_row_nnz), t));
    // (sptr / cptr / desc (host) are read by the uploads until the stream is drained here)
    MI355_TRY(sell_collect_values(rt.stream(), sp, t.counts, 2, rc));
    if(t.counts) // the periodic range of the records and lists as the device now holds them
        MI355_TRY(sell_search_range(sp, vsize));
    lt.lap("sell: values (fill, flags, range)");
    sp.count.value_fills++, sp.count.last_route = 1;
    sp.valid = sp.wanted = true;
    return aoclsparse_status_success;
}

} // namespace mi355

extern "C" {

aoclsparse_int mi355_sell_slice_records(aoclsparse_int nslices, const long long *slice_ptr, const aoclsparse_int *leaders,
                                                   long long column_entries, unsigned int *records)
{
    static_assert(sizeof(mi355::SellSliceDesc) == 4 * sizeof(unsigned int), "a slice record is four words");
    if(!records)
        return nslices < 0 ? -1 : nslices + mi355::SELL_DESC_PAD;
    if(nslices < 0 || !slice_ptr)
        return -1;
    mi355::sell_pack_descriptors(nslices, slice_ptr, leaders, column_entries, reinterpret_cast<mi355::SellSliceDesc *>(records));
    return nslices + mi355::SELL_DESC_PAD;
}

aoclsparse_status aoclsparse_mi355_get_sell_values(const aoclsparse_matrix A, aoclsparse_operation op, aoclsparse_int *table_entries)
{
    if(!A || !table_entries)
        return aoclsparse_status_invalid_pointer;
    std::shared_lock<std::shared_mutex> r(A->guard);
    const SpmvPlan                     &p = op != aoclsparse_operation_none ? A->plan_trans : A->plan_user;
    *table_entries                        = p.sell.valid ? p.sell.vals.ntab : 0;
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_mi355_get_sell_packing(const aoclsparse_matrix A, aoclsparse_operation op, aoclsparse_int *index_bits,
                                                    aoclsparse_int *word_bytes, aoclsparse_int *uniform_slices)
{
    if(!A || !index_bits || !word_bytes || !uniform_slices)
        return aoclsparse_status_invalid_pointer;
    std::shared_lock<std::shared_mutex> r(A->guard);
    const SpmvPlan                     &p = op != aoclsparse_operation_none ? A->plan_trans : A->plan_user;
    const bool packed = p.sell.valid && p.sell.vals.ntab > 0 && p.sell.vals.pbits > 0;
    *index_bits       = packed ? p.sell.vals.pbits : 0;
    *word_bytes       = packed ? p.sell.vals.pbytes : 0;
    *uniform_slices   = p.sell.valid && p.sell.vals.ucol.ptr ? p.sell.vals.uniform : 0;
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_mi355_get_sell_records(const aoclsparse_matrix A, aoclsparse_operation op, aoclsparse_int *uniform_word_slices,
                                                    aoclsparse_int *exception_slices)
{
    if(!A || !uniform_word_slices || !exception_slices)
        return aoclsparse_status_invalid_pointer;
    std::shared_lock<std::shared_mutex> r(A->guard);
    const SpmvPlan                     &p = op != aoclsparse_operation_none ? A->plan_trans : A->plan_user;
    const bool                          on = p.sell.valid && p.sell.vals.ucol.ptr;
    *uniform_word_slices                   = on ? p.sell.vals.uniform_words : 0;
    *exception_slices                      = on ? p.sell.vals.exceptions : 0;
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_mi355_get_sell_period(const aoclsparse_matrix A, aoclsparse_operation op, aoclsparse_int *first_slice,
                                                   aoclsparse_int *end_slice, aoclsparse_int *period_slices, aoclsparse_int *column_stride)
{
    if(!A || !first_slice || !end_slice || !period_slices || !column_stride)
        return aoclsparse_status_invalid_pointer;
    std::shared_lock<std::shared_mutex> r(A->guard);
    const SpmvPlan                     &p = op != aoclsparse_operation_none ? A->plan_trans : A->plan_user;
    const bool                          on = p.sell.valid && p.sell.vals.ucol.ptr;
    *first_slice                           = on ? p.sell.vals.pslo : 0;
    *end_slice                             = on ? p.sell.vals.pshi : 0;
    *period_slices                         = on ? p.sell.vals.pper : 0;
    *column_stride                         = on ? p.sell.vals.pstride : 0;
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_mi355_get_sell_march(const aoclsparse_matrix A, aoclsparse_operation op, aoclsparse_int *first_slice,
                                                  aoclsparse_int *end_slice, aoclsparse_int *periods, aoclsparse_int *alias_map)
{
    if(!A || !first_slice || !end_slice || !periods || !alias_map)
        return aoclsparse_status_invalid_pointer;
    std::shared_lock<std::shared_mutex> r(A->guard);
    const SpmvPlan                     &p = op != aoclsparse_operation_none ? A->plan_trans : A->plan_user;
    SellMarch                           mr;
    // (what sell_launch_short asks before it calls the rule: a real plan with slice records, uniform lists and packed words)
    if(p.sell.valid && p.sell.st.pack == 1 && p.sell.st.desc.ptr && p.sell.vals.ucol.ptr && p.sell.vals.ntab > 0 && p.sell.vals.ntab <= 2 && p.sell.vals.pbits > 0
       && !is_complex_type(A->val_type) && p.max_row_nnz <= SELL_SHORT_WMAX)
        mr = sell_march_rule(p.sell.st.nslices, p.max_row_nnz, p.sell.vals.pslo, p.sell.vals.pshi, p.sell.vals.pper, p.sell.vals.pstride, p.sell.vals.mstack,
                             p.sell.vals.malias, val_size(A->val_type), sell_short_spw(p.sell.st.nslices, val_size(A->val_type), true));
    *first_slice = mr.lo, *end_slice = mr.hi, *periods = mr.g, *alias_map = (aoclsparse_int)mr.alias;
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_mi355_get_sell_keep_info(const aoclsparse_matrix A, aoclsparse_operation op,
                                                      aoclsparse_mi355_sell_keep_info *info)
{
    if(!A || !info)
        return aoclsparse_status_invalid_pointer;
    if(info->struct_size < sizeof(info->struct_size))
        return aoclsparse_status_invalid_size;
    aoclsparse_mi355_sell_keep_info r{};
    if(op == aoclsparse_operation_none) // (only the handle's own operator keeps anything)
    {
        std::shared_lock<std::shared_mutex> g(A->guard);
        const SellPlan                     &sp = A->plan_user.sell;
        r.kept = sp.st.built, r.valid = sp.valid, r.last_route = sp.count.last_route;
        r.structure_builds = sp.count.structure_builds, r.value_fills = sp.count.value_fills, r.searches_skipped = sp.count.searches_skipped;
        r.kept_bytes = sp.st.built ? (long long)sp.st.kept_bytes() : 0;
    }
    r.struct_size = info->struct_size; // (the caller's: it says how much of the struct the caller has)
    std::memcpy(info, &r, std::min(info->struct_size, sizeof(r))); // no more than that is written
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_mi355_sell_find_march(aoclsparse_int nslices, const void *records, const aoclsparse_int *lists,
                                                   const aoclsparse_int range[4], aoclsparse_int word_bytes, aoclsparse_int out[2])
{
    if(!records || !lists || !range || !out)
        return aoclsparse_status_invalid_pointer;
    if(nslices < 0)
        return aoclsparse_status_invalid_size;
    sell_find_march(static_cast<const SellSliceDesc *>(records), lists, nslices, range, (int)word_bytes, out);
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_mi355_sell_march_rule(aoclsparse_int nslices, aoclsparse_int max_width, const aoclsparse_int range[4],
                                                   aoclsparse_int stack, aoclsparse_int alias_map, aoclsparse_int value_bytes,
                                                   aoclsparse_int slices_per_wavefront, aoclsparse_int out[4])
{
    if(!range || !out)
        return aoclsparse_status_invalid_pointer;
    const SellMarch mr = sell_march_rule(nslices, max_width, (int)range[0], (int)range[1], (int)range[2], (int)range[3], (int)stack,
                                         (unsigned)alias_map, (size_t)value_bytes, (int)slices_per_wavefront);
    out[0] = mr.lo, out[1] = mr.hi, out[2] = mr.g, out[3] = (aoclsparse_int)mr.alias;
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_mi355_sell_find_period(aoclsparse_int nslices, const void *records, const aoclsparse_int *lists,
                                                    aoclsparse_int max_period, aoclsparse_int range[4], long long *comparisons)
{
    if(!records || !lists || !range)
        return aoclsparse_status_invalid_pointer;
    if(nslices < 0 || max_period < 0)
        return aoclsparse_status_invalid_size;
    sell_find_period(static_cast<const SellSliceDesc *>(records), lists, nslices, max_period, range, comparisons);
    return aoclsparse_status_success;
}

} // extern "C"
