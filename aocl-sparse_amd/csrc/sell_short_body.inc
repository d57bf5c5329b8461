// The body of sell_mv_short_kernel, sell_mv_short_period_kernel and sell_mv_short_march_kernel (sell_kernels.hip): included inside
// each kernel, not a function of its own, so that the kernels without a periodic range stay the machine code they were.  Reads the
// kernel's template parameters and arguments by name, and its group of slices as bgroup; PERIOD: the kernel has the range arguments
// pslo, plen, pper, prcp, pstrideb.
// (As a PERIOD-templated __forceinline__ device function the same text gave the 120 short-row kernels without uniform lists the same
// instructions in other registers -- tools/isa_identity.py -- which is the only reason for the include: worth trying again with a
// later compiler.)
    using R = typename SellCell<T, TAB != 0>::raw;
    // the mapping of a run (below): double, several slices per wavefront, uniform lists and packed words.  (Float was built and
    // measured with it -- 28 -> 7 vector memory instructions per wavefront and the same time, DESIGN.md 5.1 -- and keeps the
    // mapping by slice; the code below is written for any real type and any SPW > 1.)
    constexpr bool WIDE = UCOL && PK && SPW > 1 && std::is_same_v<T, double>;
    // what the records say beyond offsets and mode (plans with uniform lists and one-byte words: internal.hpp, SELL_DESC_UWORD /
    // SELL_DESC_EXCEPT): a slice's rows share ONE word, held by the record; a mode-0 slice is one list shifted by lane in which
    // two lanes at most omit cells -- it counts as shifted here, for the column decision and the run test
    constexpr bool REC = UCOL && PK;
    static_assert(WAVES * SPW <= SELL_DESC_PAD && 64 * WAVES == SELL_VTAB_MAX, "padding of the slice records / one table entry per lane");
    static_assert(!PK || TAB != 0, "packed words hold table indices");
    // group g of WAVES x SPW slices; consecutive products of a handle ALTERNATE the direction (SellPlan::products): g0 = last
    // group, gstep = -1 on odd ones
    // (bgroup: the including kernel's name for that group.  MARCH -- sell_mv_short_march_kernel, whose other workgroups take the
    // slices [pslo, pslo + mskip) stacked: the groups here count the slices OUTSIDE that part, which starts and ends at a multiple
    // of 4 slices, so a wavefront's SPW slices are all before it or all behind it)
    int sbg = __builtin_amdgcn_readfirstlane((bgroup * WAVES + (int)(threadIdx.x >> 6)) * SPW);
    if constexpr(MARCH)
        sbg = sbg >= pslo ? sbg + mskip : sbg;
    const int sb   = sbg;
    const int lane = threadIdx.x & 63;
    s_pin_arg(alpha), s_pin_arg(beta), s_pin_arg(y), s_pin_arg((int)nt), s_pin_arg(x), s_pin_arg(sval), s_pin_arg(scol), s_pin_arg(follow);
    s_pin_arg(pbits), s_pin_arg(pbytes); // (not ucol / vtab: a pointer handed to an asm statement is no longer read with scalar loads)
    [[maybe_unused]] T t0, t1;
    if constexpr(TAB == 2)
        t0 = vtab[0], t1 = vtab[1];
    else if constexpr(TAB != 0)
        t0 = vtab[threadIdx.x];
    // PERIODIC RANGE (PERIOD: sell_mv_short_period_kernel; SellValues::pslo .., found at plan time by sell_find_period): the records
    // and lists of slice s in [pslo + pper, pslo + plen) are those of slice s - pper with every column moved by pstride, so a
    // wavefront whose slices lie in [pslo, pslo + plen) reads the records and lists of the FIRST period -- the same few lines for
    // every wavefront, a hit in the scalar cache or the L2 instead of a cold trip to HBM -- and gathers from x + k pstride.
    // A handful of scalar instructions, no branch and no division: k = the high word of (slice - pslo) x prcp, the launcher's
    // reciprocal of pper, taken as 0 outside the range (plen = 0: the plan has none).  The shift goes to the BASE x, not to the
    // list entries: every scalar instruction here is paid by all 131,072 wavefronts of the headline, and a select and an add per
    // entry cost more than the cold trip saved (profiles/r17/upper_bound.txt).  An unused entry (-1) of a slice in the range
    // therefore gathers at x + k pstride + the lane's offset: inside x, because a slice of the range has a first cell
    // (sell_find_period takes no slice of width 0) and that cell's columns start at or behind x + k pstride.  Range and period
    // are multiples of 4 slices: the SPW slices of a wavefront are all inside or all outside.  Everything but this batch and the
    // gathers' base (the rows' words, y, the store guard) keeps the real sb.
    [[maybe_unused]] const T *xs = x; // where the slices' columns count from: x, or x + k pstride in the periodic range
    if constexpr(PERIOD)
    {
        const unsigned rel = (unsigned)(sb - pslo);
        const unsigned k   = __umulhi(rel, rel < (unsigned)plen ? prcp : 0u);
        const unsigned sp  = (unsigned)sb - k * (unsigned)pper;
        // (ONE base for the records and one for the lists, the slices at constant offsets; the shift in bytes, below 2^32 by the
        // launcher's check)
        desc = reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(desc) + sp * (unsigned)sizeof(uint4));
        ucol = reinterpret_cast<const aoclsparse_int *>(reinterpret_cast<const char *>(ucol)
                                                        + sp * (unsigned)(SELL_SHORT_WMAX * sizeof(aoclsparse_int)));
        xs   = reinterpret_cast<const T *>(reinterpret_cast<const char *>(x) + k * pstrideb);
    }
    uint4 d[SPW];
#pragma unroll
    for(int u = 0; u < SPW; u++)
        d[u] = PERIOD ? desc[u] : desc[sb + u];
    [[maybe_unused]] int uc[SPW][WMAX]; // the slices' uniform lists: scalars
    if constexpr(UCOL)
    {
#pragma unroll
        for(int u = 0; u < SPW; u++)
#pragma unroll
            for(int q = 0; q < WMAX; q++)
                uc[u][q] = PERIOD ? ucol[u * SELL_SHORT_WMAX + q] : ucol[(sb + u) * SELL_SHORT_WMAX + q];
    }
    // the rows' packed index words.  Kernels without the run mapping load them HERE, with the records; the others behind the
    // decision, which says whose rows they are
    [[maybe_unused]] unsigned pw[SPW];
    auto words_by_slice = [&]() {
        if constexpr(PK)
        {
            // (TAB 2: <= 8 cells of one bit, always a byte; else the width is a run-time scalar and the load has no branch)
            const long long row = (long long)sb * 64 + lane;
#pragma unroll
            for(int u = 0; u < SPW; u++)
                pw[u] = TAB == 2 ? packed_word(sval, row + 64 * u, 1) : packed_word_any(sval, row + 64 * u, pbytes);
        }
    };
    if constexpr(!REC)
        words_by_slice();
    int  mode[SPW];
    bool lists = !UCOL; // the group reads its columns from the lists in col
#pragma unroll
    for(int u = 0; u < SPW; u++)
    {
        mode[u] = (int)(d[u].w >> 16) & 0xff;
        if constexpr(!REC)
            lists = lists || !(mode[u] == SELL_DESC_MODE_LANE_SHIFT || mode[u] == SELL_DESC_MODE_ONE);
    }
    [[maybe_unused]] R rr[SPW][WMAX];
    if constexpr(!PK)
    {
#pragma unroll
        for(int u = 0; u < SPW; u++)
        {
            const long long o0 = (long long)d[u].x | (long long)(d[u].z & 0xffffu) << 32;
            const int       w  = (int)(d[u].w & 0xffu);
            const auto     *v  = sval + o0 + lane;
#pragma unroll
            for(int q = 0; q < WMAX; q++)
                rr[u][q] = v[max(min(q, w - 1), 0) * 64]; // (wave-uniform index)
        }
    }
    if constexpr(UCOL)
    {
        // the lists (and the two table entries) are in their scalar registers HERE: their loads go out with the records, in front of
        // the branch, not inside the path that uses them (one more scalar round trip there); then the whole batch is issued
        // before the branch
#pragma unroll
        for(int u = 0; u < SPW; u++)
#pragma unroll
            for(int q = 0; q < WMAX; q++)
                s_pin_arg(uc[u][q]);
        if constexpr(REC)
        {
            // all four words of every record too: the run test reads only w, and the compiler would otherwise fetch x / y / z
            // (offsets, needed by the lists in col alone; a flagged slice's word and lanes) behind the test -- a fourth round
            // trip on that path
#pragma unroll
            for(int u = 0; u < SPW; u++)
                s_pin_arg(d[u].x), s_pin_arg(d[u].y), s_pin_arg(d[u].z), s_pin_arg(d[u].w);
        }
        if constexpr(TAB == 2)
            s_pin_arg(t0), s_pin_arg(t1);
        __builtin_amdgcn_sched_barrier(0);
    }
    [[maybe_unused]] unsigned ew[SPW]; // the record's w with the mode of a flagged slice read as "shifted"
    [[maybe_unused]] bool     alluw = REC, anyex = false; // every slice has its word in the record / some slice has exception lanes
    if constexpr(REC)
    {
        // (behind the batch: scalar work on the records in front of it would split it in two round trips)
#pragma unroll
        for(int u = 0; u < SPW; u++)
        {
            const bool ex = (d[u].w & SELL_DESC_EXCEPT) != 0u;
            ew[u]         = ex ? ((d[u].w & 0xff00ffffu) | (unsigned)SELL_DESC_MODE_LANE_SHIFT << 16) : d[u].w;
            alluw         = alluw && (d[u].w & SELL_DESC_UWORD) != 0u;
            anyex         = anyex || ex;
            lists         = lists || !(ex || mode[u] == SELL_DESC_MODE_LANE_SHIFT || mode[u] == SELL_DESC_MODE_ONE);
        }
    }
    // A RUN: the group's SPW slices are all mode 1, of one width, and each list continues the list before it (column + 64 in
    // every used cell): row j of the group's 64 SPW rows reads x[uc[0][q] + j].  Scalar compares on what the batch above brought.
    // Words of more than one byte per row stay on the mapping by slice.
    [[maybe_unused]] bool run = false;
    if constexpr(WIDE)
    {
        // (one word of differences, no branch per compare: mode and width are bits 0 .. 7 and 16 .. 23 of w)
        const int w0  = (int)(d[0].w & 0xffu);
        unsigned  dif = (ew[0] ^ ((unsigned)SELL_DESC_MODE_LANE_SHIFT << 16)) & 0xff0000u;
        if constexpr(TAB != 2)
            dif |= (unsigned)(pbytes - 1);
#pragma unroll
        for(int u = 1; u < SPW; u++)
        {
            dif |= (ew[u] ^ ew[0]) & 0xff00ffu;
#pragma unroll
            for(int q = 0; q < WMAX; q++)
                dif |= q < w0 ? (unsigned)(uc[u][q] - uc[0][q] - 64 * u) : 0u;
        }
        run = dif == 0u;
    }
    T        xx[SPW][WMAX];
    unsigned okm[SPW]; // bit q: cell q of this lane's row is a cell of the matrix (inside the slice's width, no padding)
    // the columns from the lists in col, as a lane finds them through the slice's mode; then the gathers
    auto from_lists = [&]() {
        int  f[SPW]; // list of this lane | column shift << 8
        bool follows = false;
#pragma unroll
        for(int u = 0; u < SPW; u++)
        {
            follows = follows || mode[u] == SELL_DESC_MODE_FOLLOW;
            f[u]    = mode[u] == SELL_DESC_MODE_LANE_SHIFT ? lane << 8 : (mode[u] == SELL_DESC_MODE_OWN ? lane : 0);
        }
        if(follows) // wave-uniform
        {
            int ff[SPW];
#pragma unroll
            for(int u = 0; u < SPW; u++)
                ff[u] = follow[min((sb + u) * 64 + lane, (int)m - 1)];
#pragma unroll
            for(int u = 0; u < SPW; u++)
                f[u] = mode[u] == SELL_DESC_MODE_FOLLOW ? ff[u] : f[u];
        }
        int cc[SPW][WMAX];
#pragma unroll
        for(int u = 0; u < SPW; u++)
        {
            const long long c0 = (long long)d[u].y | (long long)(d[u].z >> 16) << 32;
            const int       w = (int)(d[u].w & 0xffu), cs = (int)(d[u].w >> 8) & 0xff;
            const aoclsparse_int *c = scol + c0 + (f[u] & 0xff);
#pragma unroll
            for(int q = 0; q < WMAX; q++)
                cc[u][q] = c[max(min(q, w - 1), 0) * cs]; // (wave-uniform index)
        }
        __builtin_amdgcn_sched_barrier(0); // (every line load is issued before the first wait for one)
#pragma unroll
        for(int u = 0; u < SPW; u++)
        {
            const int w = (int)(d[u].w & 0xffu);
            okm[u]      = 0;
#pragma unroll
            for(int q = 0; q < WMAX; q++) // (a padding cell, -1, is never used, but its gather must stay inside x: index 0)
            {
                xx[u][q] = x[cc[u][q] >= 0 ? cc[u][q] + (f[u] >> 8) : 0];
                okm[u] |= (q < w && cc[u][q] >= 0) ? 1u << q : 0u;
            }
        }
    };
    if constexpr(UCOL)
    {
        if(__builtin_expect(lists, 0)) // wave-uniform
        {
            // (a flagged slice is read here as every reader but this kernel reads it: its rows' own words, its lists through
            // follow[] -- the word of the record sits at the canonical cell positions, which are not the rows' own)
            if constexpr(REC)
                words_by_slice();
            from_lists();
        }
        else if(WIDE && __builtin_expect(run, 1)) // wave-uniform
        {
            // lane l owns the SPW CONSECUTIVE rows SPW l .. SPW l + SPW - 1 of the group: xx[u] / pw[u] / r[u] are row SPW l + u.
            // One gather per cell, SPW elements (16 bytes) per lane at the scalar base x + column (element-aligned only: column
            // i - 1 is odd); one load of the lane's SPW adjacent word bytes.  An unused entry (-1) gathers at x + the lane's
            // offset: inside x, a run has 64 SPW distinct columns in its first cell.
            if constexpr(WIDE)
            {
                using RowVec = SellRows<T, SPW>;
                using PW = std::conditional_t<SPW == 2, unsigned short, unsigned>;
                // the lane's SPW rows lie in ONE slice of the group, slice lane / (64 / SPW): its record's word where it has one
                const int ls   = lane / (64 / SPW);
                unsigned  rw   = d[0].x & 0xffu;
                bool      huw  = (d[0].w & SELL_DESC_UWORD) != 0u;
#pragma unroll
                for(int u = 1; u < SPW; u++)
                    rw = ls == u ? (d[u].x & 0xffu) : rw, huw = ls == u ? (d[u].w & SELL_DESC_UWORD) != 0u : huw;
                unsigned word = 0;
                if(!__builtin_expect(alluw, 1)) // wave-uniform: with every word in a record none is read
                    word = *reinterpret_cast<const PW *>(reinterpret_cast<const unsigned char *>(sval) + (long long)sb * 64 + SPW * lane);
#pragma unroll
                for(int u = 0; u < SPW; u++)
                    okm[u] = (1u << (d[0].w & 0xffu)) - 1u;
                if(__builtin_expect(anyex, 0)) // wave-uniform: row 64 v + (exception lane) of the group is row u of lane owner
                {
#pragma unroll
                    for(int v = 0; v < SPW; v++)
                    {
                        const bool     ex = (d[v].w & SELL_DESC_EXCEPT) != 0u;
                        const unsigned la = (d[v].x >> 8) & 0xffu, lb = d[v].x >> 24;
                        const unsigned ma = (d[v].x >> 16) & 0xffu, mb = d[v].z & 0xffu;
                        const int      ga = ex && la != SELL_DESC_NO_LANE ? 64 * v + (int)la : -SPW;
                        const int      gb = ex && lb != SELL_DESC_NO_LANE ? 64 * v + (int)lb : -SPW;
#pragma unroll
                        for(int u = 0; u < SPW; u++)
                        {
                            okm[u] = (ga >= 0 && ga % SPW == u && lane == ga / SPW) ? ma : okm[u];
                            okm[u] = (gb >= 0 && gb % SPW == u && lane == gb / SPW) ? mb : okm[u];
                        }
                    }
                }
                using GV = const __attribute__((address_space(1))) RowVec;
                using GC = const __attribute__((address_space(1))) char;
#pragma unroll
                for(int q = 0; q < WMAX; q++)
                {
                    GC *gb = (GC *)(xs + max(uc[0][q], 0));
                    asm volatile("" : "+s"(gb)); // (the base stays a scalar pair: as on the path below)
                    const RowVec xv = *(GV *)(gb + (unsigned)lane * (unsigned)sizeof(RowVec));
#pragma unroll
                    for(int u = 0; u < SPW; u++)
                        xx[u][q] = xv[u];
                }
#pragma unroll
                for(int u = 0; u < SPW; u++) // (behind the gathers: the first use of a word that was read)
                    pw[u] = huw ? rw : (word >> (8 * u)) & 0xffu;
            }
        }
        else
        {
            if constexpr(REC)
            {
#pragma unroll
                for(int u = 0; u < SPW; u++)
                    pw[u] = 0;
                if(!__builtin_expect(alluw, 1)) // wave-uniform: with every word in a record none is read
                    words_by_slice();
            }
            // every slice of the group has one list: a gather is a scalar base, x + column, plus the lane's shift (mode 1) in
            // bytes -- no address arithmetic in vector registers.  An unused entry (-1) gathers at x + shift, which is inside x:
            // a mode-1 slice has 64 distinct columns in its first cell, and the empty records behind the last slice are mode 2
            // (no shift).  A mode 1 / 2 slice is full and its rows repeat one list: every row has exactly w cells, none padded.
#pragma unroll
            for(int u = 0; u < SPW; u++)
            {
                bool shifted = mode[u] == SELL_DESC_MODE_LANE_SHIFT;
                if constexpr(REC)
                    shifted = shifted || (d[u].w & SELL_DESC_EXCEPT) != 0u;
                const unsigned sh = shifted ? (unsigned)lane * (unsigned)sizeof(T) : 0u;
#pragma unroll
                for(int q = 0; q < WMAX; q++)
                {
                    const T *xb = xs + max(uc[u][q], 0);
                    if constexpr(std::is_floating_point_v<T>)
                    {
                        // (the base stays a scalar pair, in the global address space: the load takes it as it is.  If a compiler
                        // stops honouring this the base moves to vector registers: slower, the same loads, the same bits --
                        // profiles/r10/isa_waits_after.txt is the check)
                        using GT = const __attribute__((address_space(1))) T;
                        using GC = const __attribute__((address_space(1))) char;
                        GT *gb   = (GT *)xb;
                        asm volatile("" : "+s"(gb));
                        xx[u][q] = *(GT *)((GC *)gb + sh);
                    }
                    else
                        xx[u][q] = *reinterpret_cast<const T *>(reinterpret_cast<const char *>(xb) + sh);
                }
                okm[u] = (1u << (d[u].w & 0xffu)) - 1u;
                if constexpr(REC)
                {
                    // an exception lane has only the cells of its mask (its other gathers, at B + lane, are inside x and are
                    // dropped by the select of the chain); without the flag no lane compares equal
                    const bool     ex = (d[u].w & SELL_DESC_EXCEPT) != 0u;
                    const unsigned la = ex ? (d[u].x >> 8) & 0xffu : SELL_DESC_NO_LANE, lb = ex ? d[u].x >> 24 : SELL_DESC_NO_LANE;
                    okm[u]            = (unsigned)lane == la ? (d[u].x >> 16) & 0xffu : okm[u];
                    okm[u]            = (unsigned)lane == lb ? d[u].z & 0xffu : okm[u];
                }
            }
            if constexpr(REC)
            {
#pragma unroll
                for(int u = 0; u < SPW; u++) // (behind the gathers: the first use of a word that was read)
                    pw[u] = (d[u].w & SELL_DESC_UWORD) != 0u ? (d[u].x & 0xffu) : pw[u];
            }
        }
    }
    else
        from_lists();
    [[maybe_unused]] __shared__ T ltab[TAB > 2 ? SELL_VTAB_MAX : 1];
    if constexpr(TAB > 2) // (behind the gathers: the barrier is waited for while they are in flight)
    {
        ltab[threadIdx.x] = t0;
        __syncthreads();
    }
    T r[SPW];
#pragma unroll
    for(int u = 0; u < SPW; u++)
    {
        r[u] = T(0);
#pragma unroll
        for(int q = 0; q < WMAX; q++)
        {
            T vv;
            if constexpr(TAB == 0)
                vv = s_cj<CONJ>(rr[u][q]);
            else if constexpr(TAB == 2 && PK)
                vv = ((pw[u] >> q) & 1u) ? t1 : t0;
            else if constexpr(TAB == 2)
                vv = rr[u][q] ? t1 : t0;
            else if constexpr(PK)
                vv = ltab[packed_index(pw[u], q, pbits)];
            else
                vv = ltab[rr[u][q]];
            r[u] = ((okm[u] >> q) & 1u) ? s_fma(vv, xx[u][q], r[u]) : r[u];
        }
    }
#pragma unroll
    for(int u = 0; u < SPW; u++)
        s_pin(r[u]); // (every load above is issued before the first guarded store)
    if constexpr(WIDE)
    {
        if(__builtin_expect(run, 1)) // the lane's SPW rows are adjacent, inside m (mode 1 slices are full): one store
        {
            using RowVec = SellRows<T, SPW>;
            RowVec *yp = reinterpret_cast<RowVec *>(y + (long long)sb * 64 + SPW * lane);
            RowVec  yv = {};
            if(beta != T(0))
                yv = *yp;
#pragma unroll
            for(int u = 0; u < SPW; u++)
            {
                const T yu = yv[u];
                yv[u]      = s_finish(r[u], alpha, beta, &yu);
            }
            if(nt)
                __builtin_nontemporal_store(yv, yp);
            else
                *yp = yv;
            return;
        }
    }
#pragma unroll
    for(int u = 0; u < SPW; u++)
    {
        const int i = (sb + u) * 64 + lane;
        if(sb + u < nslices && i < m)
            s_store(y + i, s_finish(r[u], alpha, beta, y + i), nt);
    }
