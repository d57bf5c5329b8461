// The periodic range of a SELL-64 copy's slice records and uniform column lists (internal.hpp: sell_find_period).  Host only:
// build_sell runs it on a copy of the device arrays, aoclsparse_mi355_sell_find_period on the caller's.
//
// On a stencil the records and lists of grid line j + 1 are those of line j with every column moved by one line.  The short-row
// kernel (sell_kernels.hip: sell_mv_short_period_kernel) then reads the records and lists of the FIRST period for every slice of
// the range and adds k x stride to the columns, so what is reported here must be exact: every comparison is on the fields
// themselves.
//
// The rule.  A slice is ELIGIBLE when its mode is 1 or 2 or it carries SELL_DESC_EXCEPT (its group never reads the lists in col),
// its width is >= 1 and its first list entry is a column (ucol[s][0] >= 0): the kernel moves the BASE of the gathers by
// k x stride, and what keeps the gather of an unused entry inside x is that the slice's own first column lies at or behind
// that base.
// Slice s MATCHES slice s - p when both are eligible and
//   * their wsm words are equal;
//   * with SELL_DESC_UWORD, bits 0-7 of cell_lo are equal;
//   * with SELL_DESC_EXCEPT, all of cell_lo and bits 0-7 of hi are equal;
//   * for every cell q below the width, ucol[s][q] == ucol[s - p][q] + 64 p, and an entry of -1 equals -1.
// A RANGE of period p is [lo, hi) with every slice eligible and every slice of [lo + p, hi) matching its slice - p; lo and hi
// are cut to multiples of 4 slices (lo up, hi down).  It must hold half of the slices, because the plan keeps one range (two
// ranges of one period are disjoint, so at most one does), and two periods (hi - lo >= 2 p): in a range of one period every
// wavefront would read its own records, as it does without a range.  The result is the SMALLEST p that is a multiple of 4,
// at most `cap`, and has such a range; stride = 64 p, the column shift of a square stencil.
//
// How the work is bounded.  All of the above is a statement about N[s] = (wsm, the word bits that count, ucol[s][q] - 64 s): s
// matches s - p exactly when N[s] == N[s - p].  A range that holds half of the nslices slices contains slice c = nslices / 2 or
// c - 1.  (1) Its slices are all eligible, so the eligible slices around c (or c - 1) must run for nslices / 2: one pass, and a
// matrix whose stencil part is embedded in slices of other kinds ends here.  (2) As it holds two periods, c (or c - 1) matches
// its slice - p or is matched by its slice + p, and the matching run around that position is hi - lo - p >= nslices / 4 long:
// a period gets its one pass over all slices only if one of those four positions passes this test.  On a clean stencil a
// period that fails costs the rest of a grid line and the first period that gets its pass is the answer.  (3) Nothing of this
// bounds a matrix whose middle repeats with EVERY period while its ends, though eligible, repeat with none: each period would
// pass (2) and fail its pass.  So the search counts the pairs of slices it compares and GIVES UP -- no range, the kernel reads
// every slice's own records -- when the next step would take it beyond SELL_PERIOD_WORK = 8 comparisons per slice; the
// headline needs about 1.3, a 3000 x 3000 grid (period 1500 slices) about 2.
#include "internal.hpp"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

namespace mi355
{

namespace
{
// what must be equal between a slice and the slice one period before it
struct Norm
{
    uint32_t wsm, lo, hi;
    int32_t  rel[SELL_SHORT_WMAX]; // ucol - 64 s below the width (an entry of -1: INT32_MIN), 0 from the width on
};
static_assert(sizeof(Norm) == 4 * (3 + SELL_SHORT_WMAX), "compared as bytes: no padding");
} // namespace

void sell_find_period(const SellSliceDesc *desc, const aoclsparse_int *ucol, aoclsparse_int nslices, aoclsparse_int cap,
                      aoclsparse_int out[4], long long *comparisons)
{
    out[0] = out[1] = out[2] = out[3] = 0;
    long long work = 0; // pairs of slices compared
    if(comparisons)
        *comparisons = 0;
    if(!desc || !ucol || nslices < 8 || cap < 4)
        return;
    const long long      n = nslices, budget = (long long)SELL_PERIOD_WORK * n;
    std::vector<Norm>    nm;
    std::vector<uint8_t> el;
    try
    {
        nm.resize((size_t)n), el.resize((size_t)n);
    }
    catch(const std::bad_alloc &)
    {
        return; // (no range: the kernel reads every slice's own records)
    }
    for(long long s = 0; s < n; s++)
    {
        const SellSliceDesc &d    = desc[s];
        const int            mode = (int)(d.wsm >> 16) & 0xff, w = std::min<int>((int)(d.wsm & 0xffu), SELL_SHORT_WMAX);
        const bool           ex   = (d.wsm & SELL_DESC_EXCEPT) != 0u;
        el[(size_t)s]             = w >= 1 && ucol[s * SELL_SHORT_WMAX] >= 0
                        && (ex || mode == SELL_DESC_MODE_LANE_SHIFT || mode == SELL_DESC_MODE_ONE);
        Norm &o                   = nm[(size_t)s];
        o.wsm                     = d.wsm;
        o.lo                      = ex ? d.cell_lo : ((d.wsm & SELL_DESC_UWORD) ? d.cell_lo & 0xffu : 0u);
        o.hi                      = ex ? d.hi & 0xffu : 0u;
        for(int q = 0; q < SELL_SHORT_WMAX; q++)
        {
            const aoclsparse_int c = ucol[s * SELL_SHORT_WMAX + q];
            o.rel[q]               = q >= w ? 0 : (c < 0 ? INT32_MIN : (int32_t)((long long)c - 64 * s));
        }
    }
    const long long c = n / 2;
    // (1) the eligible slices around c or c - 1 run for half of the slices
    {
        long long a = c - 1, b = c - 1;
        if(!el[(size_t)(c - 1)])
            a = b = c;
        if(!el[(size_t)a])
            return;
        while(a > 0 && el[(size_t)(a - 1)])
            a--;
        while(b + 1 < n && el[(size_t)(b + 1)])
            b++;
        if(2 * (b + 1 - a) < n)
            return;
    }
    // s matches s - p (p <= s < n)
    auto match = [&](long long s, long long p) {
        work++;
        return el[(size_t)s] && el[(size_t)(s - p)] && std::memcmp(&nm[(size_t)s], &nm[(size_t)(s - p)], sizeof(Norm)) == 0;
    };
    // (2) the matches of period p around position t go on for `need` slices at least (false, too, when the budget runs out)
    auto run_around = [&](long long t, long long p, long long need) {
        if(t < p || t >= n || work >= budget || !match(t, p))
            return false;
        long long len = 1;
        for(long long s = t - 1; s >= p && len < need && work < budget && match(s, p); s--)
            len++;
        for(long long s = t + 1; s < n && len < need && work < budget && match(s, p); s++)
            len++;
        return len >= need;
    };
    const long long need = std::max<long long>(n / 4, 1);
    for(long long p = 4; p <= std::min<long long>(cap, n / 2) && work < budget; p += 4)
    {
        if(!(run_around(c, p, need) || run_around(c + p, p, need) || run_around(c - 1, p, need) || run_around(c - 1 + p, p, need)))
            continue;
        if(work + n > budget) // (3)
            break;
        // the one pass: every run [a, b) of matches gives the range [a - p, b)
        long long best_lo = 0, best_hi = 0;
        for(long long s = p; s < n;)
        {
            if(!match(s, p))
            {
                s++;
                continue;
            }
            long long b = s + 1;
            while(b < n && match(b, p))
                b++;
            const long long lo = (s - p + 3) / 4 * 4, hi = b / 4 * 4;
            if(hi - lo >= 2 * p && 2 * (hi - lo) >= n && hi - lo > best_hi - best_lo)
                best_lo = lo, best_hi = hi;
            s = b;
        }
        if(best_hi > best_lo)
        {
            out[0] = (aoclsparse_int)best_lo, out[1] = (aoclsparse_int)best_hi, out[2] = (aoclsparse_int)p;
            out[3] = (aoclsparse_int)(64 * p);
            break;
        }
    }
    if(comparisons)
        *comparisons = work;
}

// Whether a periodic range can be stacked, and the alias map of its first period (internal.hpp states both rules; the kernel that
// relies on them makes no test of its own, so every comparison is on the fields themselves, as above).
void sell_find_march(const SellSliceDesc *desc, const aoclsparse_int *ucol, aoclsparse_int nslices, const aoclsparse_int range[4],
                     int word_bytes, aoclsparse_int out[2])
{
    out[0] = out[1] = 0;
    if(!desc || !ucol || !range)
        return;
    const long long lo = range[0], hi = range[1], p = range[2], stride = range[3];
    if(p < SELL_MARCH_GROUP || p % SELL_MARCH_GROUP != 0 || lo < 0 || lo % SELL_MARCH_GROUP != 0 || hi > nslices || hi - lo < p)
        return;
    // the record's word as the kernel's run test reads it: the mode of a flagged slice counts as "shifted"
    auto shifted_word = [&](long long s) {
        const uint32_t w = desc[s].wsm;
        return (w & SELL_DESC_EXCEPT) ? ((w & 0xff00ffffu) | (uint32_t)SELL_DESC_MODE_LANE_SHIFT << 16) : w;
    };
    bool stack = word_bytes == 1;
    for(long long g = lo; g < lo + p && stack; g += SELL_MARCH_GROUP)
    {
        const uint32_t e0 = shifted_word(g);
        const int      w0 = std::min<int>((int)(e0 & 0xffu), SELL_SHORT_WMAX);
        stack             = ((e0 >> 16) & 0xffu) == (uint32_t)SELL_DESC_MODE_LANE_SHIFT && w0 >= 1;
        for(int u = 0; u < SELL_MARCH_GROUP && stack; u++)
        {
            stack = (desc[g + u].wsm & SELL_DESC_UWORD) != 0u && ((shifted_word(g + u) ^ e0) & 0xff00ffu) == 0u;
            for(int q = 0; q < w0 && stack; q++)
                stack = (long long)ucol[(g + u) * SELL_SHORT_WMAX + q] == (long long)ucol[g * SELL_SHORT_WMAX + q] + 64 * u;
        }
    }
    out[0] = stack ? 1 : 0;
    uint32_t map = 0;
    for(int q = 0; q < SELL_SHORT_WMAX; q++)
        for(int r = 0; r < SELL_SHORT_WMAX; r++)
        {
            bool all = r != q;
            for(long long s = lo; s < lo + p && all; s++)
            {
                const int            w = std::min<int>((int)(desc[s].wsm & 0xffu), SELL_SHORT_WMAX);
                const aoclsparse_int a = ucol[s * SELL_SHORT_WMAX + q], b = ucol[s * SELL_SHORT_WMAX + r];
                all                    = q < w && r < w && a >= 0 && b >= 0 && (long long)b == (long long)a + stride;
            }
            if(all && !((map >> (4 * q)) & 0xfu)) // (two equal columns in one list: the first)
                map |= (uint32_t)(r + 1) << (4 * q);
        }
    out[1] = (aoclsparse_int)map;
}

} // namespace mi355
