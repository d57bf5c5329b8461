// sell_build_kernels.hip -- plan-time kernels of the SELL-64 copy (sell_plan.cpp: build_sell); the products are in sell_kernels.hip.
//
// The layout: sliced ELL with one slice per 64-wide wavefront.  Slice s holds rows [64 s, 64 s + 64) column-major, cell (p, lane) at
// slice_ptr[s] + 64 p + lane, padded to the slice's longest row (column -1, value 0); matrices with >= 16 non-zeros per row keep
// four consecutive cells of a row adjacent instead (PACK 4: cell at slice_ptr[s] + 256 (p/4) + 4 lane + p%4, width rounded up to a
// multiple of 4), so that a wavefront's load is one contiguous 2 KB piece -- the in-flight slices of a long-row matrix are otherwise
// 512-byte accesses strided by the slice size, which costs HBM page locality.  Lane i of a wave owns row i.
#include "internal.hpp"

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include <hip/hip_runtime.h>

namespace mi355
{

namespace
{

// ---- value tables (SELL-64 with one byte per cell: an index into <= 256 distinct value bit patterns) ---------------------
// A matrix whose values take at most SELL_VTAB_MAX distinct bit patterns (a constant-coefficient stencil: two) stores one byte
// per cell and a table sorted by ascending bit pattern; the kernels read table[index], i.e. the very bits of the value, so every
// summation order gives the same results as with the values stored in the cells (CSR-VI, Kourtis, Goumas and Koziris, CF 2008).
// Bit patterns, not values: -0.0 and +0.0 are two entries, NaN payloads are kept.
template <typename T>
using vbits_t = std::conditional_t<sizeof(T) == 8, unsigned long long, unsigned>;

// index of v in the sorted table (v is in it: the table holds every pattern of the matrix)
template <typename T>
__device__ __forceinline__ unsigned char vtab_index(T v, const T *__restrict__ vtab, int ntab)
{
    using U     = vbits_t<T>;
    const U key = __builtin_bit_cast(U, v);
    int     lo = 0, hi = ntab - 1;
    while(lo < hi)
    {
        const int mid = (lo + hi) >> 1;
        if(__builtin_bit_cast(U, vtab[mid]) < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return (unsigned char)lo;
}

// writes cell o: the value, or (sidx) its table index; padding cells hold 0 / index 0 (their column is -1: never used)
template <typename T>
__device__ __forceinline__ void fill_cell(long long o, bool in, const T *__restrict__ vp, T *__restrict__ sval,
                                          unsigned char *__restrict__ sidx, const T *__restrict__ vtab, int ntab)
{
    if constexpr(std::is_floating_point_v<T>)
    {
        if(sidx)
        {
            sidx[o] = in ? vtab_index(*vp, vtab, ntab) : (unsigned char)0;
            return;
        }
    }
    sval[o] = in ? *vp : T(0);
}

// Distinct bit patterns of n values, on the device: every workgroup collects what it sees in an LDS hash set, then merges it
// into the global set (VT_SLOTS entries, VT_EMPTY = free).  state[0] = patterns in the global set, state[1] = 1 once more than
// SELL_VTAB_MAX patterns were seen (everyone stops early), state[2] = 1 if the pattern VT_EMPTY itself (a double NaN) occurs.
// A set that fills up also means "more than SELL_VTAB_MAX": a set has 4 x the slots that can be taken before a stop is seen.
constexpr int                VT_LDS_SLOTS  = 1024;
constexpr int                VT_SLOTS      = 4096;
constexpr unsigned long long VT_EMPTY      = ~0ull;

__device__ __forceinline__ unsigned vt_hash(unsigned long long k)
{
    k ^= k >> 33; // (murmur3's finaliser: the patterns of simple doubles differ in their top bits only)
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (unsigned)k;
}

// 1: k was inserted, 0: it was there already, -1: the set is full
__device__ __forceinline__ int vt_insert(unsigned long long *set, int slots, unsigned long long k)
{
    unsigned h = vt_hash(k) & (unsigned)(slots - 1);
    for(int probe = 0; probe < slots; probe++)
    {
        unsigned long long cur = __hip_atomic_load(set + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if(cur == k)
            return 0;
        if(cur == VT_EMPTY)
        {
            cur = atomicCAS(set + h, VT_EMPTY, k);
            if(cur == VT_EMPTY)
                return 1;
            if(cur == k)
                return 0;
        }
        h = (h + 1) & (unsigned)(slots - 1);
    }
    return -1;
}

template <typename U>
__global__ __launch_bounds__(256) void sell_vtab_count_kernel(long long n, const U *__restrict__ val, unsigned long long *__restrict__ set,
                                                              unsigned *__restrict__ state)
{
    constexpr int                 UNR = 4;
    __shared__ unsigned long long lset[VT_LDS_SLOTS];
    __shared__ int                lcount, lstop, lempty;
    for(int k = threadIdx.x; k < VT_LDS_SLOTS; k += blockDim.x)
        lset[k] = VT_EMPTY;
    if(threadIdx.x == 0)
        lcount = 0, lstop = 0, lempty = 0;
    __syncthreads();
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x; i0 < n; i0 += UNR * stride)
    {
        if(__hip_atomic_load(&lstop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
           || __hip_atomic_load(state + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            break;
        unsigned long long k[UNR];
#pragma unroll
        for(int u = 0; u < UNR; u++)
            k[u] = (unsigned long long)val[i0 + u * stride < n ? i0 + u * stride : i0];
#pragma unroll
        for(int u = 0; u < UNR; u++)
        {
            if(k[u] == VT_EMPTY)
            {
                lempty = 1;
                continue;
            }
            const int r = vt_insert(lset, VT_LDS_SLOTS, k[u]);
            if(r < 0 || (r > 0 && atomicAdd(&lcount, 1) + 1 > SELL_VTAB_MAX))
                lstop = 1;
        }
    }
    __syncthreads();
    if(lstop)
    {
        if(threadIdx.x == 0)
            atomicOr(state + 1, 1u);
        return;
    }
    if(threadIdx.x == 0 && lempty)
        atomicOr(state + 2, 1u);
    for(int k = threadIdx.x; k < VT_LDS_SLOTS; k += blockDim.x)
    {
        const unsigned long long key = lset[k];
        if(key == VT_EMPTY || __hip_atomic_load(state + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            continue;
        const int r = vt_insert(set, VT_SLOTS, key);
        if(r < 0 || (r > 0 && atomicAdd(state, 1u) + 1u > (unsigned)SELL_VTAB_MAX))
            atomicOr(state + 1, 1u);
    }
}

} // namespace

aoclsparse_status sell_value_table(hipStream_t s, size_t vsize, long long n, const void *val, void *table, int *ntab)
{
    *ntab = 0;
    if(vsize != 4 && vsize != 8)
        return aoclsparse_status_success;
    // (SELL_VTAB_MAX entries whatever *ntab is, the unused ones 0: the short-row kernel copies the whole table to LDS)
    std::memset(table, 0, vsize * (size_t)SELL_VTAB_MAX);
    if(n <= 0)
        return aoclsparse_status_success;
    DeviceBuffer      set;
    aoclsparse_status st = set.alloc(sizeof(unsigned long long) * VT_SLOTS + 4 * sizeof(unsigned));
    if(st != aoclsparse_status_success)
        return st;
    unsigned long long *d_set   = set.as<unsigned long long>();
    unsigned           *d_state = reinterpret_cast<unsigned *>(d_set + VT_SLOTS);
    MI355_HIP_TRY(hipMemsetAsync(d_set, 0xff, sizeof(unsigned long long) * VT_SLOTS, s)); // VT_EMPTY everywhere
    MI355_HIP_TRY(hipMemsetAsync(d_state, 0, 4 * sizeof(unsigned), s));
    // a few workgroups per CU, each walking the values with a grid stride (a workgroup that has seen > 256 patterns stops all)
    const long long blocks = std::min<long long>(2048, std::max<long long>(1, (n + 1023) / 1024));
    if(vsize == 8)
        hipLaunchKernelGGL(sell_vtab_count_kernel<unsigned long long>, dim3((unsigned)blocks), dim3(256), 0, s, n,
                           static_cast<const unsigned long long *>(val), d_set, d_state);
    else
        hipLaunchKernelGGL(sell_vtab_count_kernel<unsigned>, dim3((unsigned)blocks), dim3(256), 0, s, n,
                           static_cast<const unsigned *>(val), d_set, d_state);
    MI355_HIP_TRY(hipGetLastError());
    unsigned state[4];
    MI355_HIP_TRY(hipMemcpyAsync(state, d_state, sizeof(state), hipMemcpyDeviceToHost, s));
    MI355_HIP_TRY(hipStreamSynchronize(s));
    if(state[1] || state[0] + state[2] > (unsigned)SELL_VTAB_MAX)
        return aoclsparse_status_success;
    std::vector<unsigned long long> h((size_t)VT_SLOTS);
    MI355_HIP_TRY(hipMemcpyAsync(h.data(), d_set, sizeof(unsigned long long) * VT_SLOTS, hipMemcpyDeviceToHost, s));
    MI355_HIP_TRY(hipStreamSynchronize(s));
    int k = 0;
    unsigned long long bits[SELL_VTAB_MAX];
    for(unsigned long long v : h)
        if(v != VT_EMPTY && k < SELL_VTAB_MAX)
            bits[k++] = v;
    if(state[2] && k < SELL_VTAB_MAX)
        bits[k++] = VT_EMPTY;
    std::sort(bits, bits + k); // (ascending bit pattern: the plan does not depend on the order the device found them in)
    for(int e = 0; e < k; e++) // (the low vsize bytes of each word: the pattern of a float or a double)
    {
        const unsigned lo = (unsigned)bits[e];
        if(vsize == 4)
            std::memcpy(static_cast<unsigned char *>(table) + 4 * e, &lo, 4);
        else
            std::memcpy(static_cast<unsigned char *>(table) + 8 * e, &bits[e], 8);
    }
    *ntab = k;
    return aoclsparse_status_success;
}

namespace
{

// ---- shared column lists (SELL-64 with one column list per run of rows that repeat it) --------------------------------
// Two kinds of repetition, found the same way: the rows of a mesh node (several dofs) carry the SAME column list, and the
// rows of a stencil carry the list of the row before SHIFTED BY ONE (row i of a 5-point Laplacian: i-g, i-1, i, i+1, i+g).
// A slice stores its columns once per "leader" (lane 0, and every lane whose list is neither the previous lane's nor the
// previous lane's plus one): cell (p, leader k) of slice s at cptr[s] + nl_s p + k (PACK 4: cptr[s] + 4 nl_s (p / 4) + 4 k
// + p % 4).  follow[i] (16 bits per row) = leader index inside the slice | shift << 8, where shift = how many of the rows
// between the leader and row i were "plus one" steps: a lane's column is its leader's + shift.  Values stay where they are.
// The column stream shrinks from 4 B per cell to 4 B / (rows per list): 12 -> 8.8 B per cell for 5-dof nodes, 12 -> ~8.1 B for
// the Laplacian (one list per 64 rows, broken at the grid edges).
// One wavefront per slice: each lane compares its row with its predecessor, indices and shifts by ballot + popcount.
__global__ __launch_bounds__(256) void sell_leaders_kernel(aoclsparse_int m, int base, const aoclsparse_int *__restrict__ row_ptr,
                                                           const aoclsparse_int *__restrict__ col, aoclsparse_int nslices,
                                                           unsigned short *__restrict__ follow, aoclsparse_int *__restrict__ nl)
{
    const int s    = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if(s >= nslices)
        return;
    const int i      = s * 64 + lane;
    bool      leader = false, plus1 = false;
    if(i < m)
    {
        leader = lane == 0;
        if(!leader)
        {
            const int b = row_ptr[i] - base, len = row_ptr[i + 1] - base - b, bp = row_ptr[i - 1] - base;
            bool      same = len == b - bp, shifted = same && len > 0; // (column VALUES: only differences are used)
            for(int k = 0; k < len && (same || shifted); k++)
            {
                const int dcol = col[b + k] - col[bp + k];
                same           = same && dcol == 0;
                shifted        = shifted && dcol == 1;
            }
            leader = !same && !shifted;
            plus1  = shifted;
        }
    }
    const unsigned long long upto = (2ull << lane) - 1ull; // lanes 0 .. lane
    const unsigned long long bal  = __builtin_amdgcn_ballot_w64(leader);
    const unsigned long long p1   = __builtin_amdgcn_ballot_w64(plus1);
    if(i < m)
    {
        const unsigned long long mine = bal & upto; // never 0: lane 0 is a leader
        const int                ll   = 63 - __builtin_clzll(mine); // my leader's lane
        const unsigned long long span = upto & ~((2ull << ll) - 1ull); // lanes ll + 1 .. lane
        follow[i] = (unsigned short)((__builtin_popcountll(mine) - 1) | (__builtin_popcountll(p1 & span) << 8));
    }
    // a FULL slice with one leader whose followers are all "plus one" (the interior of a stencil) or all "same" needs no
    // follow[] at run time: mode 1 -> shift = lane, mode 2 -> shift = 0 (bits 8.. of nl[s]; the host moves them into cptr)
    if(lane == 0)
    {
        const bool full = s * 64 + 63 < m;
        const int  mode = (full && bal == 1ull) ? (p1 == ~1ull ? 1 : (p1 == 0ull ? 2 : 0)) : 0;
        nl[s]           = (aoclsparse_int)__builtin_popcountll(bal) | (mode << 8);
    }
}

} // namespace

aoclsparse_status launch_sell_leaders(hipStream_t s, aoclsparse_int m, int base, const aoclsparse_int *row_ptr, const aoclsparse_int *col,
                                      aoclsparse_int nslices, unsigned short *lead, aoclsparse_int *nl)
{
    if(nslices <= 0)
        return aoclsparse_status_success;
    hipLaunchKernelGGL(sell_leaders_kernel, dim3((nslices + 3) / 4), dim3(256), 0, s, m, base, row_ptr, col, nslices, lead, nl);
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

namespace
{

// cell (p, k) of a slice whose rows of cells are n wide (64 value cells; the column lists of a slice with shared lists: its n
// leaders): PACK 1 -> n p + k; PACK 4 -> four consecutive cells of a row are adjacent: 4 n (p / 4) + 4 k + p % 4 (slice width is a
// multiple of 4 there)
template <int PACK>
__device__ __forceinline__ long long cell_of(int p, int k, int n = 64)
{
    return PACK == 1 ? (long long)p * n + k : (long long)(p >> 2) * 4 * n + k * 4 + (p & 3);
}

// COLS: what the pass does with the structure.  SELL_COLS_OWN / SELL_COLS_SHARED (a first build): rowlen and the columns are written
// with the cells, in one pass over the rows -- every lane's own list, or the slice's shared lists (cptr, follow: see above), written by
// the first row of every list.  SELL_COLS_KEPT (the values stage on a kept structure: sell_plan.cpp, sell_values_kept): the cells from
// row_ptr and val alone -- cell p of row i is entry row_ptr[i] + p of the CSR, so no value map is needed; col and rowlen are the
// structure's and are not touched, and col_idx is read only by lane 0 of a mode 1 / 2 slice, for the uniform list.  Whether the
// column lists are shared or own makes no difference to a value cell.
// pidx (pbits > 0): the table indices of a row go into ONE word of pbytes bytes at row * pbytes instead of sidx, cell p at bit
// p * pbits; unused fields, padding cells and the rows behind m hold 0
// ucol (not OWN): the list of a mode 1 / 2 slice is ALSO written to ucol[SELL_SHORT_WMAX s ..] (preset to -1 by the host; cptr
// carries the modes and is there whenever ucol is)
enum SellCols
{
    SELL_COLS_KEPT,
    SELL_COLS_OWN,
    SELL_COLS_SHARED
};

template <typename T, int PACK, SellCols COLS>
__global__ __launch_bounds__(256) void sell_fill_kernel(aoclsparse_int m, int base,
                                                        const aoclsparse_int *__restrict__ row_ptr,
                                                        const aoclsparse_int *__restrict__ col,
                                                        const T *__restrict__ val, aoclsparse_int nslices,
                                                        const long long *__restrict__ slice_ptr,
                                                        const long long *__restrict__ cptr,
                                                        const unsigned short *__restrict__ follow, T *__restrict__ sval,
                                                        aoclsparse_int *__restrict__ scol,
                                                        aoclsparse_int *__restrict__ rowlen, unsigned char *__restrict__ sidx,
                                                        const T *__restrict__ vtab, int ntab, unsigned char *__restrict__ pidx,
                                                        int pbits, int pbytes, aoclsparse_int *__restrict__ ucol)
{
    constexpr bool SHARED = COLS == SELL_COLS_SHARED, KEPT = COLS == SELL_COLS_KEPT;
    const int      s    = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int      lane = threadIdx.x & 63;
    if(s >= nslices)
        return;
    const int       i  = s * 64 + lane;
    const long long o0 = slice_ptr[s];
    const int       w  = (int)((slice_ptr[s + 1] - o0) >> 6);
    long long       c0 = 0;
    int             nl = 0;
    bool            uni = false; // this lane writes the slice's uniform list
    if constexpr(SHARED)
    {
        const int mode = (int)(cptr[s] >> SELL_CPTR_MODE_SHIFT);
        c0  = cptr[s] & SELL_CPTR_MASK;
        nl  = w > 0 ? (int)(((cptr[s + 1] & SELL_CPTR_MASK) - c0) / w) : 0;
        uni = ucol && lane == 0 && w <= SELL_SHORT_WMAX && (mode == SELL_DESC_MODE_LANE_SHIFT || mode == SELL_DESC_MODE_ONE);
    }
    if constexpr(KEPT) // (a mode 1 / 2 slice is full: its lane 0 is a row)
        if(ucol && cptr)
        {
            const int mode = (int)(cptr[s] >> SELL_CPTR_MODE_SHIFT);
            uni = lane == 0 && i < m && w <= SELL_SHORT_WMAX && (mode == SELL_DESC_MODE_LANE_SHIFT || mode == SELL_DESC_MODE_ONE);
        }
    int  b = 0, len = 0, k = 0;
    bool leader = COLS == SELL_COLS_OWN; // (own lists: every lane writes its columns, the padding rows behind m too)
    if(i < m)
    {
        b   = row_ptr[i] - base;
        len = row_ptr[i + 1] - base - b;
        if constexpr(!KEPT)
            rowlen[i] = len;
        if constexpr(SHARED)
        {
            k      = follow[i] & 0xff;
            leader = lane == 0 || (follow[i - 1] & 0xff) != k;
        }
    }
    unsigned word = 0;
    for(int p = 0; p < w; p++)
    {
        const long long o  = o0 + cell_of<PACK>(p, lane);
        const bool      in = p < len;
        bool            packed = false;
        if constexpr(std::is_floating_point_v<T>)
            packed = pidx != nullptr;
        if(packed)
        {
            if constexpr(std::is_floating_point_v<T>)
                word |= in ? (unsigned)vtab_index(val[b + p], vtab, ntab) << (p * pbits) : 0u;
        }
        else
            fill_cell(o, in, val + b + p, sval, sidx, vtab, ntab);
        if constexpr(!KEPT)
            if(leader)
                scol[SHARED ? c0 + cell_of<PACK>(p, k, nl) : o] = in ? col[b + p] - base : -1;
        if(uni)
            ucol[(long long)s * SELL_SHORT_WMAX + p] = in ? col[b + p] - base : -1;
    }
    if(pidx) // (every lane of the slice: the rows behind m hold 0)
    {
        const long long row = (long long)s * 64 + lane;
        if(pbytes == 1)
            pidx[row] = (unsigned char)word;
        else if(pbytes == 2)
            reinterpret_cast<unsigned short *>(pidx)[row] = (unsigned short)word;
        else
            reinterpret_cast<unsigned *>(pidx)[row] = word;
    }
}

// scol == nullptr: the structure is kept (neither scol nor rowlen is written)
template <typename T>
void sell_fill_as(hipStream_t s, const DeviceCsr &d, const SellView &v, void *cells, aoclsparse_int *scol, aoclsparse_int *rowlen,
                  aoclsparse_int *ucol)
{
    T             *sval = v.ntab ? nullptr : static_cast<T *>(cells);
    unsigned char *sidx = v.ntab && !v.pbits ? static_cast<unsigned char *>(cells) : nullptr;
    unsigned char *pidx = v.ntab && v.pbits ? static_cast<unsigned char *>(cells) : nullptr;
    auto           go   = [&](auto pack, auto cols) {
        hipLaunchKernelGGL((sell_fill_kernel<T, decltype(pack)::value, decltype(cols)::value>), dim3((v.nslices + 3) / 4), dim3(256), 0,
                           s, v.m, d.base, d.ptr.as<aoclsparse_int>(), d.ind.as<aoclsparse_int>(), d.val.as<T>(), v.nslices,
                           v.slice_ptr, v.cptr, v.lead, sval, scol, rowlen, sidx, static_cast<const T *>(v.vtab), v.ntab, pidx, v.pbits,
                           v.pbytes, ucol);
    };
    auto with = [&](auto cols) {
        if(v.pack == 4)
            go(std::integral_constant<int, 4>{}, cols);
        else
            go(std::integral_constant<int, 1>{}, cols);
    };
    if(!scol)
        with(std::integral_constant<SellCols, SELL_COLS_KEPT>{});
    else if(v.cptr)
        with(std::integral_constant<SellCols, SELL_COLS_SHARED>{});
    else
        with(std::integral_constant<SellCols, SELL_COLS_OWN>{});
}

// the new set of records and uniform lists against the current one, as 32-bit words: any difference raises the verdict word.
// Every thread that sees one stores the same 1 (a plain vector store; the host zeroed the word before the launch).
__global__ __launch_bounds__(256) void sell_compare_kernel(long long nrec, const uint32_t *__restrict__ rec_a,
                                                           const uint32_t *__restrict__ rec_b, long long nlist,
                                                           const aoclsparse_int *__restrict__ list_a,
                                                           const aoclsparse_int *__restrict__ list_b, unsigned *__restrict__ verdict)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    bool            diff   = false;
    for(long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < nrec + nlist; k += stride)
        diff = diff || (k < nrec ? rec_a[k] != rec_b[k] : list_a[k - nrec] != list_b[k - nrec]);
    if(diff)
        *verdict = 1u;
}

// ---- what a slice record says beyond offsets, width and mode (SELL_DESC_UWORD / SELL_DESC_EXCEPT, internal.hpp) ---------------
// Behind the fill pass, on a copy with uniform lists and one-byte packed words; one wavefront per FULL slice.
// Mode 1 / 2 (one list): the 64 words of the fill pass are compared; if they are one word the record carries it.
// Mode 0 with a width: "one list shifted by lane, a few lanes omit a cell" (the first and last slice of a grid line):
//   - canonical row = the lowest lane whose length is the slice width, B = its columns minus its lane;
//   - every B[q] >= 0 and B[q] + 63 < n (every gather at B[q] + lane stays inside x; -1 stays ucol's "unused");
//   - every row's columns are an in-order subsequence of B + lane (greedy match: the earliest match is as good as any);
//   - at most two lanes are shorter than the width;
//   - the rows' table indices, moved to the canonical positions of their cells, agree with the canonical row's word.
// Then the record gets both flags, the word, the two (lane, mask of present canonical cells) pairs, and ucol gets B.  A slice
// that fails any condition keeps its record and its ucol entries (-1) as the fill pass left them.
__global__ __launch_bounds__(256) void sell_records_kernel(aoclsparse_int m, aoclsparse_int n, int base,
                                                           const aoclsparse_int *__restrict__ row_ptr,
                                                           const aoclsparse_int *__restrict__ col, aoclsparse_int nslices,
                                                           SellSliceDesc *__restrict__ desc, const unsigned char *__restrict__ pidx,
                                                           int pbits, aoclsparse_int *__restrict__ ucol, unsigned *__restrict__ counts)
{
    const int s    = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if(s >= nslices || (long long)s * 64 + 63 >= m) // (wave-uniform: full slices only)
        return;
    const int      i    = s * 64 + lane;
    const uint32_t wsm  = desc[s].wsm;
    const int      w    = (int)(wsm & 0xffu), mode = (int)(wsm >> 16) & 0xff;
    const unsigned own  = pidx[i]; // the row's word, fields at the row's own cell positions
    if(w > SELL_SHORT_WMAX)
        return;
    if(mode == SELL_DESC_MODE_LANE_SHIFT || mode == SELL_DESC_MODE_ONE)
    {
        const unsigned w0 = (unsigned)__shfl((int)own, 0);
        if(__builtin_amdgcn_ballot_w64(own != w0) != 0ull || lane != 0)
            return;
        desc[s].cell_lo = w0 | SELL_DESC_NO_LANE << 8 | SELL_DESC_NO_LANE << 24;
        desc[s].hi &= 0xffff0000u;
        desc[s].wsm = wsm | SELL_DESC_UWORD;
        atomicAdd(counts, 1u);
        return;
    }
    if(mode != SELL_DESC_MODE_FOLLOW || w < 1)
        return;
    const int                b = row_ptr[i] - base, len = row_ptr[i + 1] - base - b;
    const unsigned long long shortb = __builtin_amdgcn_ballot_w64(len < w);
    if(__builtin_popcountll(shortb) > 2) // (never all 64: w is the longest row's length)
        return;
    const int c  = __builtin_ctzll(~shortb); // canonical lane
    const int bc = __shfl(b, c);
    int       B[SELL_SHORT_WMAX];
    bool      ok = true;
#pragma unroll
    for(int q = 0; q < SELL_SHORT_WMAX; q++)
    {
        B[q] = q < w ? col[bc + q] - base - c : 0;
        ok   = ok && B[q] >= 0 && (long long)B[q] + 63 < (long long)n;
    }
    // this row against B + lane: mask = the canonical cells it has, cw = its index fields moved to their positions
    const unsigned field = (1u << pbits) - 1u;
    unsigned       mask = 0, cw = 0, fm = 0;
    int            p = 0;
#pragma unroll
    for(int q = 0; q < SELL_SHORT_WMAX; q++)
    {
        const bool hit = q < w && p < len && col[b + min(p, max(len - 1, 0))] - base == B[q] + lane;
        if(hit)
        {
            mask |= 1u << q, fm |= field << (q * pbits);
            cw |= ((own >> (p * pbits)) & field) << (q * pbits);
            p++;
        }
    }
    ok               = ok && p == len;
    const unsigned W = (unsigned)__shfl((int)cw, c);
    ok               = ok && ((cw ^ W) & fm) == 0u;
    if(__builtin_amdgcn_ballot_w64(!ok) != 0ull)
        return;
    unsigned la = SELL_DESC_NO_LANE, lb = SELL_DESC_NO_LANE, ma = 0, mb = 0;
    if(shortb)
    {
        la = (unsigned)__builtin_ctzll(shortb);
        ma = (unsigned)__shfl((int)mask, (int)la);
        const unsigned long long rest = shortb & (shortb - 1ull);
        if(rest)
        {
            lb = (unsigned)__builtin_ctzll(rest);
            mb = (unsigned)__shfl((int)mask, (int)lb);
        }
    }
    if(lane != 0)
        return;
#pragma unroll
    for(int q = 0; q < SELL_SHORT_WMAX; q++)
        if(q < w)
            ucol[(long long)s * SELL_SHORT_WMAX + q] = B[q];
    desc[s].cell_lo = (W & 0xffu) | la << 8 | ma << 16 | lb << 24;
    desc[s].hi      = (desc[s].hi & 0xffff0000u) | mb;
    desc[s].wsm     = wsm | SELL_DESC_UWORD | SELL_DESC_EXCEPT;
    atomicAdd(counts, 1u);
    atomicAdd(counts + 1, 1u);
}

} // namespace

aoclsparse_status launch_sell_records(hipStream_t s, const DeviceCsr &d, const SellView &v, SellSliceDesc *desc, aoclsparse_int *ucol,
                                      unsigned *counts)
{
    MI355_HIP_TRY(hipMemsetAsync(counts, 0, 2 * sizeof(unsigned), s));
    if(v.nslices <= 0 || !desc || !ucol || !v.cells || v.pbits <= 0 || v.pbytes != 1)
        return aoclsparse_status_success;
    hipLaunchKernelGGL(sell_records_kernel, dim3((v.nslices + 3) / 4), dim3(256), 0, s, v.m, d.n, d.base, d.ptr.as<aoclsparse_int>(),
                       d.ind.as<aoclsparse_int>(), v.nslices, desc, static_cast<const unsigned char *>(v.cells), v.pbits, ucol, counts);
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

aoclsparse_status launch_sell_compare(hipStream_t s, aoclsparse_int nslices, const SellSliceDesc *desc_a, const SellSliceDesc *desc_b,
                                      const aoclsparse_int *ucol_a, const aoclsparse_int *ucol_b, unsigned *verdict)
{
    MI355_HIP_TRY(hipMemsetAsync(verdict, 0, sizeof(unsigned), s));
    if(nslices <= 0)
        return aoclsparse_status_success;
    if(!desc_a || !desc_b || !ucol_a || !ucol_b)
        return aoclsparse_status_internal_error;
    const long long nrec = (long long)nslices * (long long)(sizeof(SellSliceDesc) / sizeof(uint32_t)), nlist = (long long)nslices * SELL_SHORT_WMAX;
    const long long blocks = std::min<long long>(2048, (nrec + nlist + 255) / 256);
    hipLaunchKernelGGL(sell_compare_kernel, dim3((unsigned)blocks), dim3(256), 0, s, nrec, reinterpret_cast<const uint32_t *>(desc_a),
                       reinterpret_cast<const uint32_t *>(desc_b), nlist, ucol_a, ucol_b, verdict);
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

aoclsparse_status launch_sell_fill(hipStream_t s, const DeviceCsr &d, size_t vsize, const SellView &v, void *cells, aoclsparse_int *col,
                                   aoclsparse_int *rowlen, aoclsparse_int *ucol)
{
    if(v.nslices <= 0)
        return aoclsparse_status_success;
    if(!cells || !v.slice_ptr || !d.ptr.ptr || !d.val.ptr || ((ucol || col) && !d.ind.ptr) || (col && !rowlen))
        return aoclsparse_status_internal_error;
    // (the kernel only moves values: cfloat cells are filled as 8-byte doubles, cdouble cells need their own instantiation)
    if(vsize == sizeof(cdouble))
        sell_fill_as<cdouble>(s, d, v, cells, col, rowlen, ucol);
    else if(vsize == sizeof(float))
        sell_fill_as<float>(s, d, v, cells, col, rowlen, ucol);
    else
        sell_fill_as<double>(s, d, v, cells, col, rowlen, ucol);
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

} // namespace mi355
