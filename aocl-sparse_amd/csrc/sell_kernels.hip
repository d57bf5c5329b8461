// sell_kernels.hip -- SpMV on SELL-64, the layout aoclsparse_optimize builds for an mv hint on MI355X.
//
// The reference's optimize step re-stores a hinted matrix in the format its CPU kernels like best
// (br4 / ELLT-HYB / blocked CSR, analysis.cpp:146-382).  The GPU analogue is sliced ELL with one slice
// per 64-wide wavefront: slice s holds rows [64 s, 64 s + 64) column-major, cell (p, lane) at
// slice_ptr[s] + 64 p + lane, padded to the slice's longest row (column -1, value 0); matrices with >= 16
// non-zeros per row keep four consecutive cells of a row adjacent instead (PACK 4: cell at
// slice_ptr[s] + 256 (p/4) + 4 lane + p%4, width rounded up to a multiple of 4), so that a wavefront's load is
// one contiguous 2 KB piece -- the in-flight slices of a long-row matrix are otherwise 512-byte accesses
// strided by the slice size, which costs HBM page locality.  Lane i of a wave owns row i:
//   * every val / col access is one coalesced line per wavefront instruction, no row_ptr, no LDS;
//   * a lane walks its row front to back, so the reference's summation orders are reproduced exactly:
//     order 0 is the scalar FMA chain (csrmv_kr.hpp:448-513); orders 1 / 2 keep 4 / 8 partial sums per
//     lane for the full groups, reduce them as the AVX2 / AVX-512 kernels do, then run the scalar tail
//     (csrmv_kr.hpp:949-1040, csrmv_avx512.cpp:36-134, csrmv_kr.hpp:734-831 for float).
// Bytes per launch: cells*(8+4) + 8 m (y) (+ 8 m if beta != 0) (+ 4 m row lengths for orders 1 / 2) + x
// gathers; cells <= 1.15 nnz or the handle stays on the CSR-Adaptive kernel (matrix.cpp: build_sell).
#include "internal.hpp"

#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include <hip/hip_runtime.h>

namespace mi355
{

namespace
{

__device__ __forceinline__ double s_fma(double a, double b, double c)
{
    return fma(a, b, c);
}
__device__ __forceinline__ float s_fma(float a, float b, float c)
{
    return fmaf(a, b, c);
}

template <typename T>
__device__ __forceinline__ T s_finish(T r, T alpha, T beta, const T *yi)
{
    if(alpha != T(1))
        r = alpha * r;
    if(beta != T(0))
        r = s_fma(beta, *yi, r);
    return r;
}

// complex handles (aoclsparse_{c,z}mv through the same SELL-64 copy, round 4): the component-wise multiply-add of
// complex_kernels.hip (c_mac), alpha == 1 and beta == 0 skipped exactly as there; CONJ conjugates the stored value at load
// (op = H on a general matrix, op = T on a hermitian one: complex_api.cpp)
template <typename R>
__device__ __forceinline__ cplx<R> s_fma(cplx<R> a, cplx<R> b, cplx<R> c)
{
    c.re = s_fma(a.re, b.re, c.re);
    c.re = s_fma(-a.im, b.im, c.re);
    c.im = s_fma(a.re, b.im, c.im);
    c.im = s_fma(a.im, b.re, c.im);
    return c;
}
template <typename R>
__device__ __forceinline__ cplx<R> s_finish(cplx<R> r, cplx<R> alpha, cplx<R> beta, const cplx<R> *yi)
{
    if(!(alpha.re == R(1) && alpha.im == R(0)))
        r = s_fma(alpha, r, cplx<R>(R(0), R(0)));
    if(!(beta.re == R(0) && beta.im == R(0))) // beta == 0 never reads y
        r = s_fma(beta, *yi, r);
    return r;
}
template <bool CONJ, typename T>
__device__ __forceinline__ T s_cj(T v)
{
    return v;
}
template <bool CONJ, typename R>
__device__ __forceinline__ cplx<R> s_cj(cplx<R> v)
{
    if constexpr(CONJ)
        v.im = -v.im;
    return v;
}

// pins v to a register HERE: the loads and the chain behind it are not moved into a branch that follows (the compiler sinks
// what only a guarded store uses into the guard, and then the loads of one slice wait for the store of the slice before)
__device__ __forceinline__ void s_pin(double &v)
{
    asm volatile("" : "+v"(v));
}
__device__ __forceinline__ void s_pin(float &v)
{
    asm volatile("" : "+v"(v));
}
template <typename R>
__device__ __forceinline__ void s_pin(cplx<R> &v)
{
    s_pin(v.re), s_pin(v.im);
}

// the same for a kernel argument: it is read with the first batch of scalar loads, not in front of its first use (one more
// scalar-cache round trip at the tail of a wave's life otherwise)
template <typename A>
__device__ __forceinline__ void s_pin_arg(A a)
{
    asm volatile("" : : "s"(a));
}
template <typename R>
__device__ __forceinline__ void s_pin_arg(cplx<R> a)
{
    s_pin_arg(a.re), s_pin_arg(a.im);
}

template <typename T>
__device__ __forceinline__ void s_store(T *p, T v, bool nt)
{
    if(nt)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}
template <typename R>
__device__ __forceinline__ void s_store(cplx<R> *p, cplx<R> v, bool nt)
{
    if(nt)
    {
        __builtin_nontemporal_store(v.re, &p->re);
        __builtin_nontemporal_store(v.im, &p->im);
    }
    else
        *p = v;
}

// horizontal sums of the reference's vector kernels, on a lane's private partial sums
template <typename T, int G>
__device__ __forceinline__ T lanes_sum(const T (&l)[G])
{
    if constexpr(G == 4)
        return (l[0] + l[1]) + (l[2] + l[3]); // hadd, then lo + hi (csrmv_kr.hpp:1000-1016)
    else if constexpr(sizeof(T) == 8)
        return ((l[0] + l[4]) + (l[1] + l[5])) + ((l[2] + l[6]) + (l[3] + l[7])); // csrmv_avx512.cpp:86-100
    else
        return ((l[0] + l[4]) + (l[2] + l[6])) + ((l[1] + l[5]) + (l[3] + l[7])); // csrmv_kr.hpp:788-806
}

// cell (p, lane) of a slice that starts at o0: PACK 1 -> o0 + 64 p + lane; PACK 4 -> four consecutive cells of a
// row are adjacent: o0 + 256 (p / 4) + 4 lane + p % 4 (slice width is a multiple of 4 there)
template <int PACK>
__device__ __forceinline__ long long cell_of(int p, int lane)
{
    return PACK == 1 ? (long long)p * 64 + lane : (long long)(p >> 2) * 256 + lane * 4 + (p & 3);
}

// ---- value tables (SELL-64 with one byte per cell: an index into <= 256 distinct value bit patterns) ---------------------
// A matrix whose values take at most SELL_VTAB_MAX distinct bit patterns (a constant-coefficient stencil: two) stores one byte
// per cell and a table sorted by ascending bit pattern; the kernels read table[index], i.e. the very bits of the value, so every
// summation order gives the same results as with the values stored in the cells (CSR-VI, Kourtis, Goumas and Koziris, CF 2008).
// Bit patterns, not values: -0.0 and +0.0 are two entries, NaN payloads are kept.
template <typename T>
using vbits_t = std::conditional_t<sizeof(T) == 8, unsigned long long, unsigned>;

// the value cells as the kernels read them: values, or (IDX) table indices
template <typename T, bool IDX>
struct SellCell
{
    using src = T; // stored
    using raw = T; // loaded
};
template <typename T>
struct SellCell<T, true>
{
    using src = unsigned char;
    using raw = int;
};
template <bool IDX, typename T, typename R>
__device__ __forceinline__ T cell_value(R raw, const T *__restrict__ vtab)
{
    if constexpr(IDX)
        return vtab[raw];
    else
        return raw;
}

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

template <typename T, int PACK>
__global__ __launch_bounds__(256) void sell_fill_kernel(aoclsparse_int m, int base,
                                                        const aoclsparse_int *__restrict__ row_ptr,
                                                        const aoclsparse_int *__restrict__ col,
                                                        const T *__restrict__ val, aoclsparse_int nslices,
                                                        const long long *__restrict__ slice_ptr,
                                                        T *__restrict__ sval, aoclsparse_int *__restrict__ scol,
                                                        aoclsparse_int *__restrict__ rowlen, unsigned char *__restrict__ sidx,
                                                        const T *__restrict__ vtab, int ntab)
{
    const int s    = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if(s >= nslices)
        return;
    const int       i  = s * 64 + lane;
    const long long o0 = slice_ptr[s];
    const int       w  = (int)((slice_ptr[s + 1] - o0) >> 6);
    int             b = 0, len = 0;
    if(i < m)
    {
        b   = row_ptr[i] - base;
        len = row_ptr[i + 1] - base - b;
        rowlen[i] = len;
    }
    for(int p = 0; p < w; p++)
    {
        const long long o  = o0 + cell_of<PACK>(p, lane);
        const bool      in = p < len;
        fill_cell(o, in, val + b + p, sval, sidx, vtab, ntab);
        scol[o]            = in ? col[b + p] - base : -1;
    }
}

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
constexpr int       SELL_CPTR_MODE_SHIFT = 56;
constexpr long long SELL_CPTR_MASK       = (1LL << SELL_CPTR_MODE_SHIFT) - 1;

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

template <typename T, int PACK>
__global__ __launch_bounds__(256) void sell_fill_shared_kernel(aoclsparse_int m, int base,
                                                               const aoclsparse_int *__restrict__ row_ptr,
                                                               const aoclsparse_int *__restrict__ col,
                                                               const T *__restrict__ val, aoclsparse_int nslices,
                                                               const long long *__restrict__ slice_ptr,
                                                               const long long *__restrict__ cptr,
                                                               const unsigned short *__restrict__ follow, T *__restrict__ sval,
                                                               aoclsparse_int *__restrict__ scol,
                                                               aoclsparse_int *__restrict__ rowlen, unsigned char *__restrict__ sidx,
                                                               const T *__restrict__ vtab, int ntab)
{
    const int s    = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if(s >= nslices)
        return;
    const int       i  = s * 64 + lane;
    const long long o0 = slice_ptr[s], c0 = cptr[s] & SELL_CPTR_MASK;
    const int       w  = (int)((slice_ptr[s + 1] - o0) >> 6);
    const int       nl = w > 0 ? (int)(((cptr[s + 1] & SELL_CPTR_MASK) - c0) / w) : 0;
    int             b = 0, len = 0, k = 0;
    bool            leader = false;
    if(i < m)
    {
        b   = row_ptr[i] - base;
        len = row_ptr[i + 1] - base - b;
        rowlen[i] = len;
        k         = follow[i] & 0xff;
        leader    = lane == 0 || (follow[i - 1] & 0xff) != k;
    }
    for(int p = 0; p < w; p++)
    {
        const bool in = p < len;
        fill_cell(o0 + cell_of<PACK>(p, lane), in, val + b + p, sval, sidx, vtab, ntab);
        if(leader)
            scol[c0 + (PACK == 1 ? (long long)p * nl + k : (long long)(p >> 2) * 4 * nl + 4 * k + (p & 3))] = in ? col[b + p] - base : -1;
    }
}

// four adjacent cells of one lane as vector loads (PACK 4): 32 B of values (16 B for float), 16 B of columns
__device__ __forceinline__ void load4(const double *p, double (&o)[4])
{
    const double2 a = *reinterpret_cast<const double2 *>(p), b = *reinterpret_cast<const double2 *>(p + 2);
    o[0] = a.x, o[1] = a.y, o[2] = b.x, o[3] = b.y;
}
__device__ __forceinline__ void load4(const float *p, float (&o)[4])
{
    const float4 a = *reinterpret_cast<const float4 *>(p);
    o[0] = a.x, o[1] = a.y, o[2] = a.z, o[3] = a.w;
}
__device__ __forceinline__ void load4(const aoclsparse_int *p, int (&o)[4])
{
    const int4 a = *reinterpret_cast<const int4 *>(p);
    o[0] = a.x, o[1] = a.y, o[2] = a.z, o[3] = a.w;
}
// (table indices: four bytes of one lane = one dword, 256 B per wavefront)
__device__ __forceinline__ void load4(const unsigned char *p, int (&o)[4])
{
    const unsigned a = *reinterpret_cast<const unsigned *>(p);
    o[0] = (int)(a & 0xffu), o[1] = (int)((a >> 8) & 0xffu), o[2] = (int)((a >> 16) & 0xffu), o[3] = (int)(a >> 24);
}

// loads the G cells p0 .. p0+G-1 of this lane (wave-uniform guards against the slice width w): stored S, loaded as R
// (values, or table indices)
// cs = lanes per column row: 64, or the slice's number of leaders when the column lists are shared
template <typename S, typename R, int PACK, int G>
__device__ __forceinline__ void load_step(const S *v, const aoclsparse_int *c, int p0, int w, R (&vv)[G], int (&cc)[G],
                                          int cs = 64)
{
    if constexpr(PACK == 1)
    {
#pragma unroll
        for(int q = 0; q < G; q++)
        {
            const bool ok = p0 + q < w;
            vv[q]         = ok ? (R)v[(p0 + q) * 64] : R(0);
            cc[q]         = ok ? c[(p0 + q) * cs] : -1;
        }
    }
    else
    {
#pragma unroll
        for(int k = 0; k < G / 4; k++)
        {
            R   tv[4] = {R(0), R(0), R(0), R(0)};
            int tc[4] = {-1, -1, -1, -1};
            if(p0 + 4 * k < w) // w is a multiple of 4: the pack is whole or absent
            {
                const long long o = (long long)((p0 >> 2) + k) * 256;
                load4(v + o, tv);
                load4(c + (long long)((p0 >> 2) + k) * (4 * cs), tc);
            }
#pragma unroll
            for(int q = 0; q < 4; q++)
                vv[4 * k + q] = tv[q], cc[4 * k + q] = tc[q];
        }
    }
}

// WAVES slices per workgroup (1 for small matrices so that every slice gets its own CU)
// IDX: sval holds one byte per cell, an index into vtab (the value table); otherwise the values and vtab is unused
template <typename T, int ORDER, int WAVES, int PACK, bool SHARED = false, bool CONJ = false, bool IDX = false>
__global__ __launch_bounds__(64 * WAVES) void sell_mv_kernel(aoclsparse_int m, aoclsparse_int nslices,
                                                             const long long *__restrict__ slice_ptr,
                                                             const typename SellCell<T, IDX>::src *__restrict__ sval,
                                                             const aoclsparse_int *__restrict__ scol,
                                                             const aoclsparse_int *__restrict__ rowlen, T alpha,
                                                             const T *__restrict__ x, T beta, T *__restrict__ y,
                                                             bool nt, const long long *__restrict__ cptr = nullptr,
                                                             const unsigned short *__restrict__ follow = nullptr, int rev = 0,
                                                             const T *__restrict__ vtab = nullptr)
{
    using S = typename SellCell<T, IDX>::src;
    using R = typename SellCell<T, IDX>::raw;
    // rev: the slices in descending order.  Consecutive products of a handle ALTERNATE the direction (SellPlan::products): the
    // end of the matrix, which the previous product left in the 256 MB Infinity Cache, is where this one starts -- round 5,
    // profiles/r5/sell_placement.txt: shell-like 90-101 -> 81-87 us, the headline 0.178 -> 0.165 ms.  Same slices, same bits.
    const unsigned bx = rev ? gridDim.x - 1u - blockIdx.x : blockIdx.x;
    const int s    = __builtin_amdgcn_readfirstlane((int)(bx * WAVES + (threadIdx.x >> 6)));
    const int lane = threadIdx.x & 63;
    if(s >= nslices)
        return;
    const long long       o0 = slice_ptr[s];
    const int             w  = (int)((slice_ptr[s + 1] - o0) >> 6);
    const S              *v  = sval + o0 + lane * PACK;
    const int             i  = s * 64 + lane;
    const aoclsparse_int *c  = scol + o0 + lane * PACK;
    int                   cs = 64, dl = 0;
    if constexpr(SHARED)
    {
        // one column list per leader: cs leaders in this slice; this lane reads its leader's and adds its shift
        // (cptr's top bits carry the slice's mode: 1 = one leader, shift = lane; 2 = one leader, no shift; else follow[])
        const long long cw   = cptr[s];
        const long long c0   = cw & SELL_CPTR_MASK;
        const int       mode = (int)(cw >> SELL_CPTR_MODE_SHIFT);
        int             f    = 0;
        if(mode == 0)
            f = i < m ? follow[i] : 0;
        else if(mode == 1)
            f = lane << 8;
        cs = w > 0 ? (int)(((cptr[s + 1] & SELL_CPTR_MASK) - c0) / w) : 1;
        c  = scol + c0 + (f & 0xff) * PACK;
        dl = f >> 8;
    }
    T r = T(0);
    if constexpr(ORDER == 0 && PACK == 1)
    {
        // short rows (this is the layout of matrices with < 16 non-zeros per row): four independent line loads
        // per step, then the gathers, then the chain.  Measured on the 4096^2 Laplacian (w = 5): 0.218 ms;
        // 8-wide, guard-predicated or software-pipelined steps 0.223-0.26 ms (profiles/r1)
        // Widths up to 8 (round 3): ONE batch of exactly w line loads, then the w gathers, then the chain -- the wave's life is
        // three dependent round trips (slice words -> value / column lines -> x) whatever w is.  The 4-step loop below spent
        // five on a 5-wide slice (4 + 1 entries: lines, gathers, lines, gathers), and the kernel is bound by wave lifetime x
        // occupancy, not by bytes in flight (same box: 0.1845-0.186 -> 0.1786-0.1793 ms, profiles/r3/sell_width_switch.txt).
        int p = 0;
        auto batch = [&](auto wtag) {
            constexpr int W = decltype(wtag)::value;
            T             vv[W], xx[W];
            R             rr[W];
            int           cc[W];
#pragma unroll
            for(int q = 0; q < W; q++)
                rr[q] = v[q * 64], cc[q] = c[q * cs];
#pragma unroll
            for(int q = 0; q < W; q++)
                xx[q] = x[cc[q] >= 0 ? cc[q] + dl : 0], vv[q] = s_cj<CONJ>(cell_value<IDX>(rr[q], vtab));
#pragma unroll
            for(int q = 0; q < W; q++)
                r = cc[q] >= 0 ? s_fma(vv[q], xx[q], r) : r;
            p = W;
        };
        switch(w) // wave-uniform
        {
        case 5: batch(std::integral_constant<int, 5>{}); break;
        case 6: batch(std::integral_constant<int, 6>{}); break;
        case 7: batch(std::integral_constant<int, 7>{}); break;
        case 8: batch(std::integral_constant<int, 8>{}); break;
        default: break;
        }
        for(; p + 4 <= w; p += 4)
        {
            const R   r0 = v[(p + 0) * 64], r1 = v[(p + 1) * 64], r2 = v[(p + 2) * 64], r3 = v[(p + 3) * 64];
            const int c0 = c[(p + 0) * cs], c1 = c[(p + 1) * cs], c2 = c[(p + 2) * cs], c3 = c[(p + 3) * cs];
            // (a padding cell, -1, is never used, but its gather must stay inside x: index 0)
            const T   x0 = x[c0 >= 0 ? c0 + dl : 0], x1 = x[c1 >= 0 ? c1 + dl : 0], x2 = x[c2 >= 0 ? c2 + dl : 0],
                      x3 = x[c3 >= 0 ? c3 + dl : 0];
            const T   v0 = s_cj<CONJ>(cell_value<IDX>(r0, vtab)), v1 = s_cj<CONJ>(cell_value<IDX>(r1, vtab)),
                      v2 = s_cj<CONJ>(cell_value<IDX>(r2, vtab)), v3 = s_cj<CONJ>(cell_value<IDX>(r3, vtab));
            r = c0 >= 0 ? s_fma(v0, x0, r) : r;
            r = c1 >= 0 ? s_fma(v1, x1, r) : r;
            r = c2 >= 0 ? s_fma(v2, x2, r) : r;
            r = c3 >= 0 ? s_fma(v3, x3, r) : r;
        }
        for(; p < w; p++)
        {
            const R   r0 = v[p * 64];
            const int c0 = c[p * cs];
            const T   x0 = x[c0 >= 0 ? c0 + dl : 0], v0 = s_cj<CONJ>(cell_value<IDX>(r0, vtab));
            r = c0 >= 0 ? s_fma(v0, x0, r) : r;
        }
    }
    else
    {
        // Steps of G cells, software-pipelined: the lines of step k+1 are issued BEFORE the x gathers of step k,
        // so a step costs one memory round trip instead of two (vmcnt retires in order: the gathers wait for
        // the younger-issued lines too, but everything is in flight together).
        constexpr int G    = ORDER == 2 ? 8 : 4;
        const int     len  = (ORDER != 0 && i < m) ? rowlen[i] : 0;
        const int     full = len & ~(G - 1);
        T             l[G];
#pragma unroll
        for(int q = 0; q < G; q++)
            l[q] = T(0);
        bool reduced = false;
        R    vn[G];
        int  cn[G];
        load_step<S, R, PACK, G>(v, c, 0, w, vn, cn, cs);
        for(int p0 = 0; p0 < w; p0 += G)
        {
            T   vv[G], xx[G];
            R   vr[G];
            int cc[G];
#pragma unroll
            for(int q = 0; q < G; q++)
                vr[q] = vn[q], cc[q] = cn[q];
            if(p0 + G < w)
                load_step<S, R, PACK, G>(v, c, p0 + G, w, vn, cn, cs);
            // (IDX: the table reads go out with the x gathers, after the next step's lines)
#pragma unroll
            for(int q = 0; q < G; q++)
                xx[q] = x[cc[q] >= 0 ? cc[q] + dl : 0], vv[q] = cell_value<IDX>(vr[q], vtab); // (a padding cell, -1, is never used; its gather stays inside x)
            if constexpr(ORDER == 0)
            {
#pragma unroll
                for(int q = 0; q < G; q++)
                    r = cc[q] >= 0 ? s_fma(vv[q], xx[q], r) : r;
            }
            else if(p0 < full)
            {
#pragma unroll
                for(int q = 0; q < G; q++)
                    l[q] = s_fma(vv[q], xx[q], l[q]);
            }
            else if(p0 < len)
            {
                if(!reduced)
                    r = lanes_sum<T, G>(l), reduced = true;
#pragma unroll
                for(int q = 0; q < G; q++)
                    if(p0 + q < len)
                        r = s_fma(vv[q], xx[q], r);
            }
        }
        if(ORDER != 0 && !reduced)
            r = lanes_sum<T, G>(l);
    }
    if(i < m)
        s_store(y + i, s_finish(r, alpha, beta, y + i), nt);
}

// Short rows: matrices whose widest slice has WMAX <= 8 cells, scalar summation order, PACK 1, large launches.  A wavefront
// takes SPW consecutive slices and walks them TOGETHER, with no branch and no loop on the common path, so that its life is four
// dependent round trips whatever SPW is:
//   1. the kernel arguments (one scalar batch: the sweep direction is the pair g0 / gstep, not a branch);
//   2. the SPW slice records (SellSliceDesc, one wide scalar load: offsets, width, column stride, mode -- no slice_ptr / cptr
//      pairs, no division);
//   3. all SPW x WMAX value / column line loads (index clamped to the slice's own width, and to 0 for an EMPTY slice, which
//      reads the padding cells behind the arrays: a narrower slice re-reads its last line and skips the FMA);
//   4. all SPW x WMAX x gathers; then the chains and the stores.
// Only a group with a mode-0 slice (lead[] says which list a lane follows: 2 slices in 64 on a stencil) takes a fifth, the lead[]
// loads of the whole group, issued together in front of the line loads.
// TAB: 0 = the cells hold values; 2 = one-byte indices into a table of <= 2 values, held in scalar registers and selected;
// 256 = indices into a table of <= SELL_VTAB_MAX values, copied to LDS once per workgroup (its load goes out with the records,
// the barrier sits behind the line loads) -- no table read goes through the vector memory path.
// The records, the padding cells and the table are padded at plan time (build_sell) so that nothing here needs a bound check:
// SELL_DESC_PAD empty records behind the last slice, SELL_CELL_PAD cells, SELL_VTAB_MAX table entries.
template <typename T, int WMAX, int WAVES, int SPW, bool CONJ, int TAB>
__global__ __launch_bounds__(64 * WAVES) void sell_mv_short_kernel(aoclsparse_int m, aoclsparse_int nslices, int g0, int gstep,
                                                                   const uint4 *__restrict__ desc,
                                                                   const typename SellCell<T, TAB != 0>::src *__restrict__ sval,
                                                                   const aoclsparse_int *__restrict__ scol,
                                                                   const unsigned short *__restrict__ follow, T alpha,
                                                                   const T *__restrict__ x, T beta, T *__restrict__ y, bool nt,
                                                                   const T *__restrict__ vtab)
{
    using R = typename SellCell<T, TAB != 0>::raw;
    static_assert(WAVES * SPW <= SELL_DESC_PAD && 64 * WAVES == SELL_VTAB_MAX, "padding of the slice records / one table entry per lane");
    // group g of WAVES x SPW slices; consecutive products of a handle ALTERNATE the direction (SellPlan::products): g0 = last
    // group, gstep = -1 on odd ones
    const int sb   = __builtin_amdgcn_readfirstlane(((g0 + gstep * (int)blockIdx.x) * WAVES + (int)(threadIdx.x >> 6)) * SPW);
    const int lane = threadIdx.x & 63;
    s_pin_arg(alpha), s_pin_arg(beta), s_pin_arg(y), s_pin_arg((int)nt), s_pin_arg(x), s_pin_arg(sval), s_pin_arg(scol), s_pin_arg(follow);
    [[maybe_unused]] T t0, t1;
    if constexpr(TAB == 2)
        t0 = vtab[0], t1 = vtab[1];
    else if constexpr(TAB != 0)
        t0 = vtab[threadIdx.x];
    uint4 d[SPW];
#pragma unroll
    for(int u = 0; u < SPW; u++)
        d[u] = desc[sb + u];
    int  f[SPW]; // list of this lane | column shift << 8
    bool follows = false;
#pragma unroll
    for(int u = 0; u < SPW; u++)
    {
        const int mode = (int)(d[u].w >> 16) & 0xff;
        follows        = follows || mode == SELL_DESC_MODE_FOLLOW;
        f[u]           = mode == SELL_DESC_MODE_LANE_SHIFT ? lane << 8 : (mode == SELL_DESC_MODE_OWN ? lane : 0);
    }
    if(follows) // wave-uniform
    {
        int ff[SPW];
#pragma unroll
        for(int u = 0; u < SPW; u++)
            ff[u] = follow[min((sb + u) * 64 + lane, (int)m - 1)];
#pragma unroll
        for(int u = 0; u < SPW; u++)
            f[u] = ((int)(d[u].w >> 16) & 0xff) == SELL_DESC_MODE_FOLLOW ? ff[u] : f[u];
    }
    R   rr[SPW][WMAX];
    int cc[SPW][WMAX];
#pragma unroll
    for(int u = 0; u < SPW; u++)
    {
        const long long o0 = (long long)d[u].x | (long long)(d[u].z & 0xffffu) << 32;
        const long long c0 = (long long)d[u].y | (long long)(d[u].z >> 16) << 32;
        const int       w = (int)(d[u].w & 0xffu), cs = (int)(d[u].w >> 8) & 0xff;
        const auto     *v = sval + o0 + lane;
        const aoclsparse_int *c = scol + c0 + (f[u] & 0xff);
#pragma unroll
        for(int q = 0; q < WMAX; q++)
        {
            const int qq = max(min(q, w - 1), 0); // wave-uniform
            rr[u][q]     = v[qq * 64];
            cc[u][q]     = c[qq * cs];
        }
    }
    __builtin_amdgcn_sched_barrier(0); // (every line load is issued before the first wait for one)
    T vv[SPW][WMAX], xx[SPW][WMAX];
#pragma unroll
    for(int u = 0; u < SPW; u++)
#pragma unroll
        for(int q = 0; q < WMAX; q++) // (a padding cell, -1, is never used, but its gather must stay inside x: index 0)
            xx[u][q] = x[cc[u][q] >= 0 ? cc[u][q] + (f[u] >> 8) : 0];
    [[maybe_unused]] __shared__ T ltab[TAB > 2 ? SELL_VTAB_MAX : 1];
    if constexpr(TAB > 2) // (behind the gathers: the barrier is waited for while they are in flight)
    {
        ltab[threadIdx.x] = t0;
        __syncthreads();
    }
#pragma unroll
    for(int u = 0; u < SPW; u++)
#pragma unroll
        for(int q = 0; q < WMAX; q++)
        {
            if constexpr(TAB == 0)
                vv[u][q] = s_cj<CONJ>(rr[u][q]);
            else if constexpr(TAB == 2)
                vv[u][q] = rr[u][q] ? t1 : t0;
            else
                vv[u][q] = ltab[rr[u][q]];
        }
    T r[SPW];
#pragma unroll
    for(int u = 0; u < SPW; u++)
    {
        const int w = (int)(d[u].w & 0xffu);
        r[u]        = T(0);
#pragma unroll
        for(int q = 0; q < WMAX; q++)
            r[u] = (q < w && cc[u][q] >= 0) ? s_fma(vv[u][q], xx[u][q], r[u]) : r[u];
    }
#pragma unroll
    for(int u = 0; u < SPW; u++)
        s_pin(r[u]); // (every load above is issued before the first guarded store)
#pragma unroll
    for(int u = 0; u < SPW; u++)
    {
        const int i = (sb + u) * 64 + lane;
        if(sb + u < nslices && i < m)
            s_store(y + i, s_finish(r[u], alpha, beta, y + i), nt);
    }
}

// slices per wavefront of the short-row kernel: AOCLSPARSE_MI355_SELL_SPW = 1 / 2 / 4 overrides the rule (measurements only;
// read once per process)
inline int sell_short_spw_override()
{
    static const int v = [] {
        const char *e = std::getenv("AOCLSPARSE_MI355_SELL_SPW");
        const int   k = e ? std::atoi(e) : 0;
        return (k == 1 || k == 2 || k == 4) ? k : 0;
    }();
    return v;
}

constexpr aoclsparse_int SELL_SHORT_SPW_SLICES = 60000;

// TAB as the kernel's; CONJ for complex T only
template <typename T, int TAB, bool CONJ = false>
bool sell_launch_short(hipStream_t s, int wmax, aoclsparse_int m, aoclsparse_int nslices, const SellSliceDesc *desc,
                       const typename SellCell<T, TAB != 0>::src *sval, const aoclsparse_int *scol, T alpha, const T *x, T beta, T *y,
                       bool nt, const unsigned short *lead, int rev, const T *vtab)
{
    constexpr int  WAVES   = 4;
    constexpr bool COMPLEX = !std::is_floating_point_v<T>;
    // Slices per wavefront, by measurement (5-point Laplacians, cold products, one box, median of 20, ms; 1 / 2 / 4 slices per
    // wavefront; profiles/r8/spw_sweep.txt, which also has the VGPRs and the occupancy of each variant):
    //                       4096^2 (262,144 slices)    3000^2 (140,625)          2000^2 (62,500)
    //   double, table       0.1264 / 0.1204 / 0.1276   0.0729 / 0.0683 / 0.0722  0.0354 / 0.0333 / 0.0350
    //   double, values      0.2025 / 0.2032 / 0.2073   0.1250 / 0.1252 / 0.1294  0.0686 / 0.0712 / 0.0739
    //   float, table        0.1086 / 0.0747 / 0.0706   0.0590 / 0.0413 / 0.0415  0.0282 / 0.0218 / 0.0221
    //   float, values       0.1289 / 0.1193 / 0.1234   0.0780 / 0.0803 / 0.0820  0.0418 / 0.0409 / 0.0422
    // -> from 60,000 slices on: double with a table 2, float with a table 4, float values 2; double values stay at 1 (8-byte
    // cells: the bytes in flight of ONE slice already fill the wave's share).  Not measured below 60,000 slices: 1.  Complex: 1.
    int spw = 1;
    if constexpr(!COMPLEX)
    {
        if(nslices >= SELL_SHORT_SPW_SLICES)
            spw = sizeof(T) == 4 ? (TAB != 0 ? 4 : 2) : (TAB != 0 ? 2 : 1);
        if(sell_short_spw_override())
            spw = sell_short_spw_override();
    }
    const long long per_wg = (long long)WAVES * spw;
    const int       groups = (int)((nslices + per_wg - 1) / per_wg);
    const dim3      grid((unsigned)groups), block(64 * WAVES);
    const int       g0 = rev ? groups - 1 : 0, gstep = rev ? -1 : 1;
    const uint4    *dp = reinterpret_cast<const uint4 *>(desc);
#define MI355_SHORT_SPW(W, SPW)                                                                                                 \
    hipLaunchKernelGGL((sell_mv_short_kernel<T, W, WAVES, SPW, CONJ, TAB>), grid, block, 0, s, m, nslices, g0, gstep, dp, sval, \
                       scol, lead, alpha, x, beta, y, nt, vtab)
#define MI355_SHORT(W)                      \
    case W:                                 \
        if constexpr(!COMPLEX)              \
        {                                   \
            if(spw == 4)                    \
            {                               \
                MI355_SHORT_SPW(W, 4);      \
                return true;                \
            }                               \
            if(spw == 2)                    \
            {                               \
                MI355_SHORT_SPW(W, 2);      \
                return true;                \
            }                               \
        }                                   \
        MI355_SHORT_SPW(W, 1);              \
        return true
    switch(wmax)
    {
        MI355_SHORT(1);
        MI355_SHORT(2);
        MI355_SHORT(3);
        MI355_SHORT(4);
        MI355_SHORT(5);
        MI355_SHORT(6);
        MI355_SHORT(7);
        MI355_SHORT(8);
    default: return false;
    }
#undef MI355_SHORT
#undef MI355_SHORT_SPW
}

template <typename T, int ORDER, int PACK, bool IDX>
void sell_launch(hipStream_t s, aoclsparse_int m, aoclsparse_int nslices, const long long *slice_ptr,
                 const typename SellCell<T, IDX>::src *sval, const aoclsparse_int *scol, const aoclsparse_int *rowlen, T alpha,
                 const T *x, T beta, T *y, const long long *cptr, const unsigned short *lead, int rev, const T *vtab)
{
    // one slice per workgroup while the launch is small (every slice its own CU), two otherwise
    // (swept on the headline workload: 1 / 2 / 4 / 8 slices per workgroup = 0.221 / 0.218 / 0.221 / 0.222 ms)
    const bool nt = (size_t)m * sizeof(T) > ((size_t)32 << 20);
    if(cptr)
    {
        if(nslices < 2048)
            hipLaunchKernelGGL((sell_mv_kernel<T, ORDER, 1, PACK, true, false, IDX>), dim3(nslices), dim3(64), 0, s, m, nslices,
                               slice_ptr, sval, scol, rowlen, alpha, x, beta, y, nt, cptr, lead, rev, vtab);
        else
            hipLaunchKernelGGL((sell_mv_kernel<T, ORDER, 2, PACK, true, false, IDX>), dim3((nslices + 1) / 2), dim3(128), 0, s, m,
                               nslices, slice_ptr, sval, scol, rowlen, alpha, x, beta, y, nt, cptr, lead, rev, vtab);
    }
    else if(nslices < 2048)
        hipLaunchKernelGGL((sell_mv_kernel<T, ORDER, 1, PACK, false, false, IDX>), dim3(nslices), dim3(64), 0, s, m, nslices, slice_ptr,
                           sval, scol, rowlen, alpha, x, beta, y, nt, (const long long *)nullptr, (const unsigned short *)nullptr, rev,
                           vtab);
    else
        hipLaunchKernelGGL((sell_mv_kernel<T, ORDER, 2, PACK, false, false, IDX>), dim3((nslices + 1) / 2), dim3(128), 0, s, m,
                           nslices, slice_ptr, sval, scol, rowlen, alpha, x, beta, y, nt, (const long long *)nullptr,
                           (const unsigned short *)nullptr, rev, vtab);
}

} // namespace

template <typename T>
aoclsparse_status launch_sell_fill(hipStream_t s, int pack, aoclsparse_int m, int base, const aoclsparse_int *row_ptr,
                                   const aoclsparse_int *col, const T *val, aoclsparse_int nslices,
                                   const long long *slice_ptr, T *sval, aoclsparse_int *scol, aoclsparse_int *rowlen,
                                   const long long *cptr, const unsigned short *lead, unsigned char *sidx, const T *vtab,
                                   int ntab)
{
    if(nslices <= 0)
        return aoclsparse_status_success;
    if(cptr)
    {
        if(pack == 4)
            hipLaunchKernelGGL((sell_fill_shared_kernel<T, 4>), dim3((nslices + 3) / 4), dim3(256), 0, s, m, base, row_ptr,
                               col, val, nslices, slice_ptr, cptr, lead, sval, scol, rowlen, sidx, vtab, ntab);
        else
            hipLaunchKernelGGL((sell_fill_shared_kernel<T, 1>), dim3((nslices + 3) / 4), dim3(256), 0, s, m, base, row_ptr,
                               col, val, nslices, slice_ptr, cptr, lead, sval, scol, rowlen, sidx, vtab, ntab);
    }
    else if(pack == 4)
        hipLaunchKernelGGL((sell_fill_kernel<T, 4>), dim3((nslices + 3) / 4), dim3(256), 0, s, m, base, row_ptr, col,
                           val, nslices, slice_ptr, sval, scol, rowlen, sidx, vtab, ntab);
    else
        hipLaunchKernelGGL((sell_fill_kernel<T, 1>), dim3((nslices + 3) / 4), dim3(256), 0, s, m, base, row_ptr, col,
                           val, nslices, slice_ptr, sval, scol, rowlen, sidx, vtab, ntab);
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

// distinct bit patterns of the n values of `val` (vsize 4 or 8 bytes each): on return *ntab = their number and table[0 .. *ntab)
// = the patterns in ascending order (as 8-byte words), or *ntab = 0 if there are more than SELL_VTAB_MAX of them
aoclsparse_status sell_value_table(hipStream_t s, size_t vsize, long long n, const void *val, unsigned long long *table, int *ntab)
{
    *ntab = 0;
    if(n <= 0 || (vsize != 4 && vsize != 8))
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
    for(unsigned long long v : h)
        if(v != VT_EMPTY && k < SELL_VTAB_MAX)
            table[k++] = v;
    if(state[2] && k < SELL_VTAB_MAX)
        table[k++] = VT_EMPTY;
    std::sort(table, table + k); // (ascending bit pattern: the plan does not depend on the order the device found them in)
    *ntab = k;
    return aoclsparse_status_success;
}

template <typename T>
aoclsparse_status launch_sellmv(hipStream_t s, int order, int pack, T alpha, aoclsparse_int m, aoclsparse_int nslices,
                                const long long *slice_ptr, const T *sval, const aoclsparse_int *scol,
                                const aoclsparse_int *rowlen, const T *x, T beta, T *y, const long long *cptr,
                                const unsigned short *lead, aoclsparse_int max_width, int rev, const unsigned char *sidx,
                                const T *vtab, const SellSliceDesc *desc, int ntab)
{
    if(m <= 0 || nslices <= 0)
        return aoclsparse_status_success;
    if(order < 0 || order > 2 || (pack != 1 && pack != 4))
        return aoclsparse_status_invalid_kid;
    // vtab: the cells are one-byte indices into it (sidx); else the values themselves (sval)
    auto go = [&](auto idx_tag) {
        constexpr bool IDX = decltype(idx_tag)::value;
        const typename SellCell<T, IDX>::src *cells;
        if constexpr(IDX)
            cells = sidx;
        else
            cells = sval;
        // the plan has slice records (build_sell: widest slice <= 8 cells, pack 1, a launch large enough that four slices per
        // workgroup still spread over every CU) and the order is the scalar one: the short-row kernel
        if(order == 0 && pack == 1 && desc)
        {
            const bool nt = (size_t)m * sizeof(T) > ((size_t)32 << 20);
            bool       done;
            if constexpr(!IDX)
                done = sell_launch_short<T, 0>(s, (int)max_width, m, nslices, desc, cells, scol, alpha, x, beta, y, nt, lead, rev, vtab);
            else if(ntab <= 2)
                done = sell_launch_short<T, 2>(s, (int)max_width, m, nslices, desc, cells, scol, alpha, x, beta, y, nt, lead, rev, vtab);
            else
                done = sell_launch_short<T, SELL_VTAB_MAX>(s, (int)max_width, m, nslices, desc, cells, scol, alpha, x, beta, y, nt, lead,
                                                           rev, vtab);
            if(done)
                return;
        }
#define SELL_CASE(O, P)                                                                                            \
    sell_launch<T, O, P, IDX>(s, m, nslices, slice_ptr, cells, scol, rowlen, alpha, x, beta, y, cptr, lead, rev, vtab); \
    break
        switch(order * 2 + (pack == 4 ? 1 : 0))
        {
        case 0:
            SELL_CASE(0, 1);
        case 1:
            SELL_CASE(0, 4);
        case 2:
            SELL_CASE(1, 1);
        case 3:
            SELL_CASE(1, 4);
        case 4:
            SELL_CASE(2, 1);
        case 5:
            SELL_CASE(2, 4);
        }
#undef SELL_CASE
    };
    if(vtab)
        go(std::true_type{});
    else
        go(std::false_type{});
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

// aoclsparse_{c,z}mv on the SELL-64 copy (PACK 1, the scalar chain per row): the short-row kernel where the plan has slice
// records (large launches whose widest slice has <= 8 cells), the general kernel otherwise
template <typename R>
aoclsparse_status launch_sellmv_complex(hipStream_t s, bool conj, cplx<R> alpha, aoclsparse_int m, aoclsparse_int nslices,
                                        const long long *slice_ptr, const cplx<R> *sval, const aoclsparse_int *scol,
                                        const aoclsparse_int *rowlen, const cplx<R> *x, cplx<R> beta, cplx<R> *y,
                                        const long long *cptr, const unsigned short *lead, aoclsparse_int max_width, int rev,
                                        const SellSliceDesc *desc)
{
    using C = cplx<R>;
    if(m <= 0 || nslices <= 0)
        return aoclsparse_status_success;
    const bool nt = (size_t)m * sizeof(C) > ((size_t)32 << 20);
    auto       go = [&](auto shared_tag, auto conj_tag) {
        constexpr bool SH = decltype(shared_tag)::value, CJ = decltype(conj_tag)::value;
        const long long      *cp = SH ? cptr : nullptr;
        const unsigned short *ld = SH ? lead : nullptr;
        if(desc && sell_launch_short<C, 0, CJ>(s, (int)max_width, m, nslices, desc, sval, scol, alpha, x, beta, y, nt, ld, rev, nullptr))
            return;
        if(nslices < 2048)
            hipLaunchKernelGGL((sell_mv_kernel<C, 0, 1, 1, SH, CJ>), dim3(nslices), dim3(64), 0, s, m, nslices, slice_ptr, sval, scol,
                               rowlen, alpha, x, beta, y, nt, cp, ld, rev);
        else
            hipLaunchKernelGGL((sell_mv_kernel<C, 0, 2, 1, SH, CJ>), dim3((nslices + 1) / 2), dim3(128), 0, s, m, nslices, slice_ptr,
                               sval, scol, rowlen, alpha, x, beta, y, nt, cp, ld, rev);
    };
    if(cptr)
    {
        if(conj)
            go(std::true_type{}, std::true_type{});
        else
            go(std::true_type{}, std::false_type{});
    }
    else if(conj)
        go(std::false_type{}, std::true_type{});
    else
        go(std::false_type{}, std::false_type{});
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}
template aoclsparse_status launch_sellmv_complex<double>(hipStream_t, bool, cdouble, aoclsparse_int, aoclsparse_int, const long long *,
                                                         const cdouble *, const aoclsparse_int *, const aoclsparse_int *,
                                                         const cdouble *, cdouble, cdouble *, const long long *,
                                                         const unsigned short *, aoclsparse_int, int, const SellSliceDesc *);
template aoclsparse_status launch_sellmv_complex<float>(hipStream_t, bool, cfloat, aoclsparse_int, aoclsparse_int, const long long *,
                                                        const cfloat *, const aoclsparse_int *, const aoclsparse_int *, const cfloat *,
                                                        cfloat, cfloat *, const long long *, const unsigned short *, aoclsparse_int, int,
                                                        const SellSliceDesc *);
// (the fill kernels only move values: cfloat cells are filled as 8-byte doubles, cdouble cells need their own instantiation)
template aoclsparse_status launch_sell_fill<cdouble>(hipStream_t, int, aoclsparse_int, int, const aoclsparse_int *, const aoclsparse_int *,
                                                     const cdouble *, aoclsparse_int, const long long *, cdouble *, aoclsparse_int *,
                                                     aoclsparse_int *, const long long *, const unsigned short *, unsigned char *,
                                                     const cdouble *, int);

aoclsparse_status launch_sell_leaders(hipStream_t s, aoclsparse_int m, int base, const aoclsparse_int *row_ptr, const aoclsparse_int *col,
                                      aoclsparse_int nslices, unsigned short *lead, aoclsparse_int *nl)
{
    if(nslices <= 0)
        return aoclsparse_status_success;
    hipLaunchKernelGGL(sell_leaders_kernel, dim3((nslices + 3) / 4), dim3(256), 0, s, m, base, row_ptr, col, nslices, lead, nl);
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

#define MI355_SELL_INSTANTIATE(T)                                                                                     \
    template aoclsparse_status launch_sell_fill<T>(hipStream_t, int, aoclsparse_int, int, const aoclsparse_int *,     \
                                                   const aoclsparse_int *, const T *, aoclsparse_int,                 \
                                                   const long long *, T *, aoclsparse_int *, aoclsparse_int *,        \
                                                   const long long *, const unsigned short *, unsigned char *, const T *, \
                                                   int);                                                              \
    template aoclsparse_status launch_sellmv<T>(hipStream_t, int, int, T, aoclsparse_int, aoclsparse_int,             \
                                                const long long *, const T *, const aoclsparse_int *,                 \
                                                const aoclsparse_int *, const T *, T, T *, const long long *,          \
                                                const unsigned short *, aoclsparse_int, int, const unsigned char *,    \
                                                const T *, const SellSliceDesc *, int);
MI355_SELL_INSTANTIATE(double)
MI355_SELL_INSTANTIATE(float)

} // namespace mi355
