// sell_kernels.hip -- SpMV on SELL-64, the layout aoclsparse_optimize builds for an mv hint on MI355X.
//
// The reference's optimize step re-stores a hinted matrix in the format its CPU kernels like best
// (br4 / ELLT-HYB / blocked CSR, analysis.cpp:146-382).  The GPU analogue is sliced ELL with one slice
// per 64-wide wavefront (the layout, and the kernels that build it: sell_build_kernels.hip).  Lane i of a wave owns row i:
//   * every val / col access is one coalesced line per wavefront instruction, no row_ptr, no LDS;
//   * a lane walks its row front to back, so the reference's summation orders are reproduced exactly:
//     order 0 is the scalar FMA chain (csrmv_kr.hpp:448-513); orders 1 / 2 keep 4 / 8 partial sums per
//     lane for the full groups, reduce them as the AVX2 / AVX-512 kernels do, then run the scalar tail
//     (csrmv_kr.hpp:949-1040, csrmv_avx512.cpp:36-134, csrmv_kr.hpp:734-831 for float).
// Bytes per launch: cells*(8+4) + 8 m (y) (+ 8 m if beta != 0) (+ 4 m row lengths for orders 1 / 2) + x
// gathers; cells <= 1.15 nnz or the handle stays on the CSR-Adaptive kernel (sell_plan.cpp: build_sell).
#include "internal.hpp"

#include <cstdlib>
#include <type_traits>

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

// the value cells as the kernels read them: values, or (IDX) indices into the plan's value table (sell_build_kernels.hip)
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
// Packed table indices (plans with slice records whose rows fit: build_sell): ONE word of 1 / 2 / 4 bytes per row, at row x bytes,
// the index of cell q in the bits-wide field at bit q x bits.  The width is a run-time scalar, not a template argument.
__device__ __forceinline__ int packed_index(unsigned word, int q, int bits)
{
    return (int)((word >> (q * bits)) & ((1u << bits) - 1u));
}
__device__ __forceinline__ unsigned packed_word(const void *__restrict__ words, long long row, int bytes)
{
    if(bytes == 1)
        return static_cast<const unsigned char *>(words)[row];
    if(bytes == 2)
        return static_cast<const unsigned short *>(words)[row];
    return static_cast<const unsigned *>(words)[row];
}
// the same without a branch on the width: the aligned dword that holds the word, shifted and masked (the words of a wavefront are
// one line either way; the array is a multiple of 4 bytes long, build_sell pads it by whole slices)
__device__ __forceinline__ unsigned packed_word_any(const void *__restrict__ words, long long row, int bytes)
{
    const long long a = row * bytes;
    const unsigned  d = static_cast<const unsigned *>(words)[a >> 2];
    return (d >> (((unsigned)a & 3u) * 8u)) & (0xffffffffu >> (32 - 8 * bytes));
}
// (shared column lists -- cptr, follow -- and the slice modes in cptr's top byte: sell_build_kernels.hip)
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
// pbits > 0 (table indices, PACK 1): the row's indices are the pbits-wide fields of pw, nothing is read from v
template <typename S, typename R, int PACK, int G>
__device__ __forceinline__ void load_step(const S *v, const aoclsparse_int *c, int p0, int w, R (&vv)[G], int (&cc)[G],
                                          int cs = 64, unsigned pw = 0, int pbits = 0)
{
    if constexpr(PACK == 1)
    {
#pragma unroll
        for(int q = 0; q < G; q++)
        {
            const bool ok = p0 + q < w;
            if constexpr(std::is_same_v<R, int>)
                vv[q] = ok ? (pbits ? packed_index(pw, p0 + q, pbits) : (R)v[(p0 + q) * 64]) : R(0);
            else
                vv[q] = ok ? (R)v[(p0 + q) * 64] : R(0);
            cc[q] = ok ? c[(p0 + q) * cs] : -1;
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
                                                             const T *__restrict__ vtab = nullptr, int pbits = 0, int pbytes = 0)
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
    // pbits > 0 (IDX, PACK 1: the plan has slice records, a pinned order or a transposed product came here): sval holds one
    // packed word per row, read once; cell(p) is field p of it
    [[maybe_unused]] unsigned pw = 0;
    if constexpr(IDX && PACK == 1)
    {
        if(pbits)
            pw = packed_word(sval, (long long)s * 64 + lane, pbytes);
    }
    else
        pbits = 0;
    auto cell = [&](int p) -> R {
        if constexpr(IDX && PACK == 1)
        {
            if(pbits)
                return packed_index(pw, p, pbits);
        }
        return (R)v[p * 64];
    };
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
                rr[q] = cell(q), cc[q] = c[q * cs];
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
            const R   r0 = cell(p + 0), r1 = cell(p + 1), r2 = cell(p + 2), r3 = cell(p + 3);
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
            const R   r0 = cell(p);
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
        load_step<S, R, PACK, G>(v, c, 0, w, vn, cn, cs, pw, pbits);
        for(int p0 = 0; p0 < w; p0 += G)
        {
            T   vv[G], xx[G];
            R   vr[G];
            int cc[G];
#pragma unroll
            for(int q = 0; q < G; q++)
                vr[q] = vn[q], cc[q] = cn[q];
            if(p0 + G < w)
                load_step<S, R, PACK, G>(v, c, p0 + G, w, vn, cn, cs, pw, pbits);
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

// N adjacent rows of x or y in one lane, aligned as ONE element (the operands and x + column are no better)
template <typename T, int N>
using SellRows = T __attribute__((ext_vector_type(N), aligned(sizeof(T))));

// Short rows: matrices whose widest slice has WMAX <= 8 cells, scalar summation order, PACK 1, large launches.  A wavefront
// takes SPW consecutive slices and walks them TOGETHER, with no loop on the common path.  On a plan with uniform column lists
// and packed table indices (UCOL, PK: a stencil with a value table, the headline) its life is THREE dependent round trips
// whatever SPW is:
//   1. the kernel arguments (one scalar batch: the sweep direction is the pair g0 / gstep, not a branch);
//   2. one scalar batch whose every address is a function of the slice number alone: the SPW slice records (SellSliceDesc, one
//      wide scalar load) and the SPW uniform column lists (ucol, 8 columns per slice, consecutive slices adjacent: one wide
//      scalar load);
//   3. the packed index words (one contiguous line per slice) and all the x gathers, each at a scalar base (x + column) plus the
//      lane's offset; then the chains and the stores.
// A slice of mode 1 / 2 (full, one leader: sell_leaders_kernel) has ONE column list, so its columns are wave-uniform: they live
// in scalar registers and no vector load fetches them.  A group with a slice of any other mode (mode 0, lead[] says which list a
// lane follows: 2 slices in 64 on a stencil; mode 3, lists not shared) takes ONE wave-uniform branch to the column lists in col,
// as every group does without UCOL: there the life is four round trips (records -> value / column lines, index clamped to the
// slice's own width, and to 0 for an EMPTY slice, which reads the padding cells behind the arrays -> gathers), five with lead[].
// A RUN (double, UCOL, PK, SPW > 1): the group's SPW slices are all mode 1, of one width, and every list continues the list
// before it (column + 64 in every used cell), so row j of the group's 64 SPW rows reads x[column_q + j] with ONE base per cell.
// Then lane l owns the SPW CONSECUTIVE rows SPW l .. SPW l + SPW - 1 instead of row l of every slice: one gather per cell of
// SPW elements per lane (16 bytes at the shipped SPW of 2), one load of the lane's SPW adjacent word bytes, one
// store of y -- 7 vector memory instructions on the headline instead of 14; the same three round trips, the same
// bytes, each row's chain as before.  The test is scalar compares on the records and lists of the batch; it is the third outcome
// of the wave-uniform decision (lists in col / uniform by slice / run), and the packed words are loaded behind it, by the
// mapping it chose.  x + column, x and y are aligned as elements only: the vector type says so.  Words of more than one byte
// per row (pbytes > 1) stay on the mapping by slice.
// RECORD FLAGS (UCOL, PK, one-byte words; internal.hpp: SELL_DESC_UWORD / SELL_DESC_EXCEPT, set at plan time by
// sell_records_kernel): a slice whose 64 rows share one word has it in its record, and a group in which every slice does reads
// no word at all (6 vector memory instructions in a run on the headline); a mode-0 slice that is one list shifted by lane of
// which at most two lanes omit cells (the first and last slice of a grid line) counts as a shifted slice -- for the column
// decision and the run test -- with its canonical list in ucol, and the two lanes get the mask of the cells they have instead of
// the full one: the gather of an absent cell is issued (inside x by the plan's rule) and dropped by the chain's select, so each
// row's chain is its own cells in its own order and the bits are unchanged.  A group that still reads the lists in col reads a
// flagged slice as before (its rows' own words, follow[]).
// Without PK the value (or one-byte index) lines are SPW x WMAX vector loads behind the records.
// TAB: 0 = the cells hold values; 2 = indices into a table of <= 2 values, held in scalar registers and selected;
// 256 = indices into a table of <= SELL_VTAB_MAX values, copied to LDS once per workgroup (its load goes out with the records,
// the barrier sits behind the gathers) -- no table read goes through the vector memory path.
// PK (TAB != 0): sval holds one packed word per row (packed_index; TAB 2: always one byte, one bit per cell).
// The records, the lists, the words, the padding cells and the table are padded at plan time (build_sell) so that nothing here
// needs a bound check: SELL_DESC_PAD empty records / lists of -1 / zero words behind the last slice, SELL_CELL_PAD cells,
// SELL_VTAB_MAX table entries.
template <typename T, int WMAX, int WAVES, int SPW, bool CONJ, int TAB, bool UCOL, bool PK>
__global__ __launch_bounds__(64 * WAVES) void sell_mv_short_kernel(aoclsparse_int m, aoclsparse_int nslices, int g0, int gstep,
                                                                   const uint4 *__restrict__ desc,
                                                                   const typename SellCell<T, TAB != 0>::src *__restrict__ sval,
                                                                   const aoclsparse_int *__restrict__ scol,
                                                                   const unsigned short *__restrict__ follow, T alpha,
                                                                   const T *__restrict__ x, T beta, T *__restrict__ y, bool nt,
                                                                   const T *__restrict__ vtab, const aoclsparse_int *__restrict__ ucol,
                                                                   int pbits, int pbytes)
{
    constexpr bool PERIOD = false, MARCH = false; // (no periodic range: the names the body reads under PERIOD / MARCH, never used)
    [[maybe_unused]] constexpr int      pslo = 0, plen = 0, pper = 0, mskip = 0;
    [[maybe_unused]] constexpr unsigned prcp = 0, pstrideb = 0;
    const int bgroup = g0 + gstep * (int)blockIdx.x;
#include "sell_short_body.inc"
}

// The kernel of a plan with uniform lists and packed words (real types; UCOL && PK): the same body with the plan's periodic
// range -- slices [pslo, pslo + plen), period pper slices, prcp = the launcher's reciprocal of pper, pstrideb = the column shift
// per period in bytes; plen = 0: the plan has none and every wavefront reads its own records.
template <typename T, int WMAX, int WAVES, int SPW, int TAB>
__global__ __launch_bounds__(64 * WAVES) void sell_mv_short_period_kernel(aoclsparse_int m, aoclsparse_int nslices, int g0, int gstep,
                                                                          const uint4 *__restrict__ desc,
                                                                          const typename SellCell<T, true>::src *__restrict__ sval,
                                                                          const aoclsparse_int *__restrict__ scol,
                                                                          const unsigned short *__restrict__ follow, T alpha,
                                                                          const T *__restrict__ x, T beta, T *__restrict__ y, bool nt,
                                                                          const T *__restrict__ vtab,
                                                                          const aoclsparse_int *__restrict__ ucol, int pbits, int pbytes,
                                                                          int pslo, int plen, int pper, unsigned prcp, unsigned pstrideb)
{
    constexpr bool CONJ = false, UCOL = true, PK = true, PERIOD = true, MARCH = false;
    [[maybe_unused]] constexpr int mskip = 0;
    const int bgroup = g0 + gstep * (int)blockIdx.x;
#include "sell_short_body.inc"
}

// STACKED PERIODS (double; a plan whose periodic range can be stacked: internal.hpp, sell_march_rule).  In a range of period
// pper slices and column shift pstride, the wavefront at position s of the period sees in period k + 1 exactly what it saw in
// period k -- records, lists, words, exception lanes -- and only x and y move on by pstride elements.  So ONE wavefront takes G
// consecutive periods of its strip of SPW slices, in straight-line code: it reads the first period's records once, issues every
// gather of its G periods before the first wait, runs G x SPW chains and stores G times.  No loop, no barrier, no LDS,
// no test: the plan has decided that every group of the period is a run with its words in the records, so this is the body's run
// path with the decisions taken out.
// ALIAS (four bits per cell: a(q) + 1, 0 = none; SELL_MARCH_MAPS): cell q of period k + 1 IS cell a(q) of period k -- on the
// 5-point stencil the centre strip of grid line t is the south strip of line t - 1 and the north strip of line t + 1 -- so from
// the second period on only the cells without a(q) are gathered: 3 G + 2 gathers on the 5-point stencil where G wavefronts of
// sell_mv_short_period_kernel issue 5 G.  Every gather issued is one that kernel issues for the same slice (base x + (k + t) pstride
// + column, 16 bytes per lane), so each stays inside x by its argument; none is added.  Each row's chain is its own cells front to
// back with the record's masks and the table's values, as in the body: the same bits.
// ONE launch: workgroups [0, mblocks) of the sweep (g0 / gstep, alternating as in the body) are stacked -- wavefront j takes position
// j % mhp of the period (mhp = pper / SPW, mrcp the launcher's reciprocal of it) and the periods G (j / mhp) .. + G - 1 -- and the
// others run the body over the slices outside [pslo, pslo + mskip): before the range, behind it, and the periods left over.
template <typename T, int WMAX, int WAVES, int SPW, int TAB, int G, unsigned ALIAS>
__global__ __launch_bounds__(64 * WAVES) void sell_mv_short_march_kernel(aoclsparse_int m, aoclsparse_int nslices, int g0, int gstep,
                                                                         const uint4 *__restrict__ desc,
                                                                         const typename SellCell<T, true>::src *__restrict__ sval,
                                                                         const aoclsparse_int *__restrict__ scol,
                                                                         const unsigned short *__restrict__ follow, T alpha,
                                                                         const T *__restrict__ x, T beta, T *__restrict__ y, bool nt,
                                                                         const T *__restrict__ vtab,
                                                                         const aoclsparse_int *__restrict__ ucol, int pbits, int pbytes,
                                                                         int pslo, int plen, int pper, unsigned prcp, unsigned pstrideb,
                                                                         int mblocks, int mhp, unsigned mrcp, int mskip)
{
    constexpr bool CONJ = false, UCOL = true, PK = true, PERIOD = true, MARCH = true;
    // (TAB 2 only: one-byte words of the 5 cells of the one map built leave one bit per cell, a table of two)
    static_assert(SPW > 1 && std::is_same_v<T, double> && TAB == 2 && G >= 2, "the run mapping of a double plan with a table of two");
    const int vgroup = g0 + gstep * (int)blockIdx.x;
    if(vgroup < mblocks) // uniform over the workgroup
    {
        using RowVec = SellRows<T, SPW>;
        using GV     = const __attribute__((address_space(1))) RowVec;
        using GC     = const __attribute__((address_space(1))) char;
        const unsigned j    = (unsigned)__builtin_amdgcn_readfirstlane(vgroup * WAVES + (int)(threadIdx.x >> 6));
        const int      lane = threadIdx.x & 63;
        s_pin_arg(alpha), s_pin_arg(beta), s_pin_arg(y), s_pin_arg((int)nt), s_pin_arg(x);
        const T t0 = vtab[0], t1 = vtab[1];
        // position in the period and first period: one multiply by the reciprocal, no division, no branch
        const unsigned gi  = __umulhi(j, mrcp);
        const unsigned pos = j - gi * (unsigned)mhp;
        const unsigned sp  = (unsigned)pslo + pos * (unsigned)SPW; // the strip's slices in the FIRST period
        const unsigned k0  = gi * (unsigned)G;
        const uint4          *dp = reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(desc) + sp * (unsigned)sizeof(uint4));
        const aoclsparse_int *up = reinterpret_cast<const aoclsparse_int *>(reinterpret_cast<const char *>(ucol)
                                                                            + sp * (unsigned)(SELL_SHORT_WMAX * sizeof(aoclsparse_int)));
        uint4 d[SPW];
#pragma unroll
        for(int u = 0; u < SPW; u++)
            d[u] = dp[u];
        int uc[WMAX]; // the first slice's list: the run's one base per cell
#pragma unroll
        for(int q = 0; q < WMAX; q++)
            uc[q] = up[q];
#pragma unroll
        for(int q = 0; q < WMAX; q++)
            s_pin_arg(uc[q]);
#pragma unroll
        for(int u = 0; u < SPW; u++)
            s_pin_arg(d[u].x), s_pin_arg(d[u].y), s_pin_arg(d[u].z), s_pin_arg(d[u].w); // (whole records: one wide load, no register reused inside the batch)
        s_pin_arg(t0), s_pin_arg(t1);
        __builtin_amdgcn_sched_barrier(0);
        // the gathers of all G periods: every cell of the first, the cells without a(q) of the others
        T xx[G][SPW][WMAX];
#pragma unroll
        for(int t = 0; t < G; t++)
        {
            GC *xt = (GC *)x + (k0 + (unsigned)t) * pstrideb; // (below 2^32 by the launcher's check, as in the body)
#pragma unroll
            for(int q = 0; q < WMAX; q++)
            {
                const int a = (int)((ALIAS >> (4 * q)) & 0xfu) - 1;
                if(t > 0 && a >= 0)
                {
#pragma unroll
                    for(int u = 0; u < SPW; u++)
                        xx[t][u][q] = xx[t - 1][u][a];
                }
                else
                {
                    GC *gb = xt + (long long)max(uc[q], 0) * (long long)sizeof(T);
                    asm volatile("" : "+s"(gb)); // (the base stays a scalar pair: as in the body)
                    const RowVec xv = *(GV *)(gb + (unsigned)lane * (unsigned)sizeof(RowVec));
#pragma unroll
                    for(int u = 0; u < SPW; u++)
                        xx[t][u][q] = xv[u];
                }
            }
        }
        // the lane's SPW rows lie in ONE slice of the group, slice lane / (64 / SPW): its record's word; the masks of the exception
        // lanes (row 64 v + lane of the group is row u of its owner): the same in every period
        const int ls = lane / (64 / SPW);
        unsigned  rw = d[0].x & 0xffu;
#pragma unroll
        for(int u = 1; u < SPW; u++)
            rw = ls == u ? (d[u].x & 0xffu) : rw;
        unsigned okm[SPW];
        bool     anyex = false;
#pragma unroll
        for(int u = 0; u < SPW; u++)
            okm[u] = (1u << (d[0].w & 0xffu)) - 1u, anyex = anyex || (d[u].w & SELL_DESC_EXCEPT) != 0u;
        if(__builtin_expect(anyex, 0)) // wave-uniform
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
        T r[G][SPW];
#pragma unroll
        for(int t = 0; t < G; t++)
#pragma unroll
            for(int u = 0; u < SPW; u++)
            {
                r[t][u] = T(0);
#pragma unroll
                for(int q = 0; q < WMAX; q++)
                {
                    const T vv = ((rw >> q) & 1u) ? t1 : t0;
                    r[t][u]    = ((okm[u] >> q) & 1u) ? s_fma(vv, xx[t][u][q], r[t][u]) : r[t][u];
                }
            }
#pragma unroll
        for(int t = 0; t < G; t++)
#pragma unroll
            for(int u = 0; u < SPW; u++)
                s_pin(r[t][u]); // (every load above is issued before the first store)
        // the lane's SPW rows are adjacent, inside m (the slices of a run are full): one store per period
#pragma unroll
        for(int t = 0; t < G; t++)
        {
            const long long sbt = (long long)sp + (long long)(k0 + (unsigned)t) * (long long)pper;
            RowVec         *yp  = reinterpret_cast<RowVec *>(y + sbt * 64 + SPW * lane);
            RowVec          yv  = {};
            if(beta != T(0))
                yv = *yp;
#pragma unroll
            for(int u = 0; u < SPW; u++)
            {
                const T yu = yv[u];
                yv[u]      = s_finish(r[t][u], alpha, beta, &yu);
            }
            if(nt)
                __builtin_nontemporal_store(yv, yp);
            else
                *yp = yv;
        }
        return;
    }
    const int bgroup = vgroup - mblocks;
#include "sell_short_body.inc"
}

// TAB as the kernel's; CONJ for complex T only.  false: no kernel for this width (v.max_width > SELL_SHORT_WMAX)
template <typename T, int TAB, bool CONJ>
bool sell_launch_short(hipStream_t s, const SellView &v, T alpha, const T *x, T beta, T *y, bool nt, int rev)
{
    constexpr int        WAVES   = 4;
    constexpr bool       COMPLEX = !std::is_floating_point_v<T>;
    const aoclsparse_int m = v.m, nslices = v.nslices;
    // Slices per wavefront, by measurement (5-point Laplacians, cold products, one box, median of 20, ms; 1 / 2 / 4 slices per
    // wavefront).  table = packed words, uniform lists, the periodic range: sell_mv_short_period_kernel, profiles/r17/spw_sweep.txt;
    // values = the cells hold values: sell_mv_short_kernel, profiles/r10/spw_sweep.txt, which also has the VGPRs and the
    // occupancy of each variant (measured there WITH uniform lists, which lost and are not built for them):
    //                       4096^2 (262,144 slices)    3000^2 (140,625)          2000^2 (62,500)
    //   double, table       0.0700 / 0.0539 / 0.0642   0.0431 / 0.0437 / 0.0442  0.0220 / 0.0203 / 0.0235
    //   double, values      0.1741 / 0.1774 / 0.1811   0.0905 / 0.0943 / 0.0962  0.0421 / 0.0444 / 0.0470
    //   float, table        0.0540 / 0.0407 / 0.0368   0.0342 / 0.0270 / 0.0253  0.0181 / 0.0154 / 0.0149
    //   float, values       0.1028 / 0.0864 / 0.0887   0.0555 / 0.0533 / 0.0534  0.0275 / 0.0256 / 0.0276
    // -> from 60,000 slices on: double with a table 2 (3000^2: 1, 2 and 4 within 2.5 %, inside the spread), float with a table 4,
    // float values 2; double values stay at 1 (8-byte cells: the bytes in flight of ONE slice already fill the wave's share).
    // The same rule since profiles/r8/spw_sweep.txt.  Not measured below 60,000 slices: 1.  Complex: 1.
    int spw = 1;
    if constexpr(!COMPLEX)
        spw = sell_short_spw(nslices, sizeof(T), TAB != 0);
    const long long per_wg = (long long)WAVES * spw;
    const int       groups = (int)((nslices + per_wg - 1) / per_wg);
    const dim3      grid((unsigned)groups), block(64 * WAVES);
    const int       g0 = rev ? groups - 1 : 0, gstep = rev ? -1 : 1;
    const uint4    *dp = reinterpret_cast<const uint4 *>(v.desc);
    const auto     *sval = static_cast<const typename SellCell<T, TAB != 0>::src *>(v.cells);
    const T        *vtab = static_cast<const T *>(v.vtab);
    if(TAB == 2 && !(v.pbits == 1 && v.pbytes == 1)) // (a plan with slice records and <= 2 table entries always packs)
        return false;
    // the plan's periodic range (SellView::pslo ..; none, or one the kernel can use: sell_period_usable, checked again here because
    // a range that failed it would read other slices' records) and the reciprocal of the period: 2^32 / period for a power of
    // two, else floor(2^32 / period) + 1
    int      pslo = v.pslo, pshi = v.pshi, pper = v.pper, pstride = v.pstride;
    unsigned prcp = 0;
    if(sell_period_usable(nslices, pslo, pshi, pper, pstride, sizeof(T)))
        prcp = (unsigned)((1ull << 32) / (unsigned)pper) + ((pper & (pper - 1)) == 0 ? 0u : 1u);
    else
        pslo = pshi = pper = pstride = 0;
    // STACKED PERIODS (sell_mv_short_march_kernel; the rule: internal.hpp, sell_march_rule, which aoclsparse_mi355_get_sell_march
    // reports): a double plan whose range can be stacked and whose alias map is in SELL_MARCH_MAPS runs SELL_MARCH_G = 3 periods
    // per wavefront with the shared loads of its map.  By measurement (5-point Laplacians of gx x gy points and the boundary-free
    // 5-cell stencil with lines of 256, double, cold products, one box, medians of 40 over three alternated rounds, ms;
    // profiles/r18/upper_bound.txt, g_sweep.txt: not stacked / G = 2 / 3 / 4 with shared loads | G = 2 / 3 / 4 without):
    //   gx x gy (slices, period)          not stacked   shared 2 / 3 / 4               not shared 2 / 3 / 4
    //   4096 x 4096 (262,144, 64)         0.0524        0.0447 / 0.0452 / 0.0454      0.0471 / 0.0468 / 0.0465
    //   free, lines of 256 (262,144, 4)   0.0601        0.0511 / 0.0491 / 0.0482      0.0513 / 0.0492 / 0.0485
    //   1024 x 16384 (262,144, 16)        0.0750        0.0599 / 0.0548 / 0.0528      0.0603 / 0.0560 / 0.0541
    //   8192 x 2048 (262,144, 128)        0.0533        0.0459 / 0.0450 / 0.0451      0.0480 / 0.0465 / 0.0460
    //   16384 x 1024 (262,144, 256)       0.0537        0.0463 / 0.0453 / 0.0452      0.0484 / 0.0467 / 0.0460
    //   32768 x 512 (262,144, 512)        0.0536        0.0471 / 0.0456 / 0.0454      0.0493 / 0.0477 / 0.0468
    //   4096 x 2048 (131,072, 64)         0.0313        0.0261 / 0.0256 / 0.0263      0.0270 / 0.0277 / 0.0278
    //   4096 x 1024 (65,536, 64)          0.0191        0.0165 / 0.0163 / 0.0171      0.0169 / 0.0175 / 0.0181
    //   3000 x 3000 (140,625, 1500)       0.0439        (no alias: the period is 32 lines)  0.0444 / 0.0436 / 0.0446
    //   2000 x 2000 (62,500, 500)         0.0204        (no alias: 16 lines)                0.0212 / 0.0202 / 0.0204
    //   3008 x 3000 (140,952, 188)        0.0429        (no alias: 4 lines)                 0.0438 / 0.0436 / 0.0437
    // -> with the shared loads every G gains 12 - 30 % wherever the map exists; G = 3 is the best or within 1 % of it on six of the
    // eight, 1.1 % behind 2 on the headline and 2 - 4 % behind 4 at periods of 4 and 16 slices: one value, 3.  Without shared loads
    // stacking gains where it was forced on a plan that has the map and nothing (-1 .. +2 %) on the plans that really have none,
    // so a plan without a map in the table keeps sell_mv_short_period_kernel.  Float (four rows per lane) was not built.
    if constexpr(!COMPLEX && TAB == 2 && sizeof(T) == 8) // (a larger table leaves no room for 5 cells in a one-byte word)
    {
        if(v.ucol && v.pbits && prcp)
        {
            const SellMarch mr = sell_march_rule(nslices, v.max_width, pslo, pshi, pper, pstride, v.mstack, v.malias, sizeof(T), spw);
            if(mr.g)
            {
                // stacked wavefronts: (periods / g) x (pper / SPW), a whole number of workgroups by the rule; then the workgroups
                // of the slices outside [lo, hi).  Stacked first in the ascending sweep, last in the descending one (the other order
                // was not measured: on the headline 192 of 262,144 slices lie outside).
                const int       hp      = pper / SELL_MARCH_SPW;
                const unsigned  mrcp    = (unsigned)((1ull << 32) / (unsigned)hp) + ((hp & (hp - 1)) == 0 ? 0u : 1u);
                const int       mskip   = mr.hi - mr.lo;
                const int       mblocks = (int)((long long)(mskip / pper / mr.g) * hp / WAVES);
                const long long rest    = (long long)nslices - mskip, per_rest = (long long)WAVES * SELL_MARCH_SPW;
                const int       total   = mblocks + (int)((rest + per_rest - 1) / per_rest);
                const int       mg0     = rev ? total - 1 : 0;
                static_assert(WAVES == SELL_MARCH_WAVES && SELL_MARCH_MAPS[0].width == 5 && SELL_MARCH_MAPS[0].alias == 0x503u
                                  && sizeof(SELL_MARCH_MAPS) == sizeof(SellMarchMap),
                              "one kernel per entry of SELL_MARCH_MAPS");
                hipLaunchKernelGGL((sell_mv_short_march_kernel<T, 5, WAVES, SELL_MARCH_SPW, TAB, SELL_MARCH_G, 0x503u>), dim3((unsigned)total), block,
                                   0, s, m, nslices, mg0, gstep, dp, sval, v.col, v.lead, alpha, x, beta, y, nt, vtab, v.ucol, v.pbits, v.pbytes,
                                   pslo, pshi - pslo, pper, prcp, (unsigned)pstride * (unsigned)sizeof(T), mblocks, hp, mrcp, mskip);
                return true;
            }
        }
    }
    // the kernel's path: PK when the plan's table indices are packed words (a table of two always is: <= 8 cells of one bit), UCOL
    // when it also has uniform column lists (build_sell makes them next to packed words only); with both, for a real type, the kernel
    // that takes the periodic range
    auto launch = [&](auto wt, auto st, auto ut, auto pt) {
        if constexpr(decltype(ut)::value && decltype(pt)::value && TAB != 0 && !COMPLEX)
            hipLaunchKernelGGL((sell_mv_short_period_kernel<T, decltype(wt)::value, WAVES, decltype(st)::value, TAB>), grid, block, 0, s, m,
                               nslices, g0, gstep, dp, sval, v.col, v.lead, alpha, x, beta, y, nt, vtab, v.ucol, v.pbits, v.pbytes, pslo,
                               pshi - pslo, pper, prcp, (unsigned)pstride * (unsigned)sizeof(T));
        else
            hipLaunchKernelGGL((sell_mv_short_kernel<T, decltype(wt)::value, WAVES, decltype(st)::value, CONJ, TAB, decltype(ut)::value, decltype(pt)::value>),
                               grid, block, 0, s, m, nslices, g0, gstep, dp, sval, v.col, v.lead, alpha, x, beta, y, nt, vtab, v.ucol,
                               v.pbits, v.pbytes);
    };
    auto path = [&](auto wt, auto st) {
        if constexpr(TAB == 2)
            v.ucol ? launch(wt, st, std::true_type{}, std::true_type{}) : launch(wt, st, std::false_type{}, std::true_type{});
        else
        {
            if constexpr(TAB != 0)
                if(v.pbits)
                {
                    v.ucol ? launch(wt, st, std::true_type{}, std::true_type{}) : launch(wt, st, std::false_type{}, std::true_type{});
                    return;
                }
            launch(wt, st, std::false_type{}, std::false_type{}); // (values or one byte per cell: such a plan has no uniform lists)
        }
    };
#define MI355_SHORT_SPW(W, SPW) path(std::integral_constant<int, W>{}, std::integral_constant<int, SPW>{})
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
    switch((int)v.max_width)
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

} // namespace

template <typename T>
aoclsparse_status launch_sellmv(hipStream_t s, const SellView &v, int order, bool conj, T alpha, const T *x, T beta, T *y, int rev)
{
    constexpr bool COMPLEX = !std::is_floating_point_v<T>;
    if(v.m <= 0 || v.nslices <= 0)
        return aoclsparse_status_success;
    if(order < 0 || order > 2 || (v.pack != 1 && v.pack != 4))
        return aoclsparse_status_invalid_kid;
    if(COMPLEX ? (order != 0 || v.pack != 1 || v.ntab != 0) : conj)
        return aoclsparse_status_invalid_kid;
    const bool nt = (size_t)v.m * sizeof(T) > ((size_t)32 << 20);
    // one combination of the kernels' template arguments, each a std::integral_constant
    auto run = [&](auto o, auto p, auto sh, auto cj, auto ix) {
        constexpr int  ORDER = decltype(o)::value, PACK = decltype(p)::value;
        constexpr bool SHARED = decltype(sh)::value, CONJ = decltype(cj)::value, IDX = decltype(ix)::value;
        // the plan has slice records (build_sell: widest slice <= 8 cells, pack 1, a launch large enough that four slices per
        // workgroup still spread over every CU) and the order is the scalar one: the short-row kernel
        if constexpr(ORDER == 0 && PACK == 1)
        {
            if(v.desc)
            {
                bool done;
                if constexpr(!IDX)
                    done = sell_launch_short<T, 0, CONJ>(s, v, alpha, x, beta, y, nt, rev);
                else if(v.ntab <= 2)
                    done = sell_launch_short<T, 2, CONJ>(s, v, alpha, x, beta, y, nt, rev);
                else
                    done = sell_launch_short<T, SELL_VTAB_MAX, CONJ>(s, v, alpha, x, beta, y, nt, rev);
                if(done)
                    return;
            }
        }
        // one slice per workgroup while the launch is small (every slice its own CU), two otherwise
        // (swept on the headline workload: 1 / 2 / 4 / 8 slices per workgroup = 0.221 / 0.218 / 0.221 / 0.222 ms)
        const auto *cells = static_cast<const typename SellCell<T, IDX>::src *>(v.cells);
        const T    *vtab  = static_cast<const T *>(v.vtab);
        if(v.nslices < 2048)
            hipLaunchKernelGGL((sell_mv_kernel<T, ORDER, 1, PACK, SHARED, CONJ, IDX>), dim3(v.nslices), dim3(64), 0, s, v.m, v.nslices,
                               v.slice_ptr, cells, v.col, v.rowlen, alpha, x, beta, y, nt, v.cptr, v.lead, rev, vtab, v.pbits, v.pbytes);
        else
            hipLaunchKernelGGL((sell_mv_kernel<T, ORDER, 2, PACK, SHARED, CONJ, IDX>), dim3((v.nslices + 1) / 2), dim3(128), 0, s, v.m,
                               v.nslices, v.slice_ptr, cells, v.col, v.rowlen, alpha, x, beta, y, nt, v.cptr, v.lead, rev, vtab, v.pbits,
                               v.pbytes);
    };
    auto pick = [](bool b, auto f) { b ? f(std::true_type{}) : f(std::false_type{}); };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I4 = std::integral_constant<int, 4>;
    pick(v.cptr != nullptr, [&](auto sh) {
        if constexpr(COMPLEX)
            pick(conj, [&](auto cj) { run(I0{}, I1{}, sh, cj, std::false_type{}); });
        else
            pick(v.ntab != 0, [&](auto ix) {
                constexpr std::false_type cj{};
                switch(order * 2 + (v.pack == 4 ? 1 : 0))
                {
                case 0: run(I0{}, I1{}, sh, cj, ix); break;
                case 1: run(I0{}, I4{}, sh, cj, ix); break;
                case 2: run(I1{}, I1{}, sh, cj, ix); break;
                case 3: run(I1{}, I4{}, sh, cj, ix); break;
                case 4: run(I2{}, I1{}, sh, cj, ix); break;
                case 5: run(I2{}, I4{}, sh, cj, ix); break;
                }
            });
    });
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}
template aoclsparse_status launch_sellmv<double>(hipStream_t, const SellView &, int, bool, double, const double *, double, double *, int);
template aoclsparse_status launch_sellmv<float>(hipStream_t, const SellView &, int, bool, float, const float *, float, float *, int);
template aoclsparse_status launch_sellmv<cdouble>(hipStream_t, const SellView &, int, bool, cdouble, const cdouble *, cdouble, cdouble *, int);
template aoclsparse_status launch_sellmv<cfloat>(hipStream_t, const SellView &, int, bool, cfloat, const cfloat *, cfloat, cfloat *, int);

} // namespace mi355
