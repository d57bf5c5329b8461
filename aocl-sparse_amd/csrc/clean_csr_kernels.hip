// clean_csr_kernels.hip -- the clean (full-diagonal, 0-based) copy of a CSR that lives in HBM, with idiag / iurow and the diagonal's
// values (round 24).
//
// Reference: analysis/aoclsparse_csr_util.hpp:765-967, restated on the host as csr_optimize / make_clean_copy / csr_indices
// (matrix.cpp).  aoclsparse_mi355_clean_csr_device (device_handle_api.cpp) must leave exactly what those leave: the rows' entries in
// the order they have in (ptr, ind, val) -- the caller has sorted a device copy first when the rows are not in L | D | U group order --
// and, in every row i < min(m, n) without a diagonal entry, an explicit zero in front of the row's first entry whose column is >= i
// (at the row's end when there is none).  Values are moved as items of 4, 8 or 16 bytes and never computed with; the inserted
// value is the all-zero item.
//
//   (1) cln_mark_kernel    per row: at[i] = the offset inside the row of the first entry with column >= i (the row length when
//                          there is none), miss[i] = 1 exactly when i < min(m, n) and that entry is not the diagonal, cnt[i] = the
//                          clean row length.  The search is the host's linear first match, not a binary search: rows in group order
//                          need not ascend.  Rows of up to AOCLSPARSE_MI355_CLEAN_ROW_WAVE entries take a lane each, longer ones
//                          are walked by their wavefront, 64 entries at a time, until a ballot finds the first match: one row may
//                          hold every entry.
//   (2) launch_spg_scan    (spgemm_kernels.hip) cnt -> the clean row pointer, with a 64-bit total.
//   (3) cln_expand_kernel  balanced over ENTRIES of the clean copy, 1,024 per workgroup whatever rows they belong to: a workgroup
//                          finds the rows of its first and last entry by binary search in the clean row pointer, every thread the
//                          row of its entry between the two; the entry is the inserted (i, 0) or comes from its source position
//                          (written out as well where the caller keeps value maps: csrc, -1 for an inserted entry).
//   (4) cln_finish_kernel  per row: idiag = clean_ptr + at, iurow = idiag + (the clean row holds a diagonal entry: i < min(m, n)),
//                          diag[i] = the diagonal's value, the zero item where it was inserted or i >= min(m, n).  For arrays that
//                          are clean already the "clean row pointer" is the matrix's own, and the two keep its base.
// No atomics at all, vector loads and stores only; no workgroup waits for another.
#include "internal.hpp"

#include <hip/hip_runtime.h>

#include <climits>

namespace mi355
{

namespace
{
    constexpr int CLN_ROW_WAVE = AOCLSPARSE_MI355_CLEAN_ROW_WAVE;
    constexpr int CLN_EXPAND   = 1024; // entries of the clean copy per workgroup of (3)

    struct alignas(16) Item16
    {
        unsigned long long a, b;
    };

    // the bounds of row i, clamped into [0, nnz] (the row pointer was checked before any of these kernels runs: the clamp costs nothing)
    __device__ __forceinline__ void cln_row(const aoclsparse_int *__restrict__ ptr, int i, int base, aoclsparse_int nnz, int &s, int &e)
    {
        s = min(max(ptr[i] - base, 0), nnz);
        e = min(max(ptr[i + 1] - base, s), nnz);
    }

    __global__ __launch_bounds__(256) void cln_mark_kernel(aoclsparse_int m, aoclsparse_int mn, aoclsparse_int nnz, int base,
                                                           const aoclsparse_int *__restrict__ ptr,
                                                           const aoclsparse_int *__restrict__ ind, int *__restrict__ at,
                                                           int *__restrict__ miss, int *__restrict__ cnt)
    {
        const long long gi   = (long long)blockIdx.x * 256 + threadIdx.x;
        const bool      act  = gi < m;
        const int       i    = act ? (int)gi : 0;
        const int       lane = threadIdx.x & 63;
        int             s = 0, e = 0;
        if(act)
            cln_row(ptr, i, base, nnz, s, e);
        const bool lng  = e - s > CLN_ROW_WAVE;
        int        a    = e - s; // no entry at or right of the diagonal: the row's end
        bool       diag = false;
        if(!lng) // a lane per row: csr_indices' loop as it stands
            for(int p = s; p < e; p++)
            {
                const int j = ind[p] - base;
                if(j >= i)
                {
                    a    = p - s;
                    diag = j == i;
                    break;
                }
            }
        // a long row by its wavefront: the first lane whose entry is at or right of the diagonal, in the first 64 entries that hold one
        unsigned long long mask = __ballot(lng);
        while(mask)
        {
            const int l = __builtin_ctzll(mask);
            mask &= mask - 1;
            const int li = __builtin_amdgcn_readlane(i, l), ls = __builtin_amdgcn_readlane(s, l), le = __builtin_amdgcn_readlane(e, l);
            int       ra = le - ls;
            bool      rd = false;
            for(int k = ls; k < le; k += 64) // (k, and with it the trip count, is the same on every lane)
            {
                const int                p   = k + lane;
                const int                j   = p < le ? ind[p] - base : INT_MIN;
                const unsigned long long hit = __ballot(j >= li);
                if(hit)
                {
                    const int f = __builtin_ctzll(hit);
                    ra          = k - ls + f;
                    rd          = __shfl(j, f, 64) == li;
                    break;
                }
            }
            if(lane == l)
                a = ra, diag = rd;
        }
        if(act)
        {
            const int ms = i < mn && !diag;
            at[i]        = a;
            miss[i]      = ms;
            cnt[i]       = e - s + ms;
        }
    }

    // the last row in [lo, hi] whose clean row pointer is <= q: the row that holds clean entry q when cptr[lo] <= q < cptr[hi + 1]
    // (empty rows in between share a pointer with the row behind them and are stepped over)
    __device__ __forceinline__ int cln_row_of(const aoclsparse_int *__restrict__ cptr, int lo, int hi, int q)
    {
        while(lo < hi)
        {
            const int mid = lo + (hi - lo + 1) / 2;
            if(cptr[mid] <= q)
                lo = mid;
            else
                hi = mid - 1;
        }
        return lo;
    }

    template <typename V>
    __global__ __launch_bounds__(256) void cln_expand_kernel(aoclsparse_int total, aoclsparse_int m, aoclsparse_int nnz, int base,
                                                             const aoclsparse_int *__restrict__ ptr,
                                                             const aoclsparse_int *__restrict__ ind, const V *__restrict__ val,
                                                             const aoclsparse_int *__restrict__ cptr, const int *__restrict__ at,
                                                             const int *__restrict__ miss, aoclsparse_int *__restrict__ cind,
                                                             V *__restrict__ cval, int *__restrict__ csrc)
    {
        __shared__ int  rows[2];
        const long long q0 = (long long)blockIdx.x * CLN_EXPAND; // (< total: the grid is ceil(total / CLN_EXPAND))
        if(threadIdx.x < 2)
            rows[threadIdx.x] = cln_row_of(cptr, 0, m - 1, (int)(threadIdx.x ? min(q0 + CLN_EXPAND, (long long)total) - 1 : q0));
        __syncthreads();
        const int r0 = rows[0], r1 = rows[1];
        for(int t = 0; t < CLN_EXPAND / 256; t++)
        {
            const long long ql = q0 + t * 256 + threadIdx.x;
            if(ql >= total)
                break;
            const int q = (int)ql, i = cln_row_of(cptr, r0, r1, q);
            const int k = q - cptr[i], a = at[i], ms = miss[i];
            if((ms && k == a) || nnz <= 0) // (without entries to copy every clean entry is an inserted one)
            {
                cind[q] = i;
                cval[q] = V{};
                if(csrc) // (the value map of a handle that keeps them: an inserted entry has no source)
                    csrc[q] = -1;
            }
            else
            {
                // (inside [0, nnz) for arrays that passed the checks; clamped like the row bounds)
                const int src = min(max(ptr[i] - base + k - (ms && k > a), 0), nnz - 1);
                cind[q]       = ind[src] - base;
                cval[q]       = val[src];
                if(csrc)
                    csrc[q] = src;
            }
        }
    }

    template <typename V>
    __global__ __launch_bounds__(256) void cln_finish_kernel(aoclsparse_int m, aoclsparse_int mn, aoclsparse_int nnz, int base,
                                                             const aoclsparse_int *__restrict__ ptr, const V *__restrict__ val,
                                                             const aoclsparse_int *__restrict__ cptr, const int *__restrict__ at,
                                                             const int *__restrict__ miss, aoclsparse_int *__restrict__ idiag,
                                                             aoclsparse_int *__restrict__ iurow, V *__restrict__ diag)
    {
        const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
        if(gi >= m)
            return;
        const int i = (int)gi, a = at[i];
        const int d = (cptr ? cptr[i] : ptr[i]) + a; // (the matrix's own row pointer keeps its base)
        idiag[i]    = d;
        iurow[i]    = d + (i < mn);
        V v{};
        if(i < mn && !miss[i] && nnz > 0)
            v = val[min(max(ptr[i] - base + a, 0), nnz - 1)];
        diag[i] = v;
    }

    // f(V{}) with V an item of vsize bytes
    template <typename F>
    aoclsparse_status by_item_size(size_t vsize, F &&f)
    {
        switch(vsize)
        {
        case 4:
            f((unsigned int)0);
            break;
        case 8:
            f((unsigned long long)0);
            break;
        case 16:
            f(Item16{});
            break;
        default:
            return aoclsparse_status_not_implemented;
        }
        return aoclsparse_status_success;
    }
} // namespace

aoclsparse_status launch_clean_mark(hipStream_t s, aoclsparse_int m, aoclsparse_int n, aoclsparse_int nnz, int base,
                                    const aoclsparse_int *d_ptr, const aoclsparse_int *d_ind, int *at, int *miss, int *cnt)
{
    if(m > 0)
        hipLaunchKernelGGL(cln_mark_kernel, dim3((unsigned)(((long long)m + 255) / 256)), dim3(256), 0, s, m, std::min(m, n), nnz, base,
                           d_ptr, d_ind, at, miss, cnt);
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

aoclsparse_status launch_clean_expand(hipStream_t s, aoclsparse_int m, aoclsparse_int nnz, aoclsparse_int total, int base,
                                      const aoclsparse_int *d_ptr, const aoclsparse_int *d_ind, const void *d_val, size_t vsize,
                                      const aoclsparse_int *cptr, const int *at, const int *miss, aoclsparse_int *cind, void *cval,
                                      int *csrc)
{
    if(m <= 0 || total <= 0)
        return aoclsparse_status_success;
    const unsigned    grid = (unsigned)(((long long)total + CLN_EXPAND - 1) / CLN_EXPAND);
    aoclsparse_status st   = by_item_size(vsize, [&](auto v) {
        using V = decltype(v);
        hipLaunchKernelGGL((cln_expand_kernel<V>), dim3(grid), dim3(256), 0, s, total, m, nnz, base, d_ptr, d_ind,
                           static_cast<const V *>(d_val), cptr, at, miss, cind, static_cast<V *>(cval), csrc);
    });
    if(st != aoclsparse_status_success)
        return st;
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

aoclsparse_status launch_clean_finish(hipStream_t s, aoclsparse_int m, aoclsparse_int n, aoclsparse_int nnz, int base,
                                      const aoclsparse_int *d_ptr, const void *d_val, size_t vsize, const aoclsparse_int *cptr,
                                      const int *at, const int *miss, aoclsparse_int *idiag, aoclsparse_int *iurow, void *diag)
{
    if(m <= 0)
        return aoclsparse_status_success;
    const unsigned    grid = (unsigned)(((long long)m + 255) / 256);
    aoclsparse_status st   = by_item_size(vsize, [&](auto v) {
        using V = decltype(v);
        hipLaunchKernelGGL((cln_finish_kernel<V>), dim3(grid), dim3(256), 0, s, m, std::min(m, n), nnz, base, d_ptr,
                           static_cast<const V *>(d_val), cptr, at, miss, idiag, iurow, static_cast<V *>(diag));
    });
    if(st != aoclsparse_status_success)
        return st;
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

} // namespace mi355
