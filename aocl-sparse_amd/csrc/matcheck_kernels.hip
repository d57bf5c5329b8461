// matcheck_kernels.hip -- validity, sort class and full-diagonal flag of CSR arrays that live in HBM (round 7).
//
// Reference: analysis/aoclsparse_csr_util.cpp:124-279 (aoclsparse_mat_check_internal), restated on the host as mat_check
// (matrix.cpp).  aoclsparse_mi355_create_?csr_device must answer exactly what mat_check answers for the same arrays: the status of
// the FIRST offending row (inside a row: whichever of a bad column index and a second diagonal entry comes first), the sort class
// 1 / 2 / 3 (fully sorted / L | D | U groups kept / unsorted) and whether every row i < n holds its diagonal.
//
// Two launches with a read-back between them (device_handle_api.cpp):
//   1. matcheck_ptr_kernel reads row_ptr ONLY: ptr[0] == base, ptr[m] - base == nnz, non-decreasing.  When all three hold, every
//      ptr[i] - base lies in [0, nnz].
//   2. matcheck_rows_kernel walks col_idx between those bounds -- launched only when 1. passed, so a bad row_ptr never becomes
//      an out-of-range load.
// Nothing is written but the 24-byte result record.
#include "matcheck.hpp"

#include <hip/hip_runtime.h>

#include <climits>

namespace mi355
{

namespace
{
    constexpr int MC_ROW_WAVE = 64; // rows longer than this are walked by their wavefront, not by one lane

    __global__ __launch_bounds__(256) void matcheck_ptr_kernel(aoclsparse_int m, aoclsparse_int nnz, int base,
                                                               const aoclsparse_int *__restrict__ ptr, MatCheckResult *out)
    {
        const long long i = (long long)blockIdx.x * 256 + threadIdx.x; // i in [0, m]: ptr has m + 1 entries
        bool            bad = false;
        if(i < m)
            bad = ptr[i] > ptr[i + 1];
        else if(i == m) // (unsigned: a wrapped difference is simply another value)
            bad = ptr[0] != base || (unsigned)ptr[m] - (unsigned)base != (unsigned)nnz;
        if(__ballot(bad) && (threadIdx.x & 63) == 0)
            atomicOr(&out->ptr_bad, 1u);
    }

    template <typename V>
    __device__ __forceinline__ V wave_min(V v)
    {
        for(int o = 32; o; o >>= 1)
            v = min(v, __shfl_xor(v, o, 64));
        return v;
    }
    template <typename V>
    __device__ __forceinline__ V wave_max(V v)
    {
        for(int o = 32; o; o >>= 1)
            v = max(v, __shfl_xor(v, o, 64));
        return v;
    }

    __global__ __launch_bounds__(256) void matcheck_rows_kernel(aoclsparse_int m, aoclsparse_int n, int base,
                                                                const aoclsparse_int *__restrict__ ptr,
                                                                const aoclsparse_int *__restrict__ ind, MatCheckResult *out)
    {
        const long long gi   = (long long)blockIdx.x * 256 + threadIdx.x;
        const bool      act  = gi < m;
        const int       i    = act ? (int)gi : 0;
        const int       lane = threadIdx.x & 63;
        const int       s = act ? ptr[i] - base : 0, e = act ? ptr[i + 1] - base : 0;
        const bool      lng = e - s > MC_ROW_WAVE;
        int             cls = 1, err = 0;
        bool            full = true;
        if(act && !lng) // a lane per row: mat_check's loop as it stands
        {
            bool seen_diag = false, seen_upper = false;
            int  prev = -1;
            for(int p = s; p < e && !err; p++)
            {
                const int j = ind[p] - base;
                if(j < 0 || j > n - 1)
                {
                    err = (int)aoclsparse_status_invalid_index_value;
                    break;
                }
                if(cls != 3)
                {
                    if(prev > j)
                        cls = 2;
                    else
                        prev = j;
                    if((j <= i && seen_upper) || (j < i && seen_diag))
                        cls = 3;
                }
                if(j > i)
                    seen_upper = true;
                else if(j == i)
                {
                    if(seen_diag)
                        err = (int)aoclsparse_status_invalid_value;
                    seen_diag = true;
                }
            }
            if(!seen_diag && i < n)
                full = false;
        }
        // A long row by its wavefront, lane l on entries s + l, s + l + 64, ...  The serial loop stops at the first position that
        // holds a bad index or the SECOND entry with j == i, so its status is that of min(first bad position, position of the second
        // diagonal) -- an out-of-range j is never counted as a diagonal, the range check comes first in the loop.  Without an error
        // every entry is visited, and the class is a statement about the whole row:
        //   cls >= 2  <=>  some entry is smaller than the largest before it (`prev` is a running maximum: it is not lowered on a
        //                  descent)  <=>  the row is not non-decreasing  <=>  an ADJACENT descent ind[p - 1] > ind[p] exists;
        //   cls == 3  <=>  an entry <= i follows an upper entry, or an entry < i follows the diagonal
        //             <=>  the LAST entry <= i lies behind the FIRST entry > i, or the LAST entry < i behind the FIRST entry == i
        // (seen_upper / seen_diag are raised after an entry's own test, hence "behind", not "at").  First and last positions, the two
        // smallest diagonal positions and the descent flag are reductions over the row.
        unsigned long long mask = __ballot(lng);
        while(mask)
        {
            const int l = __builtin_ctzll(mask);
            mask &= mask - 1;
            const int li = __builtin_amdgcn_readlane(i, l), ls = __builtin_amdgcn_readlane(s, l), le = __builtin_amdgcn_readlane(e, l);
            int  bad = INT_MAX, d1 = INT_MAX, d2 = INT_MAX, u1 = INT_MAX, last_le = -1, last_l = -1;
            bool desc = false;
            for(int p = ls + lane; p < le; p += 64) // (p grows: a lane meets its positions in order)
            {
                const int c = ind[p], j = c - base;
                if(p > ls && ind[p - 1] > c)
                    desc = true;
                if(j < 0 || j > n - 1)
                    bad = min(bad, p);
                else if(j > li)
                    u1 = min(u1, p);
                else
                {
                    last_le = p;
                    if(j < li)
                        last_l = p;
                    else if(d1 == INT_MAX)
                        d1 = p;
                    else if(d2 == INT_MAX)
                        d2 = p;
                }
            }
            bad = wave_min(bad), u1 = wave_min(u1), last_le = wave_max(last_le), last_l = wave_max(last_l);
            for(int o = 32; o; o >>= 1) // the two smallest of the union of two (smallest, second smallest) pairs
            {
                const int o1 = __shfl_xor(d1, o, 64), o2 = __shfl_xor(d2, o, 64);
                d2 = min(max(d1, o1), min(d2, o2));
                d1 = min(d1, o1);
            }
            const bool any_desc = __ballot(desc) != 0;
            int        r_err = 0, r_cls = 1;
            if(bad != INT_MAX || d2 != INT_MAX) // (never equal: a bad index is no diagonal)
                r_err = bad < d2 ? (int)aoclsparse_status_invalid_index_value : (int)aoclsparse_status_invalid_value;
            if(any_desc)
                r_cls = 2;
            if((u1 != INT_MAX && last_le > u1) || (d1 != INT_MAX && last_l > d1))
                r_cls = 3;
            if(lane == l)
                err = r_err, cls = r_cls, full = d1 != INT_MAX || li >= n;
        }
        // rows are independent: the earliest offending row decides the status, the worst class and any missing diagonal the rest
        if(err)
            atomicMax(&out->first_err, ~(((unsigned long long)i << 8) | (unsigned long long)err));
        const bool ok = act && !err;
        const unsigned long long b3 = __ballot(ok && cls == 3), b2 = __ballot(ok && cls == 2), nf = __ballot(ok && !full);
        if(lane == 0)
        {
            if(b3 | b2)
                atomicMax(&out->cls, b3 ? 3 : 2);
            if(nf)
                atomicOr(&out->notfull, 1u);
        }
    }
} // namespace

aoclsparse_status launch_matcheck_ptr(hipStream_t s, aoclsparse_int m, aoclsparse_int nnz, int base, const aoclsparse_int *d_ptr,
                                      MatCheckResult *d_out)
{
    MI355_HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(MatCheckResult), s));
    const unsigned grid = (unsigned)(((long long)m + 1 + 255) / 256);
    hipLaunchKernelGGL(matcheck_ptr_kernel, dim3(grid), dim3(256), 0, s, m, nnz, base, d_ptr, d_out);
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

// only after launch_matcheck_ptr's result has been read back as clean
aoclsparse_status launch_matcheck_rows(hipStream_t s, aoclsparse_int m, aoclsparse_int n, int base, const aoclsparse_int *d_ptr,
                                       const aoclsparse_int *d_ind, MatCheckResult *d_out)
{
    if(m <= 0)
        return aoclsparse_status_success;
    const unsigned grid = (unsigned)(((long long)m + 255) / 256);
    hipLaunchKernelGGL(matcheck_rows_kernel, dim3(grid), dim3(256), 0, s, m, n, base, d_ptr, d_ind, d_out);
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

} // namespace mi355
