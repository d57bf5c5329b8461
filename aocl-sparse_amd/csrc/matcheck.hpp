// matcheck.hpp -- what matcheck_kernels.hip and the one step that launches it (device_mat_check, device_handle.hpp) share.
#ifndef MI355_MATCHECK_HPP_
#define MI355_MATCHECK_HPP_

#include "internal.hpp"

namespace mi355
{

// what the two check kernels leave behind; zeroed by launch_matcheck_ptr before its launch
struct MatCheckResult
{
    unsigned long long first_err; // ~((row << 8) | status) of the earliest offending row, 0: none (atomicMax of the complement)
    int                cls; // worst sort class of a row that is not fully sorted (0: every row is)
    unsigned int       notfull; // a row i < n without a diagonal entry
    unsigned int       ptr_bad; // launch 1: row_ptr is not a row pointer of nnz entries in this base
    unsigned int       pad;
};

// launch 1: row_ptr only (ptr[0] == base, ptr[m] - base == nnz, non-decreasing) -> ptr_bad
aoclsparse_status launch_matcheck_ptr(hipStream_t s, aoclsparse_int m, aoclsparse_int nnz, int base, const aoclsparse_int *d_ptr,
                                      MatCheckResult *d_out);
// launch 2: the scan of col_idx.  ONLY after launch 1's ptr_bad has been read back as 0: the row bounds are then inside [0, nnz]
aoclsparse_status launch_matcheck_rows(hipStream_t s, aoclsparse_int m, aoclsparse_int n, int base, const aoclsparse_int *d_ptr,
                                       const aoclsparse_int *d_ind, MatCheckResult *d_out);

} // namespace mi355

#endif
