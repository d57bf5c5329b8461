// device_handle.hpp -- the steps device_handle_api.cpp takes more than once, each written here once.
#ifndef MI355_DEVICE_HANDLE_HPP_
#define MI355_DEVICE_HANDLE_HPP_

#include "matcheck.hpp"

namespace mi355
{

// the first failure of a run of HIP calls and launches; what must not follow a failure is skipped by the caller's `if(e.ok())`
struct FirstError
{
    aoclsparse_status rc = aoclsparse_status_success;
    bool              ok() const { return rc == aoclsparse_status_success; }
    void              hip(hipError_t e) { status(e == hipSuccess ? aoclsparse_status_success : aoclsparse_status_internal_error); }
    void              status(aoclsparse_status st) { rc = ok() ? st : rc; }
};

// On the way out, unless dismissed: the stream finishes what was enqueued (nothing is in flight into buffers that go next) and the
// error is cleared (a failed launch or copy is reported by this call's status, not by the next call's).  Declared AFTER the
// buffers it protects, so that it runs before they are released.
struct StreamDrain
{
    hipStream_t s;
    bool        armed = true;
    void        dismiss() { armed = false; }
    ~StreamDrain()
    {
        if(armed)
            (void)hipStreamSynchronize(s), (void)hipGetLastError();
    }
};

// AOCLSPARSE_MI355_TIMING=1: where a call's time goes.  lap() is for a point the host has already waited at; synced() waits for the
// stream first, under the switch only, so that the lap holds the work enqueued in it.
struct StreamLaps
{
    hipStream_t s;
    bool        on = PhaseTimer::on();
    LapTimer    lt{};
    void        lap(const char *what) { if(on) lt.lap(what); }
    hipError_t  synced(const char *what)
    {
        const hipError_t e = on ? hipStreamSynchronize(s) : hipSuccess;
        return lap(what), e;
    }
};

// mat_check's answer over CSR arrays in HBM (matcheck_kernels.hip): the row pointer first, and the scan of col_idx only when it
// passed -- its bounds come from this row_ptr.  ptr_checked: the row pointer was accepted before (the rows half alone).  The
// status is that of the launches and copies; what the kernels found is in `h`, for matcheck_status or for the caller to weigh.
inline aoclsparse_status device_mat_check(hipStream_t s, aoclsparse_int m, aoclsparse_int n, aoclsparse_int nnz, int base,
                                          const aoclsparse_int *d_ptr, const aoclsparse_int *d_ind, MatCheckResult &h,
                                          bool ptr_checked = false)
{
    DeviceBuffer res;
    MI355_TRY(res.alloc(sizeof(MatCheckResult)));
    MatCheckResult *d_res = res.as<MatCheckResult>();
    h                     = MatCheckResult{};
    if(ptr_checked)
        MI355_HIP_TRY(hipMemsetAsync(d_res, 0, sizeof(MatCheckResult), s));
    else
    {
        MI355_TRY(launch_matcheck_ptr(s, m, nnz, base, d_ptr, d_res));
        MI355_HIP_TRY(hipMemcpyAsync(&h, d_res, sizeof(h), hipMemcpyDeviceToHost, s));
        MI355_HIP_TRY(hipStreamSynchronize(s));
        if(h.ptr_bad)
            return aoclsparse_status_success;
    }
    MI355_TRY(launch_matcheck_rows(s, m, n, base, d_ptr, d_ind, d_res));
    MI355_HIP_TRY(hipMemcpyAsync(&h, d_res, sizeof(h), hipMemcpyDeviceToHost, s));
    MI355_HIP_TRY(hipStreamSynchronize(s));
    return aoclsparse_status_success;
}

// ... as the status mat_check returns: that of the earliest offending row
inline aoclsparse_status matcheck_status(const MatCheckResult &h)
{
    if(h.ptr_bad)
        return aoclsparse_status_invalid_value;
    return h.first_err ? (aoclsparse_status)(~h.first_err & 0xff) : aoclsparse_status_success;
}

// The handle's CSR, resident: a mirror that is not resident (a host-created handle before its first product) or not valid
// (?set_value, aoclsparse_order_mat, aoclsparse_mi355_invalidate) comes from the host view first; nothing else of the handle
// changes.  Called with the stage lock and the handle's guard held.
inline aoclsparse_status resident_mirror(aoclsparse_matrix A)
{
    DeviceCsr &d = A->dev_user;
    if(!d.valid)
        MI355_TRY(upload_csr(A->user, val_size(A->val_type), d));
    const bool shaped = d.m == A->user.m && d.nnz == A->nnz && d.ptr.ptr && d.ind.ptr && d.val.ptr;
    return shaped ? aoclsparse_status_success : aoclsparse_status_internal_error;
}

} // namespace mi355

#endif
