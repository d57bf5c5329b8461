// device_handle_api.cpp -- matrix handles whose CSR arrays are already in HBM (round 7): create, update the values, export.
//
// The reference has no counterpart (a CPU library has one address space).  Until round 7 a matrix entered the library through host
// arrays only (aoclsparse_create_?csr aliases them, the first product uploads them), so a matrix assembled on the GPU crossed PCIe
// twice.  The three groups here keep the design of aoclsparse_mi355_mm_state_adopt (comm_api.cpp): the caller's device arrays are
// COPIED into the handle's device mirror (dev_user), the handle gets an owned host view (`user`) by one copy back, and from then on
// every entry point of the library works on it unchanged -- some 280 of them read A->user.  No aliasing, no handle without host
// arrays.  What mat_check decides on the host for aoclsparse_create_?csr (validity, sort class, full diagonal) is decided by
// matcheck_kernels.hip on the device.
//
// Round 19 adds the way in for a matrix that is not CSR yet: unordered (row, col, value) triplets in HBM are sorted into CSR
// arrays on the device (coo_sort_kernels.hip), and those arrays -- the library's own -- are MOVED into the mirror by the same
// helper that copies a caller's.
//
// Round 22: a creation from triplets may keep the sort's map on the handle (aoclsparse_mi355_coo_keep_map), and
// ?refresh_values_from_coo_device then brings the values of the same triplets again without sorting: what ?update_values_device
// does with values in CSR order, behind one kernel that puts them into that order (or adds them into it).
//
// Round 23: aoclsparse_mi355_order_mat_device is aoclsparse_order_mat with the sort done on the mirror (order_kernels.hip) and the
// handle resident afterwards.
//
// Round 24: aoclsparse_mi355_clean_csr_device is csr_optimize (matrix.cpp) with the work done on the mirror
// (clean_csr_kernels.hip): the clean CSR, idiag / iurow and the diagonal's values, committed after one copy back.
#include "matcheck.hpp"

#include <cstring>
#include <limits>

using namespace mi355;

namespace
{
    // From CSR arrays in HBM to a handle: the check kernels, the device mirror, the host view.  The arrays are the caller's (own ==
    // nullptr: copied device to device into the mirror) or the library's own, built a moment ago (own[0..2] hold row_ptr, col_idx
    // and val: MOVED into the mirror -- a copy of 1 GB is for a caller's arrays, not for ours).  *mat is null on entry.
    aoclsparse_status csr_handle_from_device(aoclsparse_matrix *mat, aoclsparse_index_base base, aoclsparse_int M, aoclsparse_int N,
                                             aoclsparse_int nnz, const aoclsparse_int *row_ptr, const aoclsparse_int *col_idx,
                                             const void *val, aoclsparse_matrix_data_type vt, DeviceBuffer *own)
    {
        Runtime                              &rt = Runtime::get();
        aoclsparse_status                     rc;
        const size_t                          vsz = val_size(vt);
        std::lock_guard<std::recursive_mutex> sl(rt.stage_lock); // (one user of the library's stream at a time, as everywhere)
        hipStream_t                           s = rt.stream();
        // any base is checked like mat_check checks it: against ptr[0], and every index after subtracting it
        LapTimer     lt; // (AOCLSPARSE_MI355_TIMING=1: where a creation's time goes)
        DeviceBuffer res;
        if((rc = res.alloc(sizeof(MatCheckResult))) != aoclsparse_status_success)
            return rc;
        MatCheckResult *d_res = res.as<MatCheckResult>(), h{};
        if((rc = launch_matcheck_ptr(s, M, nnz, (int)base, row_ptr, d_res)) != aoclsparse_status_success)
            return rc;
        MI355_HIP_TRY(hipMemcpyAsync(&h, d_res, sizeof(h), hipMemcpyDeviceToHost, s));
        MI355_HIP_TRY(hipStreamSynchronize(s));
        if(h.ptr_bad)
            return aoclsparse_status_invalid_value; // col_idx is not looked at: its bounds would come from this row_ptr
        if((rc = launch_matcheck_rows(s, M, N, (int)base, row_ptr, col_idx, d_res)) != aoclsparse_status_success)
            return rc;
        MI355_HIP_TRY(hipMemcpyAsync(&h, d_res, sizeof(h), hipMemcpyDeviceToHost, s));
        MI355_HIP_TRY(hipStreamSynchronize(s));
        if(h.first_err)
            return (aoclsparse_status)(~h.first_err & 0xff);
        lt.lap("create_device: check kernels");

        aoclsparse_matrix H = nullptr;
        if((rc = new_csr_result(&H, M, N, nnz, vt, nullptr, base)) != aoclsparse_status_success)
            return rc;
        H->sort = h.cls ? h.cls : 1, H->fulldiag = !h.notfull;
        // the device mirror (a copy of the caller's arrays, or the library's own buffers moved in) and the host view
        DeviceCsr   &d  = H->dev_user;
        const size_t pb = sizeof(aoclsparse_int) * ((size_t)M + 1), ib = sizeof(aoclsparse_int) * (size_t)nnz, vb = vsz * (size_t)nnz;
        auto copy = [&](void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
            if(rc == aoclsparse_status_success && bytes && hipMemcpyAsync(dst, src, bytes, kind, s) != hipSuccess)
                rc = aoclsparse_status_internal_error;
        };
        if(own)
            d.ptr.adopt(own[0]), d.ind.adopt(own[1]), d.val.adopt(own[2]); // (row_ptr, col_idx and val point into them still)
        else
        {
            rc = d.ptr.alloc(pb);
            if(rc == aoclsparse_status_success)
                rc = d.ind.alloc(ib);
            if(rc == aoclsparse_status_success)
                rc = d.val.alloc(vb);
            copy(d.ptr.ptr, row_ptr, pb, hipMemcpyDeviceToDevice);
            copy(d.ind.ptr, col_idx, ib, hipMemcpyDeviceToDevice);
            copy(d.val.ptr, val, vb, hipMemcpyDeviceToDevice);
        }
        if(PhaseTimer::on() && rc == aoclsparse_status_success) // (the diagnostic separates the two directions)
            (void)hipStreamSynchronize(s);
        lt.lap("create_device: handle + device copy");
        copy(H->user.ptr, row_ptr, pb, hipMemcpyDeviceToHost);
        if(rc == aoclsparse_status_success && nnz > 0)
        {
            host_result_touch(H->user.ind, ib); // (fresh arrays: see host_result_alloc)
            host_result_touch(H->user.val, vb);
        }
        copy(H->user.ind, col_idx, ib, hipMemcpyDeviceToHost);
        copy(H->user.val, val, vb, hipMemcpyDeviceToHost);
        if(rc == aoclsparse_status_success && hipStreamSynchronize(s) != hipSuccess) // the caller may overwrite or free its arrays now
            rc = aoclsparse_status_internal_error;
        if(rc != aoclsparse_status_success)
        {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(s); // (nothing in flight into the handle's arrays when they go)
            aoclsparse_destroy(&H);
            return rc;
        }
        lt.lap("create_device: host view");
        d.m = M, d.n = N, d.nnz = nnz, d.base = base;
        d.valid = true; // (the row-block plan is built from the host view at the first product, as for every handle)
        *mat    = H;
        return aoclsparse_status_success;
    }

    template <typename T>
    aoclsparse_status create_csr_device(aoclsparse_matrix *mat, aoclsparse_index_base base, aoclsparse_int M, aoclsparse_int N,
                                        aoclsparse_int nnz, const aoclsparse_int *row_ptr, const aoclsparse_int *col_idx,
                                        const T *val, aoclsparse_matrix_data_type vt)
    {
        // decided before the device is touched, in the order of create_csr / mat_check (matrix.cpp)
        if(!mat)
            return aoclsparse_status_invalid_pointer;
        *mat = nullptr;
        if(!row_ptr || !col_idx || !val)
            return aoclsparse_status_invalid_pointer;
        if(N < 0 || M < 0 || nnz < 0)
            return aoclsparse_status_invalid_size;
        Runtime          &rt = Runtime::get();
        aoclsparse_status rc = rt.init();
        if(rc != aoclsparse_status_success)
            return rc;
        if(!rt.is_device_pointer(row_ptr) || !rt.is_device_pointer(col_idx) || !rt.is_device_pointer(val))
            return aoclsparse_status_invalid_pointer;
        return csr_handle_from_device(mat, base, M, N, nnz, row_ptr, col_idx, val, vt, nullptr);
    }

    // triplets in HBM -> CSR arrays in HBM (coo_sort_kernels.hip) -> handle
    template <typename T>
    aoclsparse_status create_csr_from_coo_device(aoclsparse_matrix *mat, aoclsparse_index_base base, aoclsparse_int M, aoclsparse_int N,
                                                 aoclsparse_int nnz, const aoclsparse_int *row_ind, const aoclsparse_int *col_ind,
                                                 const T *val, aoclsparse_int duplicates, aoclsparse_matrix_data_type vt)
    {
        // decided before the device is touched, in the order of create_coo (formats_api.cpp): sizes come before arrays there
        if(!mat)
            return aoclsparse_status_invalid_pointer;
        *mat = nullptr;
        if(M < 0 || N < 0 || nnz < 0)
            return aoclsparse_status_invalid_size;
        if(!row_ind || !col_ind || !val)
            return aoclsparse_status_invalid_pointer;
        const aoclsparse_int mode = duplicates & ~(aoclsparse_int)aoclsparse_mi355_coo_keep_map; // 0, 1, 16 and 17 are valid
        if(mode != aoclsparse_mi355_coo_keep && mode != aoclsparse_mi355_coo_sum)
            return aoclsparse_status_invalid_value;
        const bool keep_map = (duplicates & aoclsparse_mi355_coo_keep_map) != 0;
        Runtime          &rt = Runtime::get();
        aoclsparse_status rc = rt.init();
        if(rc != aoclsparse_status_success)
            return rc;
        if(!rt.is_device_pointer(row_ind) || !rt.is_device_pointer(col_ind) || !rt.is_device_pointer(val))
            return aoclsparse_status_invalid_pointer;
        std::lock_guard<std::recursive_mutex> sl(rt.stage_lock);
        LapTimer                              lt;
        DeviceBuffer                          own[3], map[2];
        aoclsparse_int                        nnz_csr = 0;
        const bool                            cplx    = vt == aoclsparse_cmat || vt == aoclsparse_zmat;
        rc = device_coo_to_csr(rt.stream(), M, N, nnz, (int)base, row_ind, col_ind, val, sizeof(T), cplx,
                               mode == aoclsparse_mi355_coo_sum, own[0], own[1], own[2], &nnz_csr, keep_map ? map : nullptr);
        if(rc != aoclsparse_status_success)
            return rc;
        lt.lap("create_from_coo_device: sort");
        rc = csr_handle_from_device(mat, base, M, N, nnz_csr, own[0].as<const aoclsparse_int>(), own[1].as<const aoclsparse_int>(),
                                    own[2].ptr, vt, own);
        if(rc == aoclsparse_status_success && keep_map) // the sort's map hangs on the handle from here on
        {
            aoclsparse_matrix H = *mat;
            H->coo_pos.adopt(map[0]), H->coo_runs.adopt(map[1]);
            H->coo_map_kept = true, H->coo_map_mode = mode, H->coo_map_triplets = nnz;
        }
        return rc;
    }

    // the values of a handle that kept its sort's map, again, from the triplets' new values (coo_sort_kernels.hip)
    template <typename T>
    aoclsparse_status refresh_values_from_coo_device(aoclsparse_matrix A, aoclsparse_int len, const T *val, aoclsparse_matrix_data_type vt)
    {
        // decided before the device is touched, in this order
        if(!A || !val)
            return aoclsparse_status_invalid_pointer;
        if(!A->coo_map_kept)
            return aoclsparse_status_invalid_value;
        if(len != A->coo_map_triplets)
            return aoclsparse_status_invalid_size;
        if(A->val_type != vt)
            return aoclsparse_status_wrong_type;
        Runtime          &rt = Runtime::get();
        aoclsparse_status rc = rt.init();
        if(rc != aoclsparse_status_success)
            return rc;
        if(!rt.is_device_pointer(val))
            return aoclsparse_status_invalid_pointer;
        std::lock_guard<std::recursive_mutex> sl(rt.stage_lock); // (before the handle's guard, as everywhere)
        std::unique_lock<std::shared_mutex>   w(A->guard);
        // (looked at again under the guard: aoclsparse_order_mat on another thread releases the map)
        if(!A->coo_map_kept || !A->user.val || !A->coo_pos.ptr)
            return aoclsparse_status_invalid_value;
        if(len != A->coo_map_triplets)
            return aoclsparse_status_invalid_size;
        const bool sum = A->coo_map_mode == aoclsparse_mi355_coo_sum;
        if(sum ? !A->coo_runs.ptr || A->coo_runs.bytes < sizeof(int) * ((size_t)A->nnz + 1) : A->nnz != len)
            return aoclsparse_status_internal_error;
        hipStream_t  s     = rt.stream();
        const size_t bytes = sizeof(T) * (size_t)A->nnz;
        DeviceCsr   &d     = A->dev_user;
        // as update_values_device: the values go into the resident copy while the mirror is the handle's structure, and it stays
        // resident; behind an invalid mirror (?set_value, ?update_values, aoclsparse_mi355_invalidate) they go through a buffer of
        // this call's, and the next product uploads the host view as it would have anyway
        const bool   keep = d.valid && d.m == A->m && d.nnz == A->nnz && d.ptr.ptr && d.ind.ptr && d.val.ptr && d.val.bytes >= bytes;
        DeviceBuffer tmp;
        if(!keep && (rc = tmp.alloc(bytes)) != aoclsparse_status_success)
            return rc;
        void *const out = keep ? d.val.ptr : tmp.ptr;
        const bool  cplx = vt == aoclsparse_cmat || vt == aoclsparse_zmat;
        // (in stream order behind every product enqueued on the library's stream: they read the old values)
        rc = device_coo_refresh_values(s, len, A->nnz, sum, A->coo_pos.as<const int>(), A->coo_runs.as<const int>(), val, sizeof(T), cplx,
                                       out);
        if(rc == aoclsparse_status_success && bytes && hipMemcpyAsync(A->user.val, out, bytes, hipMemcpyDeviceToHost, s) != hipSuccess)
            rc = aoclsparse_status_internal_error;
        if(hipStreamSynchronize(s) != hipSuccess && rc == aoclsparse_status_success) // (`tmp` goes only behind the work that reads it)
            rc = aoclsparse_status_internal_error;
        drop_derived_state(A); // SELL-64 / blocked-ELL copies, TRSV plans, derived operators, replicas: rebuilt lazily
        d.valid = keep && rc == aoclsparse_status_success;
        if(rc != aoclsparse_status_success)
            (void)hipGetLastError();
        return rc;
    }

    // what ?update_values_device and ?revalue_device decide before the device is touched: the statuses of update_values
    // (matrix.cpp), in its order, then the runtime and the kind of pointer
    aoclsparse_status check_update_values_device(aoclsparse_matrix A, aoclsparse_int len, const void *val, aoclsparse_matrix_data_type vt)
    {
        const bool coo = A && A->input_format == aoclsparse_coo_mat, nocsr = A && holds_no_csr(A);
        if(!A || !val || (coo ? !A->coo_val : (!nocsr && !A->user.ptr)))
            return aoclsparse_status_invalid_pointer;
        if(len != A->nnz)
            return aoclsparse_status_invalid_size;
        if(A->val_type != vt)
            return aoclsparse_status_wrong_type;
        if(nocsr) // TCSR and BSR handles
            return aoclsparse_status_not_implemented;
        // ... and the handles whose first representation is not the CSR in `user`: their values follow the order of the caller's
        // COO / CSC arrays, which live on the host
        if(coo || A->csc_ptr)
            return aoclsparse_status_not_implemented;
        if(!A->user.val)
            return aoclsparse_status_invalid_pointer;
        Runtime          &rt = Runtime::get();
        aoclsparse_status rc = rt.init();
        if(rc != aoclsparse_status_success)
            return rc;
        if(!rt.is_device_pointer(val))
            return aoclsparse_status_invalid_pointer;
        return aoclsparse_status_success;
    }

    template <typename T>
    aoclsparse_status update_values_device(aoclsparse_matrix A, aoclsparse_int len, const T *val, aoclsparse_matrix_data_type vt)
    {
        aoclsparse_status rc = check_update_values_device(A, len, val, vt);
        if(rc != aoclsparse_status_success)
            return rc;
        Runtime                              &rt = Runtime::get();
        std::lock_guard<std::recursive_mutex> sl(rt.stage_lock); // (before the handle's guard, as everywhere)
        std::unique_lock<std::shared_mutex>   w(A->guard);
        hipStream_t                           s     = rt.stream();
        const size_t                          bytes = sizeof(T) * (size_t)len;
        DeviceCsr                            &d     = A->dev_user;
        // the mirror's row pointers and columns are the handle's structure exactly while the mirror is valid (aoclsparse_order_mat
        // reorders the host arrays and leaves stale buffers behind an invalid mirror): only then do the values alone travel
        const bool keep = d.valid && d.m == A->m && d.nnz == A->nnz && d.ptr.ptr && d.ind.ptr && d.val.ptr && d.val.bytes >= bytes;
        if(bytes)
        {
            // (in stream order behind every product enqueued on the library's stream: they read the old values)
            MI355_HIP_TRY(hipMemcpyAsync(A->user.val, val, bytes, hipMemcpyDeviceToHost, s));
            if(keep && val != d.val.ptr)
                MI355_HIP_TRY(hipMemcpyAsync(d.val.ptr, val, bytes, hipMemcpyDeviceToDevice, s));
            MI355_HIP_TRY(hipStreamSynchronize(s));
        }
        drop_derived_state(A); // SELL-64 / blocked-ELL copies, TRSV plans, derived operators, replicas: rebuilt lazily
        d.valid = keep;
        return aoclsparse_status_success;
    }

    // ?update_values_device that keeps what holds a value map (round 25): the clean CSR, the diagonal and the TRSV plans get the
    // new values through their maps (revalue_kernels.hip) instead of being dropped and analysed again.  What has no map goes as
    // it goes there.
    template <typename T>
    aoclsparse_status revalue_device(aoclsparse_matrix A, aoclsparse_int len, const T *val, aoclsparse_matrix_data_type vt)
    {
        aoclsparse_status rc = check_update_values_device(A, len, val, vt);
        if(rc != aoclsparse_status_success)
            return rc;
        Runtime                              &rt = Runtime::get();
        std::lock_guard<std::recursive_mutex> sl(rt.stage_lock); // (before the handle's guard, as everywhere)
        std::unique_lock<std::shared_mutex>   w(A->guard);
        hipStream_t                           s     = rt.stream();
        const size_t                          vsz   = sizeof(T);
        const size_t                          bytes = vsz * (size_t)len;
        DeviceCsr                            &d     = A->dev_user;
        const bool keep = d.valid && d.m == A->m && d.nnz == A->nnz && d.ptr.ptr && d.ind.ptr && d.val.ptr && d.val.bytes >= bytes;
        LapTimer   lt; // (AOCLSPARSE_MI355_TIMING=1: where a revalue's time goes; the laps then wait for the stream)
        auto       hip = [&](hipError_t e) {
            if(e != hipSuccess && rc == aoclsparse_status_success)
                rc = aoclsparse_status_internal_error;
        };
        auto lap = [&](const char *what) {
            if(PhaseTimer::on() && rc == aoclsparse_status_success)
                hip(hipStreamSynchronize(s));
            lt.lap(what);
        };
        // what can follow: the clean CSR when it is the handle's own arrays or a copy that holds its map ...
        HostCsr *const       o          = A->opt;
        const bool           clean_copy = o && o != &A->user;
        const aoclsparse_int total      = o ? o->nnz : 0; // entries of the clean CSR
        const bool           clean_ok   = o && (!clean_copy || (o == A->opt_copy.get() && o->val && A->clean_src.ptr
                                                      && A->clean_src.bytes >= sizeof(int) * (size_t)total));
        // ... the diagonal when it has its map, and with it the plans whose layouts all have theirs
        const size_t mrows   = (size_t)std::max<aoclsparse_int>(A->m, 1);
        const bool   diag_ok = clean_ok && A->dev_diag.ptr && A->diag_src.ptr && A->diag_src.bytes >= sizeof(int) * mrows
                             && A->dev_diag.bytes >= vsz * (size_t)A->m;
        unsigned keep_plans = 0;
        int      kept       = 0;
        if(diag_ok)
            for(int i = 0; i < 6; i++)
            {
                const TrsvPlan &p  = A->trsv_plan[i];
                const size_t    ne = (size_t)std::max<aoclsparse_int>(p.nnz_tri, 0);
                if(p.value_mapped() && (!p.rows_valid || (p.psrc.bytes >= sizeof(int) * ne && p.pval.bytes >= vsz * ne))
                   && (!p.blk.valid || (p.blk.psrc.bytes >= sizeof(int) * ne && p.blk.pval.bytes >= vsz * ne)))
                    keep_plans |= 1u << i, kept++;
            }
        DeviceBuffer cval; // the clean copy's new values, for the gathers below and the copy back
        if(clean_ok && clean_copy && total > 0 && (rc = cval.alloc(vsz * (size_t)total)) != aoclsparse_status_success)
            return rc; // (nothing written yet: the handle is as it was)
        // -- from here on the handle is written.  In stream order behind every product and solve enqueued on the library's stream.
        if(bytes)
        {
            hip(hipMemcpyAsync(A->user.val, val, bytes, hipMemcpyDeviceToHost, s));
            if(keep && val != d.val.ptr)
                hip(hipMemcpyAsync(d.val.ptr, val, bytes, hipMemcpyDeviceToDevice, s));
        }
        lap("revalue_device: values to host view + mirror");
        // the diagnostic also times the gather kernels by device events: [0, 1] around the clean gather, [2, 3] around the
        // diagonal's and the plans' (no host synchronisation in between either way)
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        if(PhaseTimer::on())
            for(hipEvent_t &e : ev)
                if(hipEventCreate(&e) != hipSuccess)
                    e = nullptr;
        auto mark = [&](int i) {
            if(ev[i] && rc == aoclsparse_status_success)
                hip(hipEventRecord(ev[i], s));
        };
        const void *clean_vals = val; // the clean CSR's value array in HBM: the new values themselves, or the gathered copy
        long long   clean_n    = len;
        if(clean_ok && clean_copy)
        {
            mark(0);
            if(rc == aoclsparse_status_success)
                rc = launch_revalue_gather(s, total, len, A->clean_src.as<const int>(), val, cval.ptr, vsz, false);
            mark(1);
            if(rc == aoclsparse_status_success && total > 0)
                hip(hipMemcpyAsync(o->val, cval.ptr, vsz * (size_t)total, hipMemcpyDeviceToHost, s));
            clean_vals = cval.ptr, clean_n = total;
            lap("revalue_device: clean gather + copy back");
        }
        mark(2);
        if(diag_ok && rc == aoclsparse_status_success)
            rc = launch_revalue_gather(s, A->m, clean_n, A->diag_src.as<const int>(), clean_vals, A->dev_diag.ptr, vsz, false);
        for(int i = 0; i < 6 && rc == aoclsparse_status_success; i++)
        {
            if(!(keep_plans >> i & 1u))
                continue;
            TrsvPlan &p = A->trsv_plan[i];
            if(p.rows_valid)
                rc = launch_revalue_gather(s, p.nnz_tri, clean_n, p.psrc.as<const int>(), clean_vals, p.pval.ptr, vsz, p.conj);
            if(p.blk.valid && rc == aoclsparse_status_success)
                rc = launch_revalue_gather(s, p.nnz_tri, clean_n, p.blk.psrc.as<const int>(), clean_vals, p.blk.pval.ptr, vsz, p.conj);
        }
        mark(3);
        // the one wait: the copies back have landed, `cval` and the caller's array are no longer read
        if(hipStreamSynchronize(s) != hipSuccess && rc == aoclsparse_status_success)
            rc = aoclsparse_status_internal_error;
        lt.lap("revalue_device: diagonal + plan gathers");
        for(int i = 0; i < 4; i += 2)
        {
            float ms = 0.0f;
            if(rc == aoclsparse_status_success && ev[i] && ev[i + 1] && (i == 2 || (clean_ok && clean_copy))
               && hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess)
                std::fprintf(stderr, "[mi355 timing]     %-30s %8.3f ms\n",
                             i ? "revalue_device: plan gather events" : "revalue_device: clean gather events", ms);
        }
        for(hipEvent_t e : ev)
            if(e)
                (void)hipEventDestroy(e);
        if(rc != aoclsparse_status_success)
        {
            // what ?update_values_device leaves: everything dropped, no plan with some old and some new values; the maps go too.
            // The mirror may hold either values: the next product uploads the host view.
            (void)hipGetLastError();
            (void)hipStreamSynchronize(s);
            drop_derived_state(A);
            A->drop_value_maps();
            d.valid = false;
            return rc;
        }
        drop_derived_state_keeping(A, clean_ok, keep_plans); // SELL-64 / blocked-ELL copies, transposes, derived operators, replicas
        if(!diag_ok) // (a diagonal without its map: ensure_trsv gathers it again; no plan was kept)
            A->dev_diag.release(), A->diag_src.release();
        d.valid = keep;
        A->revalues++, A->last_kept_plans = kept;
        return aoclsparse_status_success;
    }
} // namespace

namespace mi355
{
aoclsparse_status revalue_device_any(aoclsparse_matrix A, aoclsparse_int len, const void *val)
{
    if(!A)
        return aoclsparse_status_invalid_pointer;
    switch(A->val_type)
    {
    case aoclsparse_smat:
        return revalue_device(A, len, static_cast<const float *>(val), aoclsparse_smat);
    case aoclsparse_dmat:
        return revalue_device(A, len, static_cast<const double *>(val), aoclsparse_dmat);
    case aoclsparse_cmat:
        return revalue_device(A, len, static_cast<const aoclsparse_float_complex *>(val), aoclsparse_cmat);
    default:
        return revalue_device(A, len, static_cast<const aoclsparse_double_complex *>(val), aoclsparse_zmat);
    }
}
} // namespace mi355

extern "C" {

aoclsparse_status aoclsparse_mi355_create_scsr_device(aoclsparse_matrix *mat, aoclsparse_index_base base, aoclsparse_int M,
                                                      aoclsparse_int N, aoclsparse_int nnz, const aoclsparse_int *row_ptr,
                                                      const aoclsparse_int *col_idx, const float *val)
{
    return create_csr_device(mat, base, M, N, nnz, row_ptr, col_idx, val, aoclsparse_smat);
}
aoclsparse_status aoclsparse_mi355_create_dcsr_device(aoclsparse_matrix *mat, aoclsparse_index_base base, aoclsparse_int M,
                                                      aoclsparse_int N, aoclsparse_int nnz, const aoclsparse_int *row_ptr,
                                                      const aoclsparse_int *col_idx, const double *val)
{
    return create_csr_device(mat, base, M, N, nnz, row_ptr, col_idx, val, aoclsparse_dmat);
}
aoclsparse_status aoclsparse_mi355_create_ccsr_device(aoclsparse_matrix *mat, aoclsparse_index_base base, aoclsparse_int M,
                                                      aoclsparse_int N, aoclsparse_int nnz, const aoclsparse_int *row_ptr,
                                                      const aoclsparse_int *col_idx, const aoclsparse_float_complex *val)
{
    return create_csr_device(mat, base, M, N, nnz, row_ptr, col_idx, val, aoclsparse_cmat);
}
aoclsparse_status aoclsparse_mi355_create_zcsr_device(aoclsparse_matrix *mat, aoclsparse_index_base base, aoclsparse_int M,
                                                      aoclsparse_int N, aoclsparse_int nnz, const aoclsparse_int *row_ptr,
                                                      const aoclsparse_int *col_idx, const aoclsparse_double_complex *val)
{
    return create_csr_device(mat, base, M, N, nnz, row_ptr, col_idx, val, aoclsparse_zmat);
}

aoclsparse_status aoclsparse_mi355_create_scsr_from_coo_device(aoclsparse_matrix *mat, aoclsparse_index_base base, aoclsparse_int M,
                                                               aoclsparse_int N, aoclsparse_int nnz, const aoclsparse_int *row_ind,
                                                               const aoclsparse_int *col_ind, const float *val,
                                                               aoclsparse_int duplicates)
{
    return create_csr_from_coo_device(mat, base, M, N, nnz, row_ind, col_ind, val, duplicates, aoclsparse_smat);
}
aoclsparse_status aoclsparse_mi355_create_dcsr_from_coo_device(aoclsparse_matrix *mat, aoclsparse_index_base base, aoclsparse_int M,
                                                               aoclsparse_int N, aoclsparse_int nnz, const aoclsparse_int *row_ind,
                                                               const aoclsparse_int *col_ind, const double *val,
                                                               aoclsparse_int duplicates)
{
    return create_csr_from_coo_device(mat, base, M, N, nnz, row_ind, col_ind, val, duplicates, aoclsparse_dmat);
}
aoclsparse_status aoclsparse_mi355_create_ccsr_from_coo_device(aoclsparse_matrix *mat, aoclsparse_index_base base, aoclsparse_int M,
                                                               aoclsparse_int N, aoclsparse_int nnz, const aoclsparse_int *row_ind,
                                                               const aoclsparse_int *col_ind, const aoclsparse_float_complex *val,
                                                               aoclsparse_int duplicates)
{
    return create_csr_from_coo_device(mat, base, M, N, nnz, row_ind, col_ind, val, duplicates, aoclsparse_cmat);
}
aoclsparse_status aoclsparse_mi355_create_zcsr_from_coo_device(aoclsparse_matrix *mat, aoclsparse_index_base base, aoclsparse_int M,
                                                               aoclsparse_int N, aoclsparse_int nnz, const aoclsparse_int *row_ind,
                                                               const aoclsparse_int *col_ind, const aoclsparse_double_complex *val,
                                                               aoclsparse_int duplicates)
{
    return create_csr_from_coo_device(mat, base, M, N, nnz, row_ind, col_ind, val, duplicates, aoclsparse_zmat);
}

aoclsparse_status aoclsparse_mi355_supdate_values_device(aoclsparse_matrix A, aoclsparse_int len, const float *val)
{
    return update_values_device(A, len, val, aoclsparse_smat);
}
aoclsparse_status aoclsparse_mi355_dupdate_values_device(aoclsparse_matrix A, aoclsparse_int len, const double *val)
{
    return update_values_device(A, len, val, aoclsparse_dmat);
}
aoclsparse_status aoclsparse_mi355_cupdate_values_device(aoclsparse_matrix A, aoclsparse_int len, const aoclsparse_float_complex *val)
{
    return update_values_device(A, len, val, aoclsparse_cmat);
}
aoclsparse_status aoclsparse_mi355_zupdate_values_device(aoclsparse_matrix A, aoclsparse_int len, const aoclsparse_double_complex *val)
{
    return update_values_device(A, len, val, aoclsparse_zmat);
}

aoclsparse_status aoclsparse_mi355_srevalue_device(aoclsparse_matrix A, aoclsparse_int len, const float *val)
{
    return revalue_device(A, len, val, aoclsparse_smat);
}
aoclsparse_status aoclsparse_mi355_drevalue_device(aoclsparse_matrix A, aoclsparse_int len, const double *val)
{
    return revalue_device(A, len, val, aoclsparse_dmat);
}
aoclsparse_status aoclsparse_mi355_crevalue_device(aoclsparse_matrix A, aoclsparse_int len, const aoclsparse_float_complex *val)
{
    return revalue_device(A, len, val, aoclsparse_cmat);
}
aoclsparse_status aoclsparse_mi355_zrevalue_device(aoclsparse_matrix A, aoclsparse_int len, const aoclsparse_double_complex *val)
{
    return revalue_device(A, len, val, aoclsparse_zmat);
}

aoclsparse_status aoclsparse_mi355_keep_value_maps(aoclsparse_matrix A, aoclsparse_int on)
{
    if(!A)
        return aoclsparse_status_invalid_pointer;
    if(holds_no_csr(A)) // TCSR and BSR handles
        return aoclsparse_status_not_implemented;
    // stage_lock, then the handle's guard, as the siblings: on == 0 frees device buffers, and whoever enqueues work that reads the
    // maps (?revalue_device) holds the stage lock until the stream has finished with them
    std::lock_guard<std::recursive_mutex> sl(Runtime::get().stage_lock);
    std::unique_lock<std::shared_mutex>   w(A->guard);
    A->keep_maps = on != 0;
    if(!on) // (what was built stays as it is: the next ?revalue_device finds it without maps and drops it)
        A->drop_value_maps();
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_mi355_get_value_map_info(aoclsparse_matrix A, aoclsparse_mi355_value_map_info *info)
{
    if(!A || !info)
        return aoclsparse_status_invalid_pointer;
    if(info->struct_size < sizeof(info->struct_size))
        return aoclsparse_status_invalid_size;
    aoclsparse_mi355_value_map_info r{};
    {
        std::shared_lock<std::shared_mutex> g(A->guard);
        r.enabled   = A->keep_maps;
        r.clean_map = A->opt && (A->opt == &A->user || A->clean_src.ptr);
        size_t bytes = A->clean_src.bytes + A->diag_src.bytes;
        for(const TrsvPlan &p : A->trsv_plan)
        {
            r.plans_mapped += p.value_mapped();
            bytes += p.psrc.bytes + p.blk.psrc.bytes;
        }
        r.plan_builds = A->plan_builds, r.clean_builds = A->clean_builds, r.revalues = A->revalues;
        r.last_kept_plans = A->last_kept_plans;
        r.map_bytes       = (long long)bytes;
    }
    r.struct_size = info->struct_size; // (the caller's: it says how much of the struct the caller has)
    std::memcpy(info, &r, std::min(info->struct_size, sizeof(r))); // no more than that is written
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_mi355_srefresh_values_from_coo_device(aoclsparse_matrix A, aoclsparse_int len, const float *val)
{
    return refresh_values_from_coo_device(A, len, val, aoclsparse_smat);
}
aoclsparse_status aoclsparse_mi355_drefresh_values_from_coo_device(aoclsparse_matrix A, aoclsparse_int len, const double *val)
{
    return refresh_values_from_coo_device(A, len, val, aoclsparse_dmat);
}
aoclsparse_status aoclsparse_mi355_crefresh_values_from_coo_device(aoclsparse_matrix A, aoclsparse_int len,
                                                                   const aoclsparse_float_complex *val)
{
    return refresh_values_from_coo_device(A, len, val, aoclsparse_cmat);
}
aoclsparse_status aoclsparse_mi355_zrefresh_values_from_coo_device(aoclsparse_matrix A, aoclsparse_int len,
                                                                   const aoclsparse_double_complex *val)
{
    return refresh_values_from_coo_device(A, len, val, aoclsparse_zmat);
}

aoclsparse_status aoclsparse_mi355_get_coo_map_info(aoclsparse_matrix A, aoclsparse_mi355_coo_map_info *info)
{
    if(!A || !info)
        return aoclsparse_status_invalid_pointer;
    if(info->struct_size < sizeof(info->struct_size))
        return aoclsparse_status_invalid_size;
    aoclsparse_mi355_coo_map_info r{};
    {
        std::shared_lock<std::shared_mutex> g(A->guard);
        if(A->coo_map_kept)
        {
            r.kept = 1, r.mode = A->coo_map_mode, r.triplets = A->coo_map_triplets, r.entries = A->nnz;
            r.map_bytes = (long long)(A->coo_pos.bytes + A->coo_runs.bytes);
        }
    }
    r.struct_size = info->struct_size; // (the caller's: it says how much of the struct the caller has)
    std::memcpy(info, &r, std::min(info->struct_size, sizeof(r))); // no more than that is written
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_mi355_order_mat_device(aoclsparse_matrix A)
{
    // the statuses of aoclsparse_order_mat (formats_api.cpp), in its order, all before the device is touched
    if(!A)
        return aoclsparse_status_invalid_pointer;
    if(A->m < 0 || A->n < 0 || A->nnz < 0)
        return aoclsparse_status_invalid_value;
    if(A->input_format != aoclsparse_csr_mat)
        return aoclsparse_status_not_implemented;
    if(A->m == 0 || A->n == 0 || A->nnz == 0)
        return aoclsparse_status_success;
    if(!A->user.ptr || !A->user.ind || !A->user.val)
        return aoclsparse_status_invalid_pointer;
    if(A->csc_ptr) // the host call sorts the caller's CSC arrays there: they live on the host
        return aoclsparse_status_not_implemented;
    Runtime          &rt = Runtime::get();
    aoclsparse_status rc = rt.init();
    if(rc != aoclsparse_status_success)
        return rc;
    std::lock_guard<std::recursive_mutex> sl(rt.stage_lock); // (before the handle's guard, as everywhere)
    std::unique_lock<std::shared_mutex>   w(A->guard);
    hipStream_t                           s   = rt.stream();
    const size_t                          vsz = val_size(A->val_type);
    DeviceCsr                            &d   = A->dev_user;
    DeviceBuffer                          res;
    if((rc = res.alloc(sizeof(MatCheckResult))) != aoclsparse_status_success)
        return rc;
    // a mirror that is not resident (a host-created handle before its first product) or not valid (?set_value, aoclsparse_order_mat,
    // aoclsparse_mi355_invalidate) comes from the host view first, as for export_csr_device.  Up to here the handle is unchanged.
    if(!d.valid && (rc = upload_csr(A->user, vsz, d)) != aoclsparse_status_success)
        return rc;
    if(d.m != A->m || d.nnz != A->nnz || !d.ptr.ptr || !d.ind.ptr || !d.val.ptr)
        return aoclsparse_status_internal_error;
    // The mirror is sorted IN PLACE, in stream order behind every product enqueued on the library's stream; the host view is
    // committed by one copy back once all device work has succeeded.  A failure before that leaves the host view as it was, the
    // mirror invalid (the next product uploads the host view again) and everything derived dropped.
    MatCheckResult *d_res = res.as<MatCheckResult>(), h{};
    long long       moved = 0;
    LapTimer        lt;
    auto            hip = [&](hipError_t e) {
        if(e != hipSuccess && rc == aoclsparse_status_success)
            rc = aoclsparse_status_internal_error;
    };
    rc = device_order_rows(s, d.m, d.n, d.nnz, (int)d.base, d.ptr.as<const aoclsparse_int>(), d.ind.as<aoclsparse_int>(), d.val.ptr, vsz,
                           &moved);
    lt.lap("order_mat_device: sort");
    // sort class and full diagonal again, over the sorted arrays: mat_check's answer (the row pointer was checked at creation)
    if(rc == aoclsparse_status_success)
        hip(hipMemsetAsync(d_res, 0, sizeof(MatCheckResult), s));
    if(rc == aoclsparse_status_success)
        rc = launch_matcheck_rows(s, d.m, d.n, (int)d.base, d.ptr.as<const aoclsparse_int>(), d.ind.as<const aoclsparse_int>(), d_res);
    if(rc == aoclsparse_status_success)
        hip(hipMemcpyAsync(&h, d_res, sizeof(h), hipMemcpyDeviceToHost, s));
    if(rc == aoclsparse_status_success)
        hip(hipStreamSynchronize(s));
    lt.lap("order_mat_device: check kernel");
    if(rc != aoclsparse_status_success)
    {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(s);
        drop_derived_state(A); // (d.valid = false with it)
        return rc;
    }
    if(moved > 0) // the one copy back; rows that were ascending were not touched, so nothing moved means nothing to bring
    {
        hip(hipMemcpyAsync(A->user.ind, d.ind.ptr, sizeof(aoclsparse_int) * (size_t)d.nnz, hipMemcpyDeviceToHost, s));
        hip(hipMemcpyAsync(A->user.val, d.val.ptr, vsz * (size_t)d.nnz, hipMemcpyDeviceToHost, s));
        hip(hipStreamSynchronize(s));
        lt.lap("order_mat_device: host view");
    }
    // A copy back that fails may have written part of the host view.  The class and the diagonal flag then stay what they were
    // for the unsorted arrays (nothing may take the host view for sorted), and the mirror -- which IS sorted, every row of it --
    // stays the handle's resident CSR, so no product uploads that view.
    if(rc == aoclsparse_status_success && !h.first_err) // (as the host call: a row mat_check refuses leaves the two as they were)
        A->sort = h.cls ? h.cls : 1, A->fulldiag = !h.notfull;
    A->drop_coo_map(); // a kept triplet map points into the arrays as they were ordered at creation
    A->ilu_sched.release(); // ... and so does the ILU(0) schedule: the next factorisation analyses the new order
    drop_derived_state(A); // every copy made of the unsorted arrays (clean CSR, SELL-64 / blocked-ELL, kept transpose, plans, replicas)
    d.valid = true; // the mirror IS the handle's CSR now: resident before any product
    if(rc != aoclsparse_status_success)
        (void)hipGetLastError();
    return rc;
}

aoclsparse_status aoclsparse_mi355_clean_csr_device(aoclsparse_matrix A)
{
    // the statuses of csr_optimize (matrix.cpp), in its order, all before the device is touched
    if(!A)
        return aoclsparse_status_invalid_pointer;
    {
        std::shared_lock<std::shared_mutex> r(A->guard);
        if(A->opt)
            return aoclsparse_status_success;
    }
    if(holds_no_csr(A)) // TCSR and BSR handles
        return aoclsparse_status_not_implemented;
    if(!A->user.ptr || !A->user.ind || !A->user.val) // COO handles
        return aoclsparse_status_invalid_pointer;
    Runtime          &rt = Runtime::get();
    aoclsparse_status rc = rt.init();
    if(rc != aoclsparse_status_success)
        return rc;
    std::lock_guard<std::recursive_mutex> sl(rt.stage_lock); // (before the handle's guard, as everywhere)
    std::unique_lock<std::shared_mutex>   w(A->guard);
    if(A->opt) // (another thread's csr_optimize got here first)
        return aoclsparse_status_success;
    hipStream_t  s   = rt.stream();
    const size_t vsz = val_size(A->val_type);
    DeviceCsr   &d   = A->dev_user;
    // Everything below is built in buffers of this call's and committed at the very end; until then the handle is as it was, except
    // that a mirror that was not resident or not valid has come from the host view (as for export_csr_device).  Whatever way out is
    // taken, the stream first finishes what was enqueued on the staging slots and on those buffers (declared first: released last).
    DeviceBuffer                      res, sind, sval, cptr, cind, cval, didiag, diurow, ddiag;
    DeviceBuffer                      pind, perm, csrc, dsrc; // the value maps of a handle that keeps them (and their scratch)
    std::unique_ptr<HostCsr>          c;
    std::unique_ptr<aoclsparse_int[]> idiag, iurow;
    struct DrainOnExit
    {
        hipStream_t s;
        ~DrainOnExit()
        {
            (void)hipStreamSynchronize(s);
            (void)hipGetLastError(); // (a failed launch or copy is reported by this call's status, not by the next call's)
        }
    } drain{s};
    if(!d.valid && (rc = upload_csr(A->user, vsz, d)) != aoclsparse_status_success)
        return rc;
    const aoclsparse_int m = A->user.m, n = A->user.n, nnz = A->nnz; // (what csr_optimize reads)
    if(d.m != m || d.nnz != nnz || !d.ptr.ptr || !d.ind.ptr || !d.val.ptr)
        return aoclsparse_status_internal_error;
    const int             base  = (int)d.base;
    const aoclsparse_int *d_ptr = d.ptr.as<const aoclsparse_int>();
    LapTimer              lt;
    // mat_check's answer over the mirror, once: the row pointer first (the kernels below trust it), then validity, sort class and
    // full diagonal.  Class <= 2 is check_sort_diag's `sorted`.
    if((rc = res.alloc(sizeof(MatCheckResult))) != aoclsparse_status_success)
        return rc;
    MatCheckResult *d_res = res.as<MatCheckResult>(), h{};
    if((rc = launch_matcheck_ptr(s, m, nnz, base, d_ptr, d_res)) != aoclsparse_status_success)
        return rc;
    MI355_HIP_TRY(hipMemcpyAsync(&h, d_res, sizeof(h), hipMemcpyDeviceToHost, s));
    MI355_HIP_TRY(hipStreamSynchronize(s));
    if(h.ptr_bad)
        return aoclsparse_status_invalid_value;
    if((rc = launch_matcheck_rows(s, m, n, base, d_ptr, d.ind.as<const aoclsparse_int>(), d_res)) != aoclsparse_status_success)
        return rc;
    MI355_HIP_TRY(hipMemcpyAsync(&h, d_res, sizeof(h), hipMemcpyDeviceToHost, s));
    MI355_HIP_TRY(hipStreamSynchronize(s));
    if(h.first_err)
        return (aoclsparse_status)(~h.first_err & 0xff);
    const bool sorted = h.cls <= 2, fulldiag = !h.notfull;
    lt.lap("clean_csr_device: mirror + check");

    // case 3: the rows into ascending order first, on a copy of the mirror's columns and values
    const void  *src_val = d.val.ptr;
    auto        *src_ind = d.ind.as<const aoclsparse_int>();
    if(!sorted)
    {
        if((rc = sind.clone_from(d.ind, s)) != aoclsparse_status_success || (rc = sval.clone_from(d.val, s)) != aoclsparse_status_success)
            return rc;
        if((rc = device_order_rows(s, m, n, nnz, base, d_ptr, sind.as<aoclsparse_int>(), sval.ptr, vsz)) != aoclsparse_status_success)
            return rc;
        src_ind = sind.as<const aoclsparse_int>(), src_val = sval.ptr;
        lt.lap("clean_csr_device: sort");
        if(A->keep_maps)
        {
            // The sort's permutation: the same sort over a second copy of the columns, moving the entries' positions as its 4-byte
            // items.  The sort never computes with an item and is a function of the columns alone, so perm[q] = where sorted entry q
            // stands in the user's arrays.  The arrays sorted above are the ones the call without maps sorts.
            if((rc = pind.clone_from(d.ind, s)) != aoclsparse_status_success
               || (rc = perm.alloc(sizeof(int) * (size_t)std::max<aoclsparse_int>(nnz, 1))) != aoclsparse_status_success
               || (rc = launch_revalue_iota(s, nnz, perm.as<int>())) != aoclsparse_status_success)
                return rc;
            if((rc = device_order_rows(s, m, n, nnz, base, d_ptr, pind.as<aoclsparse_int>(), perm.ptr, sizeof(int)))
               != aoclsparse_status_success)
                return rc;
            lt.lap("clean_csr_device: sort of the positions");
        }
    }
    // mark, and for a copy the clean row pointer with its 64-bit total
    const bool   copy = !sorted || !fulldiag;
    const size_t rb   = sizeof(int) * (size_t)std::max<aoclsparse_int>(m, 1);
    void        *p    = nullptr;
    if((rc = rt.staging(CLN_SLOT_AT, rb, &p)) != aoclsparse_status_success)
        return rc;
    int *const at_p = static_cast<int *>(p);
    if((rc = rt.staging(CLN_SLOT_MISS, rb, &p)) != aoclsparse_status_success)
        return rc;
    int *const miss_p = static_cast<int *>(p);
    if((rc = rt.staging(CLN_SLOT_CNT, rb, &p)) != aoclsparse_status_success)
        return rc;
    int *const cnt_p = static_cast<int *>(p);
    if((rc = launch_clean_mark(s, m, n, nnz, base, d_ptr, src_ind, at_p, miss_p, cnt_p)) != aoclsparse_status_success)
        return rc;
    aoclsparse_int total = nnz;
    if(copy)
    {
        if((rc = cptr.alloc(sizeof(aoclsparse_int) * ((size_t)m + 1))) != aoclsparse_status_success
           || (rc = rt.staging(CLN_SLOT_SCAN, spg_scan_scratch_bytes(m), &p)) != aoclsparse_status_success)
            return rc;
        long long *total_dev = nullptr, total_ll = 0;
        if((rc = launch_spg_scan(s, m, cnt_p, cptr.as<aoclsparse_int>(), static_cast<long long *>(p), &total_dev))
           != aoclsparse_status_success)
            return rc;
        MI355_HIP_TRY(hipMemcpyAsync(&total_ll, total_dev, sizeof(total_ll), hipMemcpyDeviceToHost, s));
        MI355_HIP_TRY(hipStreamSynchronize(s));
        if(total_ll > (long long)std::numeric_limits<aoclsparse_int>::max())
            return aoclsparse_status_invalid_size; // nnz + the inserted entries do not fit the index type
        if(total_ll < (long long)nnz || total_ll > (long long)nnz + std::min(m, n))
            return aoclsparse_status_internal_error;
        total = (aoclsparse_int)total_ll;
        lt.lap("clean_csr_device: mark + scan");
    }
    // the host arrays the result goes into: big ones as build_transpose allocates them
    idiag.reset(new(std::nothrow) aoclsparse_int[m > 0 ? m : 1]);
    iurow.reset(new(std::nothrow) aoclsparse_int[m > 0 ? m : 1]);
    if(!idiag || !iurow)
        return aoclsparse_status_memory_error;
    const size_t ib = sizeof(aoclsparse_int) * (size_t)total, vb = vsz * (size_t)total;
    if(copy)
    {
        c.reset(new(std::nothrow) HostCsr);
        if(!c)
            return aoclsparse_status_memory_error;
        c->m = m, c->n = n, c->nnz = total, c->base = aoclsparse_index_base_zero;
        c->owned = c->result_arrays = true;
        c->ptr = new(std::nothrow) aoclsparse_int[(size_t)m + 1];
        c->ind = static_cast<aoclsparse_int *>(host_result_alloc(ib));
        c->val = host_result_alloc(vb);
        if(!c->ptr || !c->ind || !c->val)
            return aoclsparse_status_memory_error;
        host_result_touch(c->ind, ib);
        host_result_touch(c->val, vb);
        lt.lap("clean_csr_device: host arrays");
    }
    // expand and finish
    if((rc = didiag.alloc(rb)) != aoclsparse_status_success || (rc = diurow.alloc(rb)) != aoclsparse_status_success
       || (rc = ddiag.alloc(vsz * (size_t)std::max<aoclsparse_int>(m, 1))) != aoclsparse_status_success)
        return rc;
    if(copy)
    {
        if((rc = cind.alloc(ib)) != aoclsparse_status_success || (rc = cval.alloc(vb)) != aoclsparse_status_success)
            return rc;
        if(A->keep_maps && (rc = csrc.alloc(sizeof(int) * (size_t)std::max<aoclsparse_int>(total, 1))) != aoclsparse_status_success)
            return rc;
        if((rc = launch_clean_expand(s, m, nnz, total, base, d_ptr, src_ind, src_val, vsz, cptr.as<const aoclsparse_int>(), at_p, miss_p,
                                     cind.as<aoclsparse_int>(), cval.ptr, csrc.as<int>()))
           != aoclsparse_status_success)
            return rc;
        // (positions in the sorted arrays so far: through the sort's permutation they are positions in the user's)
        if(csrc.ptr && !sorted
           && (rc = launch_revalue_compose(s, total, nnz, perm.as<const int>(), csrc.as<int>())) != aoclsparse_status_success)
            return rc;
    }
    if((rc = launch_clean_finish(s, m, n, nnz, base, d_ptr, src_val, vsz, copy ? cptr.as<const aoclsparse_int>() : nullptr, at_p, miss_p,
                                 didiag.as<aoclsparse_int>(), diurow.as<aoclsparse_int>(), ddiag.ptr))
       != aoclsparse_status_success)
        return rc;
    if(A->keep_maps) // the diagonal's map, from what the finish kernel has just written
    {
        if((rc = dsrc.alloc(rb)) != aoclsparse_status_success
           || (rc = launch_revalue_diag_map(s, m, n, copy ? 0 : base, total, didiag.as<const aoclsparse_int>(),
                                            diurow.as<const aoclsparse_int>(), dsrc.as<int>()))
                  != aoclsparse_status_success)
            return rc;
    }
    if(PhaseTimer::on()) // (the diagnostic separates the kernels from the copy back)
        MI355_HIP_TRY(hipStreamSynchronize(s));
    lt.lap("clean_csr_device: expand + finish");
    // the one copy back; the diagonal's values stay in HBM
    if(m > 0)
    {
        MI355_HIP_TRY(hipMemcpyAsync(idiag.get(), didiag.ptr, sizeof(aoclsparse_int) * (size_t)m, hipMemcpyDeviceToHost, s));
        MI355_HIP_TRY(hipMemcpyAsync(iurow.get(), diurow.ptr, sizeof(aoclsparse_int) * (size_t)m, hipMemcpyDeviceToHost, s));
    }
    if(copy)
    {
        MI355_HIP_TRY(hipMemcpyAsync(c->ptr, cptr.ptr, sizeof(aoclsparse_int) * ((size_t)m + 1), hipMemcpyDeviceToHost, s));
        if(total > 0)
        {
            MI355_HIP_TRY(hipMemcpyAsync(c->ind, cind.ptr, ib, hipMemcpyDeviceToHost, s));
            MI355_HIP_TRY(hipMemcpyAsync(c->val, cval.ptr, vb, hipMemcpyDeviceToHost, s));
        }
    }
    MI355_HIP_TRY(hipStreamSynchronize(s));
    lt.lap("clean_csr_device: copy back");
    // commit: what csr_optimize sets, and the diagonal ensure_trsv would otherwise gather on the host and upload
    A->sort = h.cls ? h.cls : 1, A->fulldiag = fulldiag;
    HostCsr &o = copy ? *c : A->user;
    delete[] o.idiag;
    delete[] o.iurow;
    o.idiag = idiag.release(), o.iurow = iurow.release();
    o.is_optimized = true;
    if(copy)
    {
        A->opt_copy = std::move(c);
        A->opt      = A->opt_copy.get();
    }
    else
        A->opt = &A->user;
    A->opt_csr_full_diag = fulldiag;
    A->optimized         = true;
    A->dev_diag.adopt(ddiag);
    A->clean_src.adopt(csrc), A->diag_src.adopt(dsrc); // (empty without the flag; no clean_src when the clean CSR is the handle's own)
    A->clean_builds++;
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_mi355_export_csr_device(aoclsparse_matrix A, aoclsparse_index_base *base, aoclsparse_int *M,
                                                     aoclsparse_int *N, aoclsparse_int *nnz, const aoclsparse_int **row_ptr,
                                                     const aoclsparse_int **col_idx, const void **val)
{
    if(!A || !base || !M || !N || !nnz || !row_ptr || !col_idx || !val)
        return aoclsparse_status_invalid_pointer;
    if(A->input_format != aoclsparse_csr_mat || !A->user.ptr || !A->user.ind || !A->user.val)
        return aoclsparse_status_invalid_value; // COO, TCSR and BSR handles hold no CSR
    Runtime          &rt = Runtime::get();
    aoclsparse_status rc = rt.init();
    if(rc != aoclsparse_status_success)
        return rc;
    std::lock_guard<std::recursive_mutex> sl(rt.stage_lock);
    std::unique_lock<std::shared_mutex>   w(A->guard);
    if(!A->dev_user.valid && (rc = upload_csr(A->user, val_size(A->val_type), A->dev_user)) != aoclsparse_status_success)
        return rc;
    MI355_HIP_TRY(hipStreamSynchronize(rt.stream())); // the caller reads the arrays from streams of its own
    const DeviceCsr &d = A->dev_user;
    *base = (aoclsparse_index_base)d.base, *M = d.m, *N = d.n, *nnz = d.nnz;
    *row_ptr = d.ptr.as<const aoclsparse_int>(), *col_idx = d.ind.as<const aoclsparse_int>(), *val = d.val.ptr;
    return aoclsparse_status_success;
}

} // extern "C"
