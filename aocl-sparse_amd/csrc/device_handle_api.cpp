// device_handle_api.cpp -- CSR matrix handles whose arrays live in HBM.  The reference has no counterpart (a CPU library has one
// address space); without these a matrix assembled on the GPU would cross PCIe twice.  As in aoclsparse_mi355_mm_state_adopt
// (comm_api.cpp) the device arrays are COPIED into the handle's device mirror (dev_user), the handle gets an owned host view
// (`user`) by one copy back, and every other entry point works on it unchanged: no aliasing, no handle without host arrays.
//   creation    from CSR arrays (checked by matcheck_kernels.hip as mat_check checks on the host) or from unordered triplets
//               (coo_sort_kernels.hip; the sorted arrays are MOVED into the mirror, the sort's map may stay on the handle)
//   new values  ?update_values_device, ?revalue_device (what holds a value map follows: revalue_kernels.hip) and
//               ?refresh_values_from_coo_device (through the kept triplet map) all end in commit_values_device
//   order       aoclsparse_order_mat on the mirror (order_kernels.hip);  clean: csr_optimize on it (clean_csr_kernels.hip)
//   operators   aoclsparse_mi355_build_operator_device: what ensure_derived (derived.cpp) builds on the host for a symmetric,
//               Hermitian or triangular descriptor, built from the clean CSR in HBM (derived_kernels.hip); with its source map it
//               follows ?revalue_device
//   export      the mirror's pointers.                     The steps several of them take are in device_handle.hpp.
#include "device_handle.hpp"

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
        Runtime                              &rt  = Runtime::get();
        const size_t                          vsz = val_size(vt);
        std::lock_guard<std::recursive_mutex> sl(rt.stage_lock); // (one user of the library's stream at a time, as everywhere)
        hipStream_t                           s = rt.stream();
        StreamLaps                            lt{s};
        // any base is checked like mat_check checks it: against ptr[0], and every index after subtracting it
        MatCheckResult h;
        MI355_TRY(device_mat_check(s, M, N, nnz, (int)base, row_ptr, col_idx, h));
        MI355_TRY(matcheck_status(h));
        lt.lap("create_device: check kernels");
        aoclsparse_matrix H = nullptr;
        MI355_TRY(new_csr_result(&H, M, N, nnz, vt, nullptr, base));
        H->sort = h.cls ? h.cls : 1, H->fulldiag = !h.notfull;
        // the device mirror (a copy of the caller's arrays, or the library's own buffers moved in) and the host view
        DeviceCsr   &d  = H->dev_user;
        const size_t pb = sizeof(aoclsparse_int) * ((size_t)M + 1), ib = sizeof(aoclsparse_int) * (size_t)nnz, vb = vsz * (size_t)nnz;
        FirstError   e;
        auto         copy = [&](void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
            if(e.ok() && bytes)
                e.hip(hipMemcpyAsync(dst, src, bytes, kind, s));
        };
        {
            StreamDrain drain{s}; // (after a failure: nothing in flight into the handle's arrays when they go)
            if(own)
                d.ptr.adopt(own[0]), d.ind.adopt(own[1]), d.val.adopt(own[2]); // (row_ptr, col_idx and val point into them still)
            else
            {
                e.status(d.ptr.alloc(pb));
                e.status(d.ind.alloc(ib));
                e.status(d.val.alloc(vb));
                copy(d.ptr.ptr, row_ptr, pb, hipMemcpyDeviceToDevice);
                copy(d.ind.ptr, col_idx, ib, hipMemcpyDeviceToDevice);
                copy(d.val.ptr, val, vb, hipMemcpyDeviceToDevice);
            }
            e.hip(lt.synced("create_device: handle + device copy")); // (the diagnostic separates the two directions)
            copy(H->user.ptr, row_ptr, pb, hipMemcpyDeviceToHost);
            if(e.ok() && nnz > 0)
            {
                host_result_touch(H->user.ind, ib); // (fresh arrays: see host_result_alloc)
                host_result_touch(H->user.val, vb);
            }
            copy(H->user.ind, col_idx, ib, hipMemcpyDeviceToHost);
            copy(H->user.val, val, vb, hipMemcpyDeviceToHost);
            if(e.ok())
                e.hip(hipStreamSynchronize(s)); // the caller may overwrite or free its arrays now
            if(e.ok())
                drain.dismiss();
        }
        if(!e.ok())
        {
            aoclsparse_destroy(&H);
            return e.rc;
        }
        lt.lap("create_device: host view");
        d.m = M, d.n = N, d.nnz = nnz, d.base = base;
        d.valid = true; // (the row-block plan is built from the host view at the first product, as for every handle)
        *mat    = H;
        return aoclsparse_status_success;
    }

    aoclsparse_status create_csr_device(aoclsparse_matrix *mat, aoclsparse_index_base base, aoclsparse_int M, aoclsparse_int N,
                                        aoclsparse_int nnz, const aoclsparse_int *row_ptr, const aoclsparse_int *col_idx,
                                        const void *val, aoclsparse_matrix_data_type vt)
    {
        // decided before the device is touched, in the order of create_csr / mat_check (matrix.cpp)
        if(!mat)
            return aoclsparse_status_invalid_pointer;
        *mat = nullptr;
        if(!row_ptr || !col_idx || !val)
            return aoclsparse_status_invalid_pointer;
        if(N < 0 || M < 0 || nnz < 0)
            return aoclsparse_status_invalid_size;
        Runtime &rt = Runtime::get();
        MI355_TRY(rt.init());
        if(!rt.is_device_pointer(row_ptr) || !rt.is_device_pointer(col_idx) || !rt.is_device_pointer(val))
            return aoclsparse_status_invalid_pointer;
        return csr_handle_from_device(mat, base, M, N, nnz, row_ptr, col_idx, val, vt, nullptr);
    }

    // triplets in HBM -> CSR arrays in HBM (coo_sort_kernels.hip) -> handle
    aoclsparse_status create_csr_from_coo_device(aoclsparse_matrix *mat, aoclsparse_index_base base, aoclsparse_int M, aoclsparse_int N,
                                                 aoclsparse_int nnz, const aoclsparse_int *row_ind, const aoclsparse_int *col_ind,
                                                 const void *val, aoclsparse_int duplicates, aoclsparse_matrix_data_type vt)
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
        Runtime &rt = Runtime::get();
        MI355_TRY(rt.init());
        if(!rt.is_device_pointer(row_ind) || !rt.is_device_pointer(col_ind) || !rt.is_device_pointer(val))
            return aoclsparse_status_invalid_pointer;
        std::lock_guard<std::recursive_mutex> sl(rt.stage_lock);
        LapTimer                              lt;
        DeviceBuffer                          own[3], map[2];
        aoclsparse_int                        nnz_csr = 0;
        const bool                            cplx    = vt == aoclsparse_cmat || vt == aoclsparse_zmat;
        MI355_TRY(device_coo_to_csr(rt.stream(), M, N, nnz, (int)base, row_ind, col_ind, val, val_size(vt), cplx,
                                    mode == aoclsparse_mi355_coo_sum, own[0], own[1], own[2], &nnz_csr, keep_map ? map : nullptr));
        lt.lap("create_from_coo_device: sort");
        MI355_TRY(csr_handle_from_device(mat, base, M, N, nnz_csr, own[0].as<const aoclsparse_int>(),
                                         own[1].as<const aoclsparse_int>(), own[2].ptr, vt, own));
        if(keep_map) // the sort's map hangs on the handle from here on
        {
            aoclsparse_matrix H = *mat;
            H->coo_pos.adopt(map[0]), H->coo_runs.adopt(map[1]);
            H->coo_map_kept = true, H->coo_map_mode = mode, H->coo_map_triplets = nnz;
        }
        return aoclsparse_status_success;
    }

    // The mirror follows a value change -- the values alone travel, it stays resident -- exactly while it is valid: its row pointers
    // and columns are then the handle's structure (aoclsparse_order_mat leaves stale buffers behind an invalid mirror)
    bool mirror_follows(const _aoclsparse_matrix *A, size_t bytes)
    {
        const DeviceCsr &d = A->dev_user;
        return d.valid && d.m == A->m && d.nnz == A->nnz && d.ptr.ptr && d.ind.ptr && d.val.ptr && d.val.bytes >= bytes;
    }

    // decide: what a value change leaves standing.  The mirror while it follows; under follow_maps also what holds a value map, each
    // kind of copy answering through its own `follows`.  How they hang together is decided here alone: the operators' and the diagonal's
    // maps hold positions in the clean CSR, a plan divides by the diagonal, the SELL-64 copy was built from the mirror.  Writes nothing.
    ValuesKept values_kept(const _aoclsparse_matrix *A, size_t vsz, bool follow_maps)
    {
        ValuesKept k;
        k.mirror = mirror_follows(A, vsz * (size_t)A->nnz);
        k.sell   = follow_maps && A->keep_maps && k.mirror;
        k.clean = k.operators = follow_maps && A->clean_follows();
        k.diag                = k.clean && A->diag_follows(vsz);
        for(int i = 0; i < 6 && k.diag; i++)
            if(A->trsv_plan[i].follows(vsz))
                k.plans |= 1u << i;
        return k;
    }

    // enqueue: the new values to the host view and to everything in `kept` (a clean COPY's through the scratch `cval`), in stream order
    // behind every product and solve enqueued on the library's stream (they read the old values); one host wait.  The handle is written.
    void enqueue_values(aoclsparse_matrix A, const void *val, size_t vsz, bool follow_maps, const ValuesKept &kept,
                        const DeviceBuffer &cval, StreamLaps &lt, FirstError &e)
    {
        hipStream_t    s     = Runtime::get().stream();
        const size_t   bytes = vsz * (size_t)A->nnz;
        HostCsr *const o     = A->opt;
        const bool     clean_copy = kept.clean && o != &A->user;
        // the diagnostic also times the gather kernels by device events: [0, 1] around the clean gather, [2, 3] around the
        // diagonal's and the plans' (no host synchronisation in between either way)
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        auto mark = [&](int i) {
            if(ev[i] && e.ok())
                e.hip(hipEventRecord(ev[i], s));
        };
        {
            StreamDrain drain{s};
            if(bytes && e.ok())
            {
                e.hip(hipMemcpyAsync(A->user.val, val, bytes, hipMemcpyDeviceToHost, s));
                if(kept.mirror && val != A->dev_user.val.ptr && e.ok())
                    e.hip(hipMemcpyAsync(A->dev_user.val.ptr, val, bytes, hipMemcpyDeviceToDevice, s));
            }
            e.hip(lt.synced("revalue_device: values to host view + mirror"));
            if(lt.on)
                for(hipEvent_t &v : ev)
                    if(hipEventCreate(&v) != hipSuccess)
                        v = nullptr;
            const void *clean_vals = val; // the clean CSR's value array in HBM: the new values themselves, or the gathered copy
            long long   clean_n    = A->nnz;
            if(clean_copy)
            {
                const aoclsparse_int total = o->nnz;
                mark(0);
                if(e.ok())
                    e.status(launch_revalue_gather(s, total, A->nnz, A->clean_src.as<const int>(), val, cval.ptr, vsz, false));
                mark(1);
                if(e.ok() && total > 0)
                    e.hip(hipMemcpyAsync(o->val, cval.ptr, vsz * (size_t)total, hipMemcpyDeviceToHost, s));
                clean_vals = cval.ptr, clean_n = total;
                e.hip(lt.synced("revalue_device: clean gather + copy back"));
            }
            mark(2);
            if(kept.diag && e.ok())
                e.status(launch_revalue_gather(s, A->m, clean_n, A->diag_src.as<const int>(), clean_vals, A->dev_diag.ptr, vsz, false));
            for(int i = 0; i < 6 && e.ok(); i++)
            {
                if(!(kept.plans >> i & 1u))
                    continue;
                TrsvPlan &p = A->trsv_plan[i];
                if(p.rows_valid)
                    e.status(launch_revalue_gather(s, p.nnz_tri, clean_n, p.psrc.as<const int>(), clean_vals, p.pval.ptr, vsz, p.conj));
                if(p.blk.valid && e.ok())
                    e.status(launch_revalue_gather(s, p.nnz_tri, clean_n, p.blk.psrc.as<const int>(), clean_vals, p.blk.pval.ptr, vsz, p.conj));
            }
            // the operators that follow: their device values in place, the host view by one copy back each
            if(kept.operators)
                for(auto &dv : A->derived)
                {
                    if(!dv->follows(vsz) || !e.ok() || dv->host.nnz <= 0)
                        continue;
                    e.status(launch_revalue_gather_flagged(s, dv->host.nnz, clean_n, dv->src.as<const unsigned>(), clean_vals,
                                                           dv->dev.val.ptr, vsz));
                    if(e.ok())
                        e.hip(hipMemcpyAsync(dv->host.val, dv->dev.val.ptr, vsz * (size_t)dv->host.nnz, hipMemcpyDeviceToHost, s));
                }
            mark(3);
            // the one wait: the copies back have landed; `cval`, the caller's array and a refresh's buffer are no longer read
            // (an empty update has enqueued nothing)
            if((bytes || follow_maps) && e.ok())
                e.hip(hipStreamSynchronize(s));
            if(e.ok())
                drain.dismiss();
        }
        lt.lap("revalue_device: diagonal + plan gathers");
        for(int i = 0; i < 4; i += 2)
        {
            float ms = 0.0f;
            if(e.ok() && ev[i] && ev[i + 1] && (i == 2 || clean_copy) && hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess)
                std::fprintf(stderr, "[mi355 timing]     %-30s %8.3f ms\n",
                             i ? "revalue_device: plan gather events" : "revalue_device: clean gather events", ms);
        }
        for(hipEvent_t v : ev)
            if(v)
                (void)hipEventDestroy(v);
    }

    // THE way new values enter a CSR handle from HBM; called with the stage lock and the handle's guard held.  `val`: A->nnz values
    // of vsz bytes in CSR order -- the caller's array, or the mirror's own (in place).  follow_maps: the clean CSR, the diagonal,
    // the TRSV plans and the operators that hold a value map get the new values through it (revalue_kernels.hip); what has no map,
    // and everything without the flag, is dropped and rebuilt lazily.  `produced`: the status of what wrote `val` INTO THE HANDLE
    // before the call (the triplet refresh).  One host wait.  A failure behind the first write into the handle leaves, on every
    // route: everything derived dropped, each value map with its holder (no plan with some old and some new values), the mirror
    // invalid (it may hold either values: the next product uploads the host view), the error cleared and the stream drained.
    aoclsparse_status commit_values_device(aoclsparse_matrix A, const void *val, size_t vsz, bool follow_maps,
                                           aoclsparse_status produced = aoclsparse_status_success)
    {
        StreamLaps lt{Runtime::get().stream(), PhaseTimer::on() && follow_maps}; // (where a revalue's time goes; the laps then wait for the stream)
        const ValuesKept kept = values_kept(A, vsz, follow_maps);
        DeviceBuffer     cval;
        if(kept.clean && A->opt != &A->user && A->opt->nnz > 0)
            MI355_TRY(cval.alloc(vsz * (size_t)A->opt->nnz)); // (nothing written yet: the handle is as it was; only ?revalue_device comes here)
        FirstError e{produced};
        enqueue_values(A, val, vsz, follow_maps, kept, cval, lt, e);
        // commit: the list drops what has not been given the new values -- after a failure, everything
        A->op_dropped_by_value_change += (long long)drop_derived_state(A, e.ok() ? kept : ValuesKept{});
        if(e.ok() && follow_maps)
            A->revalues++, A->last_kept_plans = __builtin_popcount(kept.plans), A->op_followed = (int)A->derived.size();
        return e.rc;
    }

    // ?update_values_device (follow_maps == false) and ?revalue_device (true).  Before the device is touched: the statuses of
    // ?update_values, then the handles whose values follow the caller's COO / CSC arrays on the host, the runtime, the pointer's kind
    aoclsparse_status update_values_device(aoclsparse_matrix A, aoclsparse_int len, const void *val, aoclsparse_matrix_data_type vt,
                                           bool follow_maps)
    {
        MI355_TRY(update_values_status(A, len, val, vt));
        if(A->input_format == aoclsparse_coo_mat || A->csc_ptr)
            return aoclsparse_status_not_implemented;
        Runtime &rt = Runtime::get();
        MI355_TRY(rt.init());
        if(!rt.is_device_pointer(val))
            return aoclsparse_status_invalid_pointer;
        std::lock_guard<std::recursive_mutex> sl(rt.stage_lock); // (before the handle's guard, as everywhere)
        std::unique_lock<std::shared_mutex>   w(A->guard);
        return commit_values_device(A, val, val_size(vt), follow_maps);
    }

    // the triplets' new values through the kept map (coo_sort_kernels.hip): one kernel puts them into CSR order (or adds them into
    // it), in the mirror's own value array while the mirror follows, else in a buffer of this call's; then as ?update_values_device
    aoclsparse_status refresh_values_from_coo_device(aoclsparse_matrix A, aoclsparse_int len, const void *val,
                                                     aoclsparse_matrix_data_type vt)
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
        Runtime &rt = Runtime::get();
        MI355_TRY(rt.init());
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
        const size_t vsz   = val_size(vt), bytes = vsz * (size_t)A->nnz;
        const bool   keep  = mirror_follows(A, bytes);
        DeviceBuffer tmp; // (released behind commit_values_device's wait: only behind the work that reads it)
        if(!keep)
            MI355_TRY(tmp.alloc(bytes));
        void *const out  = keep ? A->dev_user.val.ptr : tmp.ptr;
        const bool  cplx = vt == aoclsparse_cmat || vt == aoclsparse_zmat;
        // (in stream order behind every product enqueued on the library's stream: they read the old values)
        return commit_values_device(A, out, vsz, false,
                                    device_coo_refresh_values(rt.stream(), len, A->nnz, sum, A->coo_pos.as<const int>(),
                                                              A->coo_runs.as<const int>(), val, vsz, cplx, out));
    }

    // aoclsparse_mi355_clean_csr_device, in stages that correspond to its laps.  Everything is built in buffers of the call's and
    // committed at the very end; until then the handle is as it was (a mirror upload aside).  The mirror itself is never written.
    struct CleanBuild
    {
        aoclsparse_matrix    A;
        hipStream_t          s;
        Runtime             &rt  = Runtime::get();
        const DeviceCsr     &d   = A->dev_user;
        const size_t         vsz = val_size(A->val_type), rb = sizeof(int) * (size_t)std::max<aoclsparse_int>(A->user.m, 1);
        const aoclsparse_int m = A->user.m, n = A->user.n, nnz = A->nnz; // (what csr_optimize reads)
        StreamLaps           lt{s};
        int                   base  = 0;
        const aoclsparse_int *d_ptr = nullptr, *src_ind = nullptr; // the mirror's row pointer; the columns and values the clean CSR
        const void           *src_val = nullptr; // is made from: the mirror's, or their sorted copies
        MatCheckResult        h{};
        bool                  sorted = false, fulldiag = false, copy = false; // class <= 2 is check_sort_diag's `sorted`
        aoclsparse_int        total  = 0; // entries of the clean CSR; ib, vb: the bytes of its columns and values
        size_t                ib = 0, vb = 0;
        int                  *at_p = nullptr, *miss_p = nullptr, *cnt_p = nullptr; // staging slots, per row (CLN_SLOT_*)
        DeviceBuffer          sind, sval, cptr, cind, cval, didiag, diurow, ddiag;
        DeviceBuffer          pind, perm, csrc, dsrc; // the value maps of a handle that keeps them (and their scratch)
        std::unique_ptr<HostCsr>          c;
        std::unique_ptr<aoclsparse_int[]> idiag, iurow;
        // (declared last: whatever way out is taken, the stream first finishes what was enqueued on the staging slots and on the
        // buffers above, and only then are they released)
        StreamDrain drain{s};

        // mat_check's answer over the resident mirror, once: the row pointer first (the kernels below trust it)
        aoclsparse_status mirror_and_check()
        {
            MI355_TRY(resident_mirror(A));
            base = (int)d.base, d_ptr = d.ptr.as<const aoclsparse_int>();
            src_ind = d.ind.as<const aoclsparse_int>(), src_val = d.val.ptr;
            MI355_TRY(device_mat_check(s, m, n, nnz, base, d_ptr, src_ind, h));
            MI355_TRY(matcheck_status(h));
            sorted = h.cls <= 2, fulldiag = !h.notfull, copy = !sorted || !fulldiag;
            lt.lap("clean_csr_device: mirror + check");
            return aoclsparse_status_success;
        }

        // case 3: the rows into ascending order first, on a copy of the mirror's columns and values
        aoclsparse_status sort_rows()
        {
            if(sorted)
                return aoclsparse_status_success;
            MI355_TRY(sind.clone_from(d.ind, s));
            MI355_TRY(sval.clone_from(d.val, s));
            MI355_TRY(device_order_rows(s, m, n, nnz, base, d_ptr, sind.as<aoclsparse_int>(), sval.ptr, vsz));
            src_ind = sind.as<const aoclsparse_int>(), src_val = sval.ptr;
            lt.lap("clean_csr_device: sort");
            if(!A->keep_maps)
                return aoclsparse_status_success;
            // The sort's permutation: the same sort over a second copy of the columns, moving the entries' positions as its 4-byte
            // items.  The sort never computes with an item and is a function of the columns alone, so perm[q] = where sorted entry q
            // stands in the user's arrays.  The arrays sorted above are the ones the call without maps sorts.
            MI355_TRY(pind.clone_from(d.ind, s));
            MI355_TRY(perm.alloc(sizeof(int) * (size_t)std::max<aoclsparse_int>(nnz, 1)));
            MI355_TRY(launch_revalue_iota(s, nnz, perm.as<int>()));
            MI355_TRY(device_order_rows(s, m, n, nnz, base, d_ptr, pind.as<aoclsparse_int>(), perm.ptr, sizeof(int)));
            lt.lap("clean_csr_device: sort of the positions");
            return aoclsparse_status_success;
        }

        // mark, and for a copy the clean row pointer with its 64-bit total
        aoclsparse_status mark_and_scan()
        {
            void *p = nullptr;
            MI355_TRY(rt.staging(CLN_SLOT_AT, rb, &p));
            at_p = static_cast<int *>(p);
            MI355_TRY(rt.staging(CLN_SLOT_MISS, rb, &p));
            miss_p = static_cast<int *>(p);
            MI355_TRY(rt.staging(CLN_SLOT_CNT, rb, &p));
            cnt_p = static_cast<int *>(p);
            MI355_TRY(launch_clean_mark(s, m, n, nnz, base, d_ptr, src_ind, at_p, miss_p, cnt_p));
            total = nnz;
            if(!copy)
                return aoclsparse_status_success;
            MI355_TRY(cptr.alloc(sizeof(aoclsparse_int) * ((size_t)m + 1)));
            MI355_TRY(rt.staging(CLN_SLOT_SCAN, spg_scan_scratch_bytes(m), &p));
            long long *total_dev = nullptr, total_ll = 0;
            MI355_TRY(launch_spg_scan(s, m, cnt_p, cptr.as<aoclsparse_int>(), static_cast<long long *>(p), &total_dev));
            MI355_HIP_TRY(hipMemcpyAsync(&total_ll, total_dev, sizeof(total_ll), hipMemcpyDeviceToHost, s));
            MI355_HIP_TRY(hipStreamSynchronize(s));
            if(total_ll > (long long)std::numeric_limits<aoclsparse_int>::max())
                return aoclsparse_status_invalid_size; // nnz + the inserted entries do not fit the index type
            if(total_ll < (long long)nnz || total_ll > (long long)nnz + std::min(m, n))
                return aoclsparse_status_internal_error;
            total = (aoclsparse_int)total_ll;
            lt.lap("clean_csr_device: mark + scan");
            return aoclsparse_status_success;
        }

        // the host arrays the result goes into: big ones as build_transpose allocates them
        aoclsparse_status host_arrays()
        {
            idiag.reset(new(std::nothrow) aoclsparse_int[m > 0 ? m : 1]);
            iurow.reset(new(std::nothrow) aoclsparse_int[m > 0 ? m : 1]);
            if(!idiag || !iurow)
                return aoclsparse_status_memory_error;
            ib = sizeof(aoclsparse_int) * (size_t)total, vb = vsz * (size_t)total;
            if(!copy)
                return aoclsparse_status_success;
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
            return aoclsparse_status_success;
        }

        // the clean arrays (a copy only), idiag / iurow and the diagonal's values; the maps of a handle that keeps them
        aoclsparse_status expand_and_finish()
        {
            MI355_TRY(didiag.alloc(rb));
            MI355_TRY(diurow.alloc(rb));
            MI355_TRY(ddiag.alloc(vsz * (size_t)std::max<aoclsparse_int>(m, 1)));
            if(copy)
            {
                MI355_TRY(cind.alloc(ib));
                MI355_TRY(cval.alloc(vb));
                if(A->keep_maps)
                    MI355_TRY(csrc.alloc(sizeof(int) * (size_t)std::max<aoclsparse_int>(total, 1)));
                MI355_TRY(launch_clean_expand(s, m, nnz, total, base, d_ptr, src_ind, src_val, vsz, cptr.as<const aoclsparse_int>(), at_p,
                                              miss_p, cind.as<aoclsparse_int>(), cval.ptr, csrc.as<int>()));
                // (positions in the sorted arrays so far: through the sort's permutation they are positions in the user's)
                if(csrc.ptr && !sorted)
                    MI355_TRY(launch_revalue_compose(s, total, nnz, perm.as<const int>(), csrc.as<int>()));
            }
            MI355_TRY(launch_clean_finish(s, m, n, nnz, base, d_ptr, src_val, vsz, copy ? cptr.as<const aoclsparse_int>() : nullptr, at_p,
                                          miss_p, didiag.as<aoclsparse_int>(), diurow.as<aoclsparse_int>(), ddiag.ptr));
            if(A->keep_maps) // the diagonal's map, from what the finish kernel has just written
            {
                MI355_TRY(dsrc.alloc(rb));
                MI355_TRY(launch_revalue_diag_map(s, m, n, copy ? 0 : base, total, didiag.as<const aoclsparse_int>(),
                                                  diurow.as<const aoclsparse_int>(), dsrc.as<int>()));
            }
            MI355_HIP_TRY(lt.synced("clean_csr_device: expand + finish")); // (the diagnostic separates the kernels from the copy back)
            return aoclsparse_status_success;
        }

        // the one copy back; the diagonal's values stay in HBM
        aoclsparse_status copy_back()
        {
            if(m > 0)
            {
                MI355_HIP_TRY(hipMemcpyAsync(idiag.get(), didiag.ptr, sizeof(aoclsparse_int) * (size_t)m, hipMemcpyDeviceToHost, s));
                MI355_HIP_TRY(hipMemcpyAsync(iurow.get(), diurow.ptr, sizeof(aoclsparse_int) * (size_t)m, hipMemcpyDeviceToHost, s));
            }
            if(copy)
                MI355_HIP_TRY(hipMemcpyAsync(c->ptr, cptr.ptr, sizeof(aoclsparse_int) * ((size_t)m + 1), hipMemcpyDeviceToHost, s));
            if(copy && total > 0)
            {
                MI355_HIP_TRY(hipMemcpyAsync(c->ind, cind.ptr, ib, hipMemcpyDeviceToHost, s));
                MI355_HIP_TRY(hipMemcpyAsync(c->val, cval.ptr, vb, hipMemcpyDeviceToHost, s));
            }
            MI355_HIP_TRY(hipStreamSynchronize(s));
            lt.lap("clean_csr_device: copy back");
            return aoclsparse_status_success;
        }

        // what csr_optimize sets, and the diagonal ensure_trsv would otherwise gather on the host and upload
        void commit()
        {
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
        }
    };

    // The key ensure_derived looks an operator up by: H folds to T where the products fold it, symmetric and Hermitian operators
    // ignore the operation
    struct OperatorKey
    {
        int type, fill, diag, trans;
    };
    OperatorKey operator_key(const aoclsparse_mat_descr descr, aoclsparse_operation op)
    {
        const bool tri = descr->type == aoclsparse_matrix_type_triangular;
        return {(int)descr->type, (int)descr->fill_mode, (int)descr->diag_type, tri && op != aoclsparse_operation_none ? 1 : 0};
    }
    Derived *find_operator(const _aoclsparse_matrix *A, const OperatorKey &k)
    {
        for(auto &d : A->derived)
            if(d->type == k.type && d->fill == k.fill && d->diag == k.diag && d->trans == k.trans)
                return d.get();
        return nullptr;
    }
    // what the three operator calls decide alike, before anything else
    aoclsparse_status operator_args_status(const _aoclsparse_matrix *A, const aoclsparse_mat_descr descr, aoclsparse_operation op)
    {
        if(!A || !descr)
            return aoclsparse_status_invalid_pointer;
        const bool valid_type = descr->type >= aoclsparse_matrix_type_general && descr->type <= aoclsparse_matrix_type_triangular;
        const bool valid_op   = op == aoclsparse_operation_none || op == aoclsparse_operation_transpose
                              || op == aoclsparse_operation_conjugate_transpose;
        if(descr->base != A->base || !valid_type || !valid_op)
            return aoclsparse_status_invalid_value;
        return aoclsparse_status_success;
    }

    // aoclsparse_mi355_build_operator_device behind its statuses; called with the stage lock and the handle's guard held, the clean
    // CSR made and no operator of this key on the handle.  Everything is built in buffers of the call's and registered at the very
    // end; until then the handle is as it was (a mirror upload aside).
    aoclsparse_status build_operator_device(aoclsparse_matrix A, const OperatorKey &key)
    {
        Runtime       &rt  = Runtime::get();
        hipStream_t    s   = rt.stream();
        const HostCsr &o   = *A->opt;
        const bool     own = A->opt == &A->user;
        const size_t   vsz = val_size(A->val_type), rb = sizeof(aoclsparse_int) * (size_t)std::max<aoclsparse_int>(o.m, 1);
        if(!o.ptr || !o.ind || !o.val || !o.idiag || !o.iurow || o.m != A->m || o.n != A->n)
            return aoclsparse_status_internal_error;
        StreamLaps               lt{s};
        std::unique_ptr<Derived> d(new(std::nothrow) Derived);
        if(!d)
            return aoclsparse_status_memory_error;
        d->type = key.type, d->fill = key.fill, d->diag = key.diag, d->trans = key.trans;
        DeviceBuffer   cp, ci, cv, didiag, diurow, optr, oind, oval, osrc;
        aoclsparse_int nnz = 0;
        FirstError     e;
        {
            StreamDrain     drain{s}; // (after a failure: nothing in flight into the buffers above when they go)
            DerivedDeviceIn in;
            in.m = o.m, in.n = o.n, in.nnz = o.nnz, in.base = (int)o.base, in.vsize = vsz, in.cplx = is_complex_type(A->val_type);
            in.type = (aoclsparse_matrix_type)key.type, in.upper = key.fill == (int)aoclsparse_fill_mode_upper;
            in.diag = (aoclsparse_diag_type)key.diag, in.transposed = key.trans != 0;
            // the clean CSR as an operand: the handle's own arrays through the resident mirror, a copy through buffers of this call
            if(own)
            {
                e.status(resident_mirror(A));
                const DeviceCsr &m = A->dev_user;
                in.ptr = m.ptr.as<const aoclsparse_int>(), in.ind = m.ind.as<const aoclsparse_int>(), in.val = m.val.ptr;
                in.nnz = A->nnz;
            }
            else
            {
                const size_t ne = (size_t)std::max<aoclsparse_int>(o.nnz, 1);
                e.status(cp.upload(o.ptr, sizeof(aoclsparse_int) * ((size_t)o.m + 1), s));
                if(e.ok())
                    e.status(ci.alloc(sizeof(aoclsparse_int) * ne));
                if(e.ok())
                    e.status(cv.alloc(vsz * ne));
                if(e.ok() && o.nnz > 0)
                {
                    e.hip(hipMemcpyAsync(ci.ptr, o.ind, sizeof(aoclsparse_int) * (size_t)o.nnz, hipMemcpyHostToDevice, s));
                    e.hip(hipMemcpyAsync(cv.ptr, o.val, vsz * (size_t)o.nnz, hipMemcpyHostToDevice, s));
                }
                in.ptr = cp.as<const aoclsparse_int>(), in.ind = ci.as<const aoclsparse_int>(), in.val = cv.ptr;
            }
            if(e.ok())
                e.status(didiag.upload(o.idiag, rb, s));
            if(e.ok())
                e.status(diurow.upload(o.iurow, rb, s));
            in.idiag = didiag.as<const aoclsparse_int>(), in.iurow = diurow.as<const aoclsparse_int>();
            e.hip(lt.synced("build_operator_device: operands"));
            if(e.ok())
                e.status(device_build_derived(s, in, optr, oind, oval, osrc, &nnz));
            lt.lap("build_operator_device: kernels");
            // the host view by one copy back
            HostCsr &h = d->host;
            if(e.ok())
            {
                const bool sym = key.type != (int)aoclsparse_matrix_type_triangular;
                h.m = (sym || !key.trans) ? o.m : o.n, h.n = (sym || !key.trans) ? o.n : o.m;
                h.nnz = nnz, h.base = aoclsparse_index_base_zero;
                const size_t ib = sizeof(aoclsparse_int) * (size_t)std::max<aoclsparse_int>(nnz, 1);
                const size_t vb = vsz * (size_t)std::max<aoclsparse_int>(nnz, 1);
                h.owned = h.result_arrays = true;
                h.ptr = new(std::nothrow) aoclsparse_int[(size_t)h.m + 1];
                h.ind = static_cast<aoclsparse_int *>(host_result_alloc(ib));
                h.val = host_result_alloc(vb);
                if(!h.ptr || !h.ind || !h.val)
                    e.status(aoclsparse_status_memory_error);
                else
                {
                    host_result_touch(h.ind, ib);
                    host_result_touch(h.val, vb);
                    e.hip(hipMemcpyAsync(h.ptr, optr.ptr, sizeof(aoclsparse_int) * ((size_t)h.m + 1), hipMemcpyDeviceToHost, s));
                    if(nnz > 0)
                    {
                        e.hip(hipMemcpyAsync(h.ind, oind.ptr, sizeof(aoclsparse_int) * (size_t)nnz, hipMemcpyDeviceToHost, s));
                        e.hip(hipMemcpyAsync(h.val, oval.ptr, vsz * (size_t)nnz, hipMemcpyDeviceToHost, s));
                    }
                    e.hip(hipStreamSynchronize(s));
                }
            }
            if(e.ok())
                drain.dismiss();
        }
        lt.lap("build_operator_device: host view");
        if(!e.ok())
        {
            (void)hipGetLastError();
            return e.rc;
        }
        DeviceCsr &dv = d->dev;
        dv.ptr.adopt(optr), dv.ind.adopt(oind), dv.val.adopt(oval);
        dv.m = d->host.m, dv.n = d->host.n, dv.nnz = nnz, dv.base = aoclsparse_index_base_zero;
        dv.valid = true;
        // the row-block plan and the SELL-64 copy as ensure_derived builds them
        e.status(build_spmv_plan(d->host.m, d->host.nnz, d->host.base, d->host.ptr, d->plan, vsz));
        if(e.ok() && A->mem_policy == aoclsparse_memory_usage_unrestricted && !is_complex_type(A->val_type))
            e.status(build_sell(d->host.ptr, d->dev, vsz, d->plan));
        lt.lap("build_operator_device: plan + SELL-64 copy");
        d->on_device = true;
        if(A->keep_maps) // the source map stays: ?revalue_device gathers the values through it again
            d->src.adopt(osrc), d->mapped = true;
        if(e.ok())
            try
            {
                A->derived.push_back(std::move(d));
                A->op_device_builds++;
            }
            catch(const std::bad_alloc &)
            {
                e.status(aoclsparse_status_memory_error);
            }
        if(!e.ok()) // (the operator goes with `d`: nothing in flight into its buffers by then)
            (void)hipStreamSynchronize(s), (void)hipGetLastError();
        return e.rc;
    }
} // namespace

namespace mi355
{
aoclsparse_status revalue_device_any(aoclsparse_matrix A, aoclsparse_int len, const void *val)
{
    return A ? update_values_device(A, len, val, A->val_type, true) : aoclsparse_status_invalid_pointer;
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
    return update_values_device(A, len, val, aoclsparse_smat, false);
}
aoclsparse_status aoclsparse_mi355_dupdate_values_device(aoclsparse_matrix A, aoclsparse_int len, const double *val)
{
    return update_values_device(A, len, val, aoclsparse_dmat, false);
}
aoclsparse_status aoclsparse_mi355_cupdate_values_device(aoclsparse_matrix A, aoclsparse_int len, const aoclsparse_float_complex *val)
{
    return update_values_device(A, len, val, aoclsparse_cmat, false);
}
aoclsparse_status aoclsparse_mi355_zupdate_values_device(aoclsparse_matrix A, aoclsparse_int len, const aoclsparse_double_complex *val)
{
    return update_values_device(A, len, val, aoclsparse_zmat, false);
}

aoclsparse_status aoclsparse_mi355_srevalue_device(aoclsparse_matrix A, aoclsparse_int len, const float *val)
{
    return update_values_device(A, len, val, aoclsparse_smat, true);
}
aoclsparse_status aoclsparse_mi355_drevalue_device(aoclsparse_matrix A, aoclsparse_int len, const double *val)
{
    return update_values_device(A, len, val, aoclsparse_dmat, true);
}
aoclsparse_status aoclsparse_mi355_crevalue_device(aoclsparse_matrix A, aoclsparse_int len, const aoclsparse_float_complex *val)
{
    return update_values_device(A, len, val, aoclsparse_cmat, true);
}
aoclsparse_status aoclsparse_mi355_zrevalue_device(aoclsparse_matrix A, aoclsparse_int len, const aoclsparse_double_complex *val)
{
    return update_values_device(A, len, val, aoclsparse_zmat, true);
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

aoclsparse_status aoclsparse_mi355_build_operator_device(aoclsparse_matrix A, const aoclsparse_mat_descr descr, aoclsparse_operation op)
{
    // decided before the device is touched, in this order
    MI355_TRY(operator_args_status(A, descr, op));
    if(descr->type == aoclsparse_matrix_type_general)
        return aoclsparse_status_not_implemented;
    if(A->input_format != aoclsparse_csr_mat || A->csc_ptr) // COO-, CSC-, TCSR- and BSR-created handles, as ?revalue_device
        return aoclsparse_status_not_implemented;
    const bool sym = descr->type != aoclsparse_matrix_type_triangular;
    if(descr->type == aoclsparse_matrix_type_hermitian && !is_complex_type(A->val_type))
        return aoclsparse_status_not_implemented;
    if(sym && A->m != A->n)
        return aoclsparse_status_invalid_size;
    if(A->m == 0 || A->n == 0 || A->nnz == 0)
        return aoclsparse_status_success;
    if(!A->user.ptr || !A->user.ind || !A->user.val)
        return aoclsparse_status_invalid_pointer;
    const OperatorKey key = operator_key(descr, op);
    Runtime          &rt  = Runtime::get();
    MI355_TRY(rt.init());
    std::lock_guard<std::recursive_mutex> sl(rt.stage_lock); // (before the handle's guard, as everywhere)
    MI355_TRY(csr_optimize(A)); // the clean CSR as ensure_derived makes it, or the copy clean_csr_device has made (takes the guard itself)
    std::unique_lock<std::shared_mutex> w(A->guard);
    if(!A->opt)
        return aoclsparse_status_internal_error;
    if(find_operator(A, key)) // however it was built
        return aoclsparse_status_success;
    return build_operator_device(A, key);
}

aoclsparse_status aoclsparse_mi355_get_operator_info(aoclsparse_matrix A, const aoclsparse_mat_descr descr, aoclsparse_operation op,
                                                     aoclsparse_mi355_operator_info *info)
{
    if(!info)
        return aoclsparse_status_invalid_pointer;
    MI355_TRY(operator_args_status(A, descr, op));
    if(info->struct_size < sizeof(info->struct_size))
        return aoclsparse_status_invalid_size;
    aoclsparse_mi355_operator_info r{};
    {
        std::shared_lock<std::shared_mutex> g(A->guard);
        if(const Derived *d = find_operator(A, operator_key(descr, op)))
        {
            r.present = 1, r.built_on_device = d->on_device, r.mapped = d->mapped && d->src.ptr;
            r.rows = d->host.m, r.cols = d->host.n, r.nnz = d->host.nnz;
            r.sell_copy        = d->plan.sell.valid || (d->plan.sell.stale && d->plan.sell.st.built);
            r.sell_value_fills = d->plan.sell.count.value_fills;
            r.map_bytes        = (long long)d->src.bytes;
        }
        r.followed = A->op_followed;
        r.device_builds = A->op_device_builds, r.host_builds = A->op_host_builds;
        r.dropped_by_value_change = A->op_dropped_by_value_change;
    }
    r.struct_size = info->struct_size; // (the caller's: it says how much of the struct the caller has)
    std::memcpy(info, &r, std::min(info->struct_size, sizeof(r))); // no more than that is written
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_mi355_export_operator(aoclsparse_matrix A, const aoclsparse_mat_descr descr, aoclsparse_operation op,
                                                   aoclsparse_int *rows, aoclsparse_int *cols, aoclsparse_int *nnz,
                                                   const aoclsparse_int **row_ptr, const aoclsparse_int **col_ind, const void **val)
{
    if(!rows || !cols || !nnz || !row_ptr || !col_ind || !val)
        return aoclsparse_status_invalid_pointer;
    MI355_TRY(operator_args_status(A, descr, op));
    std::shared_lock<std::shared_mutex> g(A->guard);
    const Derived                      *d = find_operator(A, operator_key(descr, op));
    if(!d || !d->host.ptr)
        return aoclsparse_status_invalid_value;
    *rows = d->host.m, *cols = d->host.n, *nnz = d->host.nnz;
    *row_ptr = d->host.ptr, *col_ind = d->host.ind, *val = d->host.val;
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
    Runtime &rt = Runtime::get();
    MI355_TRY(rt.init());
    std::lock_guard<std::recursive_mutex> sl(rt.stage_lock); // (before the handle's guard, as everywhere)
    std::unique_lock<std::shared_mutex>   w(A->guard);
    hipStream_t                           s   = rt.stream();
    const size_t                          vsz = val_size(A->val_type);
    DeviceCsr                            &d   = A->dev_user;
    MI355_TRY(resident_mirror(A)); // (up to here the handle is unchanged)
    // The mirror is sorted IN PLACE, behind every product enqueued on the library's stream; one copy back commits the host view
    // once all device work has succeeded.  A failure before that leaves the host view as it was and everything derived dropped.
    MatCheckResult h{};
    long long      moved = 0;
    StreamLaps     lt{s};
    FirstError     e;
    {
        StreamDrain drain{s};
        e.status(device_order_rows(s, d.m, d.n, d.nnz, (int)d.base, d.ptr.as<const aoclsparse_int>(), d.ind.as<aoclsparse_int>(),
                                   d.val.ptr, vsz, &moved));
        lt.lap("order_mat_device: sort");
        // sort class and full diagonal again, over the sorted arrays: mat_check's answer (the row pointer was checked at creation)
        if(e.ok())
            e.status(device_mat_check(s, d.m, d.n, d.nnz, (int)d.base, d.ptr.as<const aoclsparse_int>(), d.ind.as<const aoclsparse_int>(),
                                      h, true));
        lt.lap("order_mat_device: check kernel");
        if(e.ok())
            drain.dismiss();
    }
    if(!e.ok())
    {
        drop_derived_state(A); // (d.valid = false with it)
        return e.rc;
    }
    if(moved > 0) // the one copy back; rows that were ascending were not touched, so nothing moved means nothing to bring
    {
        e.hip(hipMemcpyAsync(A->user.ind, d.ind.ptr, sizeof(aoclsparse_int) * (size_t)d.nnz, hipMemcpyDeviceToHost, s));
        e.hip(hipMemcpyAsync(A->user.val, d.val.ptr, vsz * (size_t)d.nnz, hipMemcpyDeviceToHost, s));
        e.hip(hipStreamSynchronize(s));
        lt.lap("order_mat_device: host view");
    }
    // A copy back that fails may have written part of the host view.  The class and the diagonal flag then stay what they were
    // for the unsorted arrays (nothing may take the host view for sorted), and the mirror -- which IS sorted, every row of it --
    // stays the handle's resident CSR, so no product uploads that view.
    if(e.ok() && !h.first_err) // (as the host call: a row mat_check refuses leaves the two as they were, and is no failure here)
        A->sort = h.cls ? h.cls : 1, A->fulldiag = !h.notfull;
    ValuesKept sorted;
    sorted.mirror = true; // the mirror IS the handle's CSR now: resident before any product
    drop_order_dependent_state(A, sorted);
    if(!e.ok())
        (void)hipGetLastError();
    return e.rc;
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
    Runtime &rt = Runtime::get();
    MI355_TRY(rt.init());
    std::lock_guard<std::recursive_mutex> sl(rt.stage_lock); // (before the handle's guard, as everywhere)
    std::unique_lock<std::shared_mutex>   w(A->guard);
    if(A->opt) // (another thread's csr_optimize got here first)
        return aoclsparse_status_success;
    CleanBuild b{A, rt.stream()};
    MI355_TRY(b.mirror_and_check());
    MI355_TRY(b.sort_rows());
    MI355_TRY(b.mark_and_scan());
    MI355_TRY(b.host_arrays());
    MI355_TRY(b.expand_and_finish());
    MI355_TRY(b.copy_back());
    b.commit(); // (nothing of the handle was written before this line, except a mirror upload)
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
    Runtime &rt = Runtime::get();
    MI355_TRY(rt.init());
    std::lock_guard<std::recursive_mutex> sl(rt.stage_lock);
    std::unique_lock<std::shared_mutex>   w(A->guard);
    MI355_TRY(resident_mirror(A));
    MI355_HIP_TRY(hipStreamSynchronize(rt.stream())); // the caller reads the arrays from streams of its own
    const DeviceCsr &d = A->dev_user;
    *base = (aoclsparse_index_base)d.base, *M = d.m, *N = d.n, *nnz = d.nnz;
    *row_ptr = d.ptr.as<const aoclsparse_int>(), *col_idx = d.ind.as<const aoclsparse_int>(), *val = d.val.ptr;
    return aoclsparse_status_success;
}

} // extern "C"
