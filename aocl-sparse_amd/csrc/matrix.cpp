// matrix.cpp -- descriptor + handle lifecycle, clean-CSR analysis, export, invalidation, value setters, copy, hints.
// (the SpMV plans built on a handle: spmv_plan.cpp, sell_plan.cpp)
//
// Behaviour follows the reference (cited per function, paths relative to
// /root/reference/library/src); the data layout behind the opaque handles is our own.
#include "spg_host.hpp"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <thread>

using namespace mi355;

namespace mi355
{

doid get_doid(const _aoclsparse_mat_descr *d, aoclsparse_operation op)
{
    // include/aoclsparse_mtx_dispatcher.hpp:79-143 for real types (conjugate == transpose)
    const bool tr = op != aoclsparse_operation_none;
    switch(d->type)
    {
    case aoclsparse_matrix_type_general:
        return tr ? doid::gt : doid::gn;
    case aoclsparse_matrix_type_symmetric:
    case aoclsparse_matrix_type_hermitian:
        return d->fill_mode == aoclsparse_fill_mode_lower ? doid::sl : doid::su;
    case aoclsparse_matrix_type_triangular:
        if(d->fill_mode == aoclsparse_fill_mode_lower)
            return tr ? doid::tlt : doid::tln;
        return tr ? doid::tut : doid::tun;
    }
    return doid::len;
}

// ---- validity / sort class / full diagonal: analysis/aoclsparse_csr_util.cpp:124-279 ---------
aoclsparse_status mat_check(aoclsparse_int maj, aoclsparse_int mind, aoclsparse_int nnz,
                            const aoclsparse_int *ptr, const aoclsparse_int *ind, const void *val,
                            int shape, aoclsparse_index_base base, int &sort, bool &fulldiag)
{
    if(!ptr || !ind || !val)
        return aoclsparse_status_invalid_pointer;
    if(mind < 0 || maj < 0 || nnz < 0)
        return aoclsparse_status_invalid_size;
    if(ptr[0] != base || ptr[maj] - base != nnz)
        return aoclsparse_status_invalid_value;
    for(aoclsparse_int i = 0; i < maj; i++)
        if(ptr[i] > ptr[i + 1])
            return aoclsparse_status_invalid_value;

    // Rows are independent (the sort class is the worst class of any row, the diagonal flag an AND, and the reference
    // returns the error of the FIRST offending row): chunks of rows in parallel, merged in row order.  52 M entries: 50 -> a few ms
    // on the GPU box's host (round 3: this pass, check_sort_diag and csr_indices were half of aoclsparse_optimize's time for
    // an sv hint).
    std::atomic<int>       cls_all{1}; // fully sorted until proven otherwise
    std::atomic<bool>      full_all{true};
    std::atomic<long long> first_err{LLONG_MAX}; // (row << 8) | status of the earliest offending row
    parallel_for(maj, 1 << 15, [&](long long i0, long long i1) {
        int  cls  = 1;
        bool full = true;
        for(aoclsparse_int i = (aoclsparse_int)i0; i < (aoclsparse_int)i1; i++)
        {
            const aoclsparse_int lo = shape == 2 ? i : 0;
            const aoclsparse_int hi = shape == 1 ? i : mind - 1;
            bool           seen_diag = false, seen_upper = false;
            aoclsparse_int prev = -1;
            int            err  = 0;
            for(aoclsparse_int p = ptr[i] - base; p < ptr[i + 1] - base && !err; p++)
            {
                const aoclsparse_int j = ind[p] - base;
                if(j < lo || j > hi)
                {
                    err = (int)aoclsparse_status_invalid_index_value;
                    break;
                }
                if(cls != 3)
                {
                    if(prev > j)
                        cls = 2; // order inside a group broken: partially sorted
                    else
                        prev = j;
                    if((j <= i && seen_upper) || (j < i && seen_diag))
                        cls = 3; // L | D | U group order broken: unsorted
                }
                if(j > i)
                    seen_upper = true;
                else if(j == i)
                {
                    if(seen_diag)
                        err = (int)aoclsparse_status_invalid_value; // duplicate diagonal
                    seen_diag = true;
                }
            }
            if(err)
            {
                const long long key = ((long long)i << 8) | err;
                long long       cur = first_err.load();
                while(key < cur && !first_err.compare_exchange_weak(cur, key))
                {
                }
                return; // later rows of this chunk cannot be the first offender
            }
            if(!seen_diag && i < mind)
                full = false;
        }
        int c0 = cls_all.load();
        while(cls > c0 && !cls_all.compare_exchange_weak(c0, cls))
        {
        }
        if(!full)
            full_all.store(false);
    });
    if(first_err.load() != LLONG_MAX)
        return (aoclsparse_status)(first_err.load() & 0xff);
    const int  cls  = cls_all.load();
    const bool full = full_all.load();
    sort     = cls;
    fulldiag = full;
    return aoclsparse_status_success;
}

// ---- group order (L | D | U) + diagonal presence: csr_util.cpp:290-364 -------------------------
aoclsparse_status check_sort_diag(aoclsparse_int m, aoclsparse_int n, aoclsparse_index_base base,
                                  const aoclsparse_int *ptr, const aoclsparse_int *ind, bool &sorted,
                                  bool &fulldiag)
{
    sorted = fulldiag = false;
    if(m < 0 || n < 0)
        return aoclsparse_status_invalid_size;
    if(!ptr || !ind)
        return aoclsparse_status_invalid_pointer;
    // the reference stops at the first row that is out of order (sorted = fulldiag = false) or holds two diagonals
    // (invalid_value): rows are scanned in parallel chunks and the earliest such row decides
    std::atomic<long long> first_evt{LLONG_MAX}; // (row << 1) | (1: duplicate diagonal, 0: unsorted)
    std::atomic<bool>      full_all{true};
    parallel_for(m, 1 << 15, [&](long long i0, long long i1) {
        bool full = true;
        for(aoclsparse_int i = (aoclsparse_int)i0; i < (aoclsparse_int)i1; i++)
        {
            bool in_lower = true, have_diag = false, ok = true;
            int  evt = -1;
            for(aoclsparse_int p = ptr[i] - base; p < ptr[i + 1] - base; p++)
            {
                const aoclsparse_int j = ind[p] - base;
                if(j == i)
                {
                    if(have_diag)
                    {
                        evt = 1;
                        break;
                    }
                    have_diag = true;
                    ok        = in_lower;
                    in_lower  = false;
                }
                else if(in_lower)
                    in_lower = j < i;
                else
                    ok = ok && j > i;
                if(!ok)
                {
                    evt = 0;
                    break;
                }
            }
            if(evt >= 0)
            {
                const long long key = ((long long)i << 1) | evt;
                long long       cur = first_evt.load();
                while(key < cur && !first_evt.compare_exchange_weak(cur, key))
                {
                }
                return;
            }
            if(!have_diag && i < n)
                full = false;
        }
        if(!full)
            full_all.store(false);
    });
    if(first_evt.load() != LLONG_MAX)
    {
        sorted = fulldiag = false;
        return (first_evt.load() & 1) ? aoclsparse_status_invalid_value : aoclsparse_status_success;
    }
    sorted   = true;
    fulldiag = full_all.load();
    return aoclsparse_status_success;
}

// ---- idiag / iurow in the matrix's base: csr_util.cpp:389-458 ----------------------------------
aoclsparse_status csr_indices(aoclsparse_int m, aoclsparse_index_base base,
                              const aoclsparse_int *ptr, const aoclsparse_int *ind,
                              aoclsparse_int **idiag, aoclsparse_int **iurow)
{
    if(m < 0)
        return aoclsparse_status_invalid_size;
    if(!ptr || !ind || !idiag || !iurow)
        return aoclsparse_status_invalid_pointer;
    aoclsparse_int *d = new(std::nothrow) aoclsparse_int[m > 0 ? m : 1];
    aoclsparse_int *u = new(std::nothrow) aoclsparse_int[m > 0 ? m : 1];
    if(!d || !u)
    {
        delete[] d;
        delete[] u;
        return aoclsparse_status_memory_error;
    }
    parallel_for(m, 1 << 15, [&](long long i0, long long i1) {
        for(aoclsparse_int i = (aoclsparse_int)i0; i < (aoclsparse_int)i1; i++)
        {
            const aoclsparse_int e = ptr[i + 1] - base;
            aoclsparse_int       p = ptr[i] - base;
            while(p < e && ind[p] - base < i)
                p++;
            // p: first entry at or right of the diagonal (or row end); positions keep the base
            d[i] = p + base;
            u[i] = (p < e && ind[p] - base == i) ? p + base + 1 : p + base;
        }
    });
    *idiag = d;
    *iurow = u;
    return aoclsparse_status_success;
}

template <typename T>
static aoclsparse_status make_clean_copy(aoclsparse_matrix A, bool sorted, bool &fulldiag,
                                         std::unique_ptr<HostCsr> &out)
{
    // csr_util.hpp:875-951: 0-based copy, per-row sort (csr_util.hpp:100-159), explicit zero
    // diagonals for rows i < n (csr_util.hpp:167-279).
    const HostCsr       &u    = A->user;
    const aoclsparse_int m    = u.m, n = u.n, nnz = A->nnz, b = u.base;
    const T             *uval = static_cast<const T *>(u.val);
    std::vector<aoclsparse_int> tptr(m + 1), tind(nnz);
    std::vector<T>              tval(nnz);
    for(aoclsparse_int i = 0; i <= m; i++)
        tptr[i] = u.ptr[i] - b;
    for(aoclsparse_int p = 0; p < nnz; p++)
    {
        tind[p] = u.ind[p] - b;
        tval[p] = uval[p];
    }
    if(!sorted)
    {
        std::vector<aoclsparse_int> perm;
        for(aoclsparse_int i = 0; i < m; i++)
        {
            const aoclsparse_int s = tptr[i], len = tptr[i + 1] - s;
            perm.resize(len);
            std::iota(perm.begin(), perm.end(), 0);
            std::stable_sort(perm.begin(), perm.end(), [&](aoclsparse_int a, aoclsparse_int c) {
                return u.ind[s + a] < u.ind[s + c];
            });
            for(aoclsparse_int k = 0; k < len; k++)
            {
                tind[s + k] = u.ind[s + perm[k]] - b;
                tval[s + k] = uval[s + perm[k]];
            }
        }
        bool              s2;
        aoclsparse_status st = check_sort_diag(m, n, aoclsparse_index_base_zero, tptr.data(),
                                               tind.data(), s2, fulldiag);
        if(st != aoclsparse_status_success)
            return st;
    }
    aoclsparse_int missing = 0;
    if(!fulldiag)
        for(aoclsparse_int i = 0; i < std::min(m, n); i++)
        {
            bool have = false;
            for(aoclsparse_int p = tptr[i]; p < tptr[i + 1] && !have; p++)
                have = tind[p] == i;
            missing += !have;
        }
    std::unique_ptr<HostCsr> c(new HostCsr);
    c->m = m, c->n = n, c->nnz = nnz + missing, c->base = aoclsparse_index_base_zero;
    c->owned = true;
    c->ptr   = new aoclsparse_int[m + 1];
    c->ind   = new aoclsparse_int[c->nnz > 0 ? c->nnz : 1];
    c->val   = ::operator new(sizeof(T) * (c->nnz > 0 ? c->nnz : 1));
    T             *cval = static_cast<T *>(c->val);
    aoclsparse_int w    = 0;
    for(aoclsparse_int i = 0; i < m; i++)
    {
        c->ptr[i]   = w;
        bool placed = fulldiag || i >= n;
        for(aoclsparse_int p = tptr[i]; p < tptr[i + 1]; p++)
        {
            if(!placed && tind[p] >= i)
            {
                if(tind[p] != i)
                {
                    c->ind[w] = i;
                    cval[w++] = T(0);
                }
                placed = true;
            }
            c->ind[w] = tind[p];
            cval[w++] = tval[p];
        }
        if(!placed)
        {
            c->ind[w] = i;
            cval[w++] = T(0);
        }
    }
    c->ptr[m] = w;
    c->nnz    = w;
    out       = std::move(c);
    return aoclsparse_status_success;
}

// ---- clean CSR, analysis/aoclsparse_csr_util.hpp:765-967 -----------------------------------------
aoclsparse_status csr_optimize(aoclsparse_matrix A)
{
    if(!A)
        return aoclsparse_status_invalid_pointer;
    {
        std::shared_lock<std::shared_mutex> r(A->guard);
        if(A->opt)
            return aoclsparse_status_success;
    }
    std::unique_lock<std::shared_mutex> w(A->guard);
    if(A->opt)
        return aoclsparse_status_success;
    HostCsr &u = A->user;
    if(holds_no_csr(A)) // csr_util.hpp:804-805: no CSR among the matrices of a TCSR or BSR handle (the solves and the
        return aoclsparse_status_not_implemented; // one-triangle products come here with a TCSR triangle's own handle)
    if(!u.ptr || !u.ind || !u.val)
        return aoclsparse_status_invalid_pointer;
    try
    {
        aoclsparse_status st
            = mat_check(u.m, u.n, A->nnz, u.ptr, u.ind, u.val, 0, u.base, A->sort, A->fulldiag);
        if(st != aoclsparse_status_success)
            return st;
        bool sorted, fulldiag;
        st = check_sort_diag(u.m, u.n, u.base, u.ptr, u.ind, sorted, fulldiag);
        if(st != aoclsparse_status_success)
            return aoclsparse_status_internal_error;
        if(sorted && fulldiag)
        {
            // already clean: keep using the caller's memory, only add idiag / iurow
            st = csr_indices(u.m, u.base, u.ptr, u.ind, &u.idiag, &u.iurow);
            if(st != aoclsparse_status_success)
                return st;
            u.is_optimized = true;
            A->opt         = &u;
        }
        else
        {
            std::unique_ptr<HostCsr> c;
            st = dispatch_value_type(A->val_type, [&](auto tag) {
                return make_clean_copy<decltype(tag)>(A, sorted, fulldiag, c);
            });
            if(st != aoclsparse_status_success)
                return st;
            st = csr_indices(c->m, c->base, c->ptr, c->ind, &c->idiag, &c->iurow);
            if(st != aoclsparse_status_success)
                return st;
            c->is_optimized = true;
            A->opt_copy     = std::move(c);
            A->opt          = A->opt_copy.get();
        }
        A->opt_csr_full_diag = fulldiag;
        A->optimized         = true;
        A->clean_builds++; // (an observer: aoclsparse_mi355_get_value_map_info)
    }
    catch(const std::bad_alloc &)
    {
        return aoclsparse_status_memory_error;
    }
    return aoclsparse_status_success;
}

// from this many entries on the handles' transposes are sorted on the device
constexpr aoclsparse_int DEVICE_TRANSPOSE_MIN_NNZ = 1 << 20;

aoclsparse_status build_transpose(aoclsparse_matrix A)
{
    {
        std::shared_lock<std::shared_mutex> r(A->guard);
        if(A->trans)
            return aoclsparse_status_success;
    }
    // (the device sort takes its temporaries from the staging slots: the stage lock comes BEFORE the handle's guard, as everywhere)
    std::lock_guard<std::recursive_mutex> sl(Runtime::get().stage_lock);
    std::unique_lock<std::shared_mutex>   w(A->guard);
    if(A->trans)
        return aoclsparse_status_success;
    try
    {
        std::unique_ptr<HostCsr> t(new HostCsr);
        const size_t             vs = val_size(A->val_type);
        const size_t             nz = (size_t)(A->nnz > 0 ? A->nnz : 1);
        t->m = A->n, t->n = A->m, t->nnz = A->nnz, t->base = aoclsparse_index_base_zero;
        t->owned = t->result_arrays = true;
        t->ptr   = new aoclsparse_int[t->m + 1];
        t->ind   = static_cast<aoclsparse_int *>(host_result_alloc(sizeof(aoclsparse_int) * nz));
        t->val   = host_result_alloc(vs * nz);
        if(!t->ind || !t->val)
            return aoclsparse_status_memory_error;
        // Large matrices: the sort runs on the device (transpose_kernels.hip: same order, 22 -> ~3 ms for 5 M entries) and leaves
        // the transpose in HBM as the handle's dev_trans; the host copy every analysis reads follows over PCIe.  Small ones, and
        // matrices with a column of more than 2,048 entries, take the host sort.
        bool on_device = false;
        if(A->nnz >= DEVICE_TRANSPOSE_MIN_NNZ && A->user.ptr[A->m] - A->base == A->nnz)
        {
            Runtime          &rt = Runtime::get();
            aoclsparse_status st = rt.init();
            if(st == aoclsparse_status_success && !A->dev_user.valid)
                st = upload_csr(A->user, vs, A->dev_user);
            DeviceCsr &dt = A->dev_trans;
            if(st == aoclsparse_status_success) // (dt.ptr / ind / val are allocated by the call once the matrix is accepted, and
                                                // released again on decline or failure: nothing is held while the host sorts)
                st = device_transpose(rt.stream(), A->m, A->n, A->nnz, A->base, A->dev_user.ptr.as<aoclsparse_int>(),
                                      A->dev_user.ind.as<aoclsparse_int>(), A->dev_user.val.ptr, vs, dt.ptr, dt.ind, dt.val);
            if(st == aoclsparse_status_success)
            {
                host_result_touch(t->ind, sizeof(aoclsparse_int) * nz);
                host_result_touch(t->val, vs * nz);
                hipStream_t s = rt.stream();
                if(hipMemcpyAsync(t->ptr, dt.ptr.ptr, sizeof(aoclsparse_int) * ((size_t)t->m + 1), hipMemcpyDeviceToHost, s) == hipSuccess
                   && hipMemcpyAsync(t->ind, dt.ind.ptr, sizeof(aoclsparse_int) * (size_t)A->nnz, hipMemcpyDeviceToHost, s) == hipSuccess
                   && hipMemcpyAsync(t->val, dt.val.ptr, vs * (size_t)A->nnz, hipMemcpyDeviceToHost, s) == hipSuccess
                   && hipStreamSynchronize(s) == hipSuccess)
                {
                    dt.m = t->m, dt.n = t->n, dt.nnz = A->nnz, dt.base = aoclsparse_index_base_zero;
                    dt.valid  = true;
                    on_device = true;
                }
            }
            if(!on_device)
            {
                (void)hipGetLastError(); // (declined or failed: the host sort below serves the handle)
                dt.ptr.release(), dt.ind.release(), dt.val.release();
            }
        }
        if(!on_device)
            dispatch_value_type(A->val_type, [&](auto tag) {
                using T          = decltype(tag); // (the counting sort of spg_host.hpp, 0-based out, over the entries the rows span)
                const HostCsr &u = A->user;
                host_transpose<T>(u.m, u.n, u.ptr[u.m] - u.base, u.base, 0, u.ptr, u.ind, static_cast<const T *>(u.val), t->ptr, t->ind,
                                  static_cast<T *>(t->val));
                return 0;
            });
        A->trans = std::move(t);
    }
    catch(const std::bad_alloc &)
    {
        return aoclsparse_status_memory_error;
    }
    return aoclsparse_status_success;
}

} // namespace mi355

// =====================================================================================================
extern "C" {

// ---- descriptor: extra/aoclsparse_auxiliary.cpp:191-360 -------------------------------------------------
aoclsparse_status aoclsparse_create_mat_descr(aoclsparse_mat_descr *descr)
{
    if(!descr)
        return aoclsparse_status_invalid_pointer;
    *descr = new(std::nothrow) _aoclsparse_mat_descr;
    return *descr ? aoclsparse_status_success : aoclsparse_status_memory_error;
}

aoclsparse_status aoclsparse_copy_mat_descr(aoclsparse_mat_descr dest, const aoclsparse_mat_descr src)
{
    if(!dest || !src)
        return aoclsparse_status_invalid_pointer;
    *dest = *src;
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_destroy_mat_descr(aoclsparse_mat_descr descr)
{
    delete descr; // NULL is a no-op success (:238-246)
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_set_mat_index_base(aoclsparse_mat_descr descr, aoclsparse_index_base base)
{
    if(!descr)
        return aoclsparse_status_invalid_pointer;
    if(base != aoclsparse_index_base_zero && base != aoclsparse_index_base_one)
        return aoclsparse_status_invalid_value;
    descr->base = base;
    return aoclsparse_status_success;
}

aoclsparse_index_base aoclsparse_get_mat_index_base(const aoclsparse_mat_descr descr)
{
    return descr ? descr->base : aoclsparse_index_base_zero;
}

aoclsparse_status aoclsparse_set_mat_type(aoclsparse_mat_descr descr, aoclsparse_matrix_type type)
{
    if(!descr)
        return aoclsparse_status_invalid_pointer;
    if(type != aoclsparse_matrix_type_general && type != aoclsparse_matrix_type_symmetric
       && type != aoclsparse_matrix_type_hermitian && type != aoclsparse_matrix_type_triangular)
        return aoclsparse_status_invalid_value;
    descr->type = type;
    return aoclsparse_status_success;
}

aoclsparse_matrix_type aoclsparse_get_mat_type(const aoclsparse_mat_descr descr)
{
    return descr ? descr->type : aoclsparse_matrix_type_general;
}

aoclsparse_status aoclsparse_set_mat_fill_mode(aoclsparse_mat_descr descr, aoclsparse_fill_mode fill_mode)
{
    if(!descr)
        return aoclsparse_status_invalid_pointer;
    if(fill_mode != aoclsparse_fill_mode_lower && fill_mode != aoclsparse_fill_mode_upper)
        return aoclsparse_status_invalid_value;
    descr->fill_mode = fill_mode;
    return aoclsparse_status_success;
}

aoclsparse_fill_mode aoclsparse_get_mat_fill_mode(const aoclsparse_mat_descr descr)
{
    return descr ? descr->fill_mode : aoclsparse_fill_mode_lower;
}

aoclsparse_status aoclsparse_set_mat_diag_type(aoclsparse_mat_descr descr, aoclsparse_diag_type diag_type)
{
    if(!descr)
        return aoclsparse_status_invalid_pointer;
    if(diag_type != aoclsparse_diag_type_unit && diag_type != aoclsparse_diag_type_non_unit
       && diag_type != aoclsparse_diag_type_zero)
        return aoclsparse_status_invalid_value;
    descr->diag_type = diag_type;
    return aoclsparse_status_success;
}

aoclsparse_diag_type aoclsparse_get_mat_diag_type(const aoclsparse_mat_descr descr)
{
    return descr ? descr->diag_type : aoclsparse_diag_type_non_unit;
}

// ---- create / destroy / export: create/aoclsparse_create.cpp:34-97, auxiliary.cpp:657-671, 1303-1353 ---
static aoclsparse_status create_csr(aoclsparse_matrix *mat, aoclsparse_index_base base,
                                    aoclsparse_int M, aoclsparse_int N, aoclsparse_int nnz,
                                    aoclsparse_int *row_ptr, aoclsparse_int *col_idx, void *val,
                                    aoclsparse_matrix_data_type vt)
{
    if(!mat)
        return aoclsparse_status_invalid_pointer;
    *mat = nullptr;
    int               sort     = 0;
    bool              fulldiag = false;
    aoclsparse_status st = mat_check(M, N, nnz, row_ptr, col_idx, val, 0, base, sort, fulldiag);
    if(st != aoclsparse_status_success)
        return st;
    return alias_csr(mat, base, M, N, nnz, row_ptr, col_idx, val, vt, sort, fulldiag);
}

aoclsparse_status aoclsparse_create_dcsr(aoclsparse_matrix *mat, aoclsparse_index_base base,
                                         aoclsparse_int M, aoclsparse_int N, aoclsparse_int nnz,
                                         aoclsparse_int *row_ptr, aoclsparse_int *col_idx, double *val)
{
    return create_csr(mat, base, M, N, nnz, row_ptr, col_idx, val, aoclsparse_dmat);
}

aoclsparse_status aoclsparse_create_scsr(aoclsparse_matrix *mat, aoclsparse_index_base base,
                                         aoclsparse_int M, aoclsparse_int N, aoclsparse_int nnz,
                                         aoclsparse_int *row_ptr, aoclsparse_int *col_idx, float *val)
{
    return create_csr(mat, base, M, N, nnz, row_ptr, col_idx, val, aoclsparse_smat);
}

aoclsparse_status aoclsparse_create_ccsr(aoclsparse_matrix *mat, aoclsparse_index_base base,
                                         aoclsparse_int M, aoclsparse_int N, aoclsparse_int nnz,
                                         aoclsparse_int *row_ptr, aoclsparse_int *col_idx,
                                         aoclsparse_float_complex *val)
{
    return create_csr(mat, base, M, N, nnz, row_ptr, col_idx, val, aoclsparse_cmat);
}

aoclsparse_status aoclsparse_create_zcsr(aoclsparse_matrix *mat, aoclsparse_index_base base,
                                         aoclsparse_int M, aoclsparse_int N, aoclsparse_int nnz,
                                         aoclsparse_int *row_ptr, aoclsparse_int *col_idx,
                                         aoclsparse_double_complex *val)
{
    return create_csr(mat, base, M, N, nnz, row_ptr, col_idx, val, aoclsparse_zmat);
}

aoclsparse_status aoclsparse_destroy(aoclsparse_matrix *mat)
{
    if(!mat)
        return aoclsparse_status_success; // :657-671 accepts NULL
    if(*mat)
    {
        if((*mat)->owns_user_arrays)
            (*mat)->user.owned = true; // sp2m results: the handle owns its CSR
        if((*mat)->ilu_factor)
            aoclsparse_destroy(&(*mat)->ilu_factor); // aliases ptr/ind/ilu_val: frees only its own plans
        for(auto &t : (*mat)->tcsr_tri) // TCSR triangles alias the caller's arrays: only what the library built on them goes
            if(t)
                aoclsparse_destroy(&t);
        for(auto &r : (*mat)->replicas) // multi-device replicas alias the same host arrays: only their device side goes
            if(r)
                aoclsparse_destroy(&r);
        std::free((*mat)->ilu_val);
        if((*mat)->trsv_timeout_host)
            (void)hipHostFree(const_cast<unsigned int *>((*mat)->trsv_timeout_host));
        delete *mat;
        *mat = nullptr;
    }
    return aoclsparse_status_success;
}

} // extern "C"

template <typename T>
static aoclsparse_status export_csr(const aoclsparse_matrix mat, aoclsparse_index_base *base,
                                    aoclsparse_int *m, aoclsparse_int *n, aoclsparse_int *nnz,
                                    aoclsparse_int **row_ptr, aoclsparse_int **col_ind, T **val,
                                    aoclsparse_matrix_data_type vt)
{
    if(!mat || !base || !m || !n || !nnz || !row_ptr || !col_ind || !val)
        return aoclsparse_status_invalid_pointer;
    if(mat->val_type != vt)
        return aoclsparse_status_wrong_type;
    std::shared_lock<std::shared_mutex> r(mat->guard);
    const HostCsr *c = mat->opt ? mat->opt : &mat->user; // optimized CSR preferred (:1326-1347)
    if(!c->ptr || !c->ind || !c->val)
        return aoclsparse_status_invalid_value;
    *row_ptr = c->ptr;
    *col_ind = c->ind;
    *val     = static_cast<T *>(c->val);
    *nnz     = c->ptr[mat->m] - c->base;
    *base    = c->base;
    *m       = mat->m;
    *n       = mat->n;
    return aoclsparse_status_success;
}

extern "C" {

aoclsparse_status aoclsparse_export_dcsr(const aoclsparse_matrix mat, aoclsparse_index_base *base,
                                         aoclsparse_int *m, aoclsparse_int *n, aoclsparse_int *nnz,
                                         aoclsparse_int **row_ptr, aoclsparse_int **col_ind, double **val)
{
    return export_csr<double>(mat, base, m, n, nnz, row_ptr, col_ind, val, aoclsparse_dmat);
}

aoclsparse_status aoclsparse_export_scsr(const aoclsparse_matrix mat, aoclsparse_index_base *base,
                                         aoclsparse_int *m, aoclsparse_int *n, aoclsparse_int *nnz,
                                         aoclsparse_int **row_ptr, aoclsparse_int **col_ind, float **val)
{
    return export_csr<float>(mat, base, m, n, nnz, row_ptr, col_ind, val, aoclsparse_smat);
}

aoclsparse_status aoclsparse_export_ccsr(const aoclsparse_matrix mat, aoclsparse_index_base *base,
                                         aoclsparse_int *m, aoclsparse_int *n, aoclsparse_int *nnz,
                                         aoclsparse_int **row_ptr, aoclsparse_int **col_ind,
                                         aoclsparse_float_complex **val)
{
    return export_csr<aoclsparse_float_complex>(mat, base, m, n, nnz, row_ptr, col_ind, val, aoclsparse_cmat);
}

aoclsparse_status aoclsparse_export_zcsr(const aoclsparse_matrix mat, aoclsparse_index_base *base,
                                         aoclsparse_int *m, aoclsparse_int *n, aoclsparse_int *nnz,
                                         aoclsparse_int **row_ptr, aoclsparse_int **col_ind,
                                         aoclsparse_double_complex **val)
{
    return export_csr<aoclsparse_double_complex>(mat, base, m, n, nnz, row_ptr, col_ind, val, aoclsparse_zmat);
}

aoclsparse_status aoclsparse_mi355_export_diag(const aoclsparse_matrix A, aoclsparse_int **idiag,
                                               aoclsparse_int **iurow, aoclsparse_int *is_internal)
{
    if(!A || !idiag || !iurow)
        return aoclsparse_status_invalid_pointer;
    std::shared_lock<std::shared_mutex> r(A->guard);
    if(!A->opt)
        return aoclsparse_status_invalid_operation;
    *idiag = A->opt->idiag;
    *iurow = A->opt->iurow;
    if(is_internal)
        *is_internal = A->opt != &A->user;
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_mi355_invalidate(aoclsparse_matrix A)
{
    if(!A)
        return aoclsparse_status_invalid_pointer;
    std::unique_lock<std::shared_mutex> w(A->guard);
    if(A->csc_ptr) // a handle created from CSC aliases the caller's CSC arrays: its own CSR is a copy of them, refreshed first
    {
        aoclsparse_status st = csc_refresh_csr(A);
        if(st != aoclsparse_status_success)
            return st;
    }
    // every copy of the values (the one list: drop_derived_state) ...
    drop_derived_state(A);
    // ... and the structural plans of the device CSR, which a value change alone leaves valid
    A->ilu_sched.release(); // (the ILU(0) level schedule among them)
    A->sp2m_plan.release(); // (and the bins of a product's numeric phase: sp2m(stage_finalize) into this handle comes here)
    for(aoclsparse_matrix t : A->tcsr_tri)
        if(t)
            (void)aoclsparse_mi355_invalidate(t);
    for(SpmvPlan *p : {&A->plan_user, &A->plan_trans})
    {
        p->valid       = false; // row blocks
        p->merge.valid = p->merge.tried = false;
        p->mm.valid = p->mm.tried = false; // row groups
        p->mm.pairs = p->mm.pairs_tried = false;
        p->mm.win = p->mm.win_tried = false;
        p->mm.row_runs = p->mm.runs_tried = false;
    }
    return aoclsparse_status_success;
}

} // extern "C"

// ---- value mutation + copy: extra/aoclsparse_auxiliary.hpp:216-270, 388-470; auxiliary.cpp:775-835 -------
// The reference writes into the FIRST representation (the caller's arrays, which the handle aliases) and
// deletes every derived copy.  Same here, device mirrors included: they are rebuilt lazily.
namespace mi355
{
aoclsparse_status alias_csr(aoclsparse_matrix *mat, aoclsparse_index_base base, aoclsparse_int M, aoclsparse_int N, aoclsparse_int nnz,
                            aoclsparse_int *row_ptr, aoclsparse_int *col_idx, void *val, aoclsparse_matrix_data_type vt, int sort,
                            bool fulldiag)
{
    _aoclsparse_matrix *A = new(std::nothrow) _aoclsparse_matrix;
    if(!A)
        return aoclsparse_status_memory_error;
    A->m = M, A->n = N, A->nnz = nnz, A->base = base, A->val_type = vt;
    A->sort = sort, A->fulldiag = fulldiag;
    A->user.m = M, A->user.n = N, A->user.nnz = nnz, A->user.base = base;
    A->user.ptr = row_ptr, A->user.ind = col_idx, A->user.val = val;
    A->user.owned = false;
    *mat          = A;
    return aoclsparse_status_success;
}

// THE list of what holds A's values besides the caller's arrays (?set_value, ?update_values, commit_values_device, aoclsparse_order_mat,
// the CSC refresh and aoclsparse_mi355_invalidate all come here).  The rule: a copy added to the handle that holds values is dropped
// here and nowhere else, and a copy that can follow a value change says so through a `follows` of its own, which values_kept
// (device_handle_api.cpp) turns into `kept`.  A value map indexes a layout and goes with its holder.
size_t drop_derived_state(aoclsparse_matrix A, const ValuesKept &kept)
{
    for(aoclsparse_matrix t : A->tcsr_tri) // TCSR: everything that holds values hangs on the two triangle handles
        if(t)
        {
            std::unique_lock<std::shared_mutex> w(t->guard);
            drop_derived_state(t);
        }
    if(A->opt != &A->user && !kept.clean) // the clean copy of unsorted arrays / arrays that miss a diagonal entry
    {
        A->opt_copy.reset(), A->clean_src.release();
        A->opt = nullptr, A->optimized = false;
    }
    A->trans.reset(); // host transpose
    // symmetric / triangular expansions (host + device + their plans); one that follows has been given the new values and stays:
    // its SELL-64 copy keeps its structure as the handle's own does, its blocked-ELL copy is rebuilt lazily
    auto        &v   = A->derived;
    const size_t had = v.size(), vsz = val_size(A->val_type);
    v.erase(std::remove_if(v.begin(), v.end(), [&](const std::unique_ptr<Derived> &d) { return !kept.operators || !d->follows(vsz); }), v.end());
    for(auto &d : v)
    {
        d->plan.sell.values_changed(true, d->host.m, d->host.nnz);
        d->plan.bell.valid = d->plan.bell.tried = false;
    }
    for(auto &r : A->replicas) // multi-device replicas hold device copies of the old values
        if(r)
            aoclsparse_destroy(&r);
    A->replicas_cloned = 0;
    A->dev_user.valid  = kept.mirror; // device CSRs; row-block plans stay valid: structure is unchanged
    A->dev_trans.valid = A->dev_bsr.valid = false; // (dev_bsr: the mirror of a BSR handle's arrays)
    // the SELL copies hold values: rebuilt on optimize (the structure of the handle's own copy outlives a ?revalue_device: stale
    // until build_sell has refilled the cells)
    A->plan_user.sell.values_changed(kept.sell, A->m, A->nnz);
    A->plan_trans.sell.values_changed(false, A->n, A->nnz);
    // ... and so does the blocked-ELL copy of csrmm (round 6: it was left standing, and a product after aoclsparse_?set_value /
    // ?update_values on a block-dense handle used the OLD values -- found by tests/test_gpu_r6.py)
    A->plan_user.bell.valid = A->plan_user.bell.tried = false;
    A->plan_trans.bell.valid = A->plan_trans.bell.tried = false;
    if(!kept.diag) // diagonal of the clean CSR (non-unit solves, SymGS scaling), and its map: ensure_trsv gathers it again
        A->dev_diag.release(), A->diag_src.release();
    for(int i = 0; i < 6; i++) // level-ordered triangles: row, block and chunk plans
    {
        TrsvPlan &p = A->trsv_plan[i];
        if(kept.plans >> i & 1u)
            continue;
        p.valid = p.rows_valid = false, p.nlevels = -1, p.blk.valid = p.blk.tried = false, p.blk.chunk.valid = p.blk.chunk.tried = false;
        p.drop_value_maps();
    }
    return had - v.size();
}

// THE list of what hangs on the ORDER of the entries within A's rows (aoclsparse_order_mat and aoclsparse_mi355_order_mat_device
// come here once the rows are sorted): every copy of the values, and the maps and schedules that index the arrays as they were
void drop_order_dependent_state(aoclsparse_matrix A, const ValuesKept &kept)
{
    A->drop_coo_map(); // a kept triplet map points into the arrays as they were ordered at creation
    A->ilu_sched.release(); // ... and so does the ILU(0) schedule: the next factorisation analyses the new order
    A->sp2m_plan.release(); // ... and the plan of aoclsparse_mi355_sp2m_numeric_device goes with it, as documented
    drop_derived_state(A, kept); // every copy made of the unsorted arrays (clean CSR, device mirrors, SELL-64 / blocked-ELL, plans, replicas)
}
} // namespace mi355

template <typename T>
static aoclsparse_status set_value(aoclsparse_matrix A, aoclsparse_int row_idx, aoclsparse_int col_idx, T val,
                                   aoclsparse_matrix_data_type vt)
{
    const bool coo = A && A->input_format == aoclsparse_coo_mat, tcsr = A && holds_no_csr(A); // (or BSR: the same answers)
    if(!A || (coo ? (!A->coo_row || !A->coo_col || !A->coo_val) : (!tcsr && (!A->user.ptr || !A->user.ind || !A->user.val))))
        return aoclsparse_status_invalid_pointer;
    const aoclsparse_int b = A->base;
    if(A->m + b <= row_idx || row_idx < b || A->n + b <= col_idx || col_idx < b)
        return aoclsparse_status_invalid_value;
    if(A->val_type != vt)
        return aoclsparse_status_wrong_type;
    if(tcsr) // auxiliary.hpp:457-458: only CSR / CSC and COO have a setter (TCSR and BSR handles)
        return aoclsparse_status_not_implemented;
    std::unique_lock<std::shared_mutex> w(A->guard);
    if(coo)
        return coo_set_value(A, row_idx, col_idx, &val);
    const aoclsparse_int r = row_idx - b;
    for(aoclsparse_int p = A->user.ptr[r] - b; p < A->user.ptr[r + 1] - b; p++)
        if(A->user.ind[p] == col_idx)
        {
            static_cast<T *>(A->user.val)[p] = val;
            if(A->csc_ptr)
                csc_set_value(A, row_idx, col_idx, &val);
            A->op_dropped_by_value_change += (long long)drop_derived_state(A);
            return aoclsparse_status_success;
        }
    return aoclsparse_status_invalid_index_value;
}

namespace mi355
{
aoclsparse_status update_values_status(const _aoclsparse_matrix *A, aoclsparse_int len, const void *val, aoclsparse_matrix_data_type vt)
{
    const bool coo = A && A->input_format == aoclsparse_coo_mat, tcsr = A && holds_no_csr(A); // (or BSR: the same answers)
    if(!A || !val || (coo ? !A->coo_val : (!tcsr && !A->user.ptr)))
        return aoclsparse_status_invalid_pointer;
    if(len != A->nnz)
        return aoclsparse_status_invalid_size;
    if(A->val_type != vt)
        return aoclsparse_status_wrong_type;
    if(tcsr) // auxiliary.hpp:255-256
        return aoclsparse_status_not_implemented;
    if(!coo && !A->user.val)
        return aoclsparse_status_invalid_pointer;
    return aoclsparse_status_success;
}
} // namespace mi355

template <typename T>
static aoclsparse_status update_values(aoclsparse_matrix A, aoclsparse_int len, T *val, aoclsparse_matrix_data_type vt)
{
    const aoclsparse_status st = update_values_status(A, len, val, vt);
    if(st != aoclsparse_status_success)
        return st;
    const bool                          coo = A->input_format == aoclsparse_coo_mat;
    std::unique_lock<std::shared_mutex> w(A->guard);
    if(coo) // the values follow the order of the caller's arrays (the first representation)
    {
        std::memcpy(A->coo_val, val, sizeof(T) * (size_t)len);
        return aoclsparse_status_success;
    }
    if(A->csc_ptr)
    {
        std::memcpy(A->csc_val, val, sizeof(T) * (size_t)len);
        aoclsparse_status st = csc_refresh_csr(A);
        if(st != aoclsparse_status_success)
            return st;
    }
    else
        std::memcpy(A->user.val, val, sizeof(T) * (size_t)len);
    A->op_dropped_by_value_change += (long long)drop_derived_state(A);
    return aoclsparse_status_success;
}

extern "C" {

aoclsparse_status aoclsparse_dset_value(aoclsparse_matrix A, aoclsparse_int row_idx, aoclsparse_int col_idx, double val)
{
    return set_value<double>(A, row_idx, col_idx, val, aoclsparse_dmat);
}
aoclsparse_status aoclsparse_sset_value(aoclsparse_matrix A, aoclsparse_int row_idx, aoclsparse_int col_idx, float val)
{
    return set_value<float>(A, row_idx, col_idx, val, aoclsparse_smat);
}
aoclsparse_status aoclsparse_cset_value(aoclsparse_matrix A, aoclsparse_int row_idx, aoclsparse_int col_idx,
                                        aoclsparse_float_complex val)
{
    return set_value<aoclsparse_float_complex>(A, row_idx, col_idx, val, aoclsparse_cmat);
}
aoclsparse_status aoclsparse_zset_value(aoclsparse_matrix A, aoclsparse_int row_idx, aoclsparse_int col_idx,
                                        aoclsparse_double_complex val)
{
    return set_value<aoclsparse_double_complex>(A, row_idx, col_idx, val, aoclsparse_zmat);
}
aoclsparse_status aoclsparse_cupdate_values(aoclsparse_matrix A, aoclsparse_int len, aoclsparse_float_complex *val)
{
    return update_values<aoclsparse_float_complex>(A, len, val, aoclsparse_cmat);
}
aoclsparse_status aoclsparse_zupdate_values(aoclsparse_matrix A, aoclsparse_int len, aoclsparse_double_complex *val)
{
    return update_values<aoclsparse_double_complex>(A, len, val, aoclsparse_zmat);
}
aoclsparse_status aoclsparse_dupdate_values(aoclsparse_matrix A, aoclsparse_int len, double *val)
{
    return update_values<double>(A, len, val, aoclsparse_dmat);
}
aoclsparse_status aoclsparse_supdate_values(aoclsparse_matrix A, aoclsparse_int len, float *val)
{
    return update_values<float>(A, len, val, aoclsparse_smat);
}

aoclsparse_status aoclsparse_copy(const aoclsparse_matrix src, const aoclsparse_mat_descr /*descr*/,
                                  aoclsparse_matrix *dest)
{
    if(!src || !dest)
        return aoclsparse_status_invalid_pointer;
    if(src->m < 0 || src->n < 0 || src->nnz < 0)
        return aoclsparse_status_invalid_size;
    if(src == *dest)
        return aoclsparse_status_invalid_pointer;
    if(src->val_type < aoclsparse_dmat || src->val_type > aoclsparse_zmat)
        return aoclsparse_status_wrong_type;
    if(holds_no_csr(src)) // auxiliary.cpp:1234-1235: only CSR / CSC and COO are copied
        return aoclsparse_status_invalid_value;
    if(!src->user.ptr || !src->user.ind || !src->user.val)
        return aoclsparse_status_invalid_pointer;
    _aoclsparse_matrix *c = new(std::nothrow) _aoclsparse_matrix;
    if(!c)
        return aoclsparse_status_memory_error;
    const size_t         vs  = val_size(src->val_type);
    const aoclsparse_int nnz = src->nnz;
    c->m = src->m, c->n = src->n, c->nnz = nnz, c->base = src->base, c->val_type = src->val_type;
    c->sort = src->sort, c->fulldiag = src->fulldiag;
    c->user.m = src->m, c->user.n = src->n, c->user.nnz = nnz, c->user.base = src->base;
    c->user.ptr = new(std::nothrow) aoclsparse_int[(size_t)src->m + 1];
    c->user.ind = new(std::nothrow) aoclsparse_int[(size_t)std::max(nnz, 1)];
    c->user.val = ::operator new(vs * (size_t)std::max(nnz, 1), std::nothrow);
    c->user.owned = true, c->owns_user_arrays = true; // deep copy: the new handle owns its arrays
    if(!c->user.ptr || !c->user.ind || !c->user.val)
    {
        delete c;
        return aoclsparse_status_memory_error;
    }
    std::memcpy(c->user.ptr, src->user.ptr, sizeof(aoclsparse_int) * ((size_t)src->m + 1));
    std::memcpy(c->user.ind, src->user.ind, sizeof(aoclsparse_int) * (size_t)nnz);
    std::memcpy(c->user.val, src->user.val, vs * (size_t)nnz);
    *dest = c;
    return aoclsparse_status_success;
}

} // extern "C"

extern "C" {

// ---- hints: analysis/aoclsparse_analysis.cpp:568-747 -----------------------------------------------------
static aoclsparse_status set_hint(aoclsparse_matrix mat, hinted_action act, aoclsparse_operation trans,
                                  const aoclsparse_mat_descr descr, aoclsparse_int ncalls,
                                  aoclsparse_int kid = -1)
{
    if(!mat || (!mat->user.ptr && !holds_no_csr(mat)) || !descr)
        return aoclsparse_status_invalid_pointer;
    if(descr->base != aoclsparse_index_base_zero && descr->base != aoclsparse_index_base_one)
        return aoclsparse_status_invalid_value;
    if(descr->base != mat->base) // is_descr_matching, mat_structures.hpp:808-814
        return aoclsparse_status_invalid_value;
    if(trans != aoclsparse_operation_none && trans != aoclsparse_operation_transpose
       && trans != aoclsparse_operation_conjugate_transpose)
        return aoclsparse_status_invalid_value;
    if(descr->fill_mode != aoclsparse_fill_mode_lower && descr->fill_mode != aoclsparse_fill_mode_upper)
        return aoclsparse_status_invalid_value;
    if(descr->diag_type != aoclsparse_diag_type_non_unit && descr->diag_type != aoclsparse_diag_type_unit
       && descr->diag_type != aoclsparse_diag_type_zero)
        return aoclsparse_status_invalid_value;
    if(descr->type != aoclsparse_matrix_type_general && descr->type != aoclsparse_matrix_type_symmetric
       && descr->type != aoclsparse_matrix_type_triangular && descr->type != aoclsparse_matrix_type_hermitian)
        return aoclsparse_status_invalid_value;
    if(ncalls < 0 || (ncalls == 0 && kid == -1))
        return aoclsparse_status_invalid_value;
    if(act <= action_none || act >= action_max)
        return aoclsparse_status_invalid_operation;
    try
    {
        Hint h{act, get_doid(descr, trans), trans, descr->type, descr->fill_mode, ncalls, kid, false};
        mat->hints.insert(mat->hints.begin(), h); // newest first
        // TCSR: the one-triangle products and the solves run on the triangle the fill mode names and read ITS list (a pinned kid)
        if(mat->input_format == aoclsparse_tcsr_mat && descr->type != aoclsparse_matrix_type_general)
        {
            aoclsparse_matrix t = tcsr_triangle(mat, descr->fill_mode);
            t->hints.insert(t->hints.begin(), h);
        }
    }
    catch(const std::bad_alloc &)
    {
        return aoclsparse_status_memory_error;
    }
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_set_mv_hint(aoclsparse_matrix mat, aoclsparse_operation trans,
                                         const aoclsparse_mat_descr descr, aoclsparse_int n)
{
    return set_hint(mat, action_mv, trans, descr, n);
}

aoclsparse_status aoclsparse_set_mv_hint_kid(aoclsparse_matrix mat, aoclsparse_operation trans,
                                             const aoclsparse_mat_descr descr, aoclsparse_int n,
                                             aoclsparse_int kid)
{
    return set_hint(mat, action_mv, trans, descr, n, kid);
}

aoclsparse_status aoclsparse_set_sv_hint(aoclsparse_matrix mat, aoclsparse_operation trans,
                                         const aoclsparse_mat_descr descr, aoclsparse_int n)
{
    return set_hint(mat, action_sv, trans, descr, n);
}

aoclsparse_status aoclsparse_set_mm_hint(aoclsparse_matrix mat, aoclsparse_operation trans,
                                         const aoclsparse_mat_descr descr, aoclsparse_int n)
{
    return set_hint(mat, action_mm, trans, descr, n);
}

aoclsparse_status aoclsparse_set_2m_hint(aoclsparse_matrix mat, aoclsparse_operation trans,
                                         const aoclsparse_mat_descr descr, aoclsparse_int n)
{
    return set_hint(mat, action_2m, trans, descr, n);
}

aoclsparse_status aoclsparse_set_dotmv_hint(aoclsparse_matrix mat, aoclsparse_operation trans,
                                            const aoclsparse_mat_descr descr, aoclsparse_int n)
{
    return set_hint(mat, action_dotmv, trans, descr, n);
}

aoclsparse_status aoclsparse_set_lu_smoother_hint(aoclsparse_matrix mat, aoclsparse_operation trans,
                                                  const aoclsparse_mat_descr descr, aoclsparse_int n)
{
    return set_hint(mat, action_ilu0, trans, descr, n);
}

aoclsparse_status aoclsparse_set_sm_hint(aoclsparse_matrix mat, aoclsparse_operation trans,
                                         const aoclsparse_mat_descr descr, const aoclsparse_order order,
                                         aoclsparse_int n)
{
    if(order != aoclsparse_order_row && order != aoclsparse_order_column) // analysis.cpp:686-689
        return aoclsparse_status_invalid_value;
    return set_hint(mat, order == aoclsparse_order_row ? action_sm_row : action_sm_col, trans, descr, n);
}

aoclsparse_status aoclsparse_set_symgs_hint(aoclsparse_matrix mat, aoclsparse_operation trans,
                                            const aoclsparse_mat_descr descr, aoclsparse_int n)
{
    return set_hint(mat, action_symgs, trans, descr, n);
}

aoclsparse_status aoclsparse_set_sorv_hint(aoclsparse_matrix mat, const aoclsparse_mat_descr descr,
                                           const aoclsparse_sor_type type, const aoclsparse_int n)
{
    if(type != aoclsparse_sor_forward && type != aoclsparse_sor_backward && type != aoclsparse_sor_symmetric)
        return aoclsparse_status_invalid_value; // analysis.cpp:713-717
    const hinted_action act = type == aoclsparse_sor_forward    ? action_sorv_forward
                              : type == aoclsparse_sor_backward ? action_sorv_backward
                                                                : action_sorv_symm;
    return set_hint(mat, act, aoclsparse_operation_none, descr, n);
}

aoclsparse_status aoclsparse_set_memory_hint(aoclsparse_matrix mat, const aoclsparse_memory_usage policy)
{
    // analysis.cpp:725-747
    if(!mat)
        return aoclsparse_status_invalid_pointer;
    if(policy != aoclsparse_memory_usage_minimal && policy != aoclsparse_memory_usage_unrestricted)
        return aoclsparse_status_invalid_value;
    mat->mem_policy = policy;
    for(aoclsparse_matrix t : mat->tcsr_tri) // the triangles of a TCSR handle build the plans: the policy is theirs too
        if(t)
            t->mem_policy = policy;
    return aoclsparse_status_success;
}

} // extern "C"
