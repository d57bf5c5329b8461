// sp2m_api.cpp -- aoclsparse_sp2m / aoclsparse_spmm / aoclsparse_?csr2m: C = op(A) * op(B), sparse result.
//
// Driver logic follows level3/aoclsparse_csr2m.cpp:592-861 of the reference: argument checks in the
// same order, empty-product quick return that still allocates an empty C, op handling (A^T / B^T by an
// explicit counting-sort transpose, A^T B^T as (B A)^T with the product transposed back at finalize),
// the two-stage request protocol (stage_nnz_count allocates C and fills row_ptr; stage_finalize fills
// col_ind / val of that same C; full_computation does both), C always 0-based.  The product itself runs
// on the GPU (spgemm_kernels.hip); C's arrays are host arrays owned by the new handle, like any handle
// created by aoclsparse_create_?csr, so export / destroy work unchanged.
#include "spg_host.hpp"
#include "device_handle.hpp"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <type_traits>

using namespace mi355;

namespace
{

// ---- the checks of csr2m.cpp:592-735, in that order; `done`: the call ends here with the status returned ----
aoclsparse_status sp2m_checks(aoclsparse_operation opA, const aoclsparse_mat_descr descrA, const aoclsparse_matrix A,
                              aoclsparse_operation opB, const aoclsparse_mat_descr descrB, const aoclsparse_matrix B,
                              aoclsparse_request request, aoclsparse_matrix *C, aoclsparse_matrix_data_type vt, bool &trA, bool &trB,
                              bool &done)
{
    done = true;
    if(!descrA || !descrB)
        return aoclsparse_status_invalid_pointer;
    if(!A || !B || !C)
        return aoclsparse_status_invalid_pointer;
    if(request != aoclsparse_stage_finalize)
        *C = nullptr;
    if(A->input_format != aoclsparse_csr_mat || B->input_format != aoclsparse_csr_mat)
        return aoclsparse_status_not_implemented;
    if(A->val_type != vt || B->val_type != vt)
        return aoclsparse_status_wrong_type;
    if(!A->user.ptr || !B->user.ptr)
        return aoclsparse_status_invalid_pointer;
    auto valid_base = [](int b) { return b == 0 || b == 1; };
    if(!valid_base(descrA->base) || !valid_base(descrB->base))
        return aoclsparse_status_invalid_value;
    if(A->base != descrA->base || B->base != descrB->base)
        return aoclsparse_status_invalid_value;
    if(descrA->type != aoclsparse_matrix_type_general || descrB->type != aoclsparse_matrix_type_general)
        return aoclsparse_status_not_implemented;
    auto is_tr = [](aoclsparse_operation o, bool &ok) {
        ok = o == aoclsparse_operation_none || o == aoclsparse_operation_transpose
             || o == aoclsparse_operation_conjugate_transpose;
        return o != aoclsparse_operation_none;
    };
    bool okA, okB;
    trA = is_tr(opA, okA), trB = is_tr(opB, okB);
    if(!okA || !okB)
        return aoclsparse_status_invalid_value;
    const aoclsparse_int m_a = trA ? A->n : A->m, n_a = trA ? A->m : A->n;
    const aoclsparse_int m_b = trB ? B->n : B->m, n_b = trB ? B->m : B->n;
    if(n_a != m_b)
        return aoclsparse_status_invalid_size;
    if(request != aoclsparse_stage_nnz_count && request != aoclsparse_stage_finalize
       && request != aoclsparse_stage_full_computation)
        return aoclsparse_status_invalid_value;
    if(m_a == 0 || n_a == 0 || n_b == 0 || A->nnz == 0 || B->nnz == 0)
    {
        if(*C == nullptr) // csr2m.cpp:705-735: valid empty result
            return new_csr_result(C, m_a, n_b, 0, vt, nullptr);
        return aoclsparse_status_success;
    }
    done = false;
    return aoclsparse_status_success;
}

// ---- operands in computation orientation (csr2m.cpp:743-830): the product computed is D = X * Y ----
template <typename T>
struct Sp2mOperands
{
    HostCsrOp<T>        va, vb, ta, tb;
    const HostCsrOp<T> *X = nullptr, *Y = nullptr;
    aoclsparse_matrix   HX = nullptr, HY = nullptr; // the handles X and Y come from
    bool                conj_x = false, conj_y = false;
    bool                back = false; // op(A) op(B) = A^T B^T is computed as D = B A: C = D^T at finalize
};

// op = T / H: the explicit transpose of csr2m.cpp:771-781.  A handle keeps its transpose (build_transpose: the same sort, 0-based)
// and its device copy, so that a chain of products with P^T pays for it once; handles whose `trans` slot holds something else
// (results of a (B A)^T product) transpose here.  (Known: t points into H->trans after the shared lock is released.)
template <typename T>
aoclsparse_status transposed(const aoclsparse_matrix H, const HostCsrOp<T> &v, HostCsrOp<T> &t)
{
    if(H->owns_user_arrays)
    {
        transpose_of(v, t);
        return aoclsparse_status_success;
    }
    const aoclsparse_status rc = build_transpose(H);
    if(rc != aoclsparse_status_success)
        return rc;
    std::shared_lock<std::shared_mutex> r(H->guard);
    view_of(*H->trans, t);
    return aoclsparse_status_success;
}

template <typename T>
aoclsparse_status sp2m_operands(aoclsparse_operation opA, const aoclsparse_matrix A, aoclsparse_operation opB, const aoclsparse_matrix B,
                                bool trA, bool trB, Sp2mOperands<T> &o)
{
    view_of(A->user, o.va);
    view_of(B->user, o.vb);
    // op = H on a complex operand: the values are conjugated as the kernel loads them (csr2m.cpp:748-835)
    constexpr bool is_cplx = !std::is_floating_point<T>::value;
    o.conj_x = is_cplx && opA == aoclsparse_operation_conjugate_transpose;
    o.conj_y = is_cplx && opB == aoclsparse_operation_conjugate_transpose;
    o.X = &o.va, o.Y = &o.vb, o.HX = A, o.HY = B;
    if(trA && trB)
    {
        o.back = true; // (B A)^T
        std::swap(o.X, o.Y), std::swap(o.HX, o.HY), std::swap(o.conj_x, o.conj_y);
        return aoclsparse_status_success;
    }
    aoclsparse_status st = aoclsparse_status_success;
    if(trA)
    {
        st  = transposed(A, o.va, o.ta);
        o.X = &o.ta;
    }
    if(trB && st == aoclsparse_status_success)
    {
        st  = transposed(B, o.vb, o.tb);
        o.Y = &o.tb;
    }
    return st;
}

// ---- operands on the device: the handles' own device copies; transposes built above on the host go through staging slots,
// without their values when the call only counts; A * A sends A once ----
template <typename T>
aoclsparse_status sp2m_to_device(Runtime &rt, const Sp2mOperands<T> &o, bool with_values, SpgDevOp &dx, SpgDevOp &dy)
{
    const bool              once = o.Y->ptr == o.X->ptr && o.Y->ind == o.X->ind && o.Y->val == o.X->val;
    const aoclsparse_status st   = spg_to_device(rt, o.HX, *o.X, SPG_SLOT_XP, with_values, dx);
    if(st == aoclsparse_status_success && !once)
        return spg_to_device(rt, o.HY, *o.Y, SPG_SLOT_YP, with_values, dy);
    dy = dx;
    return st;
}

// ---- the count stage: D's row pointer in d_cptr (it stays there for the fill pass of a full computation) and in a new *C ----
template <typename T, typename Phase>
aoclsparse_status sp2m_count(SpgProduct<T> &prod, bool back, DeviceBuffer &d_cptr, aoclsparse_matrix *C,
                             aoclsparse_matrix_data_type vt, const Phase &phase)
{
    const aoclsparse_int        m = prod.m, n = prod.n;
    long long                  *d_total = nullptr;
    aoclsparse_int              nnz_c   = 0;
    std::vector<aoclsparse_int> cptr; // the host needs the total now (to allocate) and the array itself for the handle
    aoclsparse_status           st = d_cptr.alloc(sizeof(aoclsparse_int) * ((size_t)m + 1));
    if(st == aoclsparse_status_success)
        st = prod.count(d_cptr.as<aoclsparse_int>(), &d_total);
    if(st == aoclsparse_status_success)
        st = spg_count_to_host(prod.rt, d_total, d_cptr.as<aoclsparse_int>(), m, aoclsparse_index_base_zero, &cptr, nnz_c);
    if(st != aoclsparse_status_success)
        return st;
    phase("count: scan, row_ptr to host");
    if(!back)
        return new_csr_result(C, m, n, nnz_c, vt, cptr.data());
    // C is n x m; keep D's row_ptr in the handle's transposed-product scratch until finalize
    st = new_csr_result(C, n, m, nnz_c, vt, nullptr);
    if(st != aoclsparse_status_success)
        return st;
    (*C)->trans.reset(new HostCsr);
    HostCsr &d = *(*C)->trans;
    d.m = m, d.n = n, d.nnz = nnz_c, d.base = aoclsparse_index_base_zero, d.owned = true;
    d.ptr = new aoclsparse_int[(size_t)m + 1];
    d.ind = new aoclsparse_int[(size_t)std::max(nnz_c, 1)];
    d.val = ::operator new(sizeof(T) * (size_t)std::max(nnz_c, 1));
    std::memcpy(d.ptr, cptr.data(), sizeof(aoclsparse_int) * ((size_t)m + 1));
    return st;
}

// ---- the fill stage: col_ind / val of the *C of a count stage (`counted`: of this call, its row pointer is still in d_cptr) ----
template <typename T>
aoclsparse_status sp2m_fill(SpgProduct<T> &prod, bool back, bool counted, DeviceBuffer &d_cptr, aoclsparse_matrix *C,
                            aoclsparse_matrix_data_type vt)
{
    const aoclsparse_int m = prod.m, n = prod.n;
    if(*C == nullptr)
        return aoclsparse_status_invalid_pointer;
    _aoclsparse_matrix *c = *C;
    if(c->val_type != vt || !c->owns_user_arrays)
        return aoclsparse_status_invalid_pointer;
    HostCsr *d = back ? c->trans.get() : &c->user; // where the product D lands
    if(!d || !d->ptr || !d->ind || !d->val)
        return aoclsparse_status_invalid_pointer;
    if(d->m != m || d->n != n)
        return aoclsparse_status_invalid_size; // csr2m.cpp:397-399
    const aoclsparse_int nnz_c = d->ptr[m] - d->base;
    DeviceBuffer         d_ci, d_cv; // with d_cptr: the result's own arrays
    aoclsparse_status    st = counted ? aoclsparse_status_success : d_cptr.alloc(sizeof(aoclsparse_int) * ((size_t)m + 1));
    if(st == aoclsparse_status_success)
        st = d_ci.alloc(sizeof(aoclsparse_int) * (size_t)std::max(nnz_c, 1));
    if(st == aoclsparse_status_success)
        st = d_cv.alloc(sizeof(T) * (size_t)std::max(nnz_c, 1));
    if(st == aoclsparse_status_success)
        st = spg_fill_to_host<T>(prod, !counted, d_cptr.as<aoclsparse_int>(), d_ci.as<aoclsparse_int>(), d_cv.as<T>(), *d, [c] {
            // whatever the handle derived from an earlier fill (device copies, plans, SELL twin, replicas) mirrors the old values
            // (the (B A)^T scratch of the count stage lives in c->trans, which invalidate would drop: carried across)
            auto keep = std::move(c->trans);
            (void)aoclsparse_mi355_invalidate(c);
            c->trans = std::move(keep);
        });
    if(st != aoclsparse_status_success)
        return st;
    if(!back)
    {
        // the result stays resident: a product, solve or another sp2m with this handle starts from HBM
        std::unique_lock<std::shared_mutex> w(c->guard);
        DeviceCsr                          &dc = c->dev_user;
        dc.ptr.adopt(d_cptr), dc.ind.adopt(d_ci), dc.val.adopt(d_cv);
        dc.m = m, dc.n = n, dc.nnz = nnz_c, dc.base = aoclsparse_index_base_zero;
        dc.valid = true;
    }
    else // C = D^T by the reference's counting-sort transpose (csr2m.cpp:520-538)
        host_transpose<T>(m, n, nnz_c, 0, 0, d->ptr, d->ind, static_cast<const T *>(d->val), c->user.ptr, c->user.ind,
                          static_cast<T *>(c->user.val));
    return st;
}

template <typename T>
aoclsparse_status sp2m_t(aoclsparse_operation opA, const aoclsparse_mat_descr descrA, const aoclsparse_matrix A,
                         aoclsparse_operation opB, const aoclsparse_mat_descr descrB, const aoclsparse_matrix B,
                         aoclsparse_request request, aoclsparse_matrix *C, aoclsparse_matrix_data_type vt)
{
    bool              trA = false, trB = false, done = true;
    aoclsparse_status st  = sp2m_checks(opA, descrA, A, opB, descrB, B, request, C, vt, trA, trB, done);
    if(done)
        return st;
    CallScope cs(CallScope::Always); // the SPG_SLOT_* slots are shared
    if(!cs.ok())
        return cs.st;
    Runtime &rt = cs.rt;
    // diagnostic: AOCLSPARSE_MI355_SP2M_TRACE=1 prints the wall time of every phase of the call (synchronising after each)
    static const bool trace  = getenv("AOCLSPARSE_MI355_SP2M_TRACE") != nullptr;
    auto              t_last = std::chrono::steady_clock::now();
    auto              phase  = [&](const char *what) {
        if(!trace)
            return;
        (void)hipStreamSynchronize(rt.stream());
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "sp2m %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    try
    {
        Sp2mOperands<T> o;
        st = sp2m_operands<T>(opA, A, opB, B, trA, trB, o);
        if(st != aoclsparse_status_success)
            return st;
        phase("operands (transposes)");
        const bool count = request != aoclsparse_stage_finalize, fill = request != aoclsparse_stage_nnz_count;
        // the product itself: upper bounds, bins, count pass, prefix sum, fill pass (SpgProduct)
        SpgProduct<T> prod(rt);
        prod.m = o.X->m, prod.n = o.Y->n;
        prod.conj_x = o.conj_x, prod.conj_y = o.conj_y;
        if(trace)
            prod.phase = phase;
        st = sp2m_to_device(rt, o, fill, prod.x, prod.y);
        if(st != aoclsparse_status_success)
            return st;
        phase("operands to the device");
        st = prod.analyse();
        if(st != aoclsparse_status_success)
            return st;
        phase("upper bounds (device)");
        DeviceBuffer d_cptr; // D's row pointer: a full computation goes from the count pass to the fill pass in HBM
        if(count)
            st = sp2m_count(prod, o.back, d_cptr, C, vt, phase);
        phase("result handle");
        if(fill && st == aoclsparse_status_success)
            st = sp2m_fill(prod, o.back, count, d_cptr, C, vt);
        return st;
    }
    catch(const std::bad_alloc &)
    {
        return aoclsparse_status_memory_error;
    }
}

aoclsparse_status sp2m_any(aoclsparse_operation opA, const aoclsparse_mat_descr descrA, const aoclsparse_matrix A,
                           aoclsparse_operation opB, const aoclsparse_mat_descr descrB, const aoclsparse_matrix B,
                           aoclsparse_request request, aoclsparse_matrix *C)
{
    // level3/aoclsparse_sp2m.cpp:27-50 dispatches on A's value type
    if(!A || !B || !C || !descrA || !descrB)
        return aoclsparse_status_invalid_pointer;
    if(A->val_type == aoclsparse_dmat)
        return sp2m_t<double>(opA, descrA, A, opB, descrB, B, request, C, aoclsparse_dmat);
    if(A->val_type == aoclsparse_smat)
        return sp2m_t<float>(opA, descrA, A, opB, descrB, B, request, C, aoclsparse_smat);
    if(A->val_type == aoclsparse_zmat)
        return sp2m_t<cdouble>(opA, descrA, A, opB, descrB, B, request, C, aoclsparse_zmat);
    if(A->val_type == aoclsparse_cmat)
        return sp2m_t<cfloat>(opA, descrA, A, opB, descrB, B, request, C, aoclsparse_cmat);
    return aoclsparse_status_not_implemented;
}

// ---- aoclsparse_mi355_sp2m_numeric_device: C's values again, on the structure C has ----
template <typename T>
aoclsparse_status sp2m_numeric_t(aoclsparse_operation opA, const aoclsparse_mat_descr descrA, const aoclsparse_matrix A,
                                 aoclsparse_operation opB, const aoclsparse_mat_descr descrB, const aoclsparse_matrix B,
                                 aoclsparse_matrix C, aoclsparse_matrix_data_type vt)
{
    // -- decided before the device is touched, in this order: the checks of a finalize call ...
    bool              trA = false, trB = false, done = true;
    aoclsparse_matrix c  = C;
    aoclsparse_status st = sp2m_checks(opA, descrA, A, opB, descrB, B, aoclsparse_stage_finalize, &c, vt, trA, trB, done);
    if(done)
    {
        if(!C && c) // (the empty product of a finalize call without a C: a new empty handle, which nobody asked for here)
            aoclsparse_destroy(&c);
        return st;
    }
    // ... then what this call adds
    if(!C)
        return aoclsparse_status_invalid_pointer;
    if(trA && trB)
        return aoclsparse_status_not_implemented; // C = D^T: the values would need a map
    if(C->input_format != aoclsparse_csr_mat || C->csc_ptr || !C->user.ptr || !C->user.ind || !C->user.val)
        return aoclsparse_status_not_implemented;
    if(C->val_type != vt)
        return aoclsparse_status_wrong_type;
    if(C->m != (trA ? A->n : A->m) || C->n != (trB ? B->m : B->n))
        return aoclsparse_status_invalid_size;
    if(C == A || C == B)
        return aoclsparse_status_invalid_value;
    CallScope cs(CallScope::Always); // the SPG_SLOT_* slots are shared
    if(!cs.ok())
        return cs.st;
    Runtime   &rt = cs.rt;
    StreamLaps lt{cs.s};
    try
    {
        Sp2mOperands<T> o;
        st = sp2m_operands<T>(opA, A, opB, B, trA, trB, o);
        if(st != aoclsparse_status_success)
            return st;
        SpgDevOp dx, dy, dc;
        st = sp2m_to_device(rt, o, true, dx, dy);
        if(st != aoclsparse_status_success)
            return st;
        const aoclsparse_int m = o.X->m, nnz_c = C->nnz;
        DeviceBuffer         d_val; // the new values: nothing of C is written before the verdict is in
        void                *p_small = nullptr;
        unsigned int         bad     = 0;
        bool                 built   = false;
        _aoclsparse_matrix::Sp2mPlan fresh; // a plan built by this call goes to the handle only when the call succeeds
        struct Events // the diagnostic times the numeric kernels by device events
        {
            hipEvent_t at[2] = {nullptr, nullptr};
            ~Events()
            {
                for(hipEvent_t v : at)
                    if(v)
                        (void)hipEventDestroy(v);
            }
        } events;
        hipEvent_t(&ev)[2] = events.at;
        {
            StreamDrain drain{cs.s}; // (a way out with work in flight: the stream finishes before d_val and `fresh` go)
            std::unique_lock<std::shared_mutex> w(C->guard);
            MI355_TRY(resident_mirror(C)); // uploaded when absent, as every product does
            const DeviceCsr &d = C->dev_user;
            if(d.nnz != nnz_c || d.val.bytes < sizeof(T) * (size_t)nnz_c)
                return aoclsparse_status_internal_error;
            dc = SpgDevOp{d.ptr.as<aoclsparse_int>(), d.ind.as<aoclsparse_int>(), nullptr, (int)d.base};
            lt.lap("sp2m_numeric: operands + mirror");
            if(!C->sp2m_plan.valid)
            {
                MI355_TRY(sp2m_plan_build(rt, m, dc.ptr, fresh));
                built = true;
                lt.lap("sp2m_numeric: plan build");
            }
            const _aoclsparse_matrix::Sp2mPlan &plan = built ? fresh : C->sp2m_plan;
            MI355_TRY(d_val.alloc(sizeof(T) * (size_t)std::max<aoclsparse_int>(nnz_c, 1)));
            MI355_TRY(rt.staging(SPG_SLOT_SMALL, 256, &p_small));
            unsigned int *d_bad = static_cast<unsigned int *>(p_small);
            MI355_HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(unsigned int), cs.s));
            if(lt.on)
                for(hipEvent_t &v : ev)
                    if(hipEventCreate(&v) != hipSuccess)
                        v = nullptr; // (without both events no figure; `events` destroys the one that was made)
            if(!ev[0])
                std::swap(ev[0], ev[1]); // (ev[1] set means both are)
            if(ev[1])
                MI355_HIP_TRY(hipEventRecord(ev[0], cs.s));
            MI355_TRY(spg_numeric<T>(rt, plan, dx, dy, o.conj_x, o.conj_y, dc, d_val.as<T>(), d_bad));
            if(ev[1])
                MI355_HIP_TRY(hipEventRecord(ev[1], cs.s));
            // the first of the call's two waits: the verdict
            MI355_HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, cs.s));
            MI355_HIP_TRY(hipStreamSynchronize(cs.s));
            drain.dismiss();
            float ms = 0.0f;
            if(ev[1] && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess)
                std::fprintf(stderr, "[mi355 timing]     %-30s %8.3f ms\n", "sp2m_numeric: kernel events", ms);
            lt.lap("sp2m_numeric: kernels + verdict");
            if(bad)
            {
                C->sp2m_refused++; // C's structure is not this product's: C, what hangs on it and a kept plan stay as they were
                return aoclsparse_status_invalid_value;
            }
        }
        // the second wait is the commit's: the host view by one copy back, the mirror device to device, and what a handle with
        // keep_value_maps keeps (?revalue_device's own code, which takes C's guard itself)
        {
            DeviceScope scope; // (d_val is the library's own device buffer whatever the pointer mode says)
            st = revalue_device_any(C, nnz_c, d_val.ptr);
        }
        lt.lap("sp2m_numeric: commit");
        if(st != aoclsparse_status_success)
            return st;
        std::unique_lock<std::shared_mutex> w(C->guard);
        if(built)
        {
            C->sp2m_plan.adopt(fresh);
            C->sp2m_plan_builds++;
        }
        C->sp2m_numeric_runs++;
        return aoclsparse_status_success;
    }
    catch(const std::bad_alloc &)
    {
        return aoclsparse_status_memory_error;
    }
}

} // namespace

extern "C" {

aoclsparse_status aoclsparse_mi355_sp2m_numeric_device(aoclsparse_operation opA, const aoclsparse_mat_descr descrA,
                                                       const aoclsparse_matrix A, aoclsparse_operation opB,
                                                       const aoclsparse_mat_descr descrB, const aoclsparse_matrix B,
                                                       aoclsparse_matrix C)
{
    // dispatch on A's value type, as aoclsparse_sp2m
    if(!A || !B || !descrA || !descrB)
        return aoclsparse_status_invalid_pointer;
    if(A->val_type == aoclsparse_dmat)
        return sp2m_numeric_t<double>(opA, descrA, A, opB, descrB, B, C, aoclsparse_dmat);
    if(A->val_type == aoclsparse_smat)
        return sp2m_numeric_t<float>(opA, descrA, A, opB, descrB, B, C, aoclsparse_smat);
    if(A->val_type == aoclsparse_zmat)
        return sp2m_numeric_t<cdouble>(opA, descrA, A, opB, descrB, B, C, aoclsparse_zmat);
    if(A->val_type == aoclsparse_cmat)
        return sp2m_numeric_t<cfloat>(opA, descrA, A, opB, descrB, B, C, aoclsparse_cmat);
    return aoclsparse_status_not_implemented;
}

aoclsparse_status aoclsparse_mi355_get_sp2m_plan_info(aoclsparse_matrix C, aoclsparse_mi355_sp2m_plan_info *info)
{
    if(!C || !info)
        return aoclsparse_status_invalid_pointer;
    if(info->struct_size < sizeof(info->struct_size))
        return aoclsparse_status_invalid_size;
    aoclsparse_mi355_sp2m_plan_info r{};
    {
        // (the plan is written under the runtime's stage lock and the handle's guard)
        std::lock_guard<std::recursive_mutex> sl(Runtime::get().stage_lock);
        std::shared_lock<std::shared_mutex>   rd(C->guard);
        const auto                           &pl = C->sp2m_plan;
        r.kept = pl.valid;
        if(pl.valid)
        {
            for(int b = 0; b < SPGEMM_BINS; b++)
                r.rows_in_bin[b] = pl.bounds[b + 1] - pl.bounds[b];
            r.heavy_rows = r.rows_in_bin[SPGEMM_BINS - 1];
        }
        r.plan_builds = C->sp2m_plan_builds, r.numeric_runs = C->sp2m_numeric_runs, r.refused = C->sp2m_refused;
        r.plan_bytes = pl.bytes();
    }
    r.struct_size = info->struct_size; // (the caller's: it says how much of the struct the caller has)
    std::memcpy(info, &r, std::min(info->struct_size, sizeof(r))); // no more than that is written
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_sp2m(aoclsparse_operation opA, const aoclsparse_mat_descr descrA,
                                  const aoclsparse_matrix A, aoclsparse_operation opB,
                                  const aoclsparse_mat_descr descrB, const aoclsparse_matrix B,
                                  const aoclsparse_request request, aoclsparse_matrix *C)
{
    return sp2m_any(opA, descrA, A, opB, descrB, B, request, C);
}

aoclsparse_status aoclsparse_spmm(aoclsparse_operation opA, const aoclsparse_matrix A,
                                  const aoclsparse_matrix B, aoclsparse_matrix *C)
{
    // level3/aoclsparse_spmm.cpp:27-67: general descriptors in each matrix's base, full computation
    if(!A || !B || !C)
        return aoclsparse_status_invalid_pointer;
    _aoclsparse_mat_descr dA, dB;
    dA.base = A->base;
    dB.base = B->base;
    return sp2m_any(opA, &dA, A, aoclsparse_operation_none, &dB, B, aoclsparse_stage_full_computation, C);
}

aoclsparse_status aoclsparse_dcsr2m(aoclsparse_operation trans_A, const aoclsparse_mat_descr descrA,
                                    const aoclsparse_matrix csrA, aoclsparse_operation trans_B,
                                    const aoclsparse_mat_descr descrB, const aoclsparse_matrix csrB,
                                    const aoclsparse_request request, aoclsparse_matrix *csrC)
{
    if(!descrA || !descrB || !csrA || !csrB || !csrC)
        return aoclsparse_status_invalid_pointer;
    return sp2m_t<double>(trans_A, descrA, csrA, trans_B, descrB, csrB, request, csrC, aoclsparse_dmat);
}

aoclsparse_status aoclsparse_scsr2m(aoclsparse_operation trans_A, const aoclsparse_mat_descr descrA,
                                    const aoclsparse_matrix csrA, aoclsparse_operation trans_B,
                                    const aoclsparse_mat_descr descrB, const aoclsparse_matrix csrB,
                                    const aoclsparse_request request, aoclsparse_matrix *csrC)
{
    if(!descrA || !descrB || !csrA || !csrB || !csrC)
        return aoclsparse_status_invalid_pointer;
    return sp2m_t<float>(trans_A, descrA, csrA, trans_B, descrB, csrB, request, csrC, aoclsparse_smat);
}

} // extern "C"
