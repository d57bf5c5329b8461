// trsv_api.cpp -- aoclsparse_?trsv(_kid)(_strided), ?trsm, ?csrsv: checks, schedule choice, dispatch.
//
// Argument checks and their order: level2/aoclsparse_trsv.cpp:59-137 of the reference.  The solve
// itself is the level-scheduled HIP path of trsv_kernels.hip on the plans of trsv_plan.cpp; which schedule
// runs is decided by resolve_trsv_schedule (trsv_schedule.hpp).
#include "trsv_schedule.hpp"

#include <type_traits>

using namespace mi355;

namespace
{

#define MI355_TRY(expr)                       \
    do                                        \
    {                                         \
        aoclsparse_status st__ = (expr);      \
        if(st__ != aoclsparse_status_success) \
            return st__;                      \
    } while(0)

// Shared tail of trsv / trsm: plan lookup, schedule choice, staging of host operands, launch.
// b / x describe nrhs right-hand sides: column c at b + c*b_off (element stride incb), likewise x.
// span_b / span_x = number of elements of the caller's arrays that the strided views cover.
template <typename T>
aoclsparse_status solve_core(aoclsparse_operation trans, T alpha, aoclsparse_matrix A,
                             const aoclsparse_mat_descr descr, aoclsparse_int kid, const T *b, T *x,
                             aoclsparse_int nrhs, long long b_off, aoclsparse_int incb, size_t span_b,
                             long long x_off, aoclsparse_int incx, size_t span_x, bool x_partial)
{
    const aoclsparse_int m  = A->m;
    Runtime             &rt = Runtime::get();
    aoclsparse_status    st = rt.init();
    if(st != aoclsparse_status_success)
        return st;
    const bool upper = descr->fill_mode == aoclsparse_fill_mode_upper;
    const bool tr    = trans != aoclsparse_operation_none;
    const bool unit  = descr->diag_type == aoclsparse_diag_type_unit;
    constexpr bool is_cplx = !std::is_floating_point<T>::value;
    const bool     conj    = is_cplx && trans == aoclsparse_operation_conjugate_transpose;
    st                     = ensure_trsv(A, upper, tr, conj, /*need_rows=*/false);
    if(st != aoclsparse_status_success)
        return st;
    // Round 3: the kid selects the ARITHMETIC, as it does in the reference (trsv.cpp:321-353), not the schedule.  kid 0 and auto:
    // the chain of ref_trsv_* -- every schedule reproduces it, so the fastest one runs; kid 1 / 2: the order of the 256-bit KT
    // kernels, kid 3: of the 512-bit ones (kt_trsv_l / kt_trsv_u, trsv_kt.cpp:64-150, :297-383), bit for bit, served by the
    // block kernel with run-time KT loops (triangles with chains), the per-level launches and the lane-per-position kernel.  The transposed KT kernels apply the same per-element fma
    // as the reference kernels (trsv_kt.cpp:183-268, :416-503), so for op != none every kid has the same bits.
    // aoclsparse_mi355_set_trsv_schedule forces a schedule (tests, measurements).
    const int       kt_bits = (!is_cplx && !tr && kid >= 1) ? (kid == 3 ? 512 : 256) : 0;
    const int       forced  = Runtime::primary().trsv_schedule;
    const TrsvPlan &plan    = A->trsv_plan[trsv_plan_index(upper, tr, conj)];
    auto            resolve = [&] { return resolve_trsv_schedule(plan, m, is_cplx, upper, tr, conj, forced, nrhs, incb == 1 && incx == 1, kt_bits); };
    {
        // the level-ordered row layout is built on demand, for the schedules that walk it
        bool rows_needed;
        {
            std::shared_lock<std::shared_mutex> r0(A->guard);
            rows_needed = !plan.rows_valid && resolve().needs_rows;
        }
        if(rows_needed)
        {
            st = ensure_trsv(A, upper, tr, conj, true);
            if(st != aoclsparse_status_success)
                return st;
        }
    }
    // solves on one handle share its workspaces: serialise their enqueue (kernels are stream-ordered)
    CallScope cs(CallScope::Always);
    MI355_TRY(cs.st);
    std::shared_lock<std::shared_mutex> r(A->guard);
    const TrsvChoice                    choice = resolve(); // what runs, now that the plan is complete
    // the handle's own timeout word (pinned, device-mapped): allocated once per handle
    if(!is_cplx && !A->trsv_timeout_dev)
    {
        void *tw = nullptr, *twd = nullptr;
        if(hipHostMalloc(&tw, 64, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&twd, tw, 0) == hipSuccess)
        {
            A->trsv_timeout_host  = static_cast<volatile unsigned int *>(tw);
            *A->trsv_timeout_host = 0;
            A->trsv_timeout_dev   = static_cast<unsigned int *>(twd);
        }
        else
        {
            (void)hipGetLastError(); // the solve then keeps its device-side word and a blocking read
            if(tw)
                (void)hipHostFree(tw);
        }
    }
    // a wait that expired in an EARLIER asynchronous (device-pointer) solve OF THIS HANDLE is reported now; callers that
    // never solve again ask aoclsparse_mi355_trsv_status(A) after their own stream synchronisation
    if(A->trsv_timeout_host && *A->trsv_timeout_host)
    {
        (void)hipStreamSynchronize(rt.stream());
        *A->trsv_timeout_host = 0;
        return aoclsparse_status_internal_error;
    }

    // (+ TRSV_XP_PAD elements: the block kernel parks the stores of lanes / rows that own nothing there)
    st = A->trsv_xp.alloc(sizeof(T) * ((size_t)m * (size_t)nrhs + TRSV_XP_PAD));
    if(st == aoclsparse_status_success)
        st = A->trsv_scratch.alloc(sizeof(unsigned int) * ((size_t)nrhs + 1 + (size_t)nrhs * (size_t)std::max<aoclsparse_int>(plan.blk.nlevels, 0)));
    if(st != aoclsparse_status_success)
        return st;

    // the workspaces are reused in stream order; after a change of stream (aoclsparse_mi355_set_stream) nothing orders this
    // solve behind the previous one, so everything enqueued so far completes first
    st = workspace_stream_guard(A, rt.stream());
    if(st != aoclsparse_status_success)
        return st;

    // the scope serves the views only: when to copy x back and synchronise also depends on the timeout word, below
    // (strided / padded x goes in: the untouched slots must survive the round trip)
    const T *db = cs.in(STAGE_TRSV_B, b, sizeof(T) * span_b);
    T       *dx = cs.inout(STAGE_TRSV_X, x, sizeof(T) * span_x, x_partial, /*copy_back=*/false);
    MI355_TRY(cs.st);
    const bool xdev = dx == x;
    if constexpr(is_cplx)
        st = launch_ctrsv(rt.stream(), unit, conj, alpha, m, plan, A->dev_diag.as<T>(), db, dx, A->trsv_xp.as<T>(), nrhs,
                          b_off, incb, x_off, incx);
    else
        st = launch_trsv<T>(rt.stream(), choice.schedule, unit, alpha, m, plan, A->dev_diag.as<T>(), db, dx,
                            A->trsv_xp.as<T>(), A->trsv_scratch.as<unsigned int>(), nrhs, b_off, incb, x_off, incx,
                            A->trsv_timeout_dev, kt_bits);
    if(st != aoclsparse_status_success)
        return st;
    if(!xdev)
        MI355_HIP_TRY(hipMemcpyAsync(x, dx, sizeof(T) * span_x, hipMemcpyDeviceToHost, rt.stream()));
    const bool syncfree    = choice.syncfree;
    const bool pinned_word = A->trsv_timeout_dev != nullptr;
    if(!xdev || (syncfree && !pinned_word))
    {
        // host semantics (the result must be in the caller's memory on return); without the pinned word the
        // sync-free path also has to fetch its device-side timeout word
        MI355_HIP_TRY(hipStreamSynchronize(rt.stream()));
        if(syncfree && !pinned_word)
        {
            unsigned int word = 0;
            MI355_HIP_TRY(hipMemcpy(&word, A->trsv_scratch.as<unsigned int>() + nrhs, sizeof(word),
                                    hipMemcpyDeviceToHost));
            if(word)
                return aoclsparse_status_internal_error;
        }
    }
    // device-pointer solves stay asynchronous: an expired wait (never expected) is seen at the next solve; a
    // host-pointer solve has just synchronised and reports it now
    if(syncfree && pinned_word && !xdev && *A->trsv_timeout_host)
    {
        *A->trsv_timeout_host = 0;
        return aoclsparse_status_internal_error;
    }
    return aoclsparse_status_success;
}

template <typename T>
aoclsparse_status trsv_t(aoclsparse_operation trans, const T alpha, aoclsparse_matrix A,
                         const aoclsparse_mat_descr descr, const T *b, aoclsparse_int incb, T *x,
                         aoclsparse_int incx, aoclsparse_int kid, aoclsparse_matrix_data_type vt)
{
    // trsv.cpp:59-113
    if(!A || !x || !b || !descr)
        return aoclsparse_status_invalid_pointer;
    const bool tcsr = A->input_format == aoclsparse_tcsr_mat; // trsv.cpp:62-67: CSR / CSC and TCSR handles
    if(A->input_format != aoclsparse_csr_mat && !tcsr)
        return aoclsparse_status_not_implemented;
    const aoclsparse_int m = A->m;
    if(m <= 0 || A->nnz <= 0)
        return aoclsparse_status_invalid_size;
    if(m != A->n || incb <= 0 || incx <= 0)
        return aoclsparse_status_invalid_value;
    if(!tcsr && !A->user.ptr)
        return aoclsparse_status_invalid_pointer;
    if(descr->base != A->base)
        return aoclsparse_status_invalid_value;
    if(descr->base != aoclsparse_index_base_zero && descr->base != aoclsparse_index_base_one)
        return aoclsparse_status_invalid_value;
    if(trans != aoclsparse_operation_none && trans != aoclsparse_operation_transpose
       && trans != aoclsparse_operation_conjugate_transpose)
        return aoclsparse_status_not_implemented;
    if(descr->type != aoclsparse_matrix_type_symmetric && descr->type != aoclsparse_matrix_type_triangular)
        return aoclsparse_status_invalid_value;
    if(descr->diag_type == aoclsparse_diag_type_zero)
        return aoclsparse_status_invalid_value;
    if(descr->fill_mode != aoclsparse_fill_mode_lower && descr->fill_mode != aoclsparse_fill_mode_upper)
        return aoclsparse_status_not_implemented;
    if(A->val_type != vt)
        return aoclsparse_status_wrong_type;
    // trsv.cpp:158-176: a TCSR handle is solved on the triangle the fill mode names -- L with (ilrow, idiag, iurow) = (ptr_L,
    // ptr_L[i + 1] - 1, ptr_L + 1), U with (ptr_U, ptr_U, ptr_U[i] + 1), which is what the clean-CSR step finds on that
    // triangle's own handle; its plans, schedules and kernels are the CSR ones
    if(tcsr)
        A = tcsr_triangle(A, descr->fill_mode);

    // trsv.cpp:128-137: lazy clean CSR, then the rank check
    aoclsparse_status st = csr_optimize(A);
    if(st != aoclsparse_status_success)
        return st;
    if(!A->opt_csr_full_diag && descr->diag_type != aoclsparse_diag_type_unit)
        return aoclsparse_status_invalid_value;
    // KAT of trsv.cpp:315-376 has kernels 0..3 per doid
    if(kid > 3)
        return aoclsparse_status_invalid_kid;
    // (m-1)*inc must not overflow, trsv.cpp:407-411
    if((long long)(m - 1) * incb > 2147483647LL || (long long)(m - 1) * incx > 2147483647LL)
        return aoclsparse_status_invalid_size;
    return solve_core<T>(trans, alpha, A, descr, kid, b, x, 1, 0, incb, (size_t)(m - 1) * incb + 1, 0, incx,
                         (size_t)(m - 1) * incx + 1, incx != 1);
}

// level3/aoclsparse_trsm.hpp:40-160: X = alpha * inv(op(A)) * B column by column.  The reference loops
// aoclsparse::trsv over the n columns (OpenMP over columns); here all columns run in ONE launch (the
// level structure is shared, blockIdx.y is the column), each bit-identical to the single-RHS solve.
template <typename T>
aoclsparse_status trsm_t(aoclsparse_operation trans, const T alpha, aoclsparse_matrix A,
                         const aoclsparse_mat_descr descr, aoclsparse_order order, const T *B, aoclsparse_int n,
                         aoclsparse_int ldb, T *X, aoclsparse_int ldx, aoclsparse_int kid,
                         aoclsparse_matrix_data_type vt)
{
    if(!A || !X || !B || !descr)
        return aoclsparse_status_invalid_pointer;
    const bool tcsr = A->input_format == aoclsparse_tcsr_mat; // trsm.hpp:62-67, 107-117
    if(!holds_no_csr(A) && !A->user.ptr)
        return aoclsparse_status_invalid_pointer;
    if(descr->base != A->base)
        return aoclsparse_status_invalid_value;
    if(A->input_format != aoclsparse_csr_mat && !tcsr)
        return aoclsparse_status_not_implemented;
    const aoclsparse_int m = A->m;
    if(m < 0 || A->nnz < 0 || n < 0)
        return aoclsparse_status_invalid_size;
    if(m == 0 || A->n == 0 || A->nnz == 0 || n == 0)
        return aoclsparse_status_success;
    if(m != A->n)
        return aoclsparse_status_invalid_size;
    if(ldb < 0 || ldx < 0)
        return aoclsparse_status_invalid_size;
    if(descr->base != aoclsparse_index_base_zero && descr->base != aoclsparse_index_base_one)
        return aoclsparse_status_invalid_value;
    if(trans != aoclsparse_operation_none && trans != aoclsparse_operation_transpose
       && trans != aoclsparse_operation_conjugate_transpose)
        return aoclsparse_status_invalid_value;
    if(descr->type != aoclsparse_matrix_type_symmetric && descr->type != aoclsparse_matrix_type_triangular)
        return aoclsparse_status_invalid_value;
    if(descr->fill_mode != aoclsparse_fill_mode_lower && descr->fill_mode != aoclsparse_fill_mode_upper)
        return aoclsparse_status_not_implemented;
    if(A->val_type != vt)
        return aoclsparse_status_wrong_type;
    if(tcsr) // the triangle's own handle, as in trsv_t
        A = tcsr_triangle(A, descr->fill_mode);
    aoclsparse_status st = csr_optimize(A);
    if(st != aoclsparse_status_success)
        return st;
    aoclsparse_int incb, incx;
    long long      b_off, x_off;
    if(order == aoclsparse_order_row)
        incb = ldb, incx = ldx, b_off = 1, x_off = 1;
    else if(order == aoclsparse_order_column)
        incb = 1, incx = 1, b_off = ldb, x_off = ldx;
    else
        return aoclsparse_status_invalid_value;
    if((long long)n * b_off > 2147483647LL || (long long)n * x_off > 2147483647LL)
        return aoclsparse_status_invalid_size;
    // what every per-column trsv of the reference checks (trsv.cpp:72-137)
    if(incb <= 0 || incx <= 0 || descr->diag_type == aoclsparse_diag_type_zero)
        return aoclsparse_status_invalid_value;
    if(!A->opt_csr_full_diag && descr->diag_type != aoclsparse_diag_type_unit)
        return aoclsparse_status_invalid_value;
    if(kid > 3)
        return aoclsparse_status_invalid_kid;
    const size_t span_b = (size_t)(m - 1) * incb + (size_t)(n - 1) * b_off + 1;
    const size_t span_x = (size_t)(m - 1) * incx + (size_t)(n - 1) * x_off + 1;
    if(span_b > 2147483647ULL || span_x > 2147483647ULL)
        return aoclsparse_status_invalid_size;
    const bool dense_x = order == aoclsparse_order_row ? ldx == n : ldx == m;
    return solve_core<T>(trans, alpha, A, descr, kid, B, X, n, b_off, incb, span_b, x_off, incx, span_x, !dense_x);
}

// aoclsparse_?csrsv (level2/aoclsparse_csrsv.hpp:28-190): the older raw-array solve, y = inv(T) * alpha * x with T the
// lower / upper triangle of the CSR arrays chosen by descr->fill_mode.  Its row loop is the chain of ref_trsv_l / _u
// (alpha*x_i, subtract in storage order, divide by the diagonal), so it is served by the TRSV path on a one-shot
// handle over the caller's arrays (kid 0 order: bit-identical for sorted rows with a full diagonal).
// Deviations, both on input the reference mishandles: rows are sorted by the clean-CSR step instead of being cut at
// the first upper entry, and a missing diagonal of a non-unit solve is invalid_value instead of a division by a
// stale entry.  Host arrays only (the analysis walks them).
template <typename T>
aoclsparse_status csrsv_t(aoclsparse_operation trans, const T *alpha, aoclsparse_int m, const T *csr_val,
                          const aoclsparse_int *csr_col_ind, const aoclsparse_int *csr_row_ptr,
                          const aoclsparse_mat_descr descr, const T *x, T *y)
{
    if(!csr_val || !csr_row_ptr || !csr_col_ind || !x || !y || !descr || !alpha)
        return aoclsparse_status_invalid_pointer;
    if(descr->base != aoclsparse_index_base_zero)
        return aoclsparse_status_not_implemented;
    if(descr->type != aoclsparse_matrix_type_general && descr->type != aoclsparse_matrix_type_symmetric)
        return aoclsparse_status_not_implemented;
    if(trans != aoclsparse_operation_none)
        return aoclsparse_status_not_implemented;
    if(m < 0)
        return aoclsparse_status_invalid_size;
    if(m == 0)
        return aoclsparse_status_success;
    Runtime &rt = Runtime::get();
    MI355_TRY(rt.init());
    if(rt.is_device_pointer(csr_row_ptr) || rt.is_device_pointer(csr_col_ind) || rt.is_device_pointer(csr_val))
        return aoclsparse_status_not_implemented;
    aoclsparse_matrix A  = nullptr;
    aoclsparse_status st = std::is_same<T, float>::value
                               ? aoclsparse_create_scsr(&A, descr->base, m, m, csr_row_ptr[m] - descr->base,
                                                        const_cast<aoclsparse_int *>(csr_row_ptr),
                                                        const_cast<aoclsparse_int *>(csr_col_ind),
                                                        reinterpret_cast<float *>(const_cast<T *>(csr_val)))
                               : aoclsparse_create_dcsr(&A, descr->base, m, m, csr_row_ptr[m] - descr->base,
                                                        const_cast<aoclsparse_int *>(csr_row_ptr),
                                                        const_cast<aoclsparse_int *>(csr_col_ind),
                                                        reinterpret_cast<double *>(const_cast<T *>(csr_val)));
    if(st != aoclsparse_status_success)
        return st;
    _aoclsparse_mat_descr tri = *descr;
    tri.type                  = aoclsparse_matrix_type_triangular;
    if(tri.fill_mode != aoclsparse_fill_mode_lower)
        tri.fill_mode = aoclsparse_fill_mode_upper; // csrsv.hpp:77-86: anything but lower runs the upper solve
    st = trsv_t<T>(aoclsparse_operation_none, *alpha, A, &tri, x, 1, y, 1, 0,
                   std::is_same<T, float>::value ? aoclsparse_smat : aoclsparse_dmat);
    aoclsparse_destroy(&A);
    return st;
}

} // namespace

extern "C" {

aoclsparse_status aoclsparse_dcsrsv(aoclsparse_operation trans, const double *alpha, aoclsparse_int m,
                                    const double *csr_val, const aoclsparse_int *csr_col_ind,
                                    const aoclsparse_int *csr_row_ptr, const aoclsparse_mat_descr descr, const double *x,
                                    double *y)
{
    return csrsv_t<double>(trans, alpha, m, csr_val, csr_col_ind, csr_row_ptr, descr, x, y);
}
aoclsparse_status aoclsparse_scsrsv(aoclsparse_operation trans, const float *alpha, aoclsparse_int m,
                                    const float *csr_val, const aoclsparse_int *csr_col_ind,
                                    const aoclsparse_int *csr_row_ptr, const aoclsparse_mat_descr descr, const float *x,
                                    float *y)
{
    return csrsv_t<float>(trans, alpha, m, csr_val, csr_col_ind, csr_row_ptr, descr, x, y);
}

aoclsparse_status aoclsparse_dtrsv(aoclsparse_operation trans, const double alpha, aoclsparse_matrix A,
                                   const aoclsparse_mat_descr descr, const double *b, double *x)
{
    return trsv_t<double>(trans, alpha, A, descr, b, 1, x, 1, -1, aoclsparse_dmat);
}

aoclsparse_status aoclsparse_strsv(aoclsparse_operation trans, const float alpha, aoclsparse_matrix A,
                                   const aoclsparse_mat_descr descr, const float *b, float *x)
{
    return trsv_t<float>(trans, alpha, A, descr, b, 1, x, 1, -1, aoclsparse_smat);
}

aoclsparse_status aoclsparse_dtrsv_kid(aoclsparse_operation trans, const double alpha, aoclsparse_matrix A,
                                       const aoclsparse_mat_descr descr, const double *b, double *x,
                                       aoclsparse_int kid)
{
    return trsv_t<double>(trans, alpha, A, descr, b, 1, x, 1, kid, aoclsparse_dmat);
}

aoclsparse_status aoclsparse_strsv_kid(aoclsparse_operation trans, const float alpha, aoclsparse_matrix A,
                                       const aoclsparse_mat_descr descr, const float *b, float *x,
                                       aoclsparse_int kid)
{
    return trsv_t<float>(trans, alpha, A, descr, b, 1, x, 1, kid, aoclsparse_smat);
}

aoclsparse_status aoclsparse_dtrsv_strided(aoclsparse_operation trans, const double alpha, aoclsparse_matrix A,
                                           const aoclsparse_mat_descr descr, const double *b,
                                           const aoclsparse_int incb, double *x, const aoclsparse_int incx)
{
    return trsv_t<double>(trans, alpha, A, descr, b, incb, x, incx, -1, aoclsparse_dmat);
}

aoclsparse_status aoclsparse_strsv_strided(aoclsparse_operation trans, const float alpha, aoclsparse_matrix A,
                                           const aoclsparse_mat_descr descr, const float *b,
                                           const aoclsparse_int incb, float *x, const aoclsparse_int incx)
{
    return trsv_t<float>(trans, alpha, A, descr, b, incb, x, incx, -1, aoclsparse_smat);
}

aoclsparse_status aoclsparse_dtrsm(const aoclsparse_operation trans, const double alpha, aoclsparse_matrix A,
                                   const aoclsparse_mat_descr descr, aoclsparse_order order, const double *B,
                                   aoclsparse_int n, aoclsparse_int ldb, double *X, aoclsparse_int ldx)
{
    return trsm_t<double>(trans, alpha, A, descr, order, B, n, ldb, X, ldx, -1, aoclsparse_dmat);
}

aoclsparse_status aoclsparse_strsm(const aoclsparse_operation trans, const float alpha, aoclsparse_matrix A,
                                   const aoclsparse_mat_descr descr, aoclsparse_order order, const float *B,
                                   aoclsparse_int n, aoclsparse_int ldb, float *X, aoclsparse_int ldx)
{
    return trsm_t<float>(trans, alpha, A, descr, order, B, n, ldb, X, ldx, -1, aoclsparse_smat);
}

aoclsparse_status aoclsparse_dtrsm_kid(const aoclsparse_operation trans, const double alpha, aoclsparse_matrix A,
                                       const aoclsparse_mat_descr descr, aoclsparse_order order, const double *B,
                                       aoclsparse_int n, aoclsparse_int ldb, double *X, aoclsparse_int ldx,
                                       const aoclsparse_int kid)
{
    return trsm_t<double>(trans, alpha, A, descr, order, B, n, ldb, X, ldx, kid, aoclsparse_dmat);
}

aoclsparse_status aoclsparse_strsm_kid(const aoclsparse_operation trans, const float alpha, aoclsparse_matrix A,
                                       const aoclsparse_mat_descr descr, aoclsparse_order order, const float *B,
                                       aoclsparse_int n, aoclsparse_int ldb, float *X, aoclsparse_int ldx,
                                       const aoclsparse_int kid)
{
    return trsm_t<float>(trans, alpha, A, descr, order, B, n, ldb, X, ldx, kid, aoclsparse_smat);
}

aoclsparse_status aoclsparse_ctrsv(aoclsparse_operation trans, const aoclsparse_float_complex alpha, aoclsparse_matrix A,
                                   const aoclsparse_mat_descr descr, const aoclsparse_float_complex *b, aoclsparse_float_complex *x)
{
    return trsv_t<cfloat>(trans, cfloat(alpha.real, alpha.imag), A, descr, reinterpret_cast<const cfloat *>(b), 1,
                         reinterpret_cast<cfloat *>(x), 1, -1, aoclsparse_cmat);
}
aoclsparse_status aoclsparse_ctrsv_kid(aoclsparse_operation trans, const aoclsparse_float_complex alpha, aoclsparse_matrix A,
                                       const aoclsparse_mat_descr descr, const aoclsparse_float_complex *b, aoclsparse_float_complex *x, aoclsparse_int kid)
{
    return trsv_t<cfloat>(trans, cfloat(alpha.real, alpha.imag), A, descr, reinterpret_cast<const cfloat *>(b), 1,
                         reinterpret_cast<cfloat *>(x), 1, kid, aoclsparse_cmat);
}
aoclsparse_status aoclsparse_ctrsv_strided(aoclsparse_operation trans, const aoclsparse_float_complex alpha, aoclsparse_matrix A,
                                           const aoclsparse_mat_descr descr, const aoclsparse_float_complex *b, const aoclsparse_int incb,
                                           aoclsparse_float_complex *x, const aoclsparse_int incx)
{
    return trsv_t<cfloat>(trans, cfloat(alpha.real, alpha.imag), A, descr, reinterpret_cast<const cfloat *>(b), incb,
                         reinterpret_cast<cfloat *>(x), incx, -1, aoclsparse_cmat);
}
aoclsparse_status aoclsparse_ctrsm(const aoclsparse_operation trans, const aoclsparse_float_complex alpha, aoclsparse_matrix A,
                                   const aoclsparse_mat_descr descr, aoclsparse_order order, const aoclsparse_float_complex *B,
                                   aoclsparse_int n, aoclsparse_int ldb, aoclsparse_float_complex *X, aoclsparse_int ldx)
{
    return trsm_t<cfloat>(trans, cfloat(alpha.real, alpha.imag), A, descr, order, reinterpret_cast<const cfloat *>(B), n, ldb,
                         reinterpret_cast<cfloat *>(X), ldx, -1, aoclsparse_cmat);
}
aoclsparse_status aoclsparse_ctrsm_kid(const aoclsparse_operation trans, const aoclsparse_float_complex alpha, aoclsparse_matrix A,
                                       const aoclsparse_mat_descr descr, aoclsparse_order order, const aoclsparse_float_complex *B,
                                       aoclsparse_int n, aoclsparse_int ldb, aoclsparse_float_complex *X, aoclsparse_int ldx,
                                       const aoclsparse_int kid)
{
    return trsm_t<cfloat>(trans, cfloat(alpha.real, alpha.imag), A, descr, order, reinterpret_cast<const cfloat *>(B), n, ldb,
                         reinterpret_cast<cfloat *>(X), ldx, kid, aoclsparse_cmat);
}

aoclsparse_status aoclsparse_ztrsv(aoclsparse_operation trans, const aoclsparse_double_complex alpha, aoclsparse_matrix A,
                                   const aoclsparse_mat_descr descr, const aoclsparse_double_complex *b, aoclsparse_double_complex *x)
{
    return trsv_t<cdouble>(trans, cdouble(alpha.real, alpha.imag), A, descr, reinterpret_cast<const cdouble *>(b), 1,
                         reinterpret_cast<cdouble *>(x), 1, -1, aoclsparse_zmat);
}
aoclsparse_status aoclsparse_ztrsv_kid(aoclsparse_operation trans, const aoclsparse_double_complex alpha, aoclsparse_matrix A,
                                       const aoclsparse_mat_descr descr, const aoclsparse_double_complex *b, aoclsparse_double_complex *x, aoclsparse_int kid)
{
    return trsv_t<cdouble>(trans, cdouble(alpha.real, alpha.imag), A, descr, reinterpret_cast<const cdouble *>(b), 1,
                         reinterpret_cast<cdouble *>(x), 1, kid, aoclsparse_zmat);
}
aoclsparse_status aoclsparse_ztrsv_strided(aoclsparse_operation trans, const aoclsparse_double_complex alpha, aoclsparse_matrix A,
                                           const aoclsparse_mat_descr descr, const aoclsparse_double_complex *b, const aoclsparse_int incb,
                                           aoclsparse_double_complex *x, const aoclsparse_int incx)
{
    return trsv_t<cdouble>(trans, cdouble(alpha.real, alpha.imag), A, descr, reinterpret_cast<const cdouble *>(b), incb,
                         reinterpret_cast<cdouble *>(x), incx, -1, aoclsparse_zmat);
}
aoclsparse_status aoclsparse_ztrsm(const aoclsparse_operation trans, const aoclsparse_double_complex alpha, aoclsparse_matrix A,
                                   const aoclsparse_mat_descr descr, aoclsparse_order order, const aoclsparse_double_complex *B,
                                   aoclsparse_int n, aoclsparse_int ldb, aoclsparse_double_complex *X, aoclsparse_int ldx)
{
    return trsm_t<cdouble>(trans, cdouble(alpha.real, alpha.imag), A, descr, order, reinterpret_cast<const cdouble *>(B), n, ldb,
                         reinterpret_cast<cdouble *>(X), ldx, -1, aoclsparse_zmat);
}
aoclsparse_status aoclsparse_ztrsm_kid(const aoclsparse_operation trans, const aoclsparse_double_complex alpha, aoclsparse_matrix A,
                                       const aoclsparse_mat_descr descr, aoclsparse_order order, const aoclsparse_double_complex *B,
                                       aoclsparse_int n, aoclsparse_int ldb, aoclsparse_double_complex *X, aoclsparse_int ldx,
                                       const aoclsparse_int kid)
{
    return trsm_t<cdouble>(trans, cdouble(alpha.real, alpha.imag), A, descr, order, reinterpret_cast<const cdouble *>(B), n, ldb,
                         reinterpret_cast<cdouble *>(X), ldx, kid, aoclsparse_zmat);
}

aoclsparse_status aoclsparse_mi355_strsv_full(aoclsparse_operation trans, float alpha, aoclsparse_matrix A,
                                              const aoclsparse_mat_descr descr, const float *b, aoclsparse_int incb,
                                              float *x, aoclsparse_int incx, aoclsparse_int kid)
{
    return trsv_t<float>(trans, alpha, A, descr, b, incb, x, incx, kid, aoclsparse_smat);
}
aoclsparse_status aoclsparse_mi355_dtrsv_full(aoclsparse_operation trans, double alpha, aoclsparse_matrix A,
                                              const aoclsparse_mat_descr descr, const double *b, aoclsparse_int incb,
                                              double *x, aoclsparse_int incx, aoclsparse_int kid)
{
    return trsv_t<double>(trans, alpha, A, descr, b, incb, x, incx, kid, aoclsparse_dmat);
}
aoclsparse_status aoclsparse_mi355_ctrsv_full(aoclsparse_operation trans, aoclsparse_float_complex alpha,
                                              aoclsparse_matrix A, const aoclsparse_mat_descr descr,
                                              const aoclsparse_float_complex *b, aoclsparse_int incb,
                                              aoclsparse_float_complex *x, aoclsparse_int incx, aoclsparse_int kid)
{
    return trsv_t<cfloat>(trans, cfloat(alpha.real, alpha.imag), A, descr, reinterpret_cast<const cfloat *>(b), incb,
                          reinterpret_cast<cfloat *>(x), incx, kid, aoclsparse_cmat);
}
aoclsparse_status aoclsparse_mi355_ztrsv_full(aoclsparse_operation trans, aoclsparse_double_complex alpha,
                                              aoclsparse_matrix A, const aoclsparse_mat_descr descr,
                                              const aoclsparse_double_complex *b, aoclsparse_int incb,
                                              aoclsparse_double_complex *x, aoclsparse_int incx, aoclsparse_int kid)
{
    return trsv_t<cdouble>(trans, cdouble(alpha.real, alpha.imag), A, descr, reinterpret_cast<const cdouble *>(b), incb,
                           reinterpret_cast<cdouble *>(x), incx, kid, aoclsparse_zmat);
}

aoclsparse_status aoclsparse_mi355_set_trsv_schedule(aoclsparse_int schedule)
{
    if(schedule < -1 || schedule > 5)
        return aoclsparse_status_invalid_value;
    Runtime::primary().trsv_schedule = (int)schedule;
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_mi355_trsv_status(aoclsparse_matrix A)
{
    if(!A)
        return aoclsparse_status_invalid_pointer;
    if(A->input_format == aoclsparse_tcsr_mat) // the solves ran on the triangles' own handles: either word counts (both are read and cleared)
    {
        const aoclsparse_status l = aoclsparse_mi355_trsv_status(A->tcsr_tri[0]), u = aoclsparse_mi355_trsv_status(A->tcsr_tri[1]);
        return l != aoclsparse_status_success ? l : u;
    }
    if(A->trsv_timeout_host && *A->trsv_timeout_host)
    {
        *A->trsv_timeout_host = 0;
        return aoclsparse_status_internal_error;
    }
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_mi355_get_trsv_levels(const aoclsparse_matrix A, aoclsparse_fill_mode fill,
                                                   aoclsparse_operation op, aoclsparse_int *levels)
{
    if(!A || !levels)
        return aoclsparse_status_invalid_pointer;
    if(A->input_format == aoclsparse_tcsr_mat) // the plans live on the triangle's own handle
        return aoclsparse_mi355_get_trsv_levels(tcsr_triangle(A, fill), fill, op, levels);
    std::shared_lock<std::shared_mutex> r(A->guard);
    const bool      up = fill == aoclsparse_fill_mode_upper, tr = op != aoclsparse_operation_none;
    const bool      cj = op == aoclsparse_operation_conjugate_transpose && is_complex_type(A->val_type);
    const TrsvPlan &p  = A->trsv_plan[trsv_plan_index(up, tr, cj)];
    *levels = p.valid ? p.nlevels : -1;
    return aoclsparse_status_success;
}

aoclsparse_status aoclsparse_mi355_get_trsv_info(const aoclsparse_matrix A, aoclsparse_fill_mode fill, aoclsparse_operation op,
                                                 aoclsparse_mi355_trsv_info *info)
{
    if(!A || !info)
        return aoclsparse_status_invalid_pointer;
    if(A->input_format == aoclsparse_tcsr_mat)
        return aoclsparse_mi355_get_trsv_info(tcsr_triangle(A, fill), fill, op, info);
    std::shared_lock<std::shared_mutex> r(A->guard);
    const bool      up = fill == aoclsparse_fill_mode_upper, tr = op != aoclsparse_operation_none;
    const bool      cj = op == aoclsparse_operation_conjugate_transpose && is_complex_type(A->val_type);
    const TrsvPlan &p  = A->trsv_plan[trsv_plan_index(up, tr, cj)];
    *info              = aoclsparse_mi355_trsv_info{};
    if(!p.valid)
        return aoclsparse_status_success;
    info->levels = p.nlevels;
    if(p.blk.valid)
        info->blocks = p.blk.nblocks, info->block_levels = p.blk.nlevels, info->slices = p.blk.nslices,
        info->slice_fan_in_permille = (aoclsparse_int)(p.blk.slice_fan_in * 1000.0 + 0.5);
    const TrsvChunkPlan &c = p.blk.chunk;
    info->model_chunk_us = (aoclsparse_int)c.model_us, info->model_block_us = (aoclsparse_int)c.model_block_us;
    if(p.blk.valid && c.valid)
        info->chunks = c.nchunks, info->steps = c.nsteps, info->lds_slots = c.max_rows;
    // what a single-RHS, unit-stride, kid-0 solve runs now (the request, where only the row layout is still to be built)
    info->schedule = resolve_trsv_schedule(p, A->m, is_complex_type(A->val_type), up, tr, cj, Runtime::primary().trsv_schedule, 1, true, 0).schedule;
    return aoclsparse_status_success;
}

} // extern "C"
