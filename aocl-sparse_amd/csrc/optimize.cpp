// optimize.cpp -- aoclsparse_optimize: the inspector step.
//
// Hint bookkeeping follows analysis/aoclsparse_analysis.cpp:426-566 of the reference (which hints
// count as "mv only", when the clean CSR is built, idempotence).  What an optimisation PRODUCES is
// MI355X-specific: instead of CPU formats (br4 / ELL-hybrid / blocked CSR) the matrix is made
// resident in HBM and the execution plans of the hinted operations are built once:
//   mv  hint -> device CSR (+ A^T copy for a transposed hint) + CSR-Adaptive row blocks
//   sv  hint -> clean CSR, idiag/iurow, level sets of the hinted triangle, device copies
//   mm / 2m  -> clean CSR + device CSR
#include "internal.hpp"

using namespace mi355;

extern "C" aoclsparse_status aoclsparse_optimize(aoclsparse_matrix A)
{
    if(!A)
        return aoclsparse_status_invalid_pointer;
    if(A->m < 0 || A->n < 0 || A->nnz < 0)
        return aoclsparse_status_invalid_size;
    if(A->input_format == aoclsparse_tcsr_mat)
    {
        // analysis.cpp:467-468: nothing to do on the host.  Here the hints put the triangles in HBM and build the TRSV plans ahead
        // of the first call (skipped without a device and under aoclsparse_memory_usage_minimal, as below).
        Runtime &rt = Runtime::get();
        if(A->mem_policy == aoclsparse_memory_usage_unrestricted && A->m > 0 && rt.init() == aoclsparse_status_success)
            for(Hint &h : A->hints)
            {
                if(h.optimized)
                    continue;
                aoclsparse_status st = aoclsparse_status_success;
                if(h.act == action_mv && h.type == aoclsparse_matrix_type_general)
                    for(aoclsparse_matrix t : A->tcsr_tri)
                    {
                        std::unique_lock<std::shared_mutex> w(t->guard);
                        if(st == aoclsparse_status_success && !t->dev_user.valid)
                            st = upload_csr(t->user, val_size(A->val_type), t->dev_user);
                    }
                else if((h.act == action_sv || h.act == action_sm_row || h.act == action_sm_col)
                        && (h.type == aoclsparse_matrix_type_triangular || h.type == aoclsparse_matrix_type_symmetric))
                {
                    const aoclsparse_matrix t = tcsr_triangle(A, h.fill);
                    st                        = csr_optimize(t);
                    if(st == aoclsparse_status_success)
                        st = ensure_trsv(t, h.fill == aoclsparse_fill_mode_upper, h.trans != aoclsparse_operation_none,
                                         h.trans == aoclsparse_operation_conjugate_transpose, /*need_rows=*/false);
                }
                if(st != aoclsparse_status_success)
                    return st;
            }
        for(Hint &h : A->hints)
            h.optimized = true;
        return aoclsparse_status_success;
    }
    if(A->input_format == aoclsparse_bsr_mat) // analysis.cpp:472-474: the first matrix of a BSR handle is no CSR.  Its mirror goes
        return aoclsparse_status_not_implemented; // to HBM at the first product
    if(!A->user.ptr || !A->user.ind || !A->user.val)
        return aoclsparse_status_invalid_pointer;

    // classify pending hints (analysis.cpp:484-508)
    bool           all_done = true;
    aoclsparse_int mv_count = 0, other = 0, sum = 0;
    for(Hint &h : A->hints)
    {
        if(h.optimized)
            continue;
        all_done = false;
        if((h.act == action_mv || h.act == action_dotmv) && h.trans == aoclsparse_operation_none
           && h.type == aoclsparse_matrix_type_general && A->val_type == aoclsparse_dmat && h.nop > 0)
            mv_count++; // would select optimize_mv in the reference; here every mv hint gets a plan
        else if((h.act == action_ilu0 || h.act == action_symgs) && h.nop > 0)
            ; // counted apart (analysis.cpp:499-502): neither asks for the clean CSR
        else
            other++;
        sum++;
    }
    if(all_done) // also the no-hint case: analysis.cpp:509-511 returns before doing anything
        return aoclsparse_status_success;

    aoclsparse_status st = aoclsparse_status_success;
    (void)mv_count;
    if(other || sum == 0)
    {
        st = csr_optimize(A); // clean CSR (analysis.cpp:513-553)
        if(st != aoclsparse_status_success)
            return st;
    }

    // analysis.cpp:555-564: an ILU hint makes optimize allocate the factor's value array
    for(Hint &h : A->hints)
        if(!h.optimized && h.act == action_ilu0)
        {
            st = ilu_prepare(A);
            if(st != aoclsparse_status_success)
                return st;
        }

    // Device residency + plans.  A box without a GPU (the CPU-only test tier) still completes the
    // host analysis above; device work is attempted only when a device exists and is skipped for
    // aoclsparse_memory_usage_minimal, which forbids copies of the matrix (analysis.cpp:446).
    Runtime &rt = Runtime::get();
    if(A->mem_policy == aoclsparse_memory_usage_unrestricted && A->m > 0 && A->n > 0 && A->nnz > 0
       && rt.init() == aoclsparse_status_success)
    {
        for(Hint &h : A->hints)
        {
            if(h.optimized)
                continue;
            if(h.act == action_mv && h.type == aoclsparse_matrix_type_general)
            {
                DeviceCsr *d = nullptr;
                SpmvPlan  *p = nullptr;
                st = ensure_spmv(A, h.trans != aoclsparse_operation_none, d, p);
                if(st == aoclsparse_status_success && h.nop > 0 && !is_complex_type(A->val_type))
                {
                    // the mv hint's format choice (analysis.cpp:146-382 picks br4 / ELLT-HYB / blocked CSR on
                    // the CPU): a SELL-64 copy when its padding is small
                    std::unique_lock<std::shared_mutex> w(A->guard);
                    const HostCsr &hc = h.trans != aoclsparse_operation_none ? *A->trans : A->user;
                    st                = build_sell(hc.ptr, *d, val_size(A->val_type), *p);
                }
            }
            else if((h.act == action_sv || h.act == action_sm_row || h.act == action_sm_col)
                    && (h.type == aoclsparse_matrix_type_triangular
                        || h.type == aoclsparse_matrix_type_symmetric))
            {
                // (what the automatic schedule needs: the level-ordered row layout is built on first use if a solve asks for it)
                st = ensure_trsv(A, h.fill == aoclsparse_fill_mode_upper, h.trans != aoclsparse_operation_none,
                                 h.trans == aoclsparse_operation_conjugate_transpose, /*need_rows=*/false);
            }
            else if(h.act == action_mm || h.act == action_2m)
            {
                DeviceCsr *d = nullptr;
                SpmvPlan  *p = nullptr;
                st = ensure_spmv(A, false, d, p);
                if(st == aoclsparse_status_success && h.act == action_mm && h.trans == aoclsparse_operation_none && h.nop > 0)
                {
                    // the mm hint's format choice (the reference builds its blocked CSR in optimize by a fill threshold,
                    // analysis.cpp:146-160, convert.cpp:36-147): a blocked-ELL copy for the MFMA kernel when the 16 x 16
                    // tiles are at least half full
                    std::unique_lock<std::shared_mutex> w(A->guard);
                    st = build_bell(A->user, *d, *p, A->val_type);
                }
            }
            if(st != aoclsparse_status_success)
                return st;
        }
    }
    for(Hint &h : A->hints)
        h.optimized = true;
    return aoclsparse_status_success;
}
