// sy_dense_api.cpp -- aoclsparse_?syrkd (C = alpha*A*A^H + beta*C, or alpha*A^H*A + beta*C) and aoclsparse_?syprd
// (C = alpha*A*B*A^H + beta*C, or alpha*A^H*B*A + beta*C; B dense, Hermitian, given by its upper triangle): the
// symmetric products whose result is the upper triangle of a dense matrix.
//
// Drivers follow the reference's argument checks in order: level3/aoclsparse_syrkd.cpp:38-112 and
// level3/aoclsparse_syrkd.hpp:170-319, level3/aoclsparse_syprd.cpp:42-168 and level3/aoclsparse_syprd.hpp:267-410.
// Every check comes before the first touch of the GPU.  The operands are the handle's device CSR and its cached stable
// transpose (ensure_spmv), so repeated products do not move the matrix again; B and C may live in host or device
// memory (pointer mode, as sp2md: the whole outer x ld block of a host C travels both ways, so the caller's lower
// triangle and padding survive).
//
// A handle created from CSC keeps the CSR of the SAME matrix in `user` (formats_api.cpp), where the reference keeps the
// CSR of the transpose and flips the operation (syrkd.hpp:213-236, syprd.hpp:306-348).  In terms of the caller's matrix
// both rows of the two dispatch tables compute one thing -- op = none: A*A^H / A*B*A^H, op = T / H: A^H*A / A^H*B*A --
// with the same chain per element, so one path serves both; only the sorted-input rule of syrkd reads the flip.
#include "internal.hpp"

#include <type_traits>
#include <vector>

using namespace mi355;

namespace
{

template <typename T>
constexpr bool is_cplx_v = !std::is_floating_point<T>::value;

template <typename T>
bool eq(T a, double v)
{
    if constexpr(is_cplx_v<T>)
        return a.re == v && a.im == 0;
    else
        return a == (T)v;
}

bool valid_op(aoclsparse_operation o)
{
    return o == aoclsparse_operation_none || o == aoclsparse_operation_transpose
           || o == aoclsparse_operation_conjugate_transpose;
}

bool valid_order(aoclsparse_order o)
{
    return o == aoclsparse_order_row || o == aoclsparse_order_column;
}

// a handle with a CSR (created from CSR or CSC); TCSR, BSR and COO handles have none
bool has_csr(const aoclsparse_matrix A)
{
    return A->input_format == aoclsparse_csr_mat && A->user.ptr;
}

constexpr int SORT_FULL = 1; // _aoclsparse_matrix::sort of fully sorted rows (matrix.cpp: mat_check)

// Does a row of the user CSR hold a column twice?  Looked up once per handle.
bool repeats_columns(aoclsparse_matrix A)
{
    int r = A->repeated_cols.load();
    if(r >= 0)
        return r != 0;
    const HostCsr &h = A->user;
    r                = 0;
    try
    {
        std::vector<aoclsparse_int> seen((size_t)h.n, -1);
        for(aoclsparse_int i = 0; i < h.m && !r; i++)
            for(aoclsparse_int p = h.ptr[i] - h.base; p < h.ptr[i + 1] - h.base; p++)
            {
                aoclsparse_int &s = seen[(size_t)(h.ind[p] - h.base)];
                if(s == i)
                {
                    r = 1;
                    break;
                }
                s = i;
            }
    }
    catch(const std::bad_alloc &)
    {
        return true; // the serial walk is right for every handle
    }
    A->repeated_cols.store(r);
    return r != 0;
}

template <typename T>
aoclsparse_status syrkd_t(aoclsparse_operation op, const aoclsparse_matrix A, T alpha, T beta, T *C, aoclsparse_order layout,
                          aoclsparse_int ldc, aoclsparse_matrix_data_type vt)
{
    if(!A || !C) // syrkd.hpp:179
        return aoclsparse_status_invalid_pointer;
    if(!valid_op(op)) // :182
        return aoclsparse_status_invalid_value;
    if(!valid_order(layout)) // :186
        return aoclsparse_status_invalid_value;
    if(A->input_format != aoclsparse_csr_mat) // :189 (TCSR, BSR, COO handles)
        return aoclsparse_status_not_implemented;
    if(A->val_type != vt) // :192
        return aoclsparse_status_wrong_type;
    if(is_cplx_v<T> && op == aoclsparse_operation_transpose) // :197 (the caller's op, whatever the format)
        return aoclsparse_status_not_implemented;
    if(!A->user.ptr) // :203
        return aoclsparse_status_not_implemented;
    // :229-240: the reference transposes on the fly, and needs fully sorted rows for it, when ITS effective op is not
    // none: op = T / H on a CSR handle, op = none on a handle made from CSC (whose own arrays csc_sort describes)
    const bool none     = op == aoclsparse_operation_none;
    const bool from_csc = A->csc_ptr != nullptr;
    if(from_csc ? (none && A->csc_sort != SORT_FULL) : (!none && A->sort != SORT_FULL))
        return aoclsparse_status_unsorted_input;
    const aoclsparse_int m_c = none ? A->m : A->n; // :252
    if(ldc < m_c) // :253
        return aoclsparse_status_invalid_value;
    if((long long)m_c * (long long)ldc > 2147483647LL) // :260
        return aoclsparse_status_invalid_size;
    if(m_c == 0)
        return aoclsparse_status_success;

    CallScope  cs(CallScope::Conditional);
    const bool rowmaj = layout == aoclsparse_order_row;
    T *const   dC     = cs.inout(STAGE_DENSE_C, C, sizeof(T) * (size_t)m_c * (size_t)ldc, true); // the whole m_c x ldc block
    if(!cs.ok())
        return cs.st;
    aoclsparse_status st = aoclsparse_status_success;
    // :265-313: the upper triangle is scaled before the quick return (beta == 1 leaves every value as it is)
    if(!eq(beta, 1.0))
    {
        st = launch_sy_scale_upper<T>(cs.s, dC, m_c, ldc, rowmaj, beta, eq(beta, 0.0));
        if(st != aoclsparse_status_success)
            return st;
    }
    if(A->m != 0 && A->n != 0 && A->nnz != 0) // :315
    {
        DeviceCsr *du = nullptr, *dt = nullptr;
        SpmvPlan  *pu = nullptr, *pt = nullptr;
        st = ensure_spmv(const_cast<aoclsparse_matrix>(A), false, du, pu);
        if(st == aoclsparse_status_success)
            st = ensure_spmv(const_cast<aoclsparse_matrix>(A), true, dt, pt);
        if(st != aoclsparse_status_success)
            return st;
        // op = none (:366-375, CONJLEFT = false): M = A^T, so X = A and W = A^T, the right factor conjugated;
        // op = T / H (:393-402, CONJLEFT = true): M = A, X = A^T, W = A, the left factor conjugated
        const DeviceCsr *x = none ? du : dt, *w = none ? dt : du;
        int              flags = 0;
        if(repeats_columns(const_cast<aoclsparse_matrix>(A)))
            flags |= SY_SERIAL;
        if(none && A->sort != SORT_FULL)
            flags |= SY_ORDERED;
        std::shared_lock<std::shared_mutex> ra(A->guard);
        st = launch_syrkd<T>(cs.s, m_c, x->base, x->ptr.as<aoclsparse_int>(), x->ind.as<aoclsparse_int>(),
                             x->val.as<T>(), is_cplx_v<T> && !none, w->base, w->ptr.as<aoclsparse_int>(),
                             w->ind.as<aoclsparse_int>(), w->val.as<T>(), is_cplx_v<T> && none, alpha, dC,
                             rowmaj ? (long long)ldc : 1LL, rowmaj ? 1LL : (long long)ldc, flags);
        if(st != aoclsparse_status_success)
            return st;
    }
    return cs.finish();
}

template <typename T>
aoclsparse_status syprd_t(aoclsparse_operation op, const aoclsparse_matrix A, const T *B, aoclsparse_order orderB,
                          aoclsparse_int ldb, T alpha, T beta, T *C, aoclsparse_order orderC, aoclsparse_int ldc,
                          aoclsparse_matrix_data_type vt)
{
    if(!A || !B || !C) // syprd.cpp:55, syprd.hpp:279
        return aoclsparse_status_invalid_pointer;
    if(A->val_type != vt) // syprd.cpp:60
        return aoclsparse_status_wrong_type;
    if(!valid_op(op)) // syprd.hpp:282
        return aoclsparse_status_invalid_value;
    if(!valid_order(orderB) || !valid_order(orderC)) // :286-290
        return aoclsparse_status_invalid_value;
    if(orderB != orderC) // :292
        return aoclsparse_status_invalid_operation;
    if(!has_csr(A)) // :302-304 (TCSR, BSR, COO handles)
        return aoclsparse_status_invalid_pointer;
    if(is_cplx_v<T> && op == aoclsparse_operation_transpose) // :319
        return aoclsparse_status_not_implemented;
    const aoclsparse_int m = A->m, k = A->n;
    if(m == 0) // :357
        return aoclsparse_status_success;
    if(A->nnz != 0 && (!A->user.ind || !A->user.val)) // :363
        return aoclsparse_status_invalid_pointer;
    if(eq(alpha, 0.0) && eq(beta, 1.0)) // :368
        return aoclsparse_status_success;
    // :373-402: the leading dimensions are checked against the caller's op
    const bool           none = op == aoclsparse_operation_none;
    const aoclsparse_int n_in = none ? k : m, m_c = none ? m : k;
    if(ldb < std::max<aoclsparse_int>(1, n_in))
        return aoclsparse_status_invalid_size;
    if(ldc < std::max<aoclsparse_int>(1, m_c))
        return aoclsparse_status_invalid_size;
    if((long long)m_c * (long long)ldc > 2147483647LL || (long long)n_in * (long long)ldb > 2147483647LL)
        return aoclsparse_status_invalid_size;
    if(m_c == 0)
        return aoclsparse_status_success;

    CallScope  cs(CallScope::Always); // (always: the scratch is a staging slot)
    const bool rowmaj = orderC == aoclsparse_order_row;
    T *const   dC     = cs.inout(STAGE_DENSE_C, C, sizeof(T) * (size_t)m_c * (size_t)ldc, true);
    if(!cs.ok())
        return cs.st;
    aoclsparse_status st = aoclsparse_status_success;
    if(eq(alpha, 0.0) || A->nnz == 0 || n_in == 0)
    {
        // :93-96 / :204-207: only the upper triangle is scaled (no entry: every chain is empty)
        st = launch_sy_scale_upper<T>(cs.s, dC, m_c, ldc, rowmaj, beta, eq(beta, 0.0));
        if(st != aoclsparse_status_success)
            return st;
        return cs.finish();
    }
    const T *dB = cs.in(STAGE_SYPRD_B, B, sizeof(T) * (size_t)n_in * (size_t)ldb);
    if(!cs.ok())
        return cs.st;
    T *scratch = static_cast<T *>(cs.scratch(STAGE_SYPRD_SCRATCH, sizeof(T) * (size_t)m_c * (size_t)n_in));
    if(!cs.ok())
        return aoclsparse_status_memory_error; // :101-109
    // :415-575: op = none runs on the CSR, op = T / H on its stable transpose; CONJLEFT (complex, op = H) conjugates the
    // left factor, otherwise the right one is conjugated
    DeviceCsr *dm = nullptr;
    SpmvPlan  *pm = nullptr;
    st = ensure_spmv(const_cast<aoclsparse_matrix>(A), !none, dm, pm);
    if(st != aoclsparse_status_success)
        return st;
    const bool conjleft = is_cplx_v<T> && op == aoclsparse_operation_conjugate_transpose;
    {
        std::shared_lock<std::shared_mutex> ra(A->guard);
        st = launch_syprd<T>(cs.s, m_c, n_in, dm->base, dm->ptr.as<aoclsparse_int>(), dm->ind.as<aoclsparse_int>(),
                             dm->val.as<T>(), conjleft, is_cplx_v<T> && !conjleft, alpha, dB, ldb, rowmaj,
                             scratch, beta, eq(beta, 0.0) ? 0 : eq(beta, 1.0) ? 1 : 2, dC,
                             rowmaj ? (long long)ldc : 1LL, rowmaj ? 1LL : (long long)ldc);
    }
    if(st != aoclsparse_status_success)
        return st;
    return cs.finish();
}

inline cfloat  cv(aoclsparse_float_complex v) { return cfloat(v.real, v.imag); }
inline cdouble cv(aoclsparse_double_complex v) { return cdouble(v.real, v.imag); }

} // namespace

extern "C" {

#define MI355_SY_DENSE_REAL(P, T, VT)                                                                                    \
    aoclsparse_status aoclsparse_##P##syrkd(const aoclsparse_operation op, const aoclsparse_matrix A, T alpha, T beta,   \
                                            T *C, const aoclsparse_order layout, aoclsparse_int ldc)                     \
    {                                                                                                                    \
        return syrkd_t<T>(op, A, alpha, beta, C, layout, ldc, VT);                                                       \
    }                                                                                                                    \
    aoclsparse_status aoclsparse_##P##syprd(const aoclsparse_operation op, const aoclsparse_matrix A, const T *B,        \
                                            const aoclsparse_order orderB, const aoclsparse_int ldb, const T alpha,      \
                                            const T beta, T *C, const aoclsparse_order orderC, const aoclsparse_int ldc) \
    {                                                                                                                    \
        return syprd_t<T>(op, A, B, orderB, ldb, alpha, beta, C, orderC, ldc, VT);                                       \
    }
MI355_SY_DENSE_REAL(d, double, aoclsparse_dmat)
MI355_SY_DENSE_REAL(s, float, aoclsparse_smat)

// syrkd.cpp:88-89, :109-110: the complex wrappers keep only the real part of alpha and beta; syprd.cpp:125-126, :161-162
// hand both on whole
#define MI355_SY_DENSE_CPLX(P, CT, T, R, VT)                                                                             \
    aoclsparse_status aoclsparse_##P##syrkd(const aoclsparse_operation op, const aoclsparse_matrix A, CT alpha, CT beta, \
                                            CT *C, const aoclsparse_order layout, aoclsparse_int ldc)                    \
    {                                                                                                                    \
        return syrkd_t<T>(op, A, T(alpha.real, R(0)), T(beta.real, R(0)), reinterpret_cast<T *>(C), layout, ldc, VT);    \
    }                                                                                                                    \
    aoclsparse_status aoclsparse_##P##syprd(const aoclsparse_operation op, const aoclsparse_matrix A, const CT *B,       \
                                            const aoclsparse_order orderB, const aoclsparse_int ldb, const CT alpha,     \
                                            const CT beta, CT *C, const aoclsparse_order orderC,                         \
                                            const aoclsparse_int ldc)                                                    \
    {                                                                                                                    \
        return syprd_t<T>(op, A, reinterpret_cast<const T *>(B), orderB, ldb, cv(alpha), cv(beta),                       \
                          reinterpret_cast<T *>(C), orderC, ldc, VT);                                                    \
    }
MI355_SY_DENSE_CPLX(z, aoclsparse_double_complex, cdouble, double, aoclsparse_zmat)
MI355_SY_DENSE_CPLX(c, aoclsparse_float_complex, cfloat, float, aoclsparse_cmat)

} // extern "C"
