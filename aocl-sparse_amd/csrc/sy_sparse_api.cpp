// sy_sparse_api.cpp -- aoclsparse_syrk (C = the upper triangle of A*A^H or A^H*A) and aoclsparse_sypr (C = the upper triangle
// of op(A)*B*op(A)^H, B symmetric / Hermitian and given by one triangle): the symmetric products whose result is a new
// sparse matrix.
//
// Drivers follow the reference's argument checks in order: level3/aoclsparse_syrk.cpp:38-58 and
// level3/aoclsparse_syrk.hpp:118-342, level3/aoclsparse_sypr.cpp:26-47 and level3/aoclsparse_sypr.hpp:529-1061.  Every
// check comes before the first touch of the GPU.
//
// The reference builds both from two ingredients (sypr.hpp:51-109, :400-527): rows of C are assembled in first-touch
// order with the summation chain of csr2m, and the left operand is a transpose that is never formed -- a linked-list
// walk (oftrans, :120-243) visits, for i ascending, the rows that hold column i, in an order that is NOT ascending.
// Here the walk runs on the host and is written down as an explicit CSR ("A^T in walk order"); with that as the left
// operand the product is the first-touch SpGEMM of sp2m (SpgProduct, spgemm_hash_kernel), restricted to the columns >= i
// of row i by its UPPER flag.  Stage 1 of sypr, T = sym(B)*A (:253-398), is the unrestricted product with "the stored
// triangle of B's row, then the other half in walk order" as its left operand; T stays in HBM.  syrk's dense-row path
// (syrk.hpp:221) is a kernel of its own (aat_dense_row_kernel).
//
// A handle created from CSC keeps the caller's CSC arrays, which are the CSR of A^T: exactly what the reference stores
// (auxiliary.cpp:1057-1066, doid::gt), so the flip of the operation and the move of the conjugation (syrk.hpp:156-173,
// sypr.hpp:591-625) are restated as they stand, on those arrays.
//
// Rows that repeat a column: the reference's walk pushes such a row back onto the list it is walking and loses the rest
// of the row, and its dense row keeps the last repeat only.  Neither is reproduced: every stored entry is its own
// element and the complete product is returned (walk_order, searchable).  Such inputs are outside the parity contract.
#include "spg_host.hpp"

#include <algorithm>
#include <cstring>
#include <numeric>
#include <type_traits>
#include <vector>

using namespace mi355;

namespace
{

template <typename T>
constexpr bool is_cplx_v = !std::is_floating_point<T>::value;

constexpr int SORT_FULL = 1; // _aoclsparse_matrix::sort of fully sorted rows (matrix.cpp: mat_check)

bool valid_op(aoclsparse_operation o)
{
    return o == aoclsparse_operation_none || o == aoclsparse_operation_transpose
           || o == aoclsparse_operation_conjugate_transpose;
}

template <typename T>
T conj_of(T v)
{
    if constexpr(is_cplx_v<T>)
        return T(v.re, -v.im);
    else
        return v;
}

// the CSR the reference holds for the handle (auxiliary.cpp:1057-1066): the caller's arrays; for a handle made from CSC
// they describe A^T (n x m)
template <typename T>
void stored_of(const aoclsparse_matrix A, HostCsrOp<T> &s)
{
    const bool csc = A->csc_ptr != nullptr;
    s.m = csc ? A->n : A->m, s.n = csc ? A->m : A->n, s.nnz = A->nnz, s.base = A->base;
    s.ptr = csc ? A->csc_ptr : A->user.ptr, s.ind = csc ? A->csc_ind : A->user.ind;
    s.val = static_cast<const T *>(csc ? A->csc_val : A->user.val);
}

// oftrans (sypr.hpp:120-243) run to its end.  Of every row r of an m x k CSR with sorted rows the entries at the 0-based
// positions [first(r), last(r)) take part.  Rows are pushed, r ascending, onto the stack of their first column; then for
// i = 0 .. k - 1 the stack of column i is walked from the top, and every visited row moves to the stack of its next
// entry's column at the moment it is visited (:223-242).  Output: wptr (k + 1), and per visit the row and the position
// of the entry.  A row that repeats a column is visited once per stored entry (the reference would drop its tail).
template <typename First, typename Last>
void walk_order(aoclsparse_int m, aoclsparse_int k, First first, Last last, const aoclsparse_int *ind, aoclsparse_int base,
                std::vector<aoclsparse_int> &wptr, std::vector<aoclsparse_int> &wrow, std::vector<aoclsparse_int> &wpos)
{
    std::vector<aoclsparse_int> cur((size_t)m), head((size_t)k, -1), next((size_t)m, -1);
    for(aoclsparse_int r = 0; r < m; r++)
    {
        cur[r] = first(r);
        if(cur[r] < last(r))
        {
            const aoclsparse_int j = ind[cur[r]] - base;
            next[r] = head[j], head[j] = r;
        }
    }
    wptr.assign((size_t)k + 1, 0);
    wrow.clear(), wpos.clear();
    for(aoclsparse_int i = 0; i < k; i++)
    {
        for(aoclsparse_int row = head[i]; row >= 0;)
        {
            const aoclsparse_int after = next[row], e = last(row);
            do
            {
                wrow.push_back(row), wpos.push_back(cur[row]);
                cur[row]++;
            } while(cur[row] < e && ind[cur[row]] - base == i);
            if(cur[row] < e)
            {
                const aoclsparse_int j = ind[cur[row]] - base;
                next[row] = head[j], head[j] = row;
            }
            row = after;
        }
        wptr[(size_t)i + 1] = (aoclsparse_int)wrow.size();
    }
}

// "L^T in walk order": the left operand of sp2m_online_atb (sypr.hpp:470-496) as a 0-based k x m CSR
template <typename T>
void walked_transpose(const HostCsrOp<T> &l, HostCsrOp<T> &w)
{
    const aoclsparse_int        b = l.base;
    std::vector<aoclsparse_int> pos;
    walk_order(
        l.m, l.n, [&](aoclsparse_int r) { return l.ptr[r] - b; }, [&](aoclsparse_int r) { return l.ptr[r + 1] - b; }, l.ind, b,
        w.optr, w.oind, pos);
    w.m = l.n, w.n = l.m, w.nnz = (aoclsparse_int)pos.size(), w.base = 0;
    w.oval.resize(std::max<size_t>(pos.size(), 1));
    for(size_t q = 0; q < pos.size(); q++)
        w.oval[q] = l.val[pos[q]];
    w.oind.resize(std::max<size_t>(pos.size(), 1));
    w.own();
}

// the left operand of sp2m_online_symab (sypr.hpp:301-378) as a 0-based m x m CSR: row i = the stored triangle's part of
// row i of B, diagonal included, then the other half from the walk over the strict triangle, conjugated
template <typename T>
void symmetrised(const HostCsr &o, bool lower, HostCsrOp<T> &sb)
{
    const aoclsparse_int m = o.m, b = o.base;
    const T             *v = static_cast<const T *>(o.val);
    auto s_first = [&](aoclsparse_int i) { return lower ? o.ptr[i] - b : o.idiag[i] - b; }; // :303-322 (normal)
    auto s_last  = [&](aoclsparse_int i) { return lower ? o.idiag[i] + 1 - b : o.ptr[i + 1] - b; };
    auto t_first = [&](aoclsparse_int i) { return lower ? o.ptr[i] - b : o.idiag[i] + 1 - b; }; // (for transpose)
    auto t_last  = [&](aoclsparse_int i) { return lower ? o.idiag[i] - b : o.ptr[i + 1] - b; };
    std::vector<aoclsparse_int> wptr, wrow, wpos;
    walk_order(m, m, t_first, t_last, o.ind, b, wptr, wrow, wpos);
    sb.m = sb.n = m, sb.base = 0;
    sb.optr.assign((size_t)m + 1, 0);
    sb.oind.clear(), sb.oval.clear();
    for(aoclsparse_int i = 0; i < m; i++)
    {
        for(aoclsparse_int p = s_first(i); p < s_last(i); p++)
            sb.oind.push_back(o.ind[p] - b), sb.oval.push_back(v[p]);
        for(aoclsparse_int q = wptr[i]; q < wptr[i + 1]; q++)
            sb.oind.push_back(wrow[q]), sb.oval.push_back(conj_of(v[wpos[q]])); // :361-362
        sb.optr[(size_t)i + 1] = (aoclsparse_int)sb.oind.size();
    }
    sb.nnz = (aoclsparse_int)sb.oind.size();
    if(sb.oind.empty())
        sb.oind.push_back(0), sb.oval.push_back(T(0));
    sb.own();
}

// A with every row sorted by column, 0-based, one entry per column: what a search needs to answer "trow[col]" of
// syrk.hpp:92-93.  A row that repeats a column gets the SUM of the repeats (in stored order), so that, like the walk of
// the other path, the dense-row path returns the complete product for such a row; the reference's dense row would keep
// the last repeat only, which is the product of nothing.  Without repeats -- the inputs of the parity contract -- the
// two are the same.
template <typename T>
void searchable(const HostCsrOp<T> &a, HostCsrOp<T> &s)
{
    const aoclsparse_int b = a.base;
    s.m = a.m, s.n = a.n, s.base = 0;
    s.optr.assign((size_t)a.m + 1, 0);
    s.oind.clear(), s.oval.clear();
    std::vector<aoclsparse_int> perm;
    for(aoclsparse_int i = 0; i < a.m; i++)
    {
        const aoclsparse_int p0 = a.ptr[i] - b, len = a.ptr[i + 1] - b - p0;
        perm.resize((size_t)len);
        std::iota(perm.begin(), perm.end(), p0);
        std::stable_sort(perm.begin(), perm.end(), [&](aoclsparse_int u, aoclsparse_int w) { return a.ind[u] < a.ind[w]; });
        for(aoclsparse_int q = 0; q < len; q++)
        {
            if(q > 0 && a.ind[perm[q]] == a.ind[perm[q - 1]])
            {
                T &sum = s.oval.back();
                if constexpr(is_cplx_v<T>)
                    sum = T(sum.re + a.val[perm[q]].re, sum.im + a.val[perm[q]].im);
                else
                    sum += a.val[perm[q]];
                continue;
            }
            s.oind.push_back(a.ind[perm[q]] - b), s.oval.push_back(a.val[perm[q]]);
        }
        s.optr[(size_t)i + 1] = (aoclsparse_int)s.oind.size();
    }
    s.nnz = (aoclsparse_int)s.oind.size();
    if(s.oind.empty())
        s.oind.push_back(0), s.oval.push_back(T(0));
    s.own();
}

// The count pass, the fill pass or both of `prod` (an m_c x m_c upper triangle), into a handle in index base `base`, through
// SPG_SLOT_CP / CI / CV.  count: creates *C with its row pointer and allocated ind / val.  fill without count: fills the *C it is
// given, whose row pointer is checked against this product on the device before anything of *C is written.
template <typename T>
aoclsparse_status product_to_handle(SpgProduct<T> &prod, bool count, bool fill, aoclsparse_matrix *C,
                                    aoclsparse_matrix_data_type vt, aoclsparse_index_base base)
{
    Runtime             &rt = prod.rt;
    const aoclsparse_int m  = prod.m;
    void                *pp = nullptr, *pi = nullptr, *pv = nullptr;
    aoclsparse_status    st = rt.staging(SPG_SLOT_CP, sizeof(aoclsparse_int) * ((size_t)m + 1), &pp);
    if(st != aoclsparse_status_success)
        return st;
    aoclsparse_int *d_ptr = static_cast<aoclsparse_int *>(pp);
    if(count)
    {
        long long                  *d_total = nullptr;
        aoclsparse_int              total   = 0;
        std::vector<aoclsparse_int> cptr;
        st = prod.count(d_ptr, &d_total);
        if(st == aoclsparse_status_success)
            st = spg_count_to_host(rt, d_total, d_ptr, m, base, &cptr, total); // sypr.hpp:391-396, :512-525
        if(st == aoclsparse_status_success)
            st = new_csr_result(C, m, m, total, vt, cptr.data(), base);
        if(st != aoclsparse_status_success)
            return st;
    }
    if(!fill)
        return aoclsparse_status_success;
    _aoclsparse_matrix  *c     = *C;
    const aoclsparse_int nnz_c = c->user.ptr[m] - base;
    const size_t         nz    = (size_t)std::max<aoclsparse_int>(nnz_c, 1);
    st                         = rt.staging(SPG_SLOT_CI, sizeof(aoclsparse_int) * nz, &pi);
    if(st == aoclsparse_status_success)
        st = rt.staging(SPG_SLOT_CV, sizeof(T) * nz, &pv);
    if(st == aoclsparse_status_success) // (finalize: whatever the handle derived from an earlier fill mirrors the old values)
        st = spg_fill_to_host<T>(prod, !count, d_ptr, static_cast<aoclsparse_int *>(pi), static_cast<T *>(pv), c->user, [c, count] {
            if(!count)
                (void)aoclsparse_mi355_invalidate(c);
        });
    if(st == aoclsparse_status_success && base)
        for(aoclsparse_int p = 0; p < nnz_c; p++)
            c->user.ind[p] += base;
    return st;
}

// syrk's dense-row path (syrk.hpp:46-113) for a short, wide CSR S = A: count, scan, fill with aat_dense_row_kernel
template <typename T>
aoclsparse_status syrk_dense_rows(Runtime &rt, const aoclsparse_matrix A, const HostCsrOp<T> &S, aoclsparse_matrix *C,
                                  aoclsparse_matrix_data_type vt)
{
    hipStream_t                 s = rt.stream();
    const aoclsparse_int        m = S.m;
    const aoclsparse_index_base base = A->base;
    HostCsrOp<T>                Q;
    searchable(S, Q);
    SpgDevOp          da, dq;
    aoclsparse_status st = spg_to_device(rt, A, S, SPG_SLOT_YP, true, da);
    if(st == aoclsparse_status_success)
        st = spg_send(rt, Q, SPG_SLOT_XP, true, dq);
    void *p_cnt = nullptr, *p_scan = nullptr, *pp = nullptr, *pi = nullptr, *pv = nullptr;
    if(st == aoclsparse_status_success)
        st = rt.staging(SPG_SLOT_CNT, sizeof(int) * (size_t)m, &p_cnt);
    if(st == aoclsparse_status_success)
        st = rt.staging(SPG_SLOT_SCAN, spg_scan_scratch_bytes(m), &p_scan);
    if(st == aoclsparse_status_success)
        st = rt.staging(SPG_SLOT_CP, sizeof(aoclsparse_int) * ((size_t)m + 1), &pp);
    if(st != aoclsparse_status_success)
        return st;
    std::shared_lock<std::shared_mutex> ra(A->guard);
    aoclsparse_int                     *d_ptr = static_cast<aoclsparse_int *>(pp);
    const T *av = static_cast<const T *>(da.val), *qv = static_cast<const T *>(dq.val);
    st = launch_aat_dense_row<T>(s, false, m, da.base, da.ptr, da.ind, av, dq.ptr, dq.ind, qv, nullptr, static_cast<int *>(p_cnt), base,
                                 nullptr, nullptr);
    long long                  *d_total = nullptr;
    aoclsparse_int              nnz_c   = 0; // (at most m (m + 1) / 2 < 2^23)
    std::vector<aoclsparse_int> cptr;
    if(st == aoclsparse_status_success)
        st = launch_spg_scan(s, m, static_cast<const int *>(p_cnt), d_ptr, static_cast<long long *>(p_scan), &d_total);
    if(st == aoclsparse_status_success)
        st = spg_count_to_host(rt, d_total, d_ptr, m, base, &cptr, nnz_c); // :89, :108
    if(st == aoclsparse_status_success)
        st = new_csr_result(C, m, m, nnz_c, vt, cptr.data(), base);
    if(st != aoclsparse_status_success)
        return st;
    const size_t nz = (size_t)std::max<aoclsparse_int>(nnz_c, 1);
    st              = rt.staging(SPG_SLOT_CI, sizeof(aoclsparse_int) * nz, &pi);
    if(st == aoclsparse_status_success)
        st = rt.staging(SPG_SLOT_CV, sizeof(T) * nz, &pv);
    if(st == aoclsparse_status_success)
        st = launch_aat_dense_row<T>(s, true, m, da.base, da.ptr, da.ind, av, dq.ptr, dq.ind, qv, d_ptr, nullptr, base,
                                     static_cast<aoclsparse_int *>(pi), static_cast<T *>(pv));
    if(st == aoclsparse_status_success)
        st = rt.d2h((*C)->user.ind, pi, sizeof(aoclsparse_int) * (size_t)nnz_c);
    if(st == aoclsparse_status_success)
        st = rt.d2h((*C)->user.val, pv, sizeof(T) * (size_t)nnz_c);
    if(st == aoclsparse_status_success)
        st = map_hip_error(hipStreamSynchronize(s));
    return st;
}

void drop(aoclsparse_matrix *C)
{
    if(*C)
        (void)aoclsparse_destroy(C);
    *C = nullptr;
}

// ---- syrk ---------------------------------------------------------------------------------------------------------------
template <typename T>
aoclsparse_status syrk_t(aoclsparse_operation op, const aoclsparse_matrix A, aoclsparse_matrix *C,
                         aoclsparse_matrix_data_type vt)
{
    if(!A || !C) // syrk.hpp:124
        return aoclsparse_status_invalid_pointer;
    *C = nullptr; // :127
    if(!valid_op(op)) // :129
        return aoclsparse_status_invalid_value;
    if(A->input_format != aoclsparse_csr_mat) // :133 (TCSR, BSR, COO handles)
        return aoclsparse_status_not_implemented;
    if(A->val_type != vt) // :136
        return aoclsparse_status_wrong_type;
    if(is_cplx_v<T> && op == aoclsparse_operation_transpose) // :140
        return aoclsparse_status_not_implemented;
    if(!A->user.ptr) // :146-148
        return aoclsparse_status_not_implemented;
    // :150-173: the stored CSR is A (CSR handle) or A^T (CSC handle: the operation flips, the conjugation moves)
    const bool csc = A->csc_ptr != nullptr;
    HostCsrOp<T>  S;
    stored_of<T>(A, S);
    const bool eff_none = csc ? op != aoclsparse_operation_none : op == aoclsparse_operation_none;
    if(!eff_none && (csc ? A->csc_sort : A->sort) != SORT_FULL) // :175
        return aoclsparse_status_unsorted_input;
    const aoclsparse_int        m = S.m, n = S.n, m_c = eff_none ? m : n; // :187
    const aoclsparse_index_base base = A->base;
    if(A->m == 0 || A->n == 0 || A->nnz == 0) // :206-214
        return new_csr_result(C, m_c, m_c, 0, vt, nullptr, base);

    CallScope cs(CallScope::Always); // the SPG_SLOT_* slots are shared
    if(!cs.ok())
        return cs.st;
    Runtime          &rt = cs.rt;
    aoclsparse_status st = aoclsparse_status_success;
    try
    {
        if(eff_none && !csc && m < 3000 && m < n && (long long)A->nnz <= 10LL * m) // :221
        {
            st = syrk_dense_rows(rt, A, S, C, vt);
            if(st != aoclsparse_status_success)
                drop(C); // :333-337
            return st;
        }
        // ---- online A^T * B path (sypr.hpp:400-527, BUILD_ONLY_U): L = the stored CSR (:286-331) or its csr2csc transpose
        // (:228-283); the left operand is L^T in walk order, the right one L itself
        HostCsrOp<T> Lt, W;
        if(eff_none)
            transpose_of(S, Lt);
        const HostCsrOp<T> &L = eff_none ? Lt : S;
        walked_transpose(L, W);
        SpgProduct<T> prod(rt);
        prod.m = m_c, prod.n = m_c, prod.upper = true;
        // which factor is conjugated: :263-265 with CONJ_A = true (:267); :288-289
        prod.conj_x = is_cplx_v<T> && (eff_none ? csc : !csc);
        prod.conj_y = is_cplx_v<T> && (eff_none ? !csc : csc);
        st = spg_send(rt, W, SPG_SLOT_XP, true, prod.x);
        if(st == aoclsparse_status_success)
            st = spg_to_device(rt, A, L, SPG_SLOT_YP, true, prod.y); // (resident when L is the handle's own CSR)
        if(st != aoclsparse_status_success)
            return st;
        std::shared_lock<std::shared_mutex> ra(A->guard);
        st = prod.analyse();
        if(st == aoclsparse_status_success)
            st = product_to_handle(prod, true, true, C, vt, base);
        if(st != aoclsparse_status_success)
            drop(C); // :333-337
        return st;
    }
    catch(const std::bad_alloc &)
    {
        drop(C);
        return aoclsparse_status_memory_error;
    }
}

// ---- the two products of sypr, after every check: stage 1 T = sym(B) * L, stage 2 C = the upper triangle of L^H * T ----
template <typename T>
aoclsparse_status sypr_stages(Runtime &rt, const aoclsparse_matrix A, const aoclsparse_matrix B, bool lower, bool csc, bool eff_none,
                              bool conj_flip, bool count, bool fill, aoclsparse_matrix *C, aoclsparse_matrix_data_type vt)
{
    const aoclsparse_int m = B->m;
    aoclsparse_status    st;
    // L: the stored CSR (:737-743) or its csr2csc transpose (:750-786); both stages read it, m x n
    HostCsrOp<T> S, Lt, SB, W;
    stored_of<T>(A, S);
    if(eff_none)
        transpose_of(S, Lt);
    const HostCsrOp<T> &L = eff_none ? Lt : S;
    const aoclsparse_int n = L.n; // C is n x n
    {
        std::shared_lock<std::shared_mutex> rb(B->guard);
        symmetrised<T>(*B->opt, lower, SB); // :800
    }
    // ---- stage 1, T = sym(B) * L (:822-921), every request: count, scan, fill; T stays in HBM ----
    SpgProduct<T> one(rt);
    one.m = m, one.n = n;
    // :780-785 (CSR, op = none: the transpose is conjugated before both stages), :824 (CONJ_B = conj_flip)
    one.conj_y = is_cplx_v<T> && (eff_none ? !csc : conj_flip);
    st = spg_send(rt, SB, SPG_SLOT_XP, true, one.x);
    if(st == aoclsparse_status_success)
        st = spg_to_device(rt, A, L, SPG_SLOT_YP, true, one.y); // (resident when L is the handle's own CSR)
    if(st != aoclsparse_status_success)
        return st;
    std::shared_lock<std::shared_mutex> ra(A->guard);
    void                               *tp = nullptr, *ti = nullptr, *tv = nullptr;
    long long                          *d_total = nullptr;
    aoclsparse_int                      nnz_t   = 0;
    st = one.analyse();
    if(st == aoclsparse_status_success)
        st = rt.staging(SPG_SLOT_TP, sizeof(aoclsparse_int) * ((size_t)m + 1), &tp);
    if(st == aoclsparse_status_success)
        st = one.count(static_cast<aoclsparse_int *>(tp), &d_total);
    if(st == aoclsparse_status_success) // :391-396 (the total alone: T's row pointer stays in HBM)
        st = spg_count_to_host(rt, d_total, nullptr, m, aoclsparse_index_base_zero, nullptr, nnz_t);
    if(st != aoclsparse_status_success)
        return st;
    const size_t tz = (size_t)std::max<aoclsparse_int>(nnz_t, 1);
    st              = rt.staging(SPG_SLOT_TI, sizeof(aoclsparse_int) * tz, &ti);
    if(st == aoclsparse_status_success)
        st = rt.staging(SPG_SLOT_TV, sizeof(T) * tz, &tv);
    if(st == aoclsparse_status_success)
        st = one.fill(static_cast<const aoclsparse_int *>(tp), static_cast<aoclsparse_int *>(ti), static_cast<T *>(tv));
    if(st != aoclsparse_status_success)
        return st;
    // ---- stage 2, C = the upper triangle of L^H * T (:923-1058): the left operand is L^T in walk order ----
    walked_transpose(L, W);
    SpgProduct<T> two(rt);
    two.m = n, two.n = n, two.upper = true;
    // :945-985: CONJ_A = !conj_flip, on values that :780-785 may have conjugated already
    two.conj_x = is_cplx_v<T> && (eff_none ? csc : !conj_flip);
    two.y      = SpgDevOp{static_cast<const aoclsparse_int *>(tp), static_cast<const aoclsparse_int *>(ti), tv, 0};
    st         = spg_send(rt, W, SPG_SLOT_XP, true, two.x); // (stream order: stage 1 has read these slots by then)
    if(st == aoclsparse_status_success)
        st = two.analyse();
    if(st == aoclsparse_status_success)
        st = product_to_handle(two, count, fill, C, vt, aoclsparse_index_base_zero);
    return st;
}

// ---- sypr ---------------------------------------------------------------------------------------------------------------
template <typename T>
aoclsparse_status sypr_t(aoclsparse_operation op, const aoclsparse_matrix A, const aoclsparse_matrix B,
                         const aoclsparse_mat_descr descrB, aoclsparse_matrix *C, aoclsparse_request request,
                         aoclsparse_matrix_data_type vt)
{
    if(request != aoclsparse_stage_full_computation && request != aoclsparse_stage_nnz_count
       && request != aoclsparse_stage_finalize) // sypr.hpp:548
        return aoclsparse_status_invalid_value;
    if(!valid_op(op)) // :552
        return aoclsparse_status_invalid_value;
    if(!descrB) // :556
        return aoclsparse_status_invalid_pointer;
    if(request != aoclsparse_stage_finalize) // :563
        *C = nullptr;
    if(A->input_format != aoclsparse_csr_mat || B->input_format != aoclsparse_csr_mat) // :566 (TCSR, BSR, COO handles)
        return aoclsparse_status_not_implemented;
    if(!A->user.ptr) // :571-573
        return aoclsparse_status_invalid_pointer;
    const bool csc = A->csc_ptr != nullptr; // :574 (doid::gt)
    if(!B->user.ptr) // :578-580
        return aoclsparse_status_invalid_pointer;
    if(B->csc_ptr) // :581
        return aoclsparse_status_not_implemented;
    if(is_cplx_v<T> && op == aoclsparse_operation_transpose) // :587
        return aoclsparse_status_not_implemented;
    // :607-625: from CSC arrays the operation flips; complex + op = none moves the conjugation into the kernels
    const bool none      = op == aoclsparse_operation_none;
    const bool eff_none  = csc ? !none : none;
    const bool conj_flip = csc && none && is_cplx_v<T>;
    if(A->val_type != vt || B->val_type != vt) // :626-634
        return aoclsparse_status_wrong_type;
    if(B->base != descrB->base) // :636 (is_descr_matching, mat_structures.hpp:808-814)
        return aoclsparse_status_invalid_value;
    if(descrB->type != (is_cplx_v<T> ? aoclsparse_matrix_type_hermitian : aoclsparse_matrix_type_symmetric)) // :638-651
        return aoclsparse_status_invalid_value;
    if(descrB->diag_type != aoclsparse_diag_type_non_unit) // :652
        return aoclsparse_status_not_implemented;
    if(B->m != B->n) // :658
        return aoclsparse_status_invalid_size;
    const aoclsparse_int m = B->m, n = none ? A->m : A->n; // :662-676 (the caller's op and the caller's dimensions)
    if(m != (none ? A->n : A->m))
        return aoclsparse_status_invalid_size;
    // :688-691: finalize needs the C of an earlier count
    if(request == aoclsparse_stage_finalize
       && (!*C || !(*C)->user.ptr || !(*C)->user.ind || !(*C)->user.val || (*C)->m != n || (*C)->n != n))
        return aoclsparse_status_invalid_value;
    if(request == aoclsparse_stage_finalize && ((*C)->val_type != vt || !(*C)->owns_user_arrays || (*C)->base != 0))
        return aoclsparse_status_invalid_value; // (not a result of this function)
    if(m == 0 || n == 0 || A->nnz == 0 || B->nnz == 0) // :695-723
    {
        if(!*C)
            return new_csr_result(C, n, n, 0, vt, nullptr);
        return aoclsparse_status_success;
    }
    if(((csc ? A->csc_sort : A->sort) != SORT_FULL && !eff_none) || B->sort != SORT_FULL) // :727
        return aoclsparse_status_unsorted_input;
    // :788: the optimised copy of B (sorted, zeros on missing diagonals, idiag): the handle's clean CSR
    aoclsparse_status st = csr_optimize(B);
    if(st != aoclsparse_status_success)
        return st;
    if(!B->opt || !B->opt->idiag)
        return aoclsparse_status_internal_error; // :791

    CallScope cs(CallScope::Always); // the SPG_SLOT_* slots are shared
    if(!cs.ok())
        return cs.st;
    const bool count = request != aoclsparse_stage_finalize;
    try
    {
        st = sypr_stages<T>(cs.rt, A, B, descrB->fill_mode == aoclsparse_fill_mode_lower, csc, eff_none, conj_flip, count,
                            request != aoclsparse_stage_nnz_count, C, vt);
        if(st != aoclsparse_status_success && count)
            drop(C); // :986-990, :1052-1057
        return st;
    }
    catch(const std::bad_alloc &)
    {
        if(count)
            drop(C);
        return aoclsparse_status_memory_error;
    }
}

} // namespace

extern "C" {

aoclsparse_status aoclsparse_syrk(const aoclsparse_operation opA, const aoclsparse_matrix A, aoclsparse_matrix *C)
{
    // aoclsparse_syrk.cpp:38-58
    if(!A)
        return aoclsparse_status_invalid_pointer;
    switch(A->val_type)
    {
    case aoclsparse_smat: return syrk_t<float>(opA, A, C, aoclsparse_smat);
    case aoclsparse_dmat: return syrk_t<double>(opA, A, C, aoclsparse_dmat);
    case aoclsparse_cmat: return syrk_t<cfloat>(opA, A, C, aoclsparse_cmat);
    case aoclsparse_zmat: return syrk_t<cdouble>(opA, A, C, aoclsparse_zmat);
    default: return aoclsparse_status_wrong_type;
    }
}

aoclsparse_status aoclsparse_sypr(aoclsparse_operation opA, const aoclsparse_matrix A, const aoclsparse_matrix B,
                                  const aoclsparse_mat_descr descrB, aoclsparse_matrix *C, const aoclsparse_request request)
{
    // aoclsparse_sypr.cpp:26-47: both handles must hold the same one of the four types
    if(!A || !B || !C)
        return aoclsparse_status_invalid_pointer;
    if(A->val_type != B->val_type)
        return aoclsparse_status_wrong_type;
    switch(A->val_type)
    {
    case aoclsparse_smat: return sypr_t<float>(opA, A, B, descrB, C, request, aoclsparse_smat);
    case aoclsparse_dmat: return sypr_t<double>(opA, A, B, descrB, C, request, aoclsparse_dmat);
    case aoclsparse_cmat: return sypr_t<cfloat>(opA, A, B, descrB, C, request, aoclsparse_cmat);
    case aoclsparse_zmat: return sypr_t<cdouble>(opA, A, B, descrB, C, request, aoclsparse_zmat);
    default: return aoclsparse_status_wrong_type;
    }
}

} // extern "C"
