/*
 * oracle_tmpl.h -- the restatements that exist in both precisions, written once (TEST INFRASTRUCTURE ONLY, see oracle.h).
 * oracle.c includes this file twice: ORC_T double / ORC_S d, then ORC_T float / ORC_S s, with
 *   ORC_FMA       fma / fmaf                   (a contraction both compilers of the reference make)
 *   ORC_CH        CH_D / CH_S                  (a loop-carried scalar accumulation: see orc_set_contract)
 *   ORC_SQRT, ORC_FABS, ORC_COPYSIGN           the <math.h> function of the type
 *   ORC_EPS       DBL_EPSILON / FLT_EPSILON
 * Every expression is evaluated in ORC_T (constants are cast, nothing is promoted to double), so the float instantiation
 * is the reference's float template and the double one keeps the bits that tests/golden pins.
 * FN(x) is the exported orc_<d|s>x, LN(x) a file-local helper.
 */
#define ORC_CAT3_(a, b, c) a##b##c
#define ORC_CAT3(a, b, c) ORC_CAT3_(a, b, c)
#define FN(name) ORC_CAT3(orc_, ORC_S, name)
#define LN(name) ORC_CAT3(tmpl_, ORC_S, name)
#define T ORC_T
/* aoclsparse_is_nearzero, extra/aoclsparse_utils.hpp:598-613 */
#define ORC_TINY ((T)1e-2 * (T)2 * ORC_EPS)

/* ------------------------------------------------------------------------------------ */
/* Triangular SpMV reference kernels.  rev = 1 walks the same terms in the opposite      */
/* order (no reference kernel does: it measures how far two orders of one row can lie    */
/* apart, the bound of the kernels that are not pinned to an order).                     */
/* ------------------------------------------------------------------------------------ */
static void LN(scale_y)(T *y, oint n, T beta)
{
    if(beta == (T)0)
        for(oint i = 0; i < n; i++)
            y[i] = (T)0;
    else if(beta != (T)1)
        for(oint i = 0; i < n; i++)
            y[i] = beta * y[i];
}

/* csrmv_kr.hpp:658-728 (ref_csrmv_tri): rows [rs[i], re[i]) of the clean CSR, i.e. strict triangle
 * plus the stored diagonal; unit/zero diag drop the stored diagonal, unit adds x[i]. */
static int LN(csrmv_tri)(int base, T alpha, oint m, int diag, int fill, const T *val, const oint *col, const oint *ptr,
                         const oint *idiag, const oint *iurow, const T *x, T beta, T *y, int rev)
{
    LN(scale_y)(y, m, beta);
    for(oint i = 0; i < m; i++)
    {
        /* lower: [ptr[i], iurow[i]) ; upper: [idiag[i], ptr[i+1]) (csrmv.hpp:110-123) */
        oint rs = fill == 0 ? ptr[i] : idiag[i], re = fill == 0 ? iurow[i] : ptr[i + 1];
        int  so = 0, eo = 0;
        if(diag != 0)
        {
            if(fill == 0)
                eo = -1;
            else
                so = 1;
        }
        T r = (T)0;
        if(so && diag == 1)
            r += x[i];
        if(rev)
            for(oint j = re + eo - 1; j >= rs + so; j--)
                r = ORC_CH(val[j - base], x[col[j - base] - base], r);
        else
            for(oint j = rs + so; j < re + eo; j++)
                r = ORC_CH(val[j - base], x[col[j - base] - base], r);
        if(eo && diag == 1)
            r += x[i];
        y[i] = ORC_FMA(alpha, r, y[i]);
    }
    return ORC_SUCCESS;
}

/* csrmv_kr.hpp:577-649 (ref_csrmv_tri_th): transposed triangular SpMV, column sweep. */
static int LN(csrmv_tri_t)(int base, T alpha, oint m, oint n, int diag, int fill, const T *val, const oint *col,
                           const oint *ptr, const oint *idiag, const oint *iurow, const T *x, T beta, T *y, int rev)
{
    LN(scale_y)(y, n, beta);
    for(oint ii = 0; ii < m; ii++)
    {
        oint i  = rev ? m - 1 - ii : ii;
        oint rs = fill == 0 ? ptr[i] : idiag[i], re = fill == 0 ? iurow[i] : ptr[i + 1];
        int  so = 0, eo = 0;
        if(diag != 0)
        {
            if(fill == 0)
                eo = -1;
            else
                so = 1;
        }
        T axi = alpha * x[i];
        if(so && diag == 1)
            y[i] += axi;
        for(oint j = rs + so; j < re + eo; j++)
        {
            oint c = col[j - base] - base;
            y[c]   = ORC_FMA(val[j - base], axi, y[c]);
        }
        if(eo && diag == 1)
            y[i] += axi;
    }
    return ORC_SUCCESS;
}

int FN(csrmv_tri)(int base, T alpha, oint m, int diag, int fill, const T *val, const oint *col, const oint *ptr,
                  const oint *idiag, const oint *iurow, const T *x, T beta, T *y)
{
    return LN(csrmv_tri)(base, alpha, m, diag, fill, val, col, ptr, idiag, iurow, x, beta, y, 0);
}
int FN(csrmv_tri_t)(int base, T alpha, oint m, oint n, int diag, int fill, const T *val, const oint *col, const oint *ptr,
                    const oint *idiag, const oint *iurow, const T *x, T beta, T *y)
{
    return LN(csrmv_tri_t)(base, alpha, m, n, diag, fill, val, col, ptr, idiag, iurow, x, beta, y, 0);
}

/* ------------------------------------------------------------------------------------ */
/* Transposed TRSV reference kernels ("x[c] -= a*xi" contracts to fma(-a, xi, x[c])).    */
/* ------------------------------------------------------------------------------------ */
/* trsv_kr.hpp:101-120: x = alpha*b; for i = m-1..0: x[i] /= d; x[col] -= a*x[i]. */
int FN(trsv_lt)(T alpha, oint m, int base, const T *a, const oint *icol, const oint *ilrow, const oint *idiag, const T *b,
                oint incb, T *x, oint incx, int unit)
{
    for(oint i = 0; i < m; i++)
        x[(size_t)i * incx] = alpha * b[(size_t)i * incb];
    for(oint i = m - 1; i >= 0; i--)
    {
        if(!unit)
            x[(size_t)i * incx] /= a[idiag[i] - base];
        T xi = x[(size_t)i * incx];
        for(oint idx = ilrow[i]; idx < idiag[i]; idx++)
        {
            size_t c = (size_t)(icol[idx - base] - base) * incx;
            x[c]     = ORC_FMA(-a[idx - base], xi, x[c]);
        }
    }
    return ORC_SUCCESS;
}

/* trsv_kr.hpp:196-221: x = alpha*b; for i = 0..m-1: x[i] /= d; x[col] -= a*x[i]. */
int FN(trsv_ut)(T alpha, oint m, int base, const T *a, const oint *icol, const oint *ilrow, const oint *iurow, const T *b,
                oint incb, T *x, oint incx, int unit)
{
    for(oint i = 0; i < m; i++)
        x[(size_t)i * incx] = alpha * b[(size_t)i * incb];
    for(oint i = 0; i < m; i++)
    {
        if(!unit)
            x[(size_t)i * incx] /= a[iurow[i] - 1 - base];
        T xi = x[(size_t)i * incx];
        for(oint idx = iurow[i]; idx <= ilrow[i + 1] - 1; idx++)
        {
            size_t c = (size_t)(icol[idx - base] - base) * incx;
            x[c]     = ORC_FMA(-a[idx - base], xi, x[c]);
        }
    }
    return ORC_SUCCESS;
}

/* ------------------------------------------------------------------------------------ */
/* ILU(0), solvers/aoclsparse_ilu0.hpp:35-107: IKJ in place; lu_diag_ptr[i] = 0-based     */
/* position of the diagonal.  Restated with the reference's mapper convention (a stored  */
/* position of 0 means "absent", :83-86), so the entry at array position 0 is never      */
/* updated -- kept for fidelity.                                                         */
/* ------------------------------------------------------------------------------------ */
int FN(ilu0)(oint n, int base, oint *lu_diag_ptr, T *val, const oint *row_ptr, const oint *col_ind)
{
    oint *mapper = (oint *)calloc((size_t)(n > 0 ? n : 1), sizeof(oint));
    if(!mapper)
        return ORC_MEMORY_ERROR;
    for(oint i = 0; i < n; i++)
    {
        oint j1 = row_ptr[i] - base, j2 = row_ptr[i + 1] - base, j, k = -1;
        for(j = j1; j < j2; j++)
            mapper[col_ind[j] - base] = j;
        for(j = j1; j < j2; j++)
        {
            k = col_ind[j] - base;
            if(k >= i)
                break;
            T d = val[lu_diag_ptr[k]];
            if(ORC_FABS(d) <= ORC_TINY)
            {
                free(mapper);
                return ORC_NUMERICAL_ERROR;
            }
            val[j] = val[j] / d;
            for(oint jj = lu_diag_ptr[k] + 1; jj < row_ptr[k + 1] - base; jj++)
            {
                oint jw = mapper[col_ind[jj] - base];
                if(jw != 0)
                    val[jw] = ORC_FMA(-val[j], val[jj], val[jw]);
            }
        }
        lu_diag_ptr[i] = j;
        if(j >= j2 || k != i || ORC_FABS(val[j]) <= ORC_TINY)
        {
            free(mapper);
            return ORC_NUMERICAL_ERROR;
        }
        for(oint mn = j1; mn < j2; mn++)
            mapper[col_ind[mn] - base] = 0;
    }
    free(mapper);
    return ORC_SUCCESS;
}

/* ILU(0) solve, solvers/aoclsparse_ilu0.hpp:113-156: L y = b (unit lower), U x = y; "sum - val*x"  */
/* contracts to an FMA under the reference's -ffp-contract=fast.                                    */
int FN(ilu_solve)(oint n, int base, const oint *lu_diag_ptr, const T *val, const oint *row_ptr, const oint *col_ind, T *x,
                  const T *b)
{
    for(oint i = 0; i < n; i++)
    {
        T sum = b[i];
        for(oint k = row_ptr[i] - base; k < lu_diag_ptr[i]; k++)
            sum = ORC_FMA(-val[k], x[col_ind[k] - base], sum);
        x[i] = sum;
    }
    for(oint i = n - 1; i >= 0; i--)
    {
        for(oint k = lu_diag_ptr[i] + 1; k < row_ptr[i + 1] - base; k++)
            x[i] = ORC_FMA(-val[k], x[col_ind[k] - base], x[i]);
        T d = val[lu_diag_ptr[i]];
        if(!(ORC_FABS(d) <= ORC_TINY))
            x[i] = x[i] / d;
    }
    return ORC_SUCCESS;
}

/* ------------------------------------------------------------------------------------ */
/* Symmetric Gauss-Seidel sweep, solvers/aoclsparse_symgs.hpp:62-258 (symgs_ref), built   */
/* from the triangular SpMV and TRSV restatements above exactly as the reference chains   */
/* aoclsparse::mv / aoclsparse::trsv on the clean CSR.  type: 0 general, 1 symmetric,     */
/* 3 triangular; fill 0 lower / 1 upper; trans 0 none / 1 transpose.                      */
/* ------------------------------------------------------------------------------------ */
static int LN(symgs_mv)(int tr, int base, T alpha, oint m, int diag, int fill, const T *val, const oint *col,
                        const oint *ptr, const oint *idiag, const oint *iurow, const T *x, T *y, int rev)
{
    /* beta = 0: the triangular kernels zero y first (csrmv_kr.hpp:535-542) */
    return tr ? LN(csrmv_tri_t)(base, alpha, m, m, diag, fill, val, col, ptr, idiag, iurow, x, (T)0, y, rev)
              : LN(csrmv_tri)(base, alpha, m, diag, fill, val, col, ptr, idiag, iurow, x, (T)0, y, rev);
}
static int LN(symgs_sv)(int tr, int fill, int base, oint m, const T *val, const oint *col, const oint *ptr,
                        const oint *idiag, const oint *iurow, const T *b, T *x)
{
    if(fill == 0)
        return tr ? FN(trsv_lt)((T)1, m, base, val, col, ptr, idiag, b, 1, x, 1, 0)
                  : FN(trsv_l)((T)1, m, base, val, col, ptr, idiag, b, 1, x, 1, 0);
    return tr ? FN(trsv_ut)((T)1, m, base, val, col, ptr, iurow, b, 1, x, 1, 0)
              : FN(trsv_u)((T)1, m, base, val, col, ptr, iurow, b, 1, x, 1, 0);
}
static int LN(symgs)(int type, int fill, int trans, int base, T alpha, oint m, const T *val, const oint *col,
                     const oint *ptr, const oint *idiag, const oint *iurow, const T *b, T *x, int rev)
{
    if(type == 3) /* :128-149 */
        return LN(symgs_sv)(trans, fill, base, m, val, col, ptr, idiag, iurow, b, x);
    int u_tr = 1, l_tr = 0, u_fill = 0, l_fill = 0; /* symmetric, lower stored (:151-163) */
    if(type == 1 && fill == 1)
        u_fill = l_fill = 1, u_tr = 0, l_tr = 1;
    else if(type == 0 && trans == 0)
        u_tr = l_tr = 0, u_fill = 1;
    else if(type == 0 && trans == 1)
        u_tr = l_tr = 1, l_fill = 1, u_fill = 0;
    T *r = (T *)malloc(sizeof(T) * (size_t)(m > 0 ? m : 1));
    T *q = (T *)malloc(sizeof(T) * (size_t)(m > 0 ? m : 1));
    if(!r || !q)
    {
        free(r), free(q);
        return ORC_MEMORY_ERROR;
    }
    LN(symgs_mv)(u_tr, base, alpha, m, 2, u_fill, val, col, ptr, idiag, iurow, x, q, rev); /* q = alpha U x0 */
    for(oint i = 0; i < m; i++)
        r[i] = b[i] - q[i];
    LN(symgs_sv)(l_tr, l_fill, base, m, val, col, ptr, idiag, iurow, r, q); /* (L+D) x1 = r */
    LN(symgs_mv)(l_tr, base, (T)1, m, 2, l_fill, val, col, ptr, idiag, iurow, q, r, rev); /* r = L x1 */
    for(oint i = 0; i < m; i++)
        q[i] = b[i] - r[i];
    LN(symgs_sv)(u_tr, u_fill, base, m, val, col, ptr, idiag, iurow, q, x); /* (U+D) x = q */
    free(r), free(q);
    return ORC_SUCCESS;
}

/* ------------------------------------------------------------------------------------ */
/* aoclsparse_elltmv_avx2 / _ref, ellmv.hpp:316-444: one FMA chain per row over the       */
/* column-major cells                                                                    */
/* ------------------------------------------------------------------------------------ */
int FN(elltmv)(int base, T alpha, oint m, const T *val, const oint *col, oint width, const T *x, T beta, T *y)
{
    for(oint j = 0; j < m; j++)
    {
        T r = (T)0;
        for(oint i = 0; i < width; i++)
            r = ORC_FMA(val[(size_t)i * m + j], x[col[(size_t)i * m + j] - base], r);
        if(alpha != (T)1)
            r = alpha * r;
        if(beta != (T)0)
            r = ORC_FMA(beta, y[j], r); /* "result += beta * y[i]" under -ffp-contract=fast */
        y[j] = r;
    }
    return ORC_SUCCESS;
}

/* ---- forward SOR sweep: solvers/aoclsparse_sorv.hpp:78-113 and :212-226 (x = alpha*x first; exact zeros for
 * alpha == 0).  Returns 5 (invalid_value) when a row lacks a single non-zero diagonal entry (:32-75). */
int FN(sorv)(oint n, int base, const oint *ptr, const oint *ind, const T *val, T omega, T alpha, T *x, const T *b)
{
    for(oint i = 0; i < n; i++)
    {
        int found = 0;
        for(oint j = ptr[i] - base; j < ptr[i + 1] - base; j++)
            if(ind[j] - base == i)
            {
                if(found || val[j] == (T)0)
                    return ORC_INVALID_VALUE;
                found = 1;
            }
        if(!found)
            return ORC_INVALID_VALUE;
    }
    for(oint i = 0; i < n; i++)
        x[i] = alpha != (T)0 ? alpha * x[i] : (T)0;
    for(oint i = 0; i < n; i++)
    {
        T axi = (T)0, d = (T)1;
        for(oint j = ptr[i] - base; j < ptr[i + 1] - base; j++)
        {
            const oint c = ind[j] - base;
            if(c != i)
                axi = ORC_FMA(val[j], x[c], axi);
            else
                d = val[j];
        }
        x[i] = ORC_FMA(omega, (b[i] - axi) / d - x[i], x[i]);
    }
    return ORC_SUCCESS;
}

/* ------------------------------------------------------------------------------------ */
/* Iterative solvers, solvers/aoclsparse_itsol_functions.hpp: CG :632-875 (+ the built-in */
/* SymGS preconditioner :390-479), restarted GMRES :910-1367 (+ ILU(0) preconditioner).   */
/* The reference's level-1 steps are AOCL-BLAS calls (not vendored): plain loops here,    */
/* a multiplication and an addition per term.  pairwise = 1 sums the same products by     */
/* recursive halving instead (no reference build does; the two orders bracket what a      */
/* tree reduction of the same dot product may give: the iteration margin of the tests).   */
/* A is a general clean CSR holding the whole (for CG: symmetric) matrix.                 */
/* precond: CG 0 none / 3 SymGS; GMRES 0 none / 2 ILU0.  Returns the reference's status;   */
/* rinfo[0] residual norm, rinfo[1] ||b|| (GMRES: rtol*||b||), rinfo[30] iterations.       */
/* ------------------------------------------------------------------------------------ */
static T LN(dot_pair)(oint n, const T *a, const T *b)
{
    if(n <= 8)
    {
        T s = (T)0;
        for(oint i = 0; i < n; i++)
            s += a[i] * b[i];
        return s;
    }
    oint h = n / 2;
    return LN(dot_pair)(h, a, b) + LN(dot_pair)(n - h, a + h, b + h);
}
static T LN(dot)(oint n, const T *a, const T *b, int pairwise)
{
    if(pairwise)
        return LN(dot_pair)(n, a, b);
    T s = (T)0;
    for(oint i = 0; i < n; i++)
        s += a[i] * b[i];
    return s;
}
static T LN(nrm2)(oint n, const T *v, int pairwise)
{
    return ORC_SQRT(LN(dot)(n, v, v, pairwise));
}
static void LN(mv)(oint n, int base, const oint *ptr, const oint *col, const T *val, const T *x, T *y)
{
    FN(csrmv_ref)(base, (T)1, n, val, col, ptr, x, (T)0, y);
}
static int LN(cg)(oint n, int base, const oint *ptr, const oint *col, const T *val, const oint *idiag, const oint *iurow,
                  const T *b, T *x, T rtol, T atol, oint maxit, int precond, T *rinfo, int pairwise)
{
    const T tiny = ORC_TINY;
    T      *w    = (T *)calloc(5 * (size_t)(n > 0 ? n : 1), sizeof(T));
    if(!w)
        return ORC_MEMORY_ERROR;
    T  *r = w, *z = w + n, *p = w + 2 * (size_t)n, *q = w + 3 * (size_t)n, *y = w + 4 * (size_t)n;
    int status = ORC_SUCCESS;
    for(int i = 0; i < 100; i++)
        rinfo[i] = (T)0;
    for(oint i = 0; i < n; i++)
        r[i] = -b[i], p[i] = x[i];
    T bnorm = LN(nrm2)(n, b, pairwise), brtol = rtol * bnorm;
    rinfo[1] = bnorm;
    LN(mv)(n, base, ptr, col, val, p, q);
    for(oint i = 0; i < n; i++)
        r[i] += q[i], p[i] = (T)0;
    T rnorm = LN(nrm2)(n, r, pairwise), rz = (T)1;
    rinfo[0]   = rnorm;
    oint niter = 0;
    for(;;)
    {
        if(((T)0 < atol && rnorm <= atol) || ((T)0 < rtol && rnorm <= brtol))
            break;
        if(maxit > 0 && niter > maxit)
        {
            status = 7; /* aoclsparse_status_maxit */
            break;
        }
        niter++;
        rinfo[30] = (T)niter;
        if(precond == 3)
        {
            /* (L+D) y = r ; y = D y ; (U+D) z = y */
            FN(trsv_l)((T)1, n, base, val, col, ptr, idiag, r, 1, y, 1, 0);
            for(oint i = 0; i < n; i++)
                y[i] *= val[idiag[i] - base];
            FN(trsv_u)((T)1, n, base, val, col, ptr, iurow, y, 1, z, 1, 0);
        }
        else
            for(oint i = 0; i < n; i++)
                z[i] = r[i];
        T rz_new = LN(dot)(n, r, z, pairwise);
        if(rz <= tiny)
        {
            status = ORC_NUMERICAL_ERROR;
            break;
        }
        T beta = rz_new / rz;
        rz     = rz_new;
        for(oint i = 0; i < n; i++)
            p[i] = beta * p[i] - z[i];
        LN(mv)(n, base, ptr, col, val, p, q);
        T pq = LN(dot)(n, p, q, pairwise);
        if(pq <= tiny)
        {
            status = ORC_NUMERICAL_ERROR;
            break;
        }
        T alpha = rz / pq;
        for(oint i = 0; i < n; i++)
            x[i] += alpha * p[i], r[i] += alpha * q[i];
        rnorm    = LN(nrm2)(n, r, pairwise);
        rinfo[0] = rnorm;
    }
    free(w);
    return status;
}

/* LAPACK 3.10 ?lartg, unscaled branch (the values met here are far from the over/underflow limits) */
static void LN(lartg)(T f, T g, T *c, T *s, T *r)
{
    if(g == (T)0)
        *c = (T)1, *s = (T)0, *r = f;
    else if(f == (T)0)
        *c = (T)0, *s = ORC_COPYSIGN((T)1, g), *r = ORC_FABS(g);
    else
    {
        T d = ORC_SQRT(f * f + g * g);
        *c = ORC_FABS(f) / d, *r = ORC_COPYSIGN(d, f), *s = g / *r;
    }
}
static int LN(gmres)(oint n, int base, const oint *ptr, const oint *col, const T *val, const T *b, T *x, oint m, T rtol,
                     T atol, oint maxit, int precond, T *rinfo, int pairwise)
{
    const T tiny = ORC_TINY;
    size_t  nn = (size_t)(n > 0 ? n : 1), mm = (size_t)m;
    T      *V = (T *)calloc((mm + 1) * nn, sizeof(T)), *Z = (T *)calloc((mm + 1) * nn, sizeof(T));
    T      *h = (T *)calloc(mm * mm, sizeof(T)), *g = (T *)calloc(mm + 1, sizeof(T));
    T      *c = (T *)calloc(mm, sizeof(T)), *s = (T *)calloc(mm, sizeof(T));
    T      *lu = NULL;
    oint   *ludiag = NULL;
    int     status = ORC_SUCCESS;
    if(!V || !Z || !h || !g || !c || !s)
    {
        status = ORC_MEMORY_ERROR;
        goto done;
    }
    if(precond == 2)
    {
        oint nnz = ptr[n] - base;
        lu       = (T *)malloc(sizeof(T) * (size_t)(nnz > 0 ? nnz : 1));
        ludiag   = (oint *)malloc(sizeof(oint) * nn);
        if(!lu || !ludiag)
        {
            status = ORC_MEMORY_ERROR;
            goto done;
        }
        memcpy(lu, val, sizeof(T) * (size_t)nnz);
        status = FN(ilu0)(n, base, ludiag, lu, ptr, col);
        if(status != ORC_SUCCESS)
            goto done;
    }
    oint niter = 0;
    for(;;) /* one restart cycle per pass */
    {
        LN(mv)(n, base, ptr, col, val, x, V);
        T bnorm = LN(nrm2)(n, b, pairwise), brtol = rtol * bnorm;
        rinfo[1] = brtol;
        if(ORC_FABS(atol) <= tiny && ORC_FABS(brtol) <= tiny)
        {
            status = 5; /* invalid_value */
            goto done;
        }
        for(oint i = 0; i < n; i++)
            V[i] = b[i] - V[i];
        T rnorm = LN(nrm2)(n, V, pairwise);
        g[0] = rnorm, rinfo[0] = rnorm;
        if(((T)0 < rnorm && (rnorm <= atol || rnorm <= brtol)) || rnorm == (T)0)
        {
            rinfo[30] = (T)niter;
            goto done;
        }
        for(oint i = 0; i < n; i++)
            V[i] *= (T)1 / rnorm;
        oint j = 0;
        for(; j < m; j++)
        {
            T *vj = V + (size_t)j * nn, *w = V + (size_t)(j + 1) * nn, *zj = Z + (size_t)j * nn;
            if(precond == 2)
                FN(ilu_solve)(n, base, ludiag, lu, ptr, col, zj, vj);
            LN(mv)(n, base, ptr, col, val, precond ? zj : vj, w);
            for(oint i = 0; i <= j; i++)
                h[(size_t)i * mm + j] = LN(dot)(n, w, V + (size_t)i * nn, pairwise);
            for(oint k = 0; k < n; k++)
            {
                T hv = (T)0;
                for(oint i = 0; i <= j; i++)
                    hv += h[(size_t)i * mm + j] * V[(size_t)i * nn + k];
                w[k] -= hv;
            }
            T hh = LN(nrm2)(n, w, pairwise);
            if(hh < atol || hh < brtol)
            {
                niter += j + 1;
                rinfo[30] = (T)niter, rinfo[0] = hh;
                goto done;
            }
            for(oint k = 0; k < n; k++)
                w[k] *= (T)1 / hh;
            for(oint i = 0; i < j; i++)
            {
                T r1 = h[(size_t)i * mm + j], r2 = h[(size_t)(i + 1) * mm + j];
                h[(size_t)i * mm + j]       = c[i] * r1 - s[i] * r2;
                h[(size_t)(i + 1) * mm + j] = s[i] * r1 + c[i] * r2;
            }
            T rr = h[(size_t)j * mm + j];
            LN(lartg)(rr, -hh, &c[j], &s[j], &h[(size_t)j * mm + j]);
            T g0 = g[j];
            g[j] = c[j] * g0, g[j + 1] = s[j] * g0;
            rinfo[0] = ORC_FABS(g[j]);
        }
        for(oint jj = m - 1; jj >= 0; jj--)
        {
            T yj = g[jj];
            for(oint i = jj + 1; i < m; i++)
                yj -= h[(size_t)jj * mm + i] * s[i];
            if(ORC_FABS(h[(size_t)jj * mm + jj]) <= tiny)
            {
                status = ORC_NUMERICAL_ERROR;
                goto done;
            }
            s[jj] = yj / h[(size_t)jj * mm + jj];
        }
        for(oint k = 0; k < n; k++)
        {
            T acc = (T)0;
            for(oint t = 0; t < m; t++)
                acc += (precond ? Z : V)[(size_t)t * nn + k] * s[t];
            x[k] += acc;
        }
        rnorm = ORC_FABS(g[m]);
        niter += m;
        rinfo[30] = (T)niter, rinfo[0] = rnorm;
        if(((T)0 < atol && rnorm <= atol) || ((T)0 < rnorm && rnorm <= brtol))
            goto done;
        if(maxit > 0 && niter >= maxit)
        {
            status = 7;
            goto done;
        }
    }
done:
    free(V), free(Z), free(h), free(g), free(c), free(s), free(lu), free(ludiag);
    return status;
}

#undef ORC_TINY
#undef T
#undef LN
#undef FN
#undef ORC_CAT3
#undef ORC_CAT3_
