// sy_dense_kernels.hip -- the symmetric products with a DENSE result, aoclsparse_?syrkd (C = alpha*A*A^H + beta*C or
// alpha*A^H*A + beta*C) and aoclsparse_?syprd (C = alpha*A*B*A^H + beta*C or alpha*A^H*B*A + beta*C, B dense Hermitian
// given by its upper triangle), gfx950.  Only the upper triangle of C is ever read or written.
//
// Reference: level3/aoclsparse_syrkd.hpp:41-165 (online A^T*B restricted to j >= i), level3/aoclsparse_syprd.hpp:46-264
// (row / column layout kernels).  The arithmetic follows this library's dense-product convention (sp2md_kernels.hip):
// a scaled factor is rounded once, every product is added with one fused multiply-add, complex values through the
// four-fma d_fma.  The small value helpers below are a PRIVATE COPY of the ones in sp2md_kernels.hip: that file stays
// untouched, so that its code generation cannot change.
//
// syrkd: M is the stored matrix after the effective-op decision; C(i,j), j >= i, receives fma(val, w, C) for r ascending
// over the rows of M that hold column i, val = alpha*conj(M(r,i)) and w = M(r,j) (CONJLEFT) or val = alpha*M(r,i) and
// w = conj(M(r,j)).  One WAVEFRONT owns row i of C.  It walks column i of M serially -- a row of the CSR called X below,
// the transpose of M -- and its 64 lanes spread over the entries of row r of M (the CSR called W); a lane whose column is
// below i does nothing (a predicate per entry: rows need not be sorted).  Accesses of one wavefront to one address are
// performed in program order (sp2md_kernels.hip says why the fence is only for the compiler).
//   * Handle creation lets a row repeat an off-diagonal column (matrix.cpp: mat_check only refuses a repeated
//     diagonal), and two lanes must not meet on one element of C: for such a handle the host passes SY_SERIAL and lane 0
//     walks W's row alone, in stored order, which is the reference's order for the repeated column too.
//   * op = none is legal on unsorted rows, and there the reference's r ascends along the SORTED row (its csr2csc copy):
//     with SY_ORDERED the wavefront picks the next entry of X's row by (column, position) instead of by position.
//
// syprd: stage 1 writes T(i,.) = row i of alpha*M*herm(B) (or conj(M)) into a device scratch, a chain over the entries of
// row i of M in stored order per element; lanes over j, so the half of the Hermitian read that lies along B's storage
// order coalesces and the mirrored half is strided.  Stage 2: C(i,j), j >= i, starts at beta*C (or 0) and receives
// fma(T(i,c), conj(m_jc) or m_jc, C) over row j of M; one workgroup per row i, T(i,.) in LDS when it fits.
#include "internal.hpp"

#include <hip/hip_runtime.h>

namespace mi355
{

namespace
{
__device__ __forceinline__ double d_fma(double a, double b, double c)
{
    return fma(a, b, c);
}
__device__ __forceinline__ float d_fma(float a, float b, float c)
{
    return fmaf(a, b, c);
}
template <typename R>
__device__ __forceinline__ cplx<R> d_fma(cplx<R> a, cplx<R> b, cplx<R> c)
{
    c.re = d_fma(a.re, b.re, c.re);
    c.re = d_fma(-a.im, b.im, c.re);
    c.im = d_fma(a.re, b.im, c.im);
    c.im = d_fma(a.im, b.re, c.im);
    return c;
}
__device__ __forceinline__ double d_mul(double a, double b)
{
    return a * b;
}
__device__ __forceinline__ float d_mul(float a, float b)
{
    return a * b;
}
template <typename R>
__device__ __forceinline__ cplx<R> d_mul(cplx<R> a, cplx<R> b)
{
    return cplx<R>(a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re);
}
__device__ __forceinline__ double d_conj(double a, bool)
{
    return a;
}
__device__ __forceinline__ float d_conj(float a, bool)
{
    return a;
}
template <typename R>
__device__ __forceinline__ cplx<R> d_conj(cplx<R> a, bool on)
{
    return on ? cplx<R>(a.re, -a.im) : a;
}
template <typename T>
__device__ __forceinline__ T d_zero()
{
    return T(0);
}
} // namespace

// syrkd.hpp:265-313, syprd.hpp:67-91 / :181-203: the upper triangle is scaled by beta, beta == 0 stores zeros.  Element
// (o, x) of the storage sits at o*ld + x; it belongs to the upper triangle when x >= o (row-major, o = row) or x <= o
// (column-major, o = column).
template <typename T>
__global__ void sy_scale_upper_kernel(T *C, aoclsparse_int n, long long ld, bool inner_ge, T beta, bool zero)
{
    const aoclsparse_int x = blockIdx.x * blockDim.x + threadIdx.x;
    if(x >= n)
        return;
    for(aoclsparse_int o = blockIdx.y; o < n; o += gridDim.y)
    {
        if(inner_ge ? x < o : x > o)
            continue;
        T *p = C + (long long)o * ld + x;
        *p   = zero ? d_zero<T>() : d_mul(beta, *p);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void syrkd_kernel(aoclsparse_int mc, int base_x, const aoclsparse_int *__restrict__ ptr_x,
                                                    const aoclsparse_int *__restrict__ ind_x,
                                                    const T *__restrict__ val_x, bool conj_x, int base_w,
                                                    const aoclsparse_int *__restrict__ ptr_w,
                                                    const aoclsparse_int *__restrict__ ind_w,
                                                    const T *__restrict__ val_w, bool conj_w, T alpha, T *C,
                                                    long long rs, long long cs, int flags)
{
    const int lane   = threadIdx.x & 63;
    const int wave   = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for(aoclsparse_int i = wave; i < mc; i += nwaves)
    {
        T                   *crow = C + (long long)i * rs;
        const aoclsparse_int x0 = ptr_x[i] - base_x, x1 = ptr_x[i + 1] - base_x;
        long long            last = -1; // SY_ORDERED: (column << 32 | position) of the entry taken last
        for(aoclsparse_int step = x0; step < x1; step++)
        {
            aoclsparse_int j = step;
            if(flags & SY_ORDERED)
            {
                long long best = 0x7fffffffffffffffLL;
                for(aoclsparse_int k = x0 + lane; k < x1; k += 64)
                {
                    const long long key = ((long long)(ind_x[k] - base_x) << 32) | (long long)(k - x0);
                    if(key > last && key < best)
                        best = key;
                }
                for(int off = 32; off > 0; off >>= 1)
                {
                    const long long o = __shfl_xor(best, off);
                    best              = o < best ? o : best;
                }
                last = best;
                j    = x0 + (aoclsparse_int)(best & 0xffffffffLL);
            }
            const T              v  = d_mul(alpha, d_conj(val_x[j], conj_x));
            const aoclsparse_int r  = ind_x[j] - base_x;
            const aoclsparse_int w0 = ptr_w[r] - base_w, w1 = ptr_w[r + 1] - base_w;
            if(flags & SY_SERIAL)
            {
                if(lane == 0)
                    for(aoclsparse_int k = w0; k < w1; k++)
                    {
                        const aoclsparse_int c = ind_w[k] - base_w;
                        if(c < i)
                            continue;
                        T *p = crow + (long long)c * cs;
                        *p   = d_fma(v, d_conj(val_w[k], conj_w), *p);
                    }
            }
            else
                for(aoclsparse_int k = w0 + lane; k < w1; k += 64)
                {
                    const aoclsparse_int c = ind_w[k] - base_w;
                    if(c < i)
                        continue;
                    T *p = crow + (long long)c * cs;
                    *p   = d_fma(v, d_conj(val_w[k], conj_w), *p);
                }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
    }
}

// syprd.hpp:111-135 (row-major: valM = alpha*m rounded, then fma(Bval, valM, t)) and :227-242 (column-major: fma(m, Bval, t)
// over the row, then one multiply by alpha).  B(lo, hi), lo <= hi, is read from the upper triangle and conjugated when j
// lies left of the entry's column.
template <typename T, bool ROWMAJ>
__global__ __launch_bounds__(256) void syprd_stage1_kernel(aoclsparse_int mc, aoclsparse_int nin, int base,
                                                           const aoclsparse_int *__restrict__ ptr,
                                                           const aoclsparse_int *__restrict__ ind,
                                                           const T *__restrict__ val, bool conj_m, T alpha,
                                                           const T *__restrict__ B, long long ldb, T *__restrict__ Tm)
{
    for(aoclsparse_int i = blockIdx.x; i < mc; i += gridDim.x)
    {
        const aoclsparse_int a0 = ptr[i] - base, a1 = ptr[i + 1] - base;
        for(aoclsparse_int j = threadIdx.x; j < nin; j += blockDim.x)
        {
            T t = d_zero<T>();
            for(aoclsparse_int k = a0; k < a1; k++)
            {
                const aoclsparse_int c  = ind[k] - base;
                const T              mv = d_conj(val[k], conj_m);
                const long long      lo = j < c ? j : c, hi = j < c ? c : j;
                const T              b  = d_conj(B[ROWMAJ ? lo * ldb + hi : lo + hi * ldb], j < c);
                if(ROWMAJ)
                    t = d_fma(b, d_mul(alpha, mv), t);
                else
                    t = d_fma(mv, b, t);
            }
            if(!ROWMAJ)
                t = d_mul(t, alpha);
            Tm[(long long)i * nin + j] = t;
        }
    }
}

// syprd.hpp:140-153 / :247-260.  beta_mode: 0 C starts at zero, 1 at C, 2 at beta*C.
template <typename T>
__global__ __launch_bounds__(256) void syprd_stage2_kernel(aoclsparse_int mc, aoclsparse_int nin, int base,
                                                           const aoclsparse_int *__restrict__ ptr,
                                                           const aoclsparse_int *__restrict__ ind,
                                                           const T *__restrict__ val, bool conj_m,
                                                           const T *__restrict__ Tm, T beta, int beta_mode, T *C,
                                                           long long rs, long long cs, bool use_lds)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sy_lds_raw[];
    T *trow = reinterpret_cast<T *>(sy_lds_raw);
    for(aoclsparse_int i = blockIdx.x; i < mc; i += gridDim.x)
    {
        const T *t = Tm + (long long)i * nin;
        if(use_lds)
        {
            __syncthreads(); // the previous row's readers are done
            for(aoclsparse_int c = threadIdx.x; c < nin; c += blockDim.x)
                trow[c] = t[c];
            __syncthreads();
            t = trow;
        }
        for(aoclsparse_int j = i + threadIdx.x; j < mc; j += blockDim.x)
        {
            T *p = C + (long long)i * rs + (long long)j * cs;
            T  c = beta_mode == 0 ? d_zero<T>() : beta_mode == 1 ? *p : d_mul(beta, *p);
            for(aoclsparse_int k = ptr[j] - base; k < ptr[j + 1] - base; k++)
                c = d_fma(t[ind[k] - base], d_conj(val[k], conj_m), c);
            *p = c;
        }
    }
}

template <typename T>
aoclsparse_status launch_sy_scale_upper(hipStream_t s, T *C, aoclsparse_int n, long long ld, bool rowmajor, T beta,
                                        bool zero)
{
    if(n <= 0)
        return aoclsparse_status_success;
    const int gy = n < 32768 ? n : 32768;
    hipLaunchKernelGGL((sy_scale_upper_kernel<T>), dim3((n + 255) / 256, gy), dim3(256), 0, s, C, n, ld, rowmajor, beta,
                       zero);
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

template <typename T>
aoclsparse_status launch_syrkd(hipStream_t s, aoclsparse_int mc, int base_x, const aoclsparse_int *ptr_x,
                               const aoclsparse_int *ind_x, const T *val_x, bool conj_x, int base_w,
                               const aoclsparse_int *ptr_w, const aoclsparse_int *ind_w, const T *val_w, bool conj_w,
                               T alpha, T *C, long long rs, long long cs, int flags)
{
    if(mc <= 0)
        return aoclsparse_status_success;
    long long blocks = ((long long)mc + 3) / 4;
    if(blocks > 65536)
        blocks = 65536;
    hipLaunchKernelGGL((syrkd_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, s, mc, base_x, ptr_x, ind_x, val_x, conj_x,
                       base_w, ptr_w, ind_w, val_w, conj_w, alpha, C, rs, cs, flags);
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

template <typename T>
aoclsparse_status launch_syprd(hipStream_t s, aoclsparse_int mc, aoclsparse_int nin, int base, const aoclsparse_int *ptr,
                               const aoclsparse_int *ind, const T *val, bool conj_1, bool conj_2, T alpha, const T *B,
                               long long ldb, bool rowmajor, T *scratch, T beta, int beta_mode, T *C, long long rs, long long cs)
{
    if(mc <= 0)
        return aoclsparse_status_success;
    const unsigned blocks = mc < 65536 ? (unsigned)mc : 65536u;
    if(rowmajor)
        hipLaunchKernelGGL((syprd_stage1_kernel<T, true>), dim3(blocks), dim3(256), 0, s, mc, nin, base, ptr, ind, val,
                           conj_1, alpha, B, ldb, scratch);
    else
        hipLaunchKernelGGL((syprd_stage1_kernel<T, false>), dim3(blocks), dim3(256), 0, s, mc, nin, base, ptr, ind, val,
                           conj_1, alpha, B, ldb, scratch);
    MI355_HIP_TRY(hipGetLastError());
    // T(i,.) in LDS when it fits: 64 KB without asking, up to SY_LDS_MAX with the attribute
    const size_t bytes   = sizeof(T) * (size_t)nin;
    const bool   use_lds = bytes <= SY_LDS_MAX;
    if(use_lds && bytes > 64 * 1024)
        MI355_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&syprd_stage2_kernel<T>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)SY_LDS_MAX));
    hipLaunchKernelGGL((syprd_stage2_kernel<T>), dim3(blocks), dim3(256), use_lds ? bytes : 0, s, mc, nin, base, ptr, ind,
                       val, conj_2, scratch, beta, beta_mode, C, rs, cs, use_lds);
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

#define MI355_INST_SY_DENSE(T)                                                                                          \
    template aoclsparse_status launch_sy_scale_upper<T>(hipStream_t, T *, aoclsparse_int, long long, bool, T, bool);    \
    template aoclsparse_status launch_syrkd<T>(hipStream_t, aoclsparse_int, int, const aoclsparse_int *,                \
                                               const aoclsparse_int *, const T *, bool, int, const aoclsparse_int *,    \
                                               const aoclsparse_int *, const T *, bool, T, T *, long long, long long,   \
                                               int);                                                                    \
    template aoclsparse_status launch_syprd<T>(hipStream_t, aoclsparse_int, aoclsparse_int, int, const aoclsparse_int *, \
                                               const aoclsparse_int *, const T *, bool, bool, T, const T *, long long, bool, \
                                               T *, T, int, T *, long long, long long);
MI355_INST_SY_DENSE(double)
MI355_INST_SY_DENSE(float)
MI355_INST_SY_DENSE(cdouble)
MI355_INST_SY_DENSE(cfloat)

} // namespace mi355
