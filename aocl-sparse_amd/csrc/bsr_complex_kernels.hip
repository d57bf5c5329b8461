// bsr_complex_kernels.hip -- y = alpha*A*x + beta*y for BSR arrays with complex values and column-major blocks (aoclsparse_cmv /
// aoclsparse_zmv on a BSR handle), gfx950.
//
// Reference: level2/aoclsparse_bsrmv_kr.hpp:32-153 (bsrmv_gn, bsrmv_nxn) with the builders of aoclsparse_bsrmv_bldr.hpp, instantiated
// for std::complex: per scalar row one chain sum += a * x over the blocks of the block row in stored order and the columns inside
// each block in ascending order, then sum *= alpha when alpha != 1, then sum += beta * y when beta != 0 (y is not read otherwise).
// Same mapping as the real kernel (dia_bsr_kernels.hip): ONE LANE PER SCALAR ROW, which keeps exactly that chain; a block is stored
// column-major, so the `dim` rows of a block column are consecutive and neighbouring lanes load neighbouring values.  Each step is
// a complex multiply-add in the convention of complex_kernels.hip (four contracted real multiply-adds), where the reference's compiler
// is free to form the complex product otherwise: parity is the forward-error bound, not the bit pattern.  HBM-bound: 8 / 16 B per
// stored value (dim^2 per block) + 4 B per block index, plus x and y.
#include "internal.hpp"

#include <hip/hip_runtime.h>

namespace mi355
{
namespace
{
__device__ __forceinline__ double cb_fma(double a, double b, double c) { return fma(a, b, c); }
__device__ __forceinline__ float  cb_fma(float a, float b, float c) { return fmaf(a, b, c); }

// acc += a * b (complex_kernels.hip: c_mac)
template <typename R>
__device__ __forceinline__ void cb_mac(cplx<R> &acc, cplx<R> a, cplx<R> b)
{
    acc.re = cb_fma(a.re, b.re, acc.re);
    acc.re = cb_fma(-a.im, b.im, acc.re);
    acc.im = cb_fma(a.re, b.im, acc.im);
    acc.im = cb_fma(a.im, b.re, acc.im);
}

// DIM > 0: block size known at compile time (the sizes the reference has dedicated kernels for, bsrmv.cpp:120-136), so the loads
// of one block are all in flight before its multiply-add chain starts; DIM == 0: any size.
template <typename R, int DIM>
__global__ __launch_bounds__(256) void cbsrmv_kernel(cplx<R> alpha, aoclsparse_int mb, aoclsparse_int dim_rt, int base,
                                                     const cplx<R> *__restrict__ val, const aoclsparse_int *__restrict__ col,
                                                     const aoclsparse_int *__restrict__ row_ptr, const cplx<R> *__restrict__ x,
                                                     cplx<R> beta, cplx<R> *__restrict__ y)
{
    const aoclsparse_int dim = DIM > 0 ? DIM : dim_rt;
    const long long      r = (long long)blockIdx.x * blockDim.x + threadIdx.x; // scalar row
    if(r >= (long long)mb * dim)
        return;
    const aoclsparse_int ai = (aoclsparse_int)(r / dim), bi = (aoclsparse_int)(r % dim);
    const size_t         sq = (size_t)dim * dim;
    cplx<R>              sum(R(0), R(0));
    for(aoclsparse_int aj = row_ptr[ai] - base; aj < row_ptr[ai + 1] - base; aj++)
    {
        const cplx<R> *v  = val + sq * aj + bi;
        const cplx<R> *xp = x + (size_t)dim * (col[aj] - base);
        if constexpr(DIM > 0)
        {
            cplx<R> a[DIM], b[DIM];
#pragma unroll
            for(int bj = 0; bj < DIM; bj++)
                a[bj] = v[DIM * bj], b[bj] = xp[bj];
#pragma unroll
            for(int bj = 0; bj < DIM; bj++)
                cb_mac(sum, a[bj], b[bj]);
        }
        else
            for(aoclsparse_int bj = 0; bj < dim; bj++)
                cb_mac(sum, v[(size_t)dim * bj], xp[bj]);
    }
    if(!(alpha.re == R(1) && alpha.im == R(0)))
    {
        cplx<R> t(R(0), R(0));
        cb_mac(t, sum, alpha);
        sum = t;
    }
    if(!(beta.re == R(0) && beta.im == R(0))) // beta == 0 never reads y
        cb_mac(sum, beta, y[r]);
    y[r] = sum;
}
} // namespace

template <typename R>
aoclsparse_status launch_cbsrmv(hipStream_t s, cplx<R> alpha, aoclsparse_int mb, aoclsparse_int dim, int base, const cplx<R> *val,
                                const aoclsparse_int *col, const aoclsparse_int *row_ptr, const cplx<R> *x, cplx<R> beta,
                                cplx<R> *y)
{
    const long long rows = (long long)mb * dim;
    if(rows <= 0)
        return aoclsparse_status_success;
    const dim3 grid((unsigned)((rows + 255) / 256)), block(256);
#define MI355_CBSR_CASE(D)                                                                                              \
    case D:                                                                                                             \
        hipLaunchKernelGGL((cbsrmv_kernel<R, D>), grid, block, 0, s, alpha, mb, dim, base, val, col, row_ptr, x, beta, y); \
        break;
    switch(dim)
    {
        MI355_CBSR_CASE(2)
        MI355_CBSR_CASE(3)
        MI355_CBSR_CASE(4)
        MI355_CBSR_CASE(5)
        MI355_CBSR_CASE(6)
        MI355_CBSR_CASE(7)
        MI355_CBSR_CASE(8)
        MI355_CBSR_CASE(16)
    default:
        hipLaunchKernelGGL((cbsrmv_kernel<R, 0>), grid, block, 0, s, alpha, mb, dim, base, val, col, row_ptr, x, beta, y);
    }
#undef MI355_CBSR_CASE
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

template aoclsparse_status launch_cbsrmv<float>(hipStream_t, cfloat, aoclsparse_int, aoclsparse_int, int, const cfloat *,
                                                const aoclsparse_int *, const aoclsparse_int *, const cfloat *, cfloat, cfloat *);
template aoclsparse_status launch_cbsrmv<double>(hipStream_t, cdouble, aoclsparse_int, aoclsparse_int, int, const cdouble *,
                                                 const aoclsparse_int *, const aoclsparse_int *, const cdouble *, cdouble,
                                                 cdouble *);

} // namespace mi355
