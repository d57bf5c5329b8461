// tcsr_kernels.hip -- y = alpha (L + U - D) x + beta y for a TCSR handle on gfx950 (wave64), in the summation order of the
// reference's aoclsparse_dtcsrmv_avx2 (library/src/level2/aoclsparse_tcsrmv.cpp:61-145), bit for bit.
//
// The reference's row i:
//   four lane accumulators = 0, r = 0
//   L's row, diagonal included: the first nL / 4 groups of four into the lanes (entry j + k into lane k), the nL % 4 entries left
//       into the scalar chain r
//   U's row after its diagonal: the first nU / 4 groups of four continue in the SAME lanes
//   if either triangle had a group of four: r += (l0 + l1) + (l2 + l3)
//   U's nU % 4 entries left continue the chain r
//   r = alpha * r (always), then r = fma(beta, y[i], r) unless beta == 0 (y is not read then)
// Four independent chains per row and no more, so four lanes own a row: 16 rows per wavefront, 64 per workgroup.  A group reads
// 32 contiguous bytes of values and 16 of columns per step.  The leftover entries of a triangle (at most three) are loaded by
// lanes 0..2 at once and chained in every lane of the group from quad broadcasts, so the chain costs no second round of loads
// -- on a stencil, where neither triangle fills a group of four, that IS the product.  The lane sum is two quad_perm DPP adds
// ([1,0,3,2] then [2,3,0,1]): floating-point addition commutes exactly, so every lane holds the bits of (l0 + l1) + (l2 + l3).
// Control flow is uniform inside a group (every condition is a property of the row), so a DPP never reads an inactive lane.
//
// Model, not measurement: the traffic should be the algorithmic bytes of the two triangles (the diagonal is stored twice and read
// once from L; U's copy shares a 32-byte sector with the entries behind it), which would put the kernel on the HBM roof.  Measured
// (DESIGN.md section 5): 0.40 of it on the 4096^2 Laplacian.
#include "internal.hpp"

#include <hip/hip_runtime.h>

namespace mi355
{

namespace
{

// quad_perm DPP: 0xB1 = [1,0,3,2], 0x4E = [2,3,0,1], 0x00 / 0x55 / 0xAA = broadcast of lane 0 / 1 / 2 of the quad
template <int CTRL>
__device__ __forceinline__ double quad_mov(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo     = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true); // (old value 0: never seen, every quad lane is a valid source)
    hi     = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// `rem` (0..3) entries starting at p continue the scalar chain r, in order.  Lane k of the group loads entry k.
__device__ __forceinline__ double chain_tail(double r, int rem, int p, int k, const double *__restrict__ val,
                                             const aoclsparse_int *__restrict__ col, const double *__restrict__ xb)
{
    double v = 0.0, xv = 0.0;
    if(k < rem)
    {
        v  = val[p + k];
        xv = xb[col[p + k]];
    }
    const double v0 = quad_mov<0x00>(v), x0 = quad_mov<0x00>(xv);
    const double v1 = quad_mov<0x55>(v), x1 = quad_mov<0x55>(xv);
    const double v2 = quad_mov<0xAA>(v), x2 = quad_mov<0xAA>(xv);
    if(rem > 0)
        r = fma(v0, x0, r);
    if(rem > 1)
        r = fma(v1, x1, r);
    if(rem > 2)
        r = fma(v2, x2, r);
    return r;
}

constexpr int TCSR_BLOCK = 256; // 64 rows per workgroup

__global__ __launch_bounds__(TCSR_BLOCK) void tcsrmv_kernel(int m, int base, double alpha, double beta,
                                                              const double *__restrict__ val_l, const aoclsparse_int *__restrict__ col_l,
                                                              const aoclsparse_int *__restrict__ ptr_l, const double *__restrict__ val_u,
                                                              const aoclsparse_int *__restrict__ col_u, const aoclsparse_int *__restrict__ ptr_u,
                                                              const double *__restrict__ x, double *__restrict__ y)
{
    const int     k    = threadIdx.x & 3;
    const int     i    = (int)(blockIdx.x * (TCSR_BLOCK / 4) + (threadIdx.x >> 2));
    const bool    live = i < m; // a group past the last row runs empty (no load, no store) and stays active for the DPPs
    const double *xb   = x - base;
    int           sl = 0, nl = 0, su = 0, nu = 0;
    if(live)
    {
        sl = ptr_l[i] - base, nl = ptr_l[i + 1] - base - sl;
        su = ptr_u[i] - base + 1, nu = ptr_u[i + 1] - base - su; // U's row starts with the diagonal: L has applied it
    }
    const int fl = nl & ~3, fu = nu & ~3;
    double    acc = 0.0, r = 0.0;
    for(int j = 0; j < fl; j += 4)
        acc = fma(val_l[sl + j + k], xb[col_l[sl + j + k]], acc);
    r = chain_tail(r, nl - fl, sl + fl, k, val_l, col_l, xb);
    for(int j = 0; j < fu; j += 4)
        acc = fma(val_u[su + j + k], xb[col_u[su + j + k]], acc);
    double t = acc + quad_mov<0xB1>(acc); // l0+l1 | l2+l3
    t        = t + quad_mov<0x4E>(t);
    if(fl | fu)
        r = r + t;
    r = chain_tail(r, nu - fu, su + fu, k, val_u, col_u, xb);
    r = alpha * r;
    if(live && k == 0)
    {
        if(beta != 0.0)
            r = fma(beta, y[i], r);
        y[i] = r;
    }
}

} // namespace

aoclsparse_status launch_tcsrmv(hipStream_t s, int base, double alpha, aoclsparse_int m, const double *val_l, const aoclsparse_int *col_l,
                                const aoclsparse_int *ptr_l, const double *val_u, const aoclsparse_int *col_u, const aoclsparse_int *ptr_u,
                                const double *x, double beta, double *y)
{
    if(m <= 0)
        return aoclsparse_status_success;
    const unsigned grid = (unsigned)(((long long)m + TCSR_BLOCK / 4 - 1) / (TCSR_BLOCK / 4));
    hipLaunchKernelGGL(tcsrmv_kernel, dim3(grid), dim3(TCSR_BLOCK), 0, s, (int)m, base, alpha, beta, val_l, col_l, ptr_l, val_u, col_u,
                       ptr_u, x, y);
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

} // namespace mi355
