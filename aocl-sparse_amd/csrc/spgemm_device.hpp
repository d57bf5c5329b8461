// spgemm_device.hpp -- the device helpers that spgemm_hash_kernel (spgemm_kernels.hip) and spg_numeric_kernel
// (spgemm_numeric_kernels.hip) share: the arithmetic of one product, and a group's view of its wavefront and of its hash table.
#pragma once
#include "internal.hpp"

#include <hip/hip_runtime.h>

namespace mi355
{

__device__ __forceinline__ double sp_fma(double a, double b, double c)
{
    return fma(a, b, c);
}
__device__ __forceinline__ float sp_fma(float a, float b, float c)
{
    return fmaf(a, b, c);
}
// complex: the reference's std::complex multiply-add (csr2m.cpp:489-498 with T = std::complex); component-wise fma
template <typename R>
__device__ __forceinline__ cplx<R> sp_fma(cplx<R> a, cplx<R> b, cplx<R> c)
{
    c.re = sp_fma(a.re, b.re, c.re);
    c.re = sp_fma(-a.im, b.im, c.re);
    c.im = sp_fma(a.re, b.im, c.im);
    c.im = sp_fma(a.im, b.re, c.im);
    return c;
}
__device__ __forceinline__ double sp_mul(double a, double b)
{
    return a * b;
}
__device__ __forceinline__ float sp_mul(float a, float b)
{
    return a * b;
}
template <typename R>
__device__ __forceinline__ cplx<R> sp_mul(cplx<R> a, cplx<R> b)
{
    return sp_fma(a, b, cplx<R>(R(0), R(0)));
}
__device__ __forceinline__ double sp_conj(double a, bool)
{
    return a;
}
__device__ __forceinline__ float sp_conj(float a, bool)
{
    return a;
}
template <typename R>
__device__ __forceinline__ cplx<R> sp_conj(cplx<R> a, bool on)
{
    return on ? cplx<R>(a.re, -a.im) : a;
}

// value of lane `src` of the caller's group of `width` lanes
__device__ __forceinline__ double spg_shfl(double v, int src, int width)
{
    return __shfl(v, src, width);
}
__device__ __forceinline__ float spg_shfl(float v, int src, int width)
{
    return __shfl(v, src, width);
}
template <typename R>
__device__ __forceinline__ cplx<R> spg_shfl(cplx<R> v, int src, int width)
{
    return cplx<R>(__shfl(v.re, src, width), __shfl(v.im, src, width));
}

// the bits of group `grp` (G lanes) in a wavefront's ballot
template <int G>
__device__ __forceinline__ unsigned long long spg_group_bits(unsigned long long wave_mask, int grp)
{
    if constexpr(G == 64)
        return wave_mask;
    else
        return (wave_mask >> (G * grp)) & ((1ull << G) - 1ull);
}

// a key of the table: in the global slab an agent-scope load (the inserts are atomics executed at the L2)
template <bool GLOBAL>
__device__ __forceinline__ int spg_key(const int *p)
{
    if constexpr(GLOBAL)
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        return *p;
}

// what the group has written is seen by its lanes' next loads: in the global slab a release + acquire fence (the CU's vector L1
// would otherwise keep answering with the line it loaded before)
template <bool GLOBAL>
__device__ __forceinline__ void spg_sync()
{
    if constexpr(GLOBAL)
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    else
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
}

} // namespace mi355
