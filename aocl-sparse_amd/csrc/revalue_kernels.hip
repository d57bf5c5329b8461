// revalue_kernels.hip -- new values through the value maps a handle keeps (round 25: aoclsparse_mi355_keep_value_maps,
// aoclsparse_mi355_?revalue_device in device_handle_api.cpp).
//
// The clean copy of a CSR, the diagonal the TRSV launchers read and the pval array of every TRSV layout are fixed selections of
// the handle's value array: which entry goes where is decided by the structure alone.  A map holds that selection as one int per
// target item (the 0-based position in the source array, negative: no source, the target is the all-zero item), and
//
//   rv_gather_kernel     out[k] = f(in[map[k]]), f = identity or the conjugate (the sign bit of the imaginary half flipped: what
//                        conj_of does on the host, op = H plans).  Items of 4, 8 or 16 bytes, moved and never computed with.
//                        Map reads are coalesced, value reads scattered: a lane takes RV_PER_LANE items a workgroup's width apart,
//                        issues all its map loads, then all its value loads, then stores -- eight independent dependent-load chains
//                        per lane in flight instead of one: coo_refresh_gather_kernel's shape (coo_sort_kernels.hip), with the
//                        zero item for a negative position, the conjugate and a 64-bit k added.  A position outside the source
//                        (no map holds one) gives the zero item too: the guard is one unsigned compare.
//
//   rv_gather_flagged_kernel   the same through the source map of a derived operator (Derived::src, derived_kernels.hip): the
//                        conjugate is chosen per item by one bit of the word, and an item marked as a constant (the one of a unit
//                        diagonal) is left as it is.  It also writes the operator's values when the operator is built.
//
// ... brings new values to all of them.  The maps themselves come from the host (trsv_plan.cpp) or from the three small kernels
// below, which serve aoclsparse_mi355_clean_csr_device:
//
//   rv_iota_kernel       out[k] = k: the payload the row sort permutes to give the sort's permutation.
//   rv_compose_kernel    map[k] = perm[map[k]] where map[k] >= 0: positions in the sorted arrays -> positions in the user's.
//   rv_diag_map_kernel   per row: the clean position of its diagonal entry (idiag - base where iurow == idiag + 1, row < min(m, n)),
//                        else -1: what ensure_trsv computes on the host.
// No atomics, no LDS, vector loads and stores only; no workgroup waits for another.
#include "internal.hpp"

#include <hip/hip_runtime.h>

namespace mi355
{

namespace
{
    constexpr int RV_PER_LANE = 8; // items per lane: their loads are all issued before the first store
    constexpr int RV_BLOCK    = 256;
    constexpr int RV_TILE     = RV_PER_LANE * RV_BLOCK; // items per workgroup

    struct alignas(16) Item16
    {
        unsigned long long a, b;
    };

    // the conjugate of a complex item: (re, im) as two floats in 8 bytes, or two doubles in 16
    __device__ __forceinline__ unsigned int rv_conj(unsigned int v)
    {
        return v; // (a real item: never asked for)
    }
    __device__ __forceinline__ unsigned long long rv_conj(unsigned long long v)
    {
        return v ^ 0x8000000000000000ull;
    }
    __device__ __forceinline__ Item16 rv_conj(Item16 v)
    {
        v.b ^= 0x8000000000000000ull;
        return v;
    }

    // (coo_refresh_gather_kernel's shape (coo_sort_kernels.hip): the positions stay `int` until the value loads have been issued --
    // widened inside the first loop, the compiler put every map load in a branch of its own with a full wait behind it)
    template <typename V, bool CONJ>
    __global__ __launch_bounds__(RV_BLOCK) void rv_gather_kernel(long long count, int nsrc, const int *__restrict__ map,
                                                                 const V *__restrict__ in, V *__restrict__ out)
    {
        const long long k0 = (long long)blockIdx.x * RV_TILE + threadIdx.x;
        int             p[RV_PER_LANE];
        V               v[RV_PER_LANE];
#pragma unroll
        for(int j = 0; j < RV_PER_LANE; j++)
        {
            const long long k = k0 + (long long)j * RV_BLOCK;
            p[j]              = k < count ? map[k] : -1;
        }
#pragma unroll
        for(int j = 0; j < RV_PER_LANE; j++) // (a negative position, or one past the source, which no map holds: the zero item)
            v[j] = (unsigned)p[j] < (unsigned)nsrc ? in[p[j]] : V{};
#pragma unroll
        for(int j = 0; j < RV_PER_LANE; j++)
        {
            const long long k = k0 + (long long)j * RV_BLOCK;
            if(k < count)
                out[k] = CONJ ? rv_conj(v[j]) : v[j];
        }
    }

    // rv_gather_kernel for a derived operator's map (Derived::src): a word is a position, DERIVED_SRC_CONJ set where the item is the
    // conjugate of its source, or DERIVED_SRC_CONST: the target is a constant and stays as it is.  The same batching -- every map
    // load, then every value load, then the stores; a word that names no source (none is ever written) leaves its target alone too.
    template <typename V>
    __global__ __launch_bounds__(RV_BLOCK) void rv_gather_flagged_kernel(long long count, unsigned nsrc, const unsigned *__restrict__ map,
                                                                         const V *__restrict__ in, V *__restrict__ out)
    {
        const long long k0 = (long long)blockIdx.x * RV_TILE + threadIdx.x;
        unsigned        w[RV_PER_LANE];
        V               v[RV_PER_LANE];
#pragma unroll
        for(int j = 0; j < RV_PER_LANE; j++)
        {
            const long long k = k0 + (long long)j * RV_BLOCK;
            w[j]              = k < count ? map[k] : DERIVED_SRC_CONST;
        }
#pragma unroll
        for(int j = 0; j < RV_PER_LANE; j++)
            v[j] = (w[j] & ~DERIVED_SRC_CONJ) < nsrc ? in[w[j] & ~DERIVED_SRC_CONJ] : V{};
#pragma unroll
        for(int j = 0; j < RV_PER_LANE; j++)
        {
            const long long k = k0 + (long long)j * RV_BLOCK;
            if(k < count && (w[j] & ~DERIVED_SRC_CONJ) < nsrc)
                out[k] = (w[j] & DERIVED_SRC_CONJ) ? rv_conj(v[j]) : v[j];
        }
    }

    __global__ __launch_bounds__(256) void rv_iota_kernel(aoclsparse_int count, int *__restrict__ out)
    {
        const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
        if(k < count)
            out[k] = (int)k;
    }

    __global__ __launch_bounds__(256) void rv_compose_kernel(aoclsparse_int count, aoclsparse_int nperm, const int *__restrict__ perm,
                                                             int *map)
    {
        const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
        if(k >= count)
            return;
        const int q = map[k];
        map[k]      = q < 0 || nperm <= 0 ? -1 : perm[min(q, nperm - 1)];
    }

    __global__ __launch_bounds__(256) void rv_diag_map_kernel(aoclsparse_int m, aoclsparse_int mn, int base, aoclsparse_int total,
                                                              const aoclsparse_int *__restrict__ idiag,
                                                              const aoclsparse_int *__restrict__ iurow, int *__restrict__ out)
    {
        const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
        if(i >= m)
            return;
        const int d = idiag[i] - base;
        out[i]      = i < mn && iurow[i] == idiag[i] + 1 && d >= 0 && d < total ? d : -1;
    }

    template <typename V>
    void rv_launch_gather(hipStream_t s, long long count, int nsrc, const int *map, const void *in, void *out, bool conj)
    {
        const unsigned grid = (unsigned)((count + RV_TILE - 1) / RV_TILE);
        if(conj)
            hipLaunchKernelGGL((rv_gather_kernel<V, true>), dim3(grid), dim3(RV_BLOCK), 0, s, count, nsrc, map, static_cast<const V *>(in),
                               static_cast<V *>(out));
        else
            hipLaunchKernelGGL((rv_gather_kernel<V, false>), dim3(grid), dim3(RV_BLOCK), 0, s, count, nsrc, map, static_cast<const V *>(in),
                               static_cast<V *>(out));
    }
} // namespace

aoclsparse_status launch_revalue_gather(hipStream_t s, long long count, long long nsrc, const int *map, const void *in, void *out,
                                        size_t vsize, bool conj)
{
    if(count <= 0)
        return aoclsparse_status_success;
    if(!map || !in || !out || (conj && vsize == 4) || nsrc > 0x7fffffffll)
        return aoclsparse_status_internal_error;
    const int ns = (int)std::max(nsrc, 0ll); // (a map's positions are ints: so is the size of what they index)
    switch(vsize)
    {
    case 4:
        rv_launch_gather<unsigned int>(s, count, ns, map, in, out, false);
        break;
    case 8:
        rv_launch_gather<unsigned long long>(s, count, ns, map, in, out, conj);
        break;
    case 16:
        rv_launch_gather<Item16>(s, count, ns, map, in, out, conj);
        break;
    default:
        return aoclsparse_status_not_implemented;
    }
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

aoclsparse_status launch_revalue_gather_flagged(hipStream_t s, long long count, long long nsrc, const unsigned *map, const void *in,
                                                void *out, size_t vsize)
{
    if(count <= 0)
        return aoclsparse_status_success;
    if(!map || !in || !out || nsrc > 0x7fffffffll)
        return aoclsparse_status_internal_error;
    const unsigned ns   = (unsigned)std::max(nsrc, 0ll);
    const unsigned grid = (unsigned)((count + RV_TILE - 1) / RV_TILE);
    switch(vsize)
    {
    case 4:
        hipLaunchKernelGGL((rv_gather_flagged_kernel<unsigned int>), dim3(grid), dim3(RV_BLOCK), 0, s, count, ns, map,
                           static_cast<const unsigned int *>(in), static_cast<unsigned int *>(out));
        break;
    case 8:
        hipLaunchKernelGGL((rv_gather_flagged_kernel<unsigned long long>), dim3(grid), dim3(RV_BLOCK), 0, s, count, ns, map,
                           static_cast<const unsigned long long *>(in), static_cast<unsigned long long *>(out));
        break;
    case 16:
        hipLaunchKernelGGL((rv_gather_flagged_kernel<Item16>), dim3(grid), dim3(RV_BLOCK), 0, s, count, ns, map,
                           static_cast<const Item16 *>(in), static_cast<Item16 *>(out));
        break;
    default:
        return aoclsparse_status_not_implemented;
    }
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

aoclsparse_status launch_revalue_iota(hipStream_t s, aoclsparse_int count, int *out)
{
    if(count > 0)
        hipLaunchKernelGGL(rv_iota_kernel, dim3((unsigned)(((long long)count + 255) / 256)), dim3(256), 0, s, count, out);
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

aoclsparse_status launch_revalue_compose(hipStream_t s, aoclsparse_int count, aoclsparse_int nperm, const int *perm, int *map)
{
    if(count > 0)
        hipLaunchKernelGGL(rv_compose_kernel, dim3((unsigned)(((long long)count + 255) / 256)), dim3(256), 0, s, count, nperm, perm, map);
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

aoclsparse_status launch_revalue_diag_map(hipStream_t s, aoclsparse_int m, aoclsparse_int n, int base, aoclsparse_int total,
                                          const aoclsparse_int *idiag, const aoclsparse_int *iurow, int *out)
{
    if(m > 0)
        hipLaunchKernelGGL(rv_diag_map_kernel, dim3((unsigned)(((long long)m + 255) / 256)), dim3(256), 0, s, m, std::min(m, n), base,
                           total, idiag, iurow, out);
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

} // namespace mi355
