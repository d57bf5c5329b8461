// derived_kernels.hip -- the operator of a symmetric, Hermitian or triangular descriptor, built in HBM from the clean CSR
// (aoclsparse_mi355_build_operator_device, device_handle_api.cpp).
//
// derived.cpp: build_derived is the specification -- a serial host loop that writes, for every row of the result, the strict
// triangle's entries of that row (direct), D' and the strict entries (r, i) of other rows as (i, r) (mirror), so that the row is in
// ascending column order:   lower fill: [direct] [diag] [mirror]      upper fill: [mirror] [diag] [direct]
// and the mirrored entries of a row in the order the loop visits them: ascending position in the clean arrays.  The same arrays,
// bit for bit, come from these stages:
//   dv_mirror_count     per clean row its strict entries: an integer atomic on the counter of the entry's column (any order)
//   dv_row_count        per result row direct + diag + mirror, the longest mirrored segment, the list of segments of 33 .. 2,048
//   launch_spg_scan     the row pointer
//   dv_fill_direct      the direct entries and the diagonal at the places the counts give: columns and SOURCE positions, the one
//                       of a unit diagonal; where the row's mirrored segment starts
//   dv_mirror_scatter   the stable transpose of the strict triangle: an entry lands at an atomic cursor of its column together
//                       with its clean position; dv_sort_short / dv_sort_wave then put every segment into ascending position,
//                       which is build_derived's visit order (positions are distinct; repeated columns of a row keep their order)
//   launch_revalue_gather_flagged   the values through the source map just written (revalue_kernels.hip): the pass a later
//                       ?revalue_device runs again with new inputs
// A lane per row; a row of more than DV_ROW_WAVE entries is walked by its wavefront (transpose_kernels.hip: tr_count_kernel).  The
// two sorters are those of transpose_kernels.hip over (position, row) pairs; a mirrored segment of more than DV_WAVE_CAP entries
// declines the whole build before anything but counters is allocated.  Every index read from the clean arrays is checked against
// the result's rows before it addresses anything, and every scattered position against the total.
#include "internal.hpp"

#include <hip/hip_runtime.h>

#include <limits>

#define MI355_TRY(expr)                            \
    do                                             \
    {                                              \
        aoclsparse_status st__ = (expr);           \
        if(st__ != aoclsparse_status_success)      \
            return st__;                           \
    } while(0)

namespace mi355
{

namespace
{
    constexpr int DV_ROW_WAVE  = 128; // rows longer than this are walked by a wavefront
    constexpr int DV_SHORT_CAP = 32; // mirrored segments of up to this many entries are sorted by one lane
    constexpr int DV_WAVE_CAP  = 2048; // ... of up to this many by a wavefront in LDS; a longer one declines the build

    struct DvShape
    {
        int      m, rows, dim, base; // rows of the clean CSR and of the result; min(m, n)
        int      upper, direct, mirror, diag; // diag: aoclsparse_diag_type
        unsigned conj; // DERIVED_SRC_CONJ when the mirrored half is conjugated
    };

    // the strict triangle of clean row i: positions [lo, hi), 0-based
    __device__ __forceinline__ void dv_strict(const DvShape &g, int i, const aoclsparse_int *ptr, const aoclsparse_int *idiag,
                                              const aoclsparse_int *iurow, int &lo, int &hi)
    {
        lo = (g.upper ? iurow[i] : ptr[i]) - g.base;
        hi = (g.upper ? ptr[i + 1] : idiag[i]) - g.base;
        hi = max(hi, lo);
    }
    __device__ __forceinline__ bool dv_has_diag(const DvShape &g, int r, const aoclsparse_int *idiag, const aoclsparse_int *iurow)
    {
        if(r >= g.dim || g.diag == (int)aoclsparse_diag_type_zero)
            return false;
        return g.diag == (int)aoclsparse_diag_type_unit || iurow[r] == idiag[r] + 1;
    }

    // f(p, i) for every strict position p of the clean rows i this workgroup holds: a lane per row, a wavefront per long row
    template <typename F>
    __device__ __forceinline__ void dv_for_strict(const DvShape &g, const aoclsparse_int *ptr, const aoclsparse_int *idiag,
                                                  const aoclsparse_int *iurow, F f)
    {
        const int i  = blockIdx.x * 256 + threadIdx.x;
        int       lo = 0, hi = 0;
        if(i < g.m)
            dv_strict(g, i, ptr, idiag, iurow, lo, hi);
        const bool lng = hi - lo > DV_ROW_WAVE;
        if(!lng)
            for(int p = lo; p < hi; p++)
                f(p, i);
        unsigned long long mask = __ballot(lng);
        while(mask)
        {
            const int l = __builtin_ctzll(mask);
            mask &= mask - 1;
            const int ls = __builtin_amdgcn_readlane(lo, l), le = __builtin_amdgcn_readlane(hi, l);
            const int li = __builtin_amdgcn_readlane(i, l);
            for(int p = ls + (int)(threadIdx.x & 63); p < le; p += 64)
                f(p, li);
        }
    }

    __global__ __launch_bounds__(256) void dv_mirror_count_kernel(DvShape g, const aoclsparse_int *__restrict__ ptr,
                                                                  const aoclsparse_int *__restrict__ idiag,
                                                                  const aoclsparse_int *__restrict__ iurow,
                                                                  const aoclsparse_int *__restrict__ ind, int *mcnt)
    {
        dv_for_strict(g, ptr, idiag, iurow, [&](int p, int) {
            const int c = ind[p] - g.base;
            if((unsigned)c < (unsigned)g.rows)
                atomicAdd(&mcnt[c], 1);
        });
    }

    // small[0] = the longest mirrored segment, small[1] = segments of DV_SHORT_CAP + 1 .. DV_WAVE_CAP entries (listed in mid)
    __global__ __launch_bounds__(256) void dv_row_count_kernel(DvShape g, const aoclsparse_int *__restrict__ ptr,
                                                               const aoclsparse_int *__restrict__ idiag,
                                                               const aoclsparse_int *__restrict__ iurow, const int *__restrict__ mcnt,
                                                               int *__restrict__ cnt, int *__restrict__ mid, unsigned int *small)
    {
        const int r = blockIdx.x * 256 + threadIdx.x;
        if(r >= g.rows)
            return;
        int lo = 0, hi = 0;
        if(g.direct && r < g.m)
            dv_strict(g, r, ptr, idiag, iurow, lo, hi);
        const int mc = g.mirror ? mcnt[r] : 0;
        cnt[r]       = (hi - lo) + (dv_has_diag(g, r, idiag, iurow) ? 1 : 0) + mc;
        if(mc > DV_SHORT_CAP)
        {
            atomicMax(&small[0], (unsigned)mc);
            if(mc <= DV_WAVE_CAP)
                mid[atomicAdd(&small[1], 1u)] = r;
        }
    }

    struct alignas(16) DvOne
    {
        unsigned long long a, b; // the bits of the value 1 (the first vsize bytes)
    };

    // the direct entries and the diagonal of every result row; mstart[r] = where its mirrored segment starts
    __global__ __launch_bounds__(256) void dv_fill_direct_kernel(DvShape g, const aoclsparse_int *__restrict__ ptr,
                                                                 const aoclsparse_int *__restrict__ idiag,
                                                                 const aoclsparse_int *__restrict__ iurow,
                                                                 const aoclsparse_int *__restrict__ ind, const int *__restrict__ mcnt,
                                                                 const aoclsparse_int *__restrict__ optr, long long total,
                                                                 aoclsparse_int *__restrict__ oind, unsigned *__restrict__ osrc,
                                                                 void *__restrict__ oval, int vsize, DvOne one, int *__restrict__ mstart)
    {
        const int  r   = blockIdx.x * 256 + threadIdx.x;
        const bool act = r < g.rows;
        int        lo = 0, hi = 0, ds = 0;
        if(act)
        {
            if(g.direct && r < g.m)
                dv_strict(g, r, ptr, idiag, iurow, lo, hi);
            const int  o = optr[r], mc = g.mirror ? mcnt[r] : 0, nd = hi - lo;
            const bool hd = dv_has_diag(g, r, idiag, iurow);
            const int  dp = g.upper ? o + mc : o + nd; // the diagonal's place
            ds        = g.upper ? o + mc + (hd ? 1 : 0) : o;
            mstart[r] = g.upper ? o : o + nd + (hd ? 1 : 0);
            if(hd && dp < total)
            {
                oind[dp] = r;
                if(g.diag == (int)aoclsparse_diag_type_unit)
                {
                    osrc[dp] = DERIVED_SRC_CONST;
                    if(vsize == 4)
                        static_cast<unsigned *>(oval)[dp] = (unsigned)one.a;
                    else if(vsize == 8)
                        static_cast<unsigned long long *>(oval)[dp] = one.a;
                    else
                        static_cast<DvOne *>(oval)[dp] = one;
                }
                else
                    osrc[dp] = (unsigned)(idiag[r] - g.base);
            }
        }
        const bool lng = hi - lo > DV_ROW_WAVE;
        if(!lng)
            for(int k = 0; k < hi - lo; k++)
                if(ds + k < total)
                    oind[ds + k] = ind[lo + k] - g.base, osrc[ds + k] = (unsigned)(lo + k);
        unsigned long long mask = __ballot(lng);
        while(mask)
        {
            const int l = __builtin_ctzll(mask);
            mask &= mask - 1;
            const int ls = __builtin_amdgcn_readlane(lo, l), le = __builtin_amdgcn_readlane(hi, l);
            const int ld = __builtin_amdgcn_readlane(ds, l);
            for(int k = (int)(threadIdx.x & 63); k < le - ls; k += 64)
                if(ld + k < total)
                    oind[ld + k] = ind[ls + k] - g.base, osrc[ld + k] = (unsigned)(ls + k);
        }
    }

    __global__ __launch_bounds__(256) void dv_mirror_scatter_kernel(DvShape g, const aoclsparse_int *__restrict__ ptr,
                                                                    const aoclsparse_int *__restrict__ idiag,
                                                                    const aoclsparse_int *__restrict__ iurow,
                                                                    const aoclsparse_int *__restrict__ ind,
                                                                    const int *__restrict__ mstart, const int *__restrict__ mcnt,
                                                                    int *cursor, long long total, aoclsparse_int *__restrict__ oind,
                                                                    unsigned *__restrict__ osrc)
    {
        dv_for_strict(g, ptr, idiag, iurow, [&](int p, int i) {
            const int c = ind[p] - g.base;
            if((unsigned)c >= (unsigned)g.rows)
                return;
            const int k = atomicAdd(&cursor[c], 1);
            const int q = mstart[c] + k;
            if(k < mcnt[c] && q >= 0 && q < total)
                osrc[q] = (unsigned)p | g.conj, oind[q] = i;
        });
    }

    // segments of <= DV_SHORT_CAP entries: a lane per result row, insertion sort by position (the arrival order is nearly sorted;
    // the conjugation bit is the same in every entry of a segment, so the words compare as the positions do)
    __global__ __launch_bounds__(256) void dv_sort_short_kernel(aoclsparse_int rows, const int *__restrict__ mstart,
                                                                const int *__restrict__ mcnt, long long total, unsigned *osrc,
                                                                aoclsparse_int *oind)
    {
        const int r = blockIdx.x * 256 + threadIdx.x;
        if(r >= rows)
            return;
        const int s = mstart[r], len = mcnt[r];
        if(len > DV_SHORT_CAP || s < 0 || (long long)s + len > total)
            return;
        const int e = s + len;
        for(int a = s + 1; a < e; a++)
        {
            const unsigned kp = osrc[a];
            const int      kr = oind[a];
            int            b  = a - 1;
            while(b >= s && osrc[b] > kp)
            {
                osrc[b + 1] = osrc[b], oind[b + 1] = oind[b];
                b--;
            }
            osrc[b + 1] = kp, oind[b + 1] = kr;
        }
    }

    // segments of DV_SHORT_CAP + 1 .. DV_WAVE_CAP entries: a wavefront per listed row; positions are distinct, so an entry's place is
    // the number of smaller positions in the segment
    __global__ __launch_bounds__(64) void dv_sort_wave_kernel(aoclsparse_int nmid, aoclsparse_int rows, const int *__restrict__ mid,
                                                              const int *__restrict__ mstart, const int *__restrict__ mcnt,
                                                              long long total, unsigned *osrc, aoclsparse_int *oind)
    {
        __shared__ unsigned s_pos[DV_WAVE_CAP];
        __shared__ int      s_row[DV_WAVE_CAP];
        const int           r = mid[blockIdx.x];
        if((unsigned)r >= (unsigned)rows)
            return;
        const int s = mstart[r], len = mcnt[r], lane = threadIdx.x;
        if(len <= DV_SHORT_CAP || len > DV_WAVE_CAP || s < 0 || (long long)s + len > total)
            return;
        for(int t = lane; t < len; t += 64)
            s_pos[t] = osrc[s + t], s_row[t] = oind[s + t];
        __syncthreads();
        for(int t = lane; t < len; t += 64)
        {
            const unsigned mine = s_pos[t];
            int            rank = 0;
            for(int u = 0; u < len; u++)
                rank += s_pos[u] < mine;
            osrc[s + rank] = mine, oind[s + rank] = s_row[t];
        }
    }

    aoclsparse_status derived_device_run(hipStream_t s, const DerivedDeviceIn &in, DeviceBuffer &optr_b, DeviceBuffer &oind_b,
                                         DeviceBuffer &oval_b, DeviceBuffer &osrc_b, aoclsparse_int *nnz_out)
    {
        const bool sym = in.type != aoclsparse_matrix_type_triangular;
        DvShape    g{};
        g.m = in.m, g.base = in.base, g.dim = std::min(in.m, in.n);
        g.rows   = (sym || !in.transposed) ? in.m : in.n;
        g.upper  = in.upper, g.diag = (int)in.diag;
        g.direct = sym || !in.transposed, g.mirror = sym || in.transposed;
        g.conj   = in.type == aoclsparse_matrix_type_hermitian ? DERIVED_SRC_CONJ : 0u;
        if(g.conj && in.vsize == 4)
            return aoclsparse_status_internal_error;
        const aoclsparse_int rows = g.rows;
        const size_t         rb   = sizeof(int) * (size_t)std::max<aoclsparse_int>(rows, 1);
        DeviceBuffer         mcnt, cnt, cursor, mid, small, scan;
        // (declared behind the temporaries: whatever way out is taken, the stream first finishes what was enqueued on them)
        struct DrainOnExit
        {
            hipStream_t s;
            ~DrainOnExit()
            {
                if(hipStreamSynchronize(s) != hipSuccess)
                    (void)hipGetLastError();
            }
        } drain{s};
        MI355_TRY(mcnt.alloc(rb));
        MI355_TRY(cnt.alloc(rb));
        MI355_TRY(mid.alloc(rb));
        MI355_TRY(small.alloc(64));
        MI355_TRY(scan.alloc(spg_scan_scratch_bytes(rows)));
        MI355_TRY(optr_b.alloc(sizeof(aoclsparse_int) * ((size_t)rows + 1)));
        MI355_HIP_TRY(hipMemsetAsync(mcnt.ptr, 0, rb, s));
        MI355_HIP_TRY(hipMemsetAsync(small.ptr, 0, 64, s));
        const unsigned gm = (unsigned)(((long long)in.m + 255) / 256), gr = (unsigned)(((long long)rows + 255) / 256);
        if(g.mirror && in.m > 0)
            hipLaunchKernelGGL(dv_mirror_count_kernel, dim3(gm), dim3(256), 0, s, g, in.ptr, in.idiag, in.iurow, in.ind, mcnt.as<int>());
        hipLaunchKernelGGL(dv_row_count_kernel, dim3(gr), dim3(256), 0, s, g, in.ptr, in.idiag, in.iurow, mcnt.as<const int>(),
                           cnt.as<int>(), mid.as<int>(), small.as<unsigned int>());
        MI355_HIP_TRY(hipGetLastError());
        long long *total_dev = nullptr, total = 0;
        MI355_TRY(launch_spg_scan(s, rows, cnt.as<const int>(), optr_b.as<aoclsparse_int>(), scan.as<long long>(), &total_dev));
        unsigned int h_small[2] = {0, 0};
        MI355_HIP_TRY(hipMemcpyAsync(&total, total_dev, sizeof(total), hipMemcpyDeviceToHost, s));
        MI355_HIP_TRY(hipMemcpyAsync(h_small, small.ptr, sizeof(h_small), hipMemcpyDeviceToHost, s));
        MI355_HIP_TRY(hipStreamSynchronize(s));
        if(h_small[0] > (unsigned)DV_WAVE_CAP) // a mirrored segment the segment sort does not take: the host builds this operator
            return aoclsparse_status_not_implemented;
        if(total < 0 || total > (long long)std::numeric_limits<aoclsparse_int>::max() - 1)
            return aoclsparse_status_invalid_size;
        const long long nmax = (long long)in.nnz + g.dim; // every strict entry once or twice, a diagonal entry per row
        if(total > 2 * nmax || h_small[1] > (unsigned)rows)
            return aoclsparse_status_internal_error;
        // accepted: the outputs
        const size_t ne = (size_t)std::max<long long>(total, 1);
        MI355_TRY(oind_b.alloc(sizeof(aoclsparse_int) * ne));
        MI355_TRY(oval_b.alloc(in.vsize * ne));
        MI355_TRY(osrc_b.alloc(sizeof(unsigned) * ne));
        MI355_TRY(cursor.alloc(rb));
        MI355_HIP_TRY(hipMemsetAsync(cursor.ptr, 0, rb, s));
        DvOne one{0ull, 0ull};
        if(in.vsize == 4 || (in.vsize == 8 && in.cplx))
            one.a = 0x3f800000ull; // 1.0f, or (1.0f, 0.0f)
        else
            one.a = 0x3ff0000000000000ull; // 1.0, or (1.0, 0.0)
        int *const            mstart = cnt.as<int>(); // (the counts have been scanned: their array holds the segment starts from here on)
        aoclsparse_int *const oind   = oind_b.as<aoclsparse_int>();
        unsigned *const       osrc   = osrc_b.as<unsigned>();
        hipLaunchKernelGGL(dv_fill_direct_kernel, dim3(gr), dim3(256), 0, s, g, in.ptr, in.idiag, in.iurow, in.ind, mcnt.as<const int>(),
                           optr_b.as<const aoclsparse_int>(), total, oind, osrc, oval_b.ptr, (int)in.vsize, one, mstart);
        if(g.mirror && in.m > 0)
        {
            hipLaunchKernelGGL(dv_mirror_scatter_kernel, dim3(gm), dim3(256), 0, s, g, in.ptr, in.idiag, in.iurow, in.ind, mstart,
                               mcnt.as<const int>(), cursor.as<int>(), total, oind, osrc);
            hipLaunchKernelGGL(dv_sort_short_kernel, dim3(gr), dim3(256), 0, s, rows, mstart, mcnt.as<const int>(), total, osrc, oind);
            if(h_small[1] > 0)
                hipLaunchKernelGGL(dv_sort_wave_kernel, dim3(h_small[1]), dim3(64), 0, s, (aoclsparse_int)h_small[1], rows,
                                   mid.as<const int>(), mstart, mcnt.as<const int>(), total, osrc, oind);
        }
        MI355_HIP_TRY(hipGetLastError());
        MI355_TRY(launch_revalue_gather_flagged(s, total, in.nnz, osrc, in.val, oval_b.ptr, in.vsize));
        MI355_HIP_TRY(hipStreamSynchronize(s));
        *nnz_out = (aoclsparse_int)total;
        return aoclsparse_status_success;
    }
} // namespace

aoclsparse_status device_build_derived(hipStream_t s, const DerivedDeviceIn &in, DeviceBuffer &optr, DeviceBuffer &oind,
                                       DeviceBuffer &oval, DeviceBuffer &osrc, aoclsparse_int *nnz_out)
{
    if(in.m <= 0 || in.n <= 0 || !in.ptr || !in.ind || !in.val || !in.idiag || !in.iurow || !nnz_out
       || (in.vsize != 4 && in.vsize != 8 && in.vsize != 16))
        return aoclsparse_status_internal_error;
    const aoclsparse_status st = derived_device_run(s, in, optr, oind, oval, osrc, nnz_out);
    if(st != aoclsparse_status_success)
        optr.release(), oind.release(), oval.release(), osrc.release();
    return st;
}

} // namespace mi355
