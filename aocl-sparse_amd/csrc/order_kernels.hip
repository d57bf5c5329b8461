// order_kernels.hip -- every row of a CSR that lives in HBM into ascending column order, stably, in place (round 23).
//
// Reference: the per-row std::stable_sort of aoclsparse_order_mat (here formats_api.cpp: sort_rows): a row that is ascending already
// is left alone, every other row is sorted by column, entries with equal columns keep their order.  The sort here is segmented
// (a row is a segment) and its key is (column, position in the row): positions are distinct, so there are no ties and any correct
// sort of those keys IS the stable one -- the result is a pure function of the input, whichever path a row takes.  Values are
// moved as items of 4, 8 or 16 bytes and never computed with.
//
//   (1) ord_flag_kernel   one pass over col_idx: key[i] = the length of row i when it holds an adjacent descent, 0 otherwise.
//                         A matrix whose rows are all ascending ends here.
//   (2) the rows to sort are binned by key with the bins of the SpGEMM analysis (launch_spg_hist / launch_spg_order, `fill` bins:
//       <= 32 | <= 256 | <= 2,048 | longer).  The two thresholds are AOCLSPARSE_MI355_ORDER_SHORT_MAX / _ORDER_LDS_MAX.
//   (3) short rows (<= 32): a lane per row, insertion sort in place (strict >, hence stable).  No list is needed: the lane looks at
//       key[i].
//   (4) medium rows (33 .. 2,048): a workgroup per listed row (one wavefront and 256 slots up to 256 entries, four wavefronts and
//       2,048 slots above) loads the row's 64-bit (column, position) keys and its values into LDS, sorts the keys with a bitonic
//       network -- log^2 steps per entry, not a rank by counting -- and writes columns and values back coalesced, the values
//       gathered from LDS by position.  2,048 x (8 + 16) bytes = 48 KiB for double complex: of the 160 KiB of a CU that leaves
//       room for three workgroups.
//   (5) long rows: their entries ALONE are compacted -- (place of the row in the list, column) per entry -- and go through the
//       radix passes of the triplet sort (device_sort_pairs, coo_sort_kernels.hip), which never look at a row's length: one row
//       may hold every entry.  The order by (place, column) is row-major over the same segments, so sorted entry q of the
//       compacted sequence belongs at offset q - off[j] of row j; columns and values are gathered into a compacted copy and put
//       back.  The list order of launch_spg_order depends on the arrival of workgroups; the result does not: the key is the place
//       in the list the offsets were made from.
// Integer atomics count rows; no float atomics, vector stores only.
#include "internal.hpp"

#include <hip/hip_runtime.h>

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
    constexpr int ORD_SHORT_MAX = AOCLSPARSE_MI355_ORDER_SHORT_MAX;
    constexpr int ORD_LDS_MAX   = AOCLSPARSE_MI355_ORDER_LDS_MAX;
    constexpr int ORD_WAVE_MAX  = 256; // medium rows up to this length: one wavefront, 256 LDS slots
    constexpr int ORD_ROW_WAVE  = 64; // the flag pass walks rows longer than this with the whole wavefront

    struct alignas(16) Item16
    {
        unsigned long long a, b;
    };

    // the bounds of row i, clamped into [0, nnz] (a handle's row_ptr is checked when it is created: the clamp costs nothing)
    __device__ __forceinline__ void ord_row(const aoclsparse_int *__restrict__ ptr, int i, int base, aoclsparse_int nnz, int &s, int &e)
    {
        s = min(max(ptr[i] - base, 0), nnz);
        e = min(max(ptr[i + 1] - base, s), nnz);
    }

    // (1) key[i] = e - s when ind[p - 1] > ind[p] for some p in (s, e), 0 otherwise.  flags[0]: some short row has to be sorted;
    // flags[1]: how many rows have to be sorted
    __global__ __launch_bounds__(256) void ord_flag_kernel(aoclsparse_int m, aoclsparse_int nnz, int base,
                                                           const aoclsparse_int *__restrict__ ptr,
                                                           const aoclsparse_int *__restrict__ ind, int *__restrict__ key,
                                                           unsigned int *flags)
    {
        const long long gi   = (long long)blockIdx.x * 256 + threadIdx.x;
        const bool      act  = gi < m;
        const int       i    = act ? (int)gi : 0;
        const int       lane = threadIdx.x & 63;
        int             s = 0, e = 0;
        if(act)
            ord_row(ptr, i, base, nnz, s, e);
        const bool lng  = e - s > ORD_ROW_WAVE;
        bool       desc = false;
        if(!lng && e - s > 1)
        {
            int prev = ind[s];
            for(int p = s + 1; p < e; p++)
            {
                const int c = ind[p];
                desc |= prev > c;
                prev = c;
            }
        }
        unsigned long long mask = __ballot(lng);
        while(mask)
        {
            const int l = __builtin_ctzll(mask);
            mask &= mask - 1;
            const int ls = __builtin_amdgcn_readlane(s, l), le = __builtin_amdgcn_readlane(e, l);
            bool      d  = false;
            for(int p = ls + 1 + lane; p < le; p += 64)
                d |= ind[p - 1] > ind[p];
            const bool any = __ballot(d) != 0;
            if(lane == l)
                desc = any;
        }
        if(act)
            key[i] = desc ? e - s : 0;
        const unsigned long long moved = __ballot(desc), shrt = __ballot(desc && e - s <= ORD_SHORT_MAX);
        if(lane == 0 && moved)
        {
            if(shrt)
                atomicOr(&flags[0], 1u);
            atomicAdd(&flags[1], (unsigned)__popcll(moved));
        }
    }

    // (3) rows with 2 <= key <= ORD_SHORT_MAX: a lane per row, insertion sort in place
    template <typename V>
    __global__ __launch_bounds__(256) void ord_short_kernel(aoclsparse_int m, aoclsparse_int nnz, int base,
                                                            const aoclsparse_int *__restrict__ ptr, const int *__restrict__ key,
                                                            aoclsparse_int *ind, V *val)
    {
        const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
        if(gi >= m)
            return;
        const int i = (int)gi, k = key[i];
        if(k < 2 || k > ORD_SHORT_MAX)
            return;
        int s, e;
        ord_row(ptr, i, base, nnz, s, e);
        if(e - s != k) // (never: the key was made from this row_ptr)
            return;
        aoclsparse_int *const ri = ind + s;
        V *const              rv = val + s;
        for(int a = 1; a < k; a++)
        {
            const int kc = ri[a];
            if(ri[a - 1] <= kc)
                continue;
            const V kv = rv[a];
            int     b  = a - 1;
            while(b >= 0 && ri[b] > kc)
            {
                ri[b + 1] = ri[b], rv[b + 1] = rv[b];
                b--;
            }
            ri[b + 1] = kc, rv[b + 1] = kv;
        }
    }

    // (4) a workgroup of THREADS lanes per listed row of at most CAP entries: bitonic sort of (column, position) keys in LDS.  The
    // column is stored with its sign bit flipped, so that the unsigned order of the keys is the signed order of the columns.
    template <typename V, int CAP, int THREADS>
    __global__ __launch_bounds__(THREADS) void ord_lds_kernel(aoclsparse_int nrows, const aoclsparse_int *__restrict__ rows,
                                                              aoclsparse_int m, aoclsparse_int nnz, int base,
                                                              const aoclsparse_int *__restrict__ ptr, aoclsparse_int *ind, V *val)
    {
        __shared__ unsigned long long s_key[CAP];
        __shared__ V                  s_val[CAP];
        const int                     r = rows[blockIdx.x], tid = threadIdx.x;
        if((unsigned)r >= (unsigned)m) // (never: the list holds rows)
            return;
        int s, e;
        ord_row(ptr, r, base, nnz, s, e);
        const int len = e - s;
        if(len < 2 || len > CAP) // (never: the bins say otherwise)
            return;
        int n2 = 64;
        while(n2 < len)
            n2 <<= 1;
        for(int t = tid; t < n2; t += THREADS)
        {
            unsigned long long k = ~0ull; // padding: behind every entry
            if(t < len)
            {
                k        = ((unsigned long long)((unsigned)ind[s + t] ^ 0x80000000u) << 32) | (unsigned)t;
                s_val[t] = val[s + t];
            }
            s_key[t] = k;
        }
        __syncthreads();
        for(int k = 2; k <= n2; k <<= 1)
            for(int j = k >> 1; j > 0; j >>= 1)
            {
                for(int t = tid; t < n2; t += THREADS)
                {
                    const int u = t ^ j;
                    if(u > t)
                    {
                        const unsigned long long a = s_key[t], b = s_key[u];
                        if((a > b) == ((t & k) == 0))
                            s_key[t] = b, s_key[u] = a;
                    }
                }
                __syncthreads();
            }
        for(int t = tid; t < len; t += THREADS)
        {
            const unsigned long long k = s_key[t];
            const unsigned           p = (unsigned)k;
            if(p < (unsigned)len) // (always: the first len keys are the entries)
            {
                ind[s + t] = (aoclsparse_int)((unsigned)(k >> 32) ^ 0x80000000u);
                val[s + t] = s_val[p];
            }
        }
    }

    // (5) the long row that holds compacted entry q: off[j] <= q < off[j + 1] (off[0] = 0, off[nlong] = the compacted count)
    __device__ __forceinline__ int ord_long_find(const aoclsparse_int *__restrict__ off, int nlong, int q)
    {
        int lo = 0, hi = nlong; // off[lo] <= q < off[hi]
        while(hi - lo > 1)
        {
            const int mid = (lo + hi) >> 1;
            if(off[mid] <= q)
                lo = mid;
            else
                hi = mid;
        }
        return lo;
    }

    // major[q] = the place j of the entry's row in the list, minor[q] = its column (0-based)
    __global__ __launch_bounds__(256) void ord_long_keys_kernel(aoclsparse_int total, int nlong, const aoclsparse_int *__restrict__ rows,
                                                                const aoclsparse_int *__restrict__ off, aoclsparse_int m,
                                                                aoclsparse_int nnz, int base, const aoclsparse_int *__restrict__ ptr,
                                                                const aoclsparse_int *__restrict__ ind,
                                                                aoclsparse_int *__restrict__ major, aoclsparse_int *__restrict__ minor)
    {
        const long long gq = (long long)blockIdx.x * 256 + threadIdx.x;
        if(gq >= total)
            return;
        const int q = (int)gq, j = ord_long_find(off, nlong, q), r = rows[j];
        int       s = 0, e = 0, c = 0;
        if((unsigned)r < (unsigned)m)
            ord_row(ptr, r, base, nnz, s, e);
        const int t = q - off[j];
        if(t >= 0 && s + t < e) // (always: off is the prefix sum of these rows' lengths)
            c = ind[s + t] - base;
        major[q] = j, minor[q] = c;
    }

    // sorted entry q of the compacted sequence: the column and the value of compacted entry perm[q], which lies in the same row
    template <typename V>
    __global__ __launch_bounds__(256) void ord_long_gather_kernel(aoclsparse_int total, int nlong, const aoclsparse_int *__restrict__ rows,
                                                                  const aoclsparse_int *__restrict__ off, const int *__restrict__ perm,
                                                                  aoclsparse_int m, aoclsparse_int nnz, int base,
                                                                  const aoclsparse_int *__restrict__ ptr,
                                                                  const aoclsparse_int *__restrict__ ind, const V *__restrict__ val,
                                                                  aoclsparse_int *__restrict__ tind, V *__restrict__ tval)
    {
        const long long gq = (long long)blockIdx.x * 256 + threadIdx.x;
        if(gq >= total)
            return;
        const int q = (int)gq, j = ord_long_find(off, nlong, q), r = rows[j];
        int       s = 0, e = 0;
        if((unsigned)r < (unsigned)m)
            ord_row(ptr, r, base, nnz, s, e);
        const int t = perm[q] - off[j];
        if(t >= 0 && s + t < e) // (always: the sort keeps the entries of place j together, in place j's segment)
            tind[q] = ind[s + t], tval[q] = val[s + t];
        else
            tind[q] = 0, tval[q] = V{};
    }

    template <typename V>
    __global__ __launch_bounds__(256) void ord_long_put_kernel(aoclsparse_int total, int nlong, const aoclsparse_int *__restrict__ rows,
                                                               const aoclsparse_int *__restrict__ off, aoclsparse_int m,
                                                               aoclsparse_int nnz, int base, const aoclsparse_int *__restrict__ ptr,
                                                               const aoclsparse_int *__restrict__ tind, const V *__restrict__ tval,
                                                               aoclsparse_int *__restrict__ ind, V *__restrict__ val)
    {
        const long long gq = (long long)blockIdx.x * 256 + threadIdx.x;
        if(gq >= total)
            return;
        const int q = (int)gq, j = ord_long_find(off, nlong, q), r = rows[j];
        int       s = 0, e = 0;
        if((unsigned)r < (unsigned)m)
            ord_row(ptr, r, base, nnz, s, e);
        const int t = q - off[j];
        if(t >= 0 && s + t < e)
            ind[s + t] = tind[q], val[s + t] = tval[q];
    }

    template <typename F>
    aoclsparse_status by_item_size(size_t vsize, F &&f)
    {
        if(vsize == 4)
            f((unsigned int)0);
        else if(vsize == 8)
            f((unsigned long long)0);
        else if(vsize == 16)
            f(Item16{});
        else
            return aoclsparse_status_not_implemented;
        return aoclsparse_status_success;
    }

    // Diagnostic (AOCLSPARSE_MI355_TIMING=1, as PhaseTimer): device time from the flag pass to the last kernel
    struct OrderMarks
    {
        hipEvent_t ev[2] = {nullptr, nullptr};
        bool       got[2] = {false, false};
        OrderMarks()
        {
            if(PhaseTimer::on())
                for(hipEvent_t &e : ev)
                    if(hipEventCreate(&e) != hipSuccess)
                        e = nullptr, (void)hipGetLastError();
        }
        ~OrderMarks()
        {
            for(hipEvent_t e : ev)
                if(e)
                    (void)hipEventDestroy(e);
        }
        void record(int k, hipStream_t s)
        {
            if(ev[k])
                got[k] = hipEventRecord(ev[k], s) == hipSuccess;
        }
    };
} // namespace

aoclsparse_status device_order_rows(hipStream_t s, aoclsparse_int m, aoclsparse_int n, aoclsparse_int nnz, int base,
                                    const aoclsparse_int *d_ptr, aoclsparse_int *d_ind, void *d_val, size_t vsize, long long *moved)
{
    if(moved)
        *moved = 0;
    if(m <= 0 || n <= 0 || nnz <= 0)
        return aoclsparse_status_success;
    if(vsize != 4 && vsize != 8 && vsize != 16)
        return aoclsparse_status_not_implemented;
    // the thresholds in the header are the bins of the SpGEMM analysis, which sorts the rows into the lists
    if(spgemm_bin_of(ORD_SHORT_MAX, true) != 0 || spgemm_bin_of(ORD_SHORT_MAX + 1, true) != 1 || spgemm_bin_of(ORD_WAVE_MAX, true) != 1
       || spgemm_bin_of(ORD_WAVE_MAX + 1, true) != 2 || spgemm_bin_of(ORD_LDS_MAX, true) != 2
       || spgemm_bin_of(ORD_LDS_MAX + 1, true) != SPGEMM_BINS - 1)
        return aoclsparse_status_internal_error;
    Runtime                              &rt = Runtime::get();
    std::lock_guard<std::recursive_mutex> sl(rt.stage_lock);
    // every way out first lets the stream finish what was enqueued on the slots: the next holder of the lock may grow (free) them
    struct DrainOnExit
    {
        hipStream_t s;
        ~DrainOnExit()
        {
            if(hipStreamSynchronize(s) != hipSuccess)
                (void)hipGetLastError();
        }
    } drain{s};
    OrderMarks marks;
    void      *p = nullptr;
    MI355_TRY(rt.staging(ORD_SLOT_KEY, sizeof(int) * (size_t)m, &p));
    int *const key_p = static_cast<int *>(p);
    MI355_TRY(rt.staging(ORD_SLOT_SMALL, 256, &p));
    unsigned int *const small_p = static_cast<unsigned int *>(p);
    unsigned int *const d_hist = small_p, *const d_cursor = small_p + 16, *const d_flags = small_p + 32;
    const unsigned      gm     = (unsigned)(((long long)m + 255) / 256);
    MI355_HIP_TRY(hipMemsetAsync(small_p, 0, 256, s));
    marks.record(0, s);
    hipLaunchKernelGGL(ord_flag_kernel, dim3(gm), dim3(256), 0, s, m, nnz, base, d_ptr, d_ind, key_p, d_flags);
    MI355_TRY(launch_spg_hist(s, m, key_p, nullptr, true, d_hist));
    unsigned int hist[SPGEMM_BINS + 1] = {}, flags[2] = {};
    MI355_HIP_TRY(hipMemcpyAsync(hist, d_hist, sizeof(hist), hipMemcpyDeviceToHost, s));
    MI355_HIP_TRY(hipMemcpyAsync(flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost, s));
    MI355_HIP_TRY(hipStreamSynchronize(s));
    if(moved)
        *moved = flags[1];
    long long total_long = 0;
    if(flags[1])
    {
        if(flags[0])
            MI355_TRY(by_item_size(vsize, [&](auto v) {
                using V = decltype(v);
                hipLaunchKernelGGL((ord_short_kernel<V>), dim3(gm), dim3(256), 0, s, m, nnz, base, d_ptr, key_p, d_ind,
                                   static_cast<V *>(d_val));
            }));
        const aoclsparse_int nwave = (aoclsparse_int)hist[1], nwg = (aoclsparse_int)hist[2];
        const aoclsparse_int nlong = (aoclsparse_int)(hist[3] + hist[4]);
        if(nwave + nwg + nlong > 0)
        {
            aoclsparse_int bounds[SPGEMM_BINS + 1];
            bounds[0] = 0;
            for(int b = 0; b < SPGEMM_BINS; b++)
                bounds[b + 1] = bounds[b] + (aoclsparse_int)hist[b];
            MI355_TRY(rt.staging(ORD_SLOT_ORDER, sizeof(aoclsparse_int) * (size_t)m, &p));
            aoclsparse_int *const order_p = static_cast<aoclsparse_int *>(p);
            MI355_TRY(launch_spg_order(s, m, key_p, true, bounds, d_cursor, order_p));
            MI355_TRY(by_item_size(vsize, [&](auto v) {
                using V = decltype(v);
                if(nwave > 0)
                    hipLaunchKernelGGL((ord_lds_kernel<V, ORD_WAVE_MAX, 64>), dim3((unsigned)nwave), dim3(64), 0, s, nwave,
                                       order_p + bounds[1], m, nnz, base, d_ptr, d_ind, static_cast<V *>(d_val));
                if(nwg > 0)
                    hipLaunchKernelGGL((ord_lds_kernel<V, ORD_LDS_MAX, 256>), dim3((unsigned)nwg), dim3(256), 0, s, nwg,
                                       order_p + bounds[2], m, nnz, base, d_ptr, d_ind, static_cast<V *>(d_val));
            }));
            if(nlong > 0)
            {
                const aoclsparse_int *const rows_p = order_p + bounds[3];
                MI355_TRY(rt.staging(ORD_SLOT_LEN, sizeof(int) * (size_t)nlong, &p));
                int *const len_p = static_cast<int *>(p);
                MI355_TRY(rt.staging(ORD_SLOT_OFF, sizeof(aoclsparse_int) * ((size_t)nlong + 1), &p));
                aoclsparse_int *const off_p = static_cast<aoclsparse_int *>(p);
                MI355_TRY(rt.staging(ORD_SLOT_SCAN, spg_scan_scratch_bytes(nlong), &p));
                long long *total_dev = nullptr;
                MI355_TRY(launch_spg_gather(s, nlong, rows_p, key_p, len_p));
                MI355_TRY(launch_spg_scan(s, nlong, len_p, off_p, static_cast<long long *>(p), &total_dev));
                MI355_HIP_TRY(hipMemcpyAsync(&total_long, total_dev, sizeof(total_long), hipMemcpyDeviceToHost, s));
                MI355_HIP_TRY(hipStreamSynchronize(s));
                if(total_long <= 0 || total_long > (long long)nnz)
                    return aoclsparse_status_internal_error;
                const aoclsparse_int total = (aoclsparse_int)total_long;
                const unsigned       gq    = (unsigned)((total_long + 255) / 256);
                MI355_TRY(rt.staging(ORD_SLOT_MAJOR, sizeof(aoclsparse_int) * (size_t)total, &p));
                aoclsparse_int *const major_p = static_cast<aoclsparse_int *>(p);
                MI355_TRY(rt.staging(ORD_SLOT_MINOR, sizeof(aoclsparse_int) * (size_t)total, &p));
                aoclsparse_int *const minor_p = static_cast<aoclsparse_int *>(p);
                MI355_TRY(rt.staging(ORD_SLOT_VAL, vsize * (size_t)total, &p));
                void *const tval_p = p;
                hipLaunchKernelGGL(ord_long_keys_kernel, dim3(gq), dim3(256), 0, s, total, (int)nlong, rows_p, off_p, m, nnz, base, d_ptr,
                                   d_ind, major_p, minor_p);
                const int *perm = nullptr;
                MI355_TRY(device_sort_pairs(s, total, major_p, nlong, minor_p, n, &perm));
                aoclsparse_int *const tind_p = major_p; // (the sort has read the places; from here on: the sorted columns)
                MI355_TRY(by_item_size(vsize, [&](auto v) {
                    using V = decltype(v);
                    hipLaunchKernelGGL((ord_long_gather_kernel<V>), dim3(gq), dim3(256), 0, s, total, (int)nlong, rows_p, off_p, perm, m,
                                       nnz, base, d_ptr, d_ind, static_cast<const V *>(d_val), tind_p, static_cast<V *>(tval_p));
                    hipLaunchKernelGGL((ord_long_put_kernel<V>), dim3(gq), dim3(256), 0, s, total, (int)nlong, rows_p, off_p, m, nnz, base,
                                       d_ptr, tind_p, static_cast<const V *>(tval_p), d_ind, static_cast<V *>(d_val));
                }));
            }
        }
    }
    marks.record(1, s);
    MI355_HIP_TRY(hipGetLastError());
    MI355_HIP_TRY(hipStreamSynchronize(s)); // (the staging slots may be handed to the next caller once the lock is released)
    float ms = 0.f;
    if(marks.got[0] && marks.got[1] && hipEventElapsedTime(&ms, marks.ev[0], marks.ev[1]) == hipSuccess)
        std::fprintf(stderr, "[mi355 timing]     order rows kernels: %8.3f ms, %u rows sorted, %lld entries in long rows\n", ms, flags[1],
                     total_long);
    return aoclsparse_status_success; // (`drain` runs before the lock guard declared above it is released)
}

} // namespace mi355
