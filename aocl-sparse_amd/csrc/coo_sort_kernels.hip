// coo_sort_kernels.hip -- CSR arrays from unordered (row, col, value) triplets in HBM (round 19).
//
// Reference: conversion/aoclsparse_convert.hpp:657-750 (aoclsparse_coo2csr, here formats_api.cpp: coo2csr): count the entries of
// every row, prefix sum, then walk the triplets in order and drop each into the next free slot of its row -- a STABLE sort by row.
// `keep` mode returns exactly that.  `sum` mode sorts by (row, column), stably, and adds every run of equal coordinates from left
// to right in triplet order.
//
// The device transpose (transpose_kernels.hip) sorts by scattering through atomic cursors and repairing every segment afterwards,
// and declines a segment of more than 2,048 entries.  Triplets have rows like that as a matter of course (an arrow matrix, a
// constraint row, a hub node), so the sort here never looks at a row's length: a least-significant-digit radix sort of
// (key, position) pairs with 8-bit digits, ceil(bits(M - 1) / 8) passes over the rows, in `sum` mode ceil(bits(N - 1) / 8) passes
// over the columns in front of them.  One pass:
//   (1) coo_hist_kernel    a workgroup counts the digits of its tile of COO_TILE entries      -> hist[digit * tiles + tile]
//   (2) launch_spg_scan    one exclusive prefix sum over bins x tiles: for (digit, tile) the entries with a smaller digit plus
//                          the entries with this digit in earlier tiles
//   (3) coo_scatter_kernel an entry's place = that + the digit's count in earlier wavefronts of the tile + in earlier rounds of its
//                          own wavefront + its rank among the lanes of its round that hold the same digit
// The rank comes from eight __ballot's, one per digit bit, ANDed into the mask of the lanes with an equal digit, then
// popcount(mask & lanes_below).  That rank -- not the arrival at a cursor -- is what makes a pass stable, and with it the result a
// pure function of the input.  A tile is read in the order (wavefront, round, lane): wavefront w owns entries [w * 64 * COO_ROUNDS,
// (w + 1) * 64 * COO_ROUNDS) of the tile and reads 64 consecutive ones per round.
//
// After the last pass `keep` counts the rows of the sorted keys, scans them into row_ptr (+ base) and gathers columns and values
// once by position.  `sum` flags the head of every run of equal (row, column), scans the flags into output positions, and one lane
// per output entry walks its run in order: v0 + v1, + v2, ... (a run of more than 64 entries is walked by the lane's wavefront,
// which fetches 64 values at a time and adds them in the same order).  No float atomics anywhere; the integer atomics that count
// rows commute exactly.
//
// Round 22: on request the sort's map -- the final positions, in `sum` mode the run starts -- leaves the staging slots in buffers
// that hang on the handle, and device_coo_refresh_values makes the values again from new triplet values with one kernel that reads
// no key and no column: a gather with COO_REFRESH_ILP loads in flight per lane (`keep`), or the creation's own chain
// (coo_run_chain) per run (`sum`).
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
    constexpr int COO_WAVES  = 4; // wavefronts of a workgroup
    constexpr int COO_ROUNDS = 16; // entries a lane takes per pass
    constexpr int COO_TILE   = COO_WAVES * 64 * COO_ROUNDS; // entries a workgroup takes per pass
    static_assert(COO_TILE == AOCLSPARSE_MI355_COO_SORT_TILE, "the header tells the tests where a tile ends");

    // row outside [base, base + m) or column outside [base, base + n): *bad is raised, nothing else happens
    __global__ __launch_bounds__(256) void coo_check_kernel(aoclsparse_int nnz, aoclsparse_int m, aoclsparse_int n, int base,
                                                            const aoclsparse_int *__restrict__ row,
                                                            const aoclsparse_int *__restrict__ col, unsigned int *bad)
    {
        const long long stride = (long long)gridDim.x * 256;
        bool            any    = false;
        for(long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nnz; i += stride)
        {
            const long long r = (long long)row[i] - base, c = (long long)col[i] - base;
            any |= r < 0 || r >= m || c < 0 || c >= n;
        }
        if(any)
            atomicOr(bad, 1u);
    }

    // key[i] = src[i] - base, pos[i] = i: the pairs the first pass reads (and the result when no pass runs: one row, one column)
    __global__ __launch_bounds__(256) void coo_init_kernel(aoclsparse_int nnz, int base, const aoclsparse_int *__restrict__ src,
                                                           int *__restrict__ key, int *__restrict__ pos)
    {
        const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
        if(i < nnz)
            key[i] = src[i] - base, pos[i] = (int)i;
    }

    // key[i] = src[pos[i]] - base: the row keys behind the column passes
    __global__ __launch_bounds__(256) void coo_rekey_kernel(aoclsparse_int nnz, int base, const aoclsparse_int *__restrict__ src,
                                                            const int *__restrict__ pos, int *__restrict__ key)
    {
        const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
        if(i < nnz)
            key[i] = src[pos[i]] - base;
    }

    // the lanes of this wavefront that are valid and hold the digit d (this lane included when it is valid)
    __device__ __forceinline__ unsigned long long coo_match(bool valid, unsigned d)
    {
        unsigned long long mask = __ballot(valid);
#pragma unroll
        for(int b = 0; b < 8; b++)
        {
            const bool               bit = (d >> b) & 1u;
            const unsigned long long bb  = __ballot(bit);
            mask &= bit ? bb : ~bb;
        }
        return mask;
    }

    __device__ __forceinline__ unsigned long long coo_lanes_below(int lane)
    {
        return (1ull << lane) - 1ull;
    }

    // (1): hist[d * tiles + tile] = entries of the tile whose digit is d
    __global__ __launch_bounds__(256) void coo_hist_kernel(aoclsparse_int nnz, const int *__restrict__ key, int shift,
                                                           long long tiles, int *__restrict__ hist)
    {
        __shared__ int  s_cnt[COO_WAVES][256];
        const int       tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
        const long long i0  = (long long)blockIdx.x * COO_TILE + (long long)w * 64 * COO_ROUNDS + lane;
        for(int q = 0; q < COO_WAVES; q++)
            s_cnt[q][tid] = 0;
        __syncthreads();
#pragma unroll 4
        for(int r = 0; r < COO_ROUNDS; r++)
        {
            const long long          i     = i0 + r * 64;
            const bool               valid = i < nnz;
            const unsigned           d     = valid ? ((unsigned)key[i] >> shift) & 255u : 0u;
            const unsigned long long mask  = coo_match(valid, d);
            // one lane per distinct digit of the round adds the whole group: no two lanes touch one counter
            if(valid && (mask & coo_lanes_below(lane)) == 0)
                s_cnt[w][d] += __popcll(mask);
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
        hist[(size_t)tid * (size_t)tiles + blockIdx.x] = (s_cnt[0][tid] + s_cnt[1][tid]) + (s_cnt[2][tid] + s_cnt[3][tid]);
    }

    // (3): offs = the exclusive prefix sum of hist
    __global__ __launch_bounds__(256) void coo_scatter_kernel(aoclsparse_int nnz, const int *__restrict__ key_in,
                                                              const int *__restrict__ pos_in, int shift, long long tiles,
                                                              const aoclsparse_int *__restrict__ offs, int *__restrict__ key_out,
                                                              int *__restrict__ pos_out)
    {
        __shared__ int     s_cnt[COO_WAVES][256];
        const int          tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
        const long long    i0  = (long long)blockIdx.x * COO_TILE + (long long)w * 64 * COO_ROUNDS + lane;
        int                k[COO_ROUNDS], p[COO_ROUNDS];
        unsigned long long mk[COO_ROUNDS];
        for(int q = 0; q < COO_WAVES; q++)
            s_cnt[q][tid] = 0;
#pragma unroll
        for(int r = 0; r < COO_ROUNDS; r++)
        {
            const long long i = i0 + r * 64;
            k[r]              = i < nnz ? key_in[i] : 0;
            p[r]              = i < nnz ? pos_in[i] : 0;
        }
        __syncthreads();
#pragma unroll
        for(int r = 0; r < COO_ROUNDS; r++)
        {
            const bool     valid = i0 + r * 64 < nnz;
            const unsigned d     = ((unsigned)k[r] >> shift) & 255u;
            mk[r]                = coo_match(valid, d);
            if(valid && (mk[r] & coo_lanes_below(lane)) == 0)
                s_cnt[w][d] += __popcll(mk[r]);
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
        {
            // digit tid: where its entries of this tile start, wavefront by wavefront
            int run = offs[(size_t)tid * (size_t)tiles + blockIdx.x];
            for(int q = 0; q < COO_WAVES; q++)
            {
                const int c   = s_cnt[q][tid];
                s_cnt[q][tid] = run;
                run += c;
            }
        }
        __syncthreads();
#pragma unroll
        for(int r = 0; r < COO_ROUNDS; r++)
        {
            const bool     valid = i0 + r * 64 < nnz;
            const unsigned d     = ((unsigned)k[r] >> shift) & 255u;
            const int      below = __popcll(mk[r] & coo_lanes_below(lane));
            int            dst   = 0;
            if(valid)
                dst = s_cnt[w][d] + below; // (0 <= dst < nnz: hist counted exactly these entries)
            __builtin_amdgcn_wave_barrier(); // every lane has read the cursor of its digit before the group's first lane moves it
            if(valid && below == 0)
                s_cnt[w][d] += __popcll(mk[r]);
            __builtin_amdgcn_wave_barrier();
            if(valid)
                key_out[dst] = k[r], pos_out[dst] = p[r];
        }
    }

    // cnt[key[i]]++ (keys are rows in [0, m): checked before anything was sorted)
    __global__ __launch_bounds__(256) void coo_count_kernel(aoclsparse_int nnz, const int *__restrict__ key, int *cnt)
    {
        const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
        if(i < nnz)
            atomicAdd(&cnt[key[i]], 1);
    }

    __global__ __launch_bounds__(256) void coo_add_base_kernel(aoclsparse_int count, int base, aoclsparse_int *ptr)
    {
        const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
        if(i < count)
            ptr[i] += base;
    }

    // out[q] = src[pos[q]]: the columns (4 bytes) and the values (4 / 8 / 8 / 16 bytes) of `keep` mode, the columns of `sum` mode
    template <typename V>
    __global__ __launch_bounds__(256) void coo_gather_kernel(aoclsparse_int nnz, const int *__restrict__ pos, const V *__restrict__ src,
                                                             V *__restrict__ out)
    {
        const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
        if(q < nnz)
            out[q] = src[pos[q]];
    }

    // flag[i] = 1 where sorted entry i opens a run of equal (row, column)
    __global__ __launch_bounds__(256) void coo_flag_kernel(aoclsparse_int nnz, const int *__restrict__ key,
                                                           const aoclsparse_int *__restrict__ scol, int *__restrict__ flag)
    {
        const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
        if(i < nnz)
            flag[i] = i == 0 || key[i] != key[i - 1] || scol[i] != scol[i - 1];
    }

    // runs[o] = where run o starts in the sorted sequence, runs[nout] = nnz (outpos: the exclusive scan of the flags)
    __global__ __launch_bounds__(256) void coo_runs_kernel(aoclsparse_int nnz, aoclsparse_int nout, const int *__restrict__ flag,
                                                           const aoclsparse_int *__restrict__ outpos, int *__restrict__ runs)
    {
        const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
        if(i == 0)
            runs[nout] = nnz;
        if(i < nnz && flag[i] && (unsigned)outpos[i] < (unsigned)nout) // (always: nout is the scan's own total)
            runs[outpos[i]] = (int)i;
    }

    __device__ __forceinline__ float coo_lane_value(float v, int l)
    {
        return __shfl(v, l, 64);
    }
    __device__ __forceinline__ double coo_lane_value(double v, int l)
    {
        return __shfl(v, l, 64);
    }
    __device__ __forceinline__ float2 coo_lane_value(float2 v, int l)
    {
        return make_float2(__shfl(v.x, l, 64), __shfl(v.y, l, 64));
    }
    __device__ __forceinline__ double2 coo_lane_value(double2 v, int l)
    {
        return make_double2(__shfl(v.x, l, 64), __shfl(v.y, l, 64));
    }

    constexpr int COO_RUN_WAVE = 64; // runs longer than this are walked by the lane's whole wavefront

    // The sum of the run [s, e) of sorted entries, for the lane that owns it (act: it owns one): its values from left to right,
    // v0 + v1, + v2, ...  A run of more than COO_RUN_WAVE entries is walked by the wavefront instead: the lanes fetch 64 values
    // at a time, and the same chain is then added from the fetched values in lane order (as one lane's loop a run of a million
    // repeats would be a million dependent loads).  Every lane of the wavefront comes here together.  THE chain: the creation
    // (coo_sum_kernel) and the value refresh (coo_refresh_sum_kernel) both call it, so the two give the same bits.
    template <typename V>
    __device__ __forceinline__ V coo_run_chain(bool act, int s, int e, int lane, const int *__restrict__ pos,
                                               const V *__restrict__ val)
    {
        const bool lng = act && e - s > COO_RUN_WAVE;
        V          acc{};
        if(act && !lng)
        {
            acc = val[pos[s]];
            for(int j = s + 1; j < e; j++)
                acc = acc + val[pos[j]];
        }
        unsigned long long mask = __ballot(lng);
        while(mask)
        {
            const int l = __builtin_ctzll(mask);
            mask &= mask - 1;
            const int ls = __builtin_amdgcn_readlane(s, l), le = __builtin_amdgcn_readlane(e, l);
            V         a  = val[pos[ls]];
            for(int c = ls + 1; c < le; c += 64)
            {
                const int j = c + lane, have = min(64, le - c);
                const V   v = j < le ? val[pos[j]] : V{};
                for(int t = 0; t < have; t++)
                    a = a + coo_lane_value(v, t);
            }
            if(lane == l)
                acc = a;
        }
        return acc;
    }

    // A lane per output entry: it writes the run's column, counts it for its row and adds the run's values (coo_run_chain).
    template <typename V>
    __global__ __launch_bounds__(256) void coo_sum_kernel(aoclsparse_int nnz, aoclsparse_int nout, const int *__restrict__ key,
                                                          const int *__restrict__ pos, const aoclsparse_int *__restrict__ scol,
                                                          const int *__restrict__ runs, const V *__restrict__ val, int *cnt,
                                                          aoclsparse_int *__restrict__ oind, V *__restrict__ oval)
    {
        const long long o    = (long long)blockIdx.x * 256 + threadIdx.x;
        const int       lane = threadIdx.x & 63;
        const int       s = o < nout ? runs[o] : 0, e = o < nout ? runs[o + 1] : 0;
        const bool      act = o < nout && 0 <= s && s < e && e <= nnz; // (every run is like that: the guard costs nothing)
        const V         acc = coo_run_chain(act, s, e, lane, pos, val);
        if(act)
        {
            oind[o] = scol[s], oval[o] = acc;
            atomicAdd(&cnt[key[s]], 1);
        }
    }

    // ---- the values again, from new triplet values and the map a creation kept (device_coo_refresh_values) ----
    // `keep` mode, out[q] = val[pos[q]]: a lane takes COO_REFRESH_ILP entries a workgroup's width apart (pos and out coalesced),
    // loads all their positions, then all their values, then stores -- COO_REFRESH_ILP independent gathers in flight per lane where
    // coo_gather_kernel has one position load, one dependent value load and a store in a row.
    constexpr int COO_REFRESH_ILP = 8;

    template <typename V>
    __global__ __launch_bounds__(256) void coo_refresh_gather_kernel(aoclsparse_int nnz, const int *__restrict__ pos,
                                                                     const V *__restrict__ val, V *__restrict__ out)
    {
        const long long q0 = (long long)blockIdx.x * (256 * COO_REFRESH_ILP) + threadIdx.x;
        int             p[COO_REFRESH_ILP];
        V               v[COO_REFRESH_ILP];
#pragma unroll
        for(int r = 0; r < COO_REFRESH_ILP; r++)
        {
            const long long q = q0 + r * 256;
            p[r]              = q < nnz ? pos[q] : -1;
        }
#pragma unroll
        for(int r = 0; r < COO_REFRESH_ILP; r++)
            v[r] = (unsigned)p[r] < (unsigned)nnz ? val[p[r]] : V{}; // (every kept position is a triplet's: the guard costs nothing)
#pragma unroll
        for(int r = 0; r < COO_REFRESH_ILP; r++)
        {
            const long long q = q0 + r * 256;
            if(q < nnz)
                out[q] = v[r];
        }
    }

    // `sum` mode: coo_sum_kernel's lane per output entry without its columns and row counts -- runs, pos and val in, oval out
    template <typename V>
    __global__ __launch_bounds__(256) void coo_refresh_sum_kernel(aoclsparse_int nnz, aoclsparse_int nout, const int *__restrict__ pos,
                                                                  const int *__restrict__ runs, const V *__restrict__ val,
                                                                  V *__restrict__ oval)
    {
        const long long o    = (long long)blockIdx.x * 256 + threadIdx.x;
        const int       lane = threadIdx.x & 63;
        const int       s = o < nout ? runs[o] : 0, e = o < nout ? runs[o + 1] : 0;
        const bool      act = o < nout && 0 <= s && s < e && e <= nnz;
        const V         acc = coo_run_chain(act, s, e, lane, pos, val);
        if(act)
            oval[o] = acc;
    }

    int bits_of(aoclsparse_int v) // bits needed to write 0 .. v
    {
        int b = 0;
        while(v > 0)
            b++, v >>= 1;
        return b;
    }

    template <typename V>
    void launch_gather(hipStream_t s, aoclsparse_int nnz, const int *pos, const void *src, void *out)
    {
        hipLaunchKernelGGL((coo_gather_kernel<V>), dim3((unsigned)(((long long)nnz + 255) / 256)), dim3(256), 0, s, nnz, pos,
                           static_cast<const V *>(src), static_cast<V *>(out));
    }

    template <typename V>
    void launch_sum(hipStream_t s, aoclsparse_int nnz, aoclsparse_int nout, const int *key, const int *pos,
                    const aoclsparse_int *scol, const int *runs, const void *val, int *cnt, aoclsparse_int *oind, void *oval)
    {
        hipLaunchKernelGGL((coo_sum_kernel<V>), dim3((unsigned)(((long long)nout + 255) / 256)), dim3(256), 0, s, nnz, nout, key, pos,
                           scol, runs, static_cast<const V *>(val), cnt, oind, static_cast<V *>(oval));
    }

    // (staging slots of the sort: COO_SLOT_* of StageSlot, internal.hpp)
    struct SortState
    {
        int *key[2] = {nullptr, nullptr}, *pos[2] = {nullptr, nullptr};
        int  cur = 0; // the pair that holds the latest pass's output
        int            *hist = nullptr;
        aoclsparse_int *offs = nullptr;
        long long      *scan = nullptr;
        long long       tiles = 0;
    };

    // the passes over the digits of `bits` bits of src - base (src: the caller's array; read through the positions sorted so far)
    aoclsparse_status radix_passes(hipStream_t s, aoclsparse_int nnz, SortState &st, int bits)
    {
        for(int shift = 0; shift < bits; shift += 8)
        {
            const int  in = st.cur, out = st.cur ^ 1;
            long long *total = nullptr;
            hipLaunchKernelGGL(coo_hist_kernel, dim3((unsigned)st.tiles), dim3(256), 0, s, nnz, st.key[in], shift, st.tiles, st.hist);
            MI355_TRY(launch_spg_scan(s, (aoclsparse_int)(256 * st.tiles), st.hist, st.offs, st.scan, &total));
            hipLaunchKernelGGL(coo_scatter_kernel, dim3((unsigned)st.tiles), dim3(256), 0, s, nnz, st.key[in], st.pos[in], shift,
                               st.tiles, st.offs, st.key[out], st.pos[out]);
            st.cur = out;
        }
        MI355_HIP_TRY(hipGetLastError());
        return aoclsparse_status_success;
    }

    // Diagnostic (AOCLSPARSE_MI355_TIMING=1, as PhaseTimer): events around the radix passes and around everything behind them,
    // printed to stderr once the stream has been waited for.  Without the switch nothing is created or recorded.
    struct SortMarks
    {
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
        bool       got[3] = {false, false, false};
        SortMarks()
        {
            if(PhaseTimer::on())
                for(hipEvent_t &e : ev)
                    if(hipEventCreate(&e) != hipSuccess)
                        e = nullptr, (void)hipGetLastError();
        }
        ~SortMarks()
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
        void report(int passes) // (after the stream has been synchronised)
        {
            float sort_ms = 0.f, rest_ms = 0.f;
            if(got[0] && got[1] && got[2] && hipEventElapsedTime(&sort_ms, ev[0], ev[1]) == hipSuccess
               && hipEventElapsedTime(&rest_ms, ev[1], ev[2]) == hipSuccess)
                std::fprintf(stderr, "[mi355 timing]     coo sort kernels: %d passes %8.2f ms, count / gather / sum / scan %8.2f ms\n", passes,
                             sort_ms, rest_ms);
        }
    };

    template <typename F>
    aoclsparse_status by_value_type(size_t vsize, bool cplx, F &&f)
    {
        if(vsize == 4)
            f(float{});
        else if(vsize == 8 && cplx)
            f(float2{});
        else if(vsize == 8)
            f(double{});
        else if(vsize == 16)
            f(double2{});
        else
            return aoclsparse_status_not_implemented;
        return aoclsparse_status_success;
    }
} // namespace

// row / col / val: nnz triplets of an M x N matrix in HBM (index base `base`), any order.  ptr_b (M + 1), ind_b and val_b (*nnz_out
// entries; values of vsize bytes, cplx: pairs of reals): the CSR arrays in the same base, ALLOCATED HERE once every index is known
// to be in range.  sum == false: the reference's coo2csr (stable by row, *nnz_out = nnz); sum == true: sorted by (row, column),
// every run of equal coordinates added left to right in triplet order (*nnz_out = distinct coordinates).
// aoclsparse_status_invalid_index_value for a row or column out of range: nothing was allocated or written then.
static aoclsparse_status device_coo_to_csr_run(hipStream_t s, aoclsparse_int M, aoclsparse_int N, aoclsparse_int nnz, int base,
                                               const aoclsparse_int *row, const aoclsparse_int *col, const void *val, size_t vsize,
                                               bool cplx, bool sum, DeviceBuffer &ptr_b, DeviceBuffer &ind_b, DeviceBuffer &val_b,
                                               aoclsparse_int *nnz_out, DeviceBuffer *map)
{
    if(M < 0 || N < 0 || nnz < 0 || (vsize != 4 && vsize != 8 && vsize != 16))
        return aoclsparse_status_not_implemented;
    Runtime                              &rt = Runtime::get();
    std::lock_guard<std::recursive_mutex> sl(rt.stage_lock);
    // every way out of this function first lets the stream finish what was enqueued on the slots: the next holder of the lock may
    // grow (free) them
    struct DrainOnExit
    {
        hipStream_t s;
        ~DrainOnExit()
        {
            if(hipStreamSynchronize(s) != hipSuccess)
                (void)hipGetLastError();
        }
    } drain{s};
    SortMarks       marks;
    const size_t    n4    = sizeof(int) * (size_t)nnz;
    const unsigned  gq    = (unsigned)(((long long)nnz + 255) / 256);
    const long long tiles = ((long long)nnz + COO_TILE - 1) / COO_TILE;
    const size_t    cells = 256 * (size_t)tiles; // bins x tiles: nnz < 2^31, so < 2^27 + 256
    void           *p     = nullptr;
    MI355_TRY(rt.staging(COO_SLOT_SMALL, 256, &p));
    unsigned int *const d_bad = static_cast<unsigned int *>(p);
    if(nnz > 0)
    {
        unsigned int bad = 0;
        MI355_HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(unsigned int), s));
        hipLaunchKernelGGL(coo_check_kernel, dim3(std::min(gq, 4096u)), dim3(256), 0, s, nnz, M, N, base, row, col, d_bad);
        MI355_HIP_TRY(hipGetLastError());
        MI355_HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, s));
        MI355_HIP_TRY(hipStreamSynchronize(s));
        if(bad)
            return aoclsparse_status_invalid_index_value;
    }
    // from here on: when nnz > 0, every row key is in [0, M) and every column key in [0, N)
    MI355_TRY(ptr_b.alloc(sizeof(aoclsparse_int) * ((size_t)M + 1)));
    MI355_TRY(rt.staging(COO_SLOT_CNT, sizeof(int) * ((size_t)M + 1), &p));
    int *const cnt_p = static_cast<int *>(p);
    MI355_TRY(rt.staging(COO_SLOT_SCAN, spg_scan_scratch_bytes((aoclsparse_int)std::max<size_t>(cells, (size_t)std::max(M, nnz))), &p));
    long long *const scan_p = static_cast<long long *>(p);
    if(M > 0)
        MI355_HIP_TRY(hipMemsetAsync(cnt_p, 0, sizeof(int) * (size_t)M, s));
    long long *total = nullptr;
    *nnz_out         = nnz;
    if(nnz == 0)
    {
        MI355_TRY(ind_b.alloc(0)); // (non-null allocations, as the handle's mirror has them)
        MI355_TRY(val_b.alloc(0));
        if(map)
        {
            MI355_TRY(map[0].alloc(0));
            if(sum) // runs[0] = 0: no run, and where none starts
            {
                MI355_TRY(map[1].alloc(sizeof(int)));
                MI355_HIP_TRY(hipMemsetAsync(map[1].ptr, 0, sizeof(int), s));
            }
        }
    }
    else
    {
        SortState st;
        st.tiles = tiles, st.scan = scan_p;
        for(int q = 0; q < 2; q++)
        {
            MI355_TRY(rt.staging(q ? COO_SLOT_KEY_B : COO_SLOT_KEY_A, n4, &p));
            st.key[q] = static_cast<int *>(p);
            MI355_TRY(rt.staging(q ? COO_SLOT_POS_B : COO_SLOT_POS_A, n4, &p));
            st.pos[q] = static_cast<int *>(p);
        }
        MI355_TRY(rt.staging(COO_SLOT_HIST, sizeof(int) * cells, &p));
        st.hist = static_cast<int *>(p);
        MI355_TRY(rt.staging(COO_SLOT_OFFS, sizeof(aoclsparse_int) * (cells + 1), &p));
        st.offs = static_cast<aoclsparse_int *>(p);
        // the (key, position) pairs to start from: the columns in `sum` mode, the rows otherwise
        marks.record(0, s);
        hipLaunchKernelGGL(coo_init_kernel, dim3(gq), dim3(256), 0, s, nnz, base, sum ? col : row, st.key[0], st.pos[0]);
        if(sum)
        {
            MI355_TRY(radix_passes(s, nnz, st, bits_of(N - 1)));
            hipLaunchKernelGGL(coo_rekey_kernel, dim3(gq), dim3(256), 0, s, nnz, base, row, st.pos[st.cur], st.key[st.cur]);
        }
        MI355_TRY(radix_passes(s, nnz, st, bits_of(M - 1)));
        marks.record(1, s);
        const int *const keys = st.key[st.cur], *const pos = st.pos[st.cur];
        if(map) // the positions outlive the call in a buffer of the handle's: the slot is the next caller's to grow or free
        {
            MI355_TRY(map[0].alloc(n4));
            MI355_HIP_TRY(hipMemcpyAsync(map[0].ptr, pos, n4, hipMemcpyDeviceToDevice, s));
        }
        if(!sum)
        {
            MI355_TRY(ind_b.alloc(n4));
            MI355_TRY(val_b.alloc(vsize * (size_t)nnz));
            hipLaunchKernelGGL(coo_count_kernel, dim3(gq), dim3(256), 0, s, nnz, keys, cnt_p);
            launch_gather<aoclsparse_int>(s, nnz, pos, col, ind_b.ptr);
            MI355_TRY(by_value_type(vsize, cplx, [&](auto v) { launch_gather<decltype(v)>(s, nnz, pos, val, val_b.ptr); }));
        }
        else
        {
            // the sorted columns and the run heads go where the last pass read from; the scan of the heads has a slot of its own
            aoclsparse_int *const scol = st.key[st.cur ^ 1];
            int *const            flag = st.pos[st.cur ^ 1];
            MI355_TRY(rt.staging(COO_SLOT_FLAG, sizeof(aoclsparse_int) * ((size_t)nnz + 1), &p));
            aoclsparse_int *const outpos = static_cast<aoclsparse_int *>(p);
            launch_gather<aoclsparse_int>(s, nnz, pos, col, scol);
            hipLaunchKernelGGL(coo_flag_kernel, dim3(gq), dim3(256), 0, s, nnz, keys, scol, flag);
            MI355_TRY(launch_spg_scan(s, nnz, flag, outpos, scan_p, &total));
            long long distinct = 0;
            MI355_HIP_TRY(hipMemcpyAsync(&distinct, total, sizeof(distinct), hipMemcpyDeviceToHost, s));
            MI355_HIP_TRY(hipStreamSynchronize(s));
            if(distinct <= 0 || distinct > nnz)
                return aoclsparse_status_internal_error;
            const aoclsparse_int nout = (aoclsparse_int)distinct;
            MI355_TRY(ind_b.alloc(sizeof(aoclsparse_int) * (size_t)nout));
            MI355_TRY(val_b.alloc(vsize * (size_t)nout));
            if(map) // the run starts are built where they stay
                MI355_TRY(map[1].alloc(sizeof(int) * ((size_t)nout + 1)));
            else
                MI355_TRY(rt.staging(COO_SLOT_RUNS, sizeof(int) * ((size_t)nout + 1), &p));
            int *const runs = map ? map[1].as<int>() : static_cast<int *>(p);
            hipLaunchKernelGGL(coo_runs_kernel, dim3(gq), dim3(256), 0, s, nnz, nout, flag, outpos, runs);
            MI355_TRY(by_value_type(vsize, cplx, [&](auto v) {
                launch_sum<decltype(v)>(s, nnz, nout, keys, pos, scol, runs, val, cnt_p, ind_b.as<aoclsparse_int>(), val_b.ptr);
            }));
            *nnz_out = nout;
        }
        MI355_HIP_TRY(hipGetLastError());
    }
    aoclsparse_int *const optr = ptr_b.as<aoclsparse_int>();
    MI355_TRY(launch_spg_scan(s, M, cnt_p, optr, scan_p, &total));
    if(base != 0)
        hipLaunchKernelGGL(coo_add_base_kernel, dim3((unsigned)(((long long)M + 256) / 256)), dim3(256), 0, s, M + 1, base, optr);
    marks.record(2, s);
    MI355_HIP_TRY(hipGetLastError());
    MI355_HIP_TRY(hipStreamSynchronize(s)); // (the staging slots may be handed to the next caller once the lock is released)
    marks.report(nnz > 0 ? (sum ? (bits_of(N - 1) + 7) / 8 : 0) + (bits_of(M - 1) + 7) / 8 : 0);
    return aoclsparse_status_success; // (`drain` runs before the lock guard declared above it is released)
}

aoclsparse_status device_coo_to_csr(hipStream_t s, aoclsparse_int M, aoclsparse_int N, aoclsparse_int nnz, int base,
                                    const aoclsparse_int *row, const aoclsparse_int *col, const void *val, size_t vsize, bool cplx,
                                    bool sum, DeviceBuffer &ptr, DeviceBuffer &ind, DeviceBuffer &valb, aoclsparse_int *nnz_out,
                                    DeviceBuffer *map)
{
    const aoclsparse_status st = device_coo_to_csr_run(s, M, N, nnz, base, row, col, val, vsize, cplx, sum, ptr, ind, valb, nnz_out, map);
    if(st != aoclsparse_status_success)
    {
        ptr.release(), ind.release(), valb.release();
        if(map)
            map[0].release(), map[1].release();
    }
    return st;
}

// The radix passes alone, for a caller with pairs of its own (order_kernels.hip: the entries of a CSR's long rows): the sequence of
// `sum` mode above -- the minor keys first, then the major keys read through the positions sorted so far -- in the same slots.
aoclsparse_status device_sort_pairs(hipStream_t s, aoclsparse_int count, const aoclsparse_int *major, aoclsparse_int major_range,
                                    const aoclsparse_int *minor, aoclsparse_int minor_range, const int **perm)
{
    if(count <= 0 || major_range <= 0 || minor_range <= 0 || !major || !minor || !perm)
        return aoclsparse_status_internal_error;
    Runtime                              &rt = Runtime::get();
    std::lock_guard<std::recursive_mutex> sl(rt.stage_lock); // (the caller's already; it drains the stream before it lets go)
    const size_t   n4 = sizeof(int) * (size_t)count;
    const unsigned gq = (unsigned)(((long long)count + 255) / 256);
    SortState      st;
    void          *p = nullptr;
    st.tiles           = ((long long)count + COO_TILE - 1) / COO_TILE;
    const size_t cells = 256 * (size_t)st.tiles;
    for(int q = 0; q < 2; q++)
    {
        MI355_TRY(rt.staging(q ? COO_SLOT_KEY_B : COO_SLOT_KEY_A, n4, &p));
        st.key[q] = static_cast<int *>(p);
        MI355_TRY(rt.staging(q ? COO_SLOT_POS_B : COO_SLOT_POS_A, n4, &p));
        st.pos[q] = static_cast<int *>(p);
    }
    MI355_TRY(rt.staging(COO_SLOT_HIST, sizeof(int) * cells, &p));
    st.hist = static_cast<int *>(p);
    MI355_TRY(rt.staging(COO_SLOT_OFFS, sizeof(aoclsparse_int) * (cells + 1), &p));
    st.offs = static_cast<aoclsparse_int *>(p);
    MI355_TRY(rt.staging(COO_SLOT_SCAN, spg_scan_scratch_bytes((aoclsparse_int)cells), &p));
    st.scan = static_cast<long long *>(p);
    hipLaunchKernelGGL(coo_init_kernel, dim3(gq), dim3(256), 0, s, count, 0, minor, st.key[0], st.pos[0]);
    MI355_TRY(radix_passes(s, count, st, bits_of(minor_range - 1)));
    hipLaunchKernelGGL(coo_rekey_kernel, dim3(gq), dim3(256), 0, s, count, 0, major, st.pos[st.cur], st.key[st.cur]);
    MI355_TRY(radix_passes(s, count, st, bits_of(major_range - 1)));
    MI355_HIP_TRY(hipGetLastError());
    *perm = st.pos[st.cur];
    return aoclsparse_status_success;
}

aoclsparse_status device_coo_refresh_values(hipStream_t s, aoclsparse_int triplets, aoclsparse_int entries, bool sum, const int *pos,
                                            const int *runs, const void *val, size_t vsize, bool cplx, void *out)
{
    if(triplets < 0 || entries < 0 || entries > triplets || (!sum && entries != triplets) || !pos || (sum && !runs) || !val || !out)
        return aoclsparse_status_internal_error;
    if(entries == 0)
        return aoclsparse_status_success;
    SortMarks marks; // (AOCLSPARSE_MI355_TIMING=1: the kernel's own time; the stream is waited for only then)
    marks.record(0, s);
    MI355_TRY(by_value_type(vsize, cplx, [&](auto v) {
        using V = decltype(v);
        if(sum)
            hipLaunchKernelGGL((coo_refresh_sum_kernel<V>), dim3((unsigned)(((long long)entries + 255) / 256)), dim3(256), 0, s,
                               triplets, entries, pos, runs, static_cast<const V *>(val), static_cast<V *>(out));
        else
            hipLaunchKernelGGL((coo_refresh_gather_kernel<V>),
                               dim3((unsigned)(((long long)entries + 256 * COO_REFRESH_ILP - 1) / (256 * COO_REFRESH_ILP))), dim3(256), 0,
                               s, entries, pos, static_cast<const V *>(val), static_cast<V *>(out));
    }));
    marks.record(1, s);
    MI355_HIP_TRY(hipGetLastError());
    float ms = 0.f;
    if(marks.got[0] && marks.got[1] && hipEventSynchronize(marks.ev[1]) == hipSuccess
       && hipEventElapsedTime(&ms, marks.ev[0], marks.ev[1]) == hipSuccess)
        std::fprintf(stderr, "[mi355 timing]     coo refresh kernel (%s): %8.3f ms\n", sum ? "sum" : "keep", ms);
    return aoclsparse_status_success;
}

} // namespace mi355
