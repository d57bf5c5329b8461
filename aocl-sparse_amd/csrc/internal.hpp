// internal.hpp -- object model of the MI355X engine behind the aoclsparse_* C ABI.
//
// Host side keeps the reference's semantics (handles alias the user's CSR arrays, clean CSR
// with idiag/iurow, hint list, status codes); everything a kernel touches lives in HBM in the
// DeviceCsr mirrors below.  Layout rationale is in DESIGN.md.
#pragma once

#include "aoclsparse.h"
#include "aoclsparse_mi355.h"

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <algorithm>
#include <thread>
#include <cstdlib>
#include <cstdio>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstdint>
#include <exception>
#include <memory>
#include <mutex>
#include <functional>
#include <new>
#include <shared_mutex>
#include <system_error>
#include <vector>

// ---- descriptor (library/src/include/aoclsparse_descr.h:37-47) --------------------------
struct _aoclsparse_mat_descr
{
    aoclsparse_matrix_type type      = aoclsparse_matrix_type_general;
    aoclsparse_fill_mode   fill_mode = aoclsparse_fill_mode_lower;
    aoclsparse_diag_type   diag_type = aoclsparse_diag_type_non_unit;
    aoclsparse_index_base  base      = aoclsparse_index_base_zero;
};

namespace mi355
{

// ---- status helpers ----------------------------------------------------------------------
#define MI355_HIP_TRY(expr)                                   \
    do                                                        \
    {                                                         \
        hipError_t e__ = (expr);                              \
        if(e__ != hipSuccess)                                 \
            return ::mi355::map_hip_error(e__);               \
    } while(0)

// (the same for a status; several files spell this one out themselves, token for token)
#define MI355_TRY(expr)                       \
    do                                        \
    {                                         \
        aoclsparse_status st__ = (expr);      \
        if(st__ != aoclsparse_status_success) \
            return st__;                      \
    } while(0)

aoclsparse_status map_hip_error(hipError_t e);

// ---- complex values (aoclsparse_float_complex / aoclsparse_double_complex layout: {real, imag}) ---------
template <typename R>
struct cplx
{
    R re, im;
    __host__ __device__ cplx() = default;
    __host__ __device__ constexpr cplx(R r, R i = R(0))
        : re(r)
        , im(i)
    {
    }
};
using cfloat  = cplx<float>;
using cdouble = cplx<double>;
inline float  conj_of(float v) { return v; }
inline double conj_of(double v) { return v; }
template <typename R>
inline cplx<R> conj_of(cplx<R> v)
{
    return cplx<R>(v.re, -v.im);
}
// f(T{}) with T = float / double / cfloat / cdouble for the handle's value type
template <typename F>
auto dispatch_value_type(aoclsparse_matrix_data_type t, F &&f)
{
    switch(t)
    {
    case aoclsparse_smat:
        return f(float{});
    case aoclsparse_cmat:
        return f(cfloat{});
    case aoclsparse_zmat:
        return f(cdouble{});
    default:
        return f(double{});
    }
}
inline bool is_complex_type(aoclsparse_matrix_data_type t)
{
    return t == aoclsparse_cmat || t == aoclsparse_zmat;
}

// ---- hinted actions (library/src/include/aoclsparse_mat_structures.hpp:36-68) -------------
enum hinted_action
{
    action_none = 0,
    action_mv,
    action_sv,
    action_mm,
    action_2m,
    action_ilu0,
    action_sm_row,
    action_sm_col,
    action_dotmv,
    action_symgs,
    action_sorv_forward,
    action_sorv_backward,
    action_sorv_symm,
    action_max
};

// descriptor+operation id; same enumeration idea as include/aoclsparse_mtx_dispatcher.hpp:41-74
// restricted to what real types can produce (conjugate == plain for real data).
enum class doid : int
{
    gn = 0, // general, no-trans
    gt, // general, transpose
    sl, // symmetric lower / upper (transpose is the same operation)
    su,
    tln, // triangular lower/upper x none/transpose
    tlt,
    tun,
    tut,
    len
};

doid get_doid(const _aoclsparse_mat_descr *d, aoclsparse_operation op);

struct Hint
{
    hinted_action          act;
    doid                   id;
    aoclsparse_operation   trans;
    aoclsparse_matrix_type type;
    aoclsparse_fill_mode   fill;
    aoclsparse_int         nop;
    aoclsparse_int         kid;
    bool                   optimized = false;
};


// Host-side analysis loops over rows / blocks that are independent of each other: fixed chunking (results do not depend on
// the thread count), at most 16 threads, inline below `grain` items.  fn(begin, end).
template <typename F>
inline void parallel_for(long long n, long long grain, F fn)
{
    const unsigned hw = std::thread::hardware_concurrency();
    const int      nt = (int)std::min<long long>(std::min<unsigned>(16u, hw ? hw : 1u), (n + grain - 1) / std::max<long long>(grain, 1));
    if(nt <= 1)
    {
        fn(0LL, n);
        return;
    }
    // An exception inside a chunk (bad_alloc) is carried to the caller, and a thread that cannot be started costs nothing
    // but its parallelism (the chunk then runs here): the C ABI above this never sees std::terminate.
    std::vector<std::thread> th;
    th.reserve((size_t)nt);
    std::exception_ptr       err;
    std::mutex               err_lock;
    auto                     chunk = [&](int t) {
        try
        {
            fn(n * t / nt, n * (t + 1) / nt);
        }
        catch(...)
        {
            std::lock_guard<std::mutex> g(err_lock);
            if(!err)
                err = std::current_exception();
        }
    };
    for(int t = 0; t < nt; t++)
    {
        try
        {
            th.emplace_back(chunk, t);
        }
        catch(const std::system_error &)
        {
            chunk(t);
        }
    }
    for(auto &t : th)
        t.join();
    if(err)
        std::rethrow_exception(err);
}

// Diagnostic: AOCLSPARSE_MI355_TIMING=1 prints the wall time of the analysis phases it brackets to stderr.
struct PhaseTimer
{
    const char                           *name;
    std::chrono::steady_clock::time_point t0;
    static bool                           on()
    {
        static const bool v = [] { const char *e = std::getenv("AOCLSPARSE_MI355_TIMING"); return e && std::atoi(e) != 0; }();
        return v;
    }
    explicit PhaseTimer(const char *n) : name(n), t0(std::chrono::steady_clock::now()) {}
    ~PhaseTimer()
    {
        if(on())
            std::fprintf(stderr, "[mi355 timing] %-34s %8.1f ms\n", name,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
};

struct LapTimer // same switch: lap("what") prints the time since the previous lap
{
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void                                  lap(const char *what)
    {
        if(!PhaseTimer::on())
            return;
        const auto t1 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[mi355 timing]     %-30s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

// ---- device memory -------------------------------------------------------------------------
struct DeviceBuffer
{
    void  *ptr   = nullptr;
    size_t bytes = 0;
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &)            = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    ~DeviceBuffer();
    aoclsparse_status alloc(size_t nbytes);
    aoclsparse_status upload(const void *host, size_t nbytes, hipStream_t s); // alloc + H2D
    // alloc on the CURRENT device + device-to-device copy of src (which may live on another device: peer copy over xGMI when
    // peer access is enabled, staged by the runtime otherwise); enqueued on s, not waited for
    aoclsparse_status clone_from(const DeviceBuffer &src, hipStream_t s);
    void              release();
    // take over other's allocation (this one's own is released first)
    void adopt(DeviceBuffer &other)
    {
        if(this == &other)
            return;
        release();
        ptr = other.ptr, bytes = other.bytes;
        other.ptr = nullptr, other.bytes = 0;
    }
    template <typename T>
    T *as() const
    {
        return static_cast<T *>(ptr);
    }
};

// CSR arrays resident in HBM, always 4/8-byte element arrays in the SAME base as the host
// copy they mirror (kernels subtract base at load time).
struct DeviceCsr
{
    aoclsparse_int m = 0, n = 0, nnz = 0, base = 0;
    DeviceBuffer   ptr, ind, val;
    bool           valid = false;
};

// What the short-row SELL-64 kernel (sell_kernels.hip: sell_mv_short_kernel) reads about a slice, in ONE scalar load: where its
// value cells and its column lists start (48-bit offsets), its width, the stride between the column rows of a lane (the number
// of leaders with shared column lists, 64 without) and how a lane finds its list (mode).
struct SellSliceDesc
{
    uint32_t cell_lo, col_lo; // low words of the first value cell (slice_ptr[s]) and of the first column entry
    uint32_t hi; // bits 0-15: bits 32-47 of the value-cell offset; bits 16-31: those of the column offset
    uint32_t wsm; // bits 0-7 width (cells per row), 8-15 column stride, 16-23 mode, 24-31 flags (SELL_DESC_UWORD / _EXCEPT)
};
// Flags in the DEVICE copy of a record (sell_build_kernels.hip: sell_records_kernel writes them behind the fill pass; the host
// function below never sets them).  Only on a plan with uniform lists and one-byte packed words, whose kernels (UCOL && PK) read
// neither cell_lo nor the low half of hi: those bits then carry what the flags announce.
//   SELL_DESC_UWORD:  all 64 rows of the (full, one-list) slice have the same packed word: cell_lo bits 0-7 hold it and the
//                     kernel does not read the rows' words.
//   SELL_DESC_EXCEPT: (always with UWORD) the slice is mode 0 in every other reader's eyes, but its rows are ONE list shifted by
//                     lane of which at most two lanes omit cells: ucol holds the canonical list B (row of lane l: B + l), cell_lo
//                     bits 8-15 / 16-23 = first exception lane / the mask of the canonical cells it has, bits 24-31 and hi bits
//                     0-7 = the same for the second; lane 0xff = none.  The word sits at the CANONICAL cell positions.
constexpr uint32_t       SELL_DESC_UWORD = 1u << 24, SELL_DESC_EXCEPT = 1u << 25;
constexpr uint32_t       SELL_DESC_NO_LANE = 0xffu;
// modes: 0 lead[row] = list | shift << 8; 1 one list, shift = lane; 2 one list, no shift; 3 list = lane, no shift (lists not shared)
constexpr int            SELL_DESC_MODE_FOLLOW = 0, SELL_DESC_MODE_LANE_SHIFT = 1, SELL_DESC_MODE_ONE = 2, SELL_DESC_MODE_OWN = 3;
// the general kernel reads the same mode (0 / 1 / 2) from the top byte of a slice's cptr word, the offset from the bits below
constexpr int            SELL_CPTR_MODE_SHIFT = 56;
constexpr long long      SELL_CPTR_MASK       = (1LL << SELL_CPTR_MODE_SHIFT) - 1;
constexpr int            SELL_SHORT_WMAX       = 8;
constexpr aoclsparse_int SELL_SHORT_MIN_SLICES = 4096;
// records after the last slice (width 0, pointing at the padding cells): the last workgroup's 4 waves x 4 slices read them
constexpr int            SELL_DESC_PAD = 16;
// cells after the last one in val / vidx, entries after the last one in col (value 0 / index 0, column -1): what a slice of
// width 0 reads instead of nothing, so that the kernel has no branch around its loads
constexpr int            SELL_CELL_PAD = 64;
// nslices + SELL_DESC_PAD records from the host arrays: slice_ptr (nslices + 1), leaders[s] = leaders | mode << 8 as
// sell_leaders_kernel writes them (nullptr: column lists not shared, entry of a cell = its cell offset), ccells = column entries in all
void sell_pack_descriptors(aoclsparse_int nslices, const long long *slice_ptr, const aoclsparse_int *leaders, long long ccells,
                           SellSliceDesc *out);
// The periodic range of the DEVICE records and uniform lists (sell_period.cpp, which states the rule; host arrays, nslices records
// and nslices x SELL_SHORT_WMAX columns): out = {first slice, end slice, period in slices, column shift per period}: the records
// and lists of slice s in [first + period, end) are those of slice s - period with every column moved by the shift.  The smallest
// period that is a multiple of 4 slices and at most cap, first and end multiples of 4; all zero when no such range holds two
// periods and half of the slices, or when the search gives up (sell_period.cpp).
void sell_find_period(const SellSliceDesc *desc, const aoclsparse_int *ucol, aoclsparse_int nslices, aoclsparse_int cap,
                      aoclsparse_int out[4], long long *comparisons = nullptr);
// the longest period looked for: 4096 slices = 192 KB of records and lists, which stay in an L2
constexpr aoclsparse_int SELL_PERIOD_CAP = 4096;
// What the short-row kernel can do with a range: it divides by the period with ONE multiply -- the high word of (slice - first) x
// the reciprocal, exact for a power of two and otherwise while slices x period < 2^32 -- and adds the column shift to x in
// bytes, 32 bits (vsize = bytes per value).  build_sell keeps no range that fails this, so what aoclsparse_mi355_get_sell_period
// reports is what the kernel is handed.
inline bool sell_period_usable(aoclsparse_int nslices, long long lo, long long hi, long long per, long long stride, size_t vsize)
{
    if(per <= 0 || hi <= lo || lo < 0 || stride < 0)
        return false;
    if((unsigned long long)((hi - lo) / per) * (unsigned long long)stride * vsize >= (1ull << 32))
        return false;
    return (per & (per - 1)) == 0 || (unsigned long long)nslices * (unsigned long long)per < (1ull << 32);
}
// pairs of slices the search compares per slice at most; beyond that it reports no range (*comparisons: how many it made)
constexpr int SELL_PERIOD_WORK = 8;

// STACKED PERIODS (sell_kernels.hip: sell_mv_short_march_kernel).  Two further facts about a periodic range, decided on its FIRST
// period alone (sell_period.cpp: sell_find_march; range = what sell_find_period reported, word_bytes = the plan's pbytes):
//   out[0] = 1: the range can be stacked -- every group of SELL_MARCH_GROUP consecutive slices of the first period is a run in
//            the kernel's sense (all shifted, counting SELL_DESC_EXCEPT slices; one width; every list the list before it + 64 in
//            every used cell), every slice carries SELL_DESC_UWORD and the words are one byte; else 0;
//   out[1] = the alias map, four bits per cell: nibble q = a(q) + 1, where a(q) is the cell q' with ucol[q'] == ucol[q] + stride
//            in EVERY slice of the period (both cells used in every slice; an entry of -1 never aliases), 0: none.
// Cell q of a slice in period k + 1 is then cell a(q) of the same slice in period k: a wavefront that walks G periods of its
// strip loads it once.
constexpr int SELL_MARCH_GROUP = 4; // covers 2 and 4 slices per wavefront: range bounds and period are multiples of 4
void sell_find_march(const SellSliceDesc *desc, const aoclsparse_int *ucol, aoclsparse_int nslices, const aoclsparse_int range[4],
                     int word_bytes, aoclsparse_int out[2]);
// slices from which a wavefront of the short-row kernel takes several (sell_kernels.hip: sell_launch_short, which has the table)
constexpr aoclsparse_int SELL_SHORT_SPW_SLICES = 60000;
// slices per wavefront of the short-row kernel: AOCLSPARSE_MI355_SELL_SPW = 1 / 2 / 4 overrides the rule (measurements only;
// read once per process)
inline int sell_short_spw_override()
{
    static const int v = [] {
        const char *e = std::getenv("AOCLSPARSE_MI355_SELL_SPW");
        const int   k = e ? std::atoi(e) : 0;
        return (k == 1 || k == 2 || k == 4) ? k : 0;
    }();
    return v;
}
// the rule for a real type of vsize bytes (the table it comes from: sell_launch_short); table = the cells hold table indices
inline int sell_short_spw(aoclsparse_int nslices, size_t vsize, bool table)
{
    int spw = 1;
    if(nslices >= SELL_SHORT_SPW_SLICES)
        spw = vsize == 4 ? (table ? 4 : 2) : (table ? 2 : 1);
    return sell_short_spw_override() ? sell_short_spw_override() : spw;
}
// The alias maps the march kernel is built for, each at ONE width (= the plan's widest slice); read by the rule below and by the
// launcher.  Today the 5-point stencil whose period is one grid line (cells -P, -1, 0, +1, +P: a(0) = 2, a(2) = 4).  A plan with
// any other map is not stacked: where a plan really has no alias -- grid lines that are no multiple of 64 rows, whose period is
// several lines: 3000^2, 2000^2, 3008 x 3000 -- stacking without shared loads measured within 2 % of the kernel without stacking
// on either side (profiles/r18/g_sweep.txt).  The 7-offset map (0x6040) was not measured and is not built.
struct SellMarchMap
{
    int      width;
    unsigned alias;
};
constexpr SellMarchMap SELL_MARCH_MAPS[] = {{5, 0x503u}};
// periods per stacked wavefront (profiles/r18/upper_bound.txt, g_sweep.txt: the table is in sell_launch_short), slices per
// wavefront and wavefronts per workgroup of that kernel
constexpr int SELL_MARCH_G = 3, SELL_MARCH_SPW = 2, SELL_MARCH_WAVES = 4;
// What the launcher does with a plan (the ONE rule: sell_launch_short and aoclsparse_mi355_get_sell_march both call it): slices
// [lo, hi) run stacked, g periods per wavefront, with the map alias; g = 0: nothing is stacked and the product runs
// sell_mv_short_period_kernel.  vsize = bytes per value (double only: float was not measured), spw = the slices per wavefront the
// launcher chose, stack / alias = SellView::mstack / malias.  hi - lo is a whole number of g periods AND of workgroups, so the
// kernel has no partial workgroup on the stacked side; what is left of the range runs with the slices outside it.
struct SellMarch
{
    int      lo = 0, hi = 0, g = 0;
    unsigned alias = 0;
};
inline SellMarch sell_march_rule(aoclsparse_int nslices, aoclsparse_int max_width, int pslo, int pshi, int pper, int pstride, int stack,
                                 unsigned alias, size_t vsize, int spw)
{
    constexpr int g = SELL_MARCH_G;
    SellMarch     r;
    if(!stack || vsize != 8 || spw != SELL_MARCH_SPW || !sell_period_usable(nslices, pslo, pshi, pper, pstride, vsize))
        return r;
    bool known = false;
    for(const SellMarchMap &k : SELL_MARCH_MAPS)
        known = known || (k.width == (int)max_width && k.alias == alias);
    if(!known)
        return r;
    long long groups = (pshi - pslo) / pper / g; // of g whole periods
    while(groups > 0 && (groups * (pper / SELL_MARCH_SPW)) % SELL_MARCH_WAVES != 0)
        groups--;
    if(groups <= 0)
        return r;
    r.lo = pslo, r.hi = pslo + (int)(groups * g * pper), r.g = g, r.alias = alias;
    return r;
}

// What a SELL-64 launcher reads of a plan (SellPlan::view): sizes and device pointers, nothing owned.
struct SellView
{
    aoclsparse_int        m = 0, nslices = 0;
    int                   pack = 1;
    aoclsparse_int        max_width = 0; // widest slice, in cells per row
    int                   ntab = 0;
    const long long      *slice_ptr = nullptr;
    const void           *cells = nullptr; // the values, or (ntab > 0) the one-byte indices into vtab
    const aoclsparse_int *col = nullptr, *rowlen = nullptr;
    const long long      *cptr = nullptr; // cptr, lead: nullptr when the column lists are not shared
    const unsigned short *lead = nullptr;
    const void           *vtab = nullptr; // nullptr without a table
    const SellSliceDesc  *desc = nullptr; // nullptr when the plan has no slice records
    // packed table indices (pbits > 0): cells holds one word of pbytes bytes per ROW, row i at i * pbytes, the index of cell q
    // of the row at bit q * pbits; pbits = 0: one byte per cell (or the values)
    int                   pbits = 0, pbytes = 0;
    // one list of SELL_SHORT_WMAX columns per slice (mode 1 / 2 slices; -1 everywhere else); nullptr when the plan has none
    const aoclsparse_int *ucol = nullptr;
    // the periodic range of the records and lists (SellValues::pslo ..; all zero: none)
    int                   pslo = 0, pshi = 0, pper = 0, pstride = 0;
    // whether that range can be stacked, and its alias map (SellValues::mstack, malias)
    int                   mstack = 0;
    unsigned              malias = 0;
};

// SELL-64 twin of a device CSR (sell_plan.cpp: build_sell; layout in sell_build_kernels.hip, products in sell_kernels.hip): built by
// aoclsparse_optimize for an mv hint when the padding stays small; the handle's ?mv then runs on it instead of the CSR-Adaptive
// kernel.  Its members are grouped by what invalidates them: SellStructure (row_ptr, col_idx, the sizes or the option change),
// SellValues (any value changes), SellCounters (nothing: since creation).

// WHAT THE STRUCTURE STAGE OWNS (build_sell = structure, then values): pack, the widths, slice_ptr, the shared decision with cptr /
// lead / ccells, col, rowlen and the records describe the CSR of m rows and nnz entries under aoclsparse_mi355_option_sell == mode.
struct SellStructure
{
    aoclsparse_int nslices = 0;
    int            pack    = 1; // 1: cell (p, lane) at 64 p + lane; 4: at 256 (p/4) + 4 lane + p%4
    long long      cells   = 0; // stored cells = sum over slices of 64 * (longest row of the slice)
    DeviceBuffer   slice_ptr; // nslices+1 cell offsets (long long)
    DeviceBuffer   col; // ccells 0-based columns (-1 = padding)
    DeviceBuffer   rowlen; // m row lengths (read by the 4- and 8-lane orders only)
    // shared column lists (sell_build_kernels.hip): col holds one list per leader lane of a slice, ccells entries in all;
    // cptr = nslices+1 offsets into it, lead = m x 16 bits (leader index of a row inside its slice | column shift << 8)
    bool           shared = false;
    long long      ccells = 0;
    DeviceBuffer   cptr, lead;
    aoclsparse_int wmax     = 0; // widest slice, in cells
    bool           records  = false; // the copy can have slice records
    aoclsparse_int nuniform = 0; // slices of mode 1 / 2 (what SellValues::uniform is on a plan with ucol)
    // one 16-byte record per slice for the short-row kernel (SellSliceDesc; nslices + SELL_DESC_PAD of them), allocated only
    // when that kernel can serve the copy (pack 1, widest slice <= SELL_SHORT_WMAX, >= SELL_SHORT_MIN_SLICES slices).  desc0 (host):
    // the records as sell_pack_descriptors made them; desc: the device copy, in which the values stage sets sell_records_kernel's flags
    std::vector<SellSliceDesc> desc0;
    DeviceBuffer               desc;
    // built: all of the above is there, for the CSR and option value below
    bool           built = false;
    int            mode  = -1;
    aoclsparse_int m = 0, nnz = 0;
    // what only a values stage on a kept structure allocates: the pristine records' device copy, one spare set of records and
    // uniform lists (the stage writes the new set there, compares it with the current one, and the two change places), and three
    // words (sell_records_kernel's two counters, the compare kernel's verdict)
    DeviceBuffer   desc0_dev, desc_spare, ucol_spare, kwords;
    // nothing of the structure is trusted from here on (the buffers of the copy itself stay for the next build to reuse)
    void drop()
    {
        built = false;
        desc0.clear(), desc0.shrink_to_fit();
        desc0_dev.release(), desc_spare.release(), ucol_spare.release(), kwords.release();
    }
    size_t kept_bytes() const
    {
        return sizeof(SellSliceDesc) * desc0.capacity() + desc0_dev.bytes + desc_spare.bytes + ucol_spare.bytes + kwords.bytes;
    }
};

// WHAT THE VALUES STAGE OWNS: the table and the cell encoding chosen from it, the cells, the uniform lists, what the records kernel
// counted, the periodic range and the stacking facts.
struct SellValues
{
    // value table (sell_build_kernels.hip): ntab > 0 -> vidx holds one byte per cell (same cell order and offsets as val would) indexing
    // vtab, ntab values sorted by bit pattern, and val is not allocated; ntab = 0 -> the values are in val
    // ... or, on a plan with slice records whose rows fit (widest slice x pbits <= 32): pidx holds one word of pbytes bytes per row
    // with pbits bits per cell ((nslices + SELL_DESC_PAD) x 64 words, the padding 0) and vidx is not allocated either
    int            ntab = 0, pbits = 0, pbytes = 0;
    DeviceBuffer   val, vtab, vidx, pidx;
    // with slice records and shared lists: SELL_SHORT_WMAX columns per slice (nslices + SELL_DESC_PAD entries), the single list of
    // a mode 1 / 2 slice, -1 elsewhere; uniform = how many slices have one
    DeviceBuffer   ucol;
    aoclsparse_int uniform = 0;
    // slices whose device record carries SELL_DESC_UWORD / SELL_DESC_EXCEPT (counted by the kernel that sets them)
    aoclsparse_int uniform_words = 0, exceptions = 0;
    // the periodic range of the records and lists (sell_find_period on a copy of the device arrays, behind the kernel that writes
    // the flags): slices [pslo, pshi), period pper slices, column shift pstride per period; all zero: none.  Four integers, no
    // array: the short-row kernel reads the first period's records for every slice of the range
    int            pslo = 0, pshi = 0, pper = 0, pstride = 0;
    // the range can be stacked (1 / 0) and the alias map of its first period (sell_find_march, on the same host copies)
    int            mstack = 0;
    unsigned       malias = 0;
    void no_range()
    {
        pslo = pshi = pper = pstride = 0;
        mstack = 0, malias = 0;
    }
    // nothing of the old values is trusted: no table, no lists, no flags, no range.  The tables, index cells and lists go; val
    // stays for the cells of the next fill (sell_alloc_cells reuses it, or releases it for a table)
    void reset()
    {
        ntab = pbits = pbytes = 0;
        uniform = uniform_words = exceptions = 0;
        no_range();
        vtab.release(), vidx.release(), pidx.release(), ucol.release();
    }
};

// since creation: times the structure stage / the values stage ran, times a values stage carried the periodic range over, and
// what the last build_sell did (0 nothing yet, 1 structure + values, 2 values with the search, 3 values, range carried over)
struct SellCounters
{
    long long structure_builds = 0, value_fills = 0, searches_skipped = 0;
    int       last_route = 0;
};

struct SellPlan
{
    SellStructure st;
    SellValues    vals;
    SellCounters  count;
    bool          valid = false, tried = false;
    bool          wanted = false; // optimize chose SELL: rebuilt lazily after the values change
    // stale: aoclsparse_mi355_?revalue_device kept the structure and the cells hold the OLD values -- valid is false, no launcher
    // runs the copy, and the next build_sell runs the values stage alone
    bool          stale = false;
    void drop_structure()
    {
        stale = false;
        st.drop();
    }
    // The values of the CSR this copy mirrors have changed: no launcher runs it and the next build_sell builds it again.  keep: the
    // structure stays for that build (stale) if there is one, the copy served products or was stale already (two changes in a row
    // leave the same state), and it describes a CSR of m rows and nnz entries; every other change drops it.
    void values_changed(bool keep, aoclsparse_int m, aoclsparse_int nnz)
    {
        const bool live = valid || stale;
        valid = tried = false;
        if(keep && st.built && live && st.m == m && st.nnz == nnz)
            stale = true;
        else
            drop_structure();
    }
    // products served by this copy: odd ones walk the slices in descending order, so that what one product leaves in the
    // Infinity Cache (the END of its sweep) is where the next one starts (sell_kernels.hip); the bits do not depend on it
    mutable std::atomic<unsigned> products{0};
    int next_direction() const;
    // m = rows of the CSR this copy mirrors, max_width = its longest row
    SellView view(aoclsparse_int m, aoclsparse_int max_width) const
    {
        SellView v;
        v.m = m, v.nslices = st.nslices, v.pack = st.pack, v.max_width = max_width, v.ntab = vals.ntab;
        v.slice_ptr = st.slice_ptr.as<long long>();
        v.cells     = vals.ntab ? (vals.pbits ? vals.pidx.ptr : vals.vidx.ptr) : vals.val.ptr;
        v.pbits = vals.ntab ? vals.pbits : 0, v.pbytes = vals.ntab ? vals.pbytes : 0;
        v.ucol = vals.ucol.as<aoclsparse_int>();
        v.pslo = vals.pslo, v.pshi = vals.pshi, v.pper = vals.pper, v.pstride = vals.pstride;
        v.mstack = vals.mstack, v.malias = vals.malias;
        v.col = st.col.as<aoclsparse_int>(), v.rowlen = st.rowlen.as<aoclsparse_int>();
        v.cptr = st.shared ? st.cptr.as<long long>() : nullptr;
        v.lead = st.shared ? st.lead.as<unsigned short>() : nullptr;
        v.vtab = vals.ntab ? vals.vtab.ptr : nullptr;
        v.desc = st.desc.as<SellSliceDesc>();
        return v;
    }
};

// csrmm row groups (csrmm_kernels.hip: csrmm_rowgroup_kernel): runs of consecutive rows with one column pattern
constexpr int CSRMM_GROUP = 8; // rows per group at most
struct MmGroups
{
    // row-major, n >= 128, no groups: most rows repeat the previous row's column list shifted by one (a stencil) and have
    // <= 8 entries -> csrmm_row_run_kernel (a wave walks 8 rows and keeps the previous row's B rows in registers)
    bool           runs_tried = false, row_runs = false;
    // ... and, when the matrix is BANDED (most rows end `band` columns right of the diagonal, band >= 256, a 2-D / 3-D
    // stencil), the order in which the kernel's 8-row blocks are walked: strips of <= 256 rows of the band, every strip
    // from the top of the matrix to the bottom (run_order[b] = first row of the b-th block).  In row order the three
    // touches of a B row (from the band above, the row itself, the band below) are `band` rows of traffic apart --
    // 2 and 4 MB at band 1000 and 128 columns, more than an XCD's 4 MB L2 keeps: measured 2.5 x B fetched; in strip
    // order they are one strip apart.
    DeviceBuffer   run_order;
    aoclsparse_int band = 0;
    // ... and row blocks for the narrow (n < 128) row-major kernel that follow the lines of the band: every line of `band` rows in 8
    // blocks, {first row, first non-zero} like SpmvPlan::rowblocks (+ a terminal entry).  In launch order block b runs on XCD b % 8, so
    // rows i and i +- band meet in one L2 and all eight XCDs work inside one line (csrmm_tile_kernel; 0 blocks: not built)
    DeviceBuffer   slab_blocks;
    aoclsparse_int slab_nblocks = 0;
    aoclsparse_int ngroups = 0;
    int            max_rows = 0; // rows of the largest group
    DeviceBuffer   first; // ngroups + 1 row indices
    bool           valid = false, tried = false;
    // column-major csrmm: row pairs (2r, 2r+1) where row 2r+1 carries row 2r's pattern shifted by one column (scalar
    // stencils, banded matrices) and both fit the register cache -- csrmm_colpair_kernel serves them with 16-byte loads
    bool           pairs_tried = false, pairs = false;
    aoclsparse_int npairs = 0, nsingles = 0;
    DeviceBuffer   pair_first, single_rows; // first row of every pair; rows without a partner
    // column-major csrmm, round 4: every block of win_rows consecutive rows touches one short stretch of columns (banded
    // matrices, stencils in natural order) -- csrmm_colwin_kernel stages that stretch of each B column in LDS.
    // windows[2b], windows[2b+1] = first column (0-based, 16-byte granule) and 16-byte pieces of block b's stretch
    bool           win_tried = false, win = false;
    int            win_rows  = 0;
    DeviceBuffer   windows;
};

// merge-path tiling of a device CSR (mergepath_kernels.hip): tile w starts at {row ends, non-zeros} =
// starts[2w], starts[2w+1]
constexpr int MP_ITEMS = 1024; // rows + non-zeros per workgroup
constexpr int SELL_PROMOTE_CALLS = 8; // an un-hinted handle gets its SELL-64 copy at this many products
struct MergePlan
{
    aoclsparse_int ntiles = 0;
    DeviceBuffer   starts; // (ntiles + 1) x {i, j}
    // 2 * ntiles: first[w] = first tile that holds a head piece of the row whose END lies in tile w, or -1; then endt[v] = the
    // tile in which the row of tile v's head piece ends, or -1
    DeviceBuffer   first;
    bool           valid = false, tried = false;
    // Pieces of cut rows meet through a piece set: per tile a head piece, a tail piece (8 bytes each) and an arrival counter
    // (mergepath_kernels.hip).  A launch leaves every counter at 0, so a set carries nothing from one launch to the next; two
    // launches in flight at once must not share one, and launches on one stream never are: every stream that has run this plan
    // owns a set.  No launch ever waits for another stream.  Streams are told apart by {address, hipStreamGetId}: an address
    // the runtime hands out again after the caller destroyed a stream is a NEW stream, and work of the old one may still be
    // running -- the set is taken over after a device synchronisation.  (mutable: products run on a const plan under the
    // handle's shared lock; `launch_lock` makes {find the set, enqueue} one step.)
    struct GranuleSet
    {
        void              *stream = nullptr;
        unsigned long long uid    = 0;
        DeviceBuffer       granules; // 3 * ntiles x 8 bytes: head pieces, tail pieces, counters; zeroed at allocation
    };
    static constexpr size_t                           MAX_SETS = 16; // more streams than this: the oldest sets are recycled after a device sync
    mutable std::mutex                               launch_lock;
    mutable std::vector<std::unique_ptr<GranuleSet>> sets;
};

// Blocked-ELL copy of a block-dense matrix for the MFMA csrmm (csrmm_bell_kernels.hip; round 4): 16 x 16 blocks, `width` block
// slots per block row (bcol = -1: empty slot), values dense per block in the v_mfma_f64_16x16x4 A-operand order (element
// (i, k) of a block: fragment t = k / 4, lane = 16 * (k % 4) + i, stored at 128 * (t / 2) + 2 * lane + t % 2).  Built for double matrices whose 16 x 16 tiles are at least half full
// (the reference picks its blocked CSR by the same kind of fill threshold: conversion/aoclsparse_convert.cpp:36-147).
constexpr int BELL_BS = 16;
struct BellPlan
{
    bool           tried = false, valid = false;
    aoclsparse_int nbr = 0, width = 0; // block rows, block slots per block row
    long long      nblocks = 0; // stored (non-empty) blocks
    double         fill = 0.0; // nnz / (256 * nblocks)
    DeviceBuffer   val, bcol; // nbr * width * 256 values; nbr * width block columns
    // Which XCD works through which block rows, in which order (build_bell's model of the eight L2s, csrmm_api.cpp): order[8 p + x] = the
    // p-th block row of XCD x (-1 past the end of its list), order_len lists entries per XCD; order_len == 0: launch order.
    DeviceBuffer   order;
    aoclsparse_int order_len = 0;
    int            xcd_chunk = 1; // chunked deal: consecutive block rows per XCD turn (1: launch order; 0: a lattice sweep)
    aoclsparse_int lattice[3] = {0, 0, 0}; // lattice sweep: block rows per line, lines per plane, planes (else 0)
    int            region[2]  = {0, 0}; // ... and the cross-section of an XCD's region (block rows along the line x lines)
    int            region_cut[2] = {0, 0}; // ... pieces per line, segments of the plane range
    double         model_fetches = 0.0, model_fetches_launch_order = 0.0; // modelled L2 misses per distinct B block row, chosen / launch order
};

// SpMV execution plan (CSR-Adaptive row blocks), see spmv_kernels.hip
struct SpmvPlan
{
    aoclsparse_int nblocks     = 0;
    aoclsparse_int long_rows   = 0;
    aoclsparse_int max_row_nnz = 0;
    aoclsparse_int tile        = 0; // LDS tile (non-zeros per row block): 1024 or 2048
    DeviceBuffer   rowblocks; // nblocks+1 entries {first row, first non-zero (0-based)}
    // the same blocks as {first row, first non-zero, rows, non-zeros}, blocks holding a long row FIRST (a row is one
    // lane's serial chain: a block with a 300-entry row runs twice as long as the others, and started last it is the
    // kernel's tail); empty when no block is heavy.  Only csr_adaptive_kernel reads it.
    DeviceBuffer   rowblocks4;
    bool           heavy_first = false;
    bool           valid = false;
    SellPlan       sell;
    MergePlan      merge;
    MmGroups       mm;
    BellPlan       bell;
    std::atomic<int> mv_calls{0}; // products served from this plan without a SELL copy (promotion counter;
                                  // concurrent ?mv calls on one handle are allowed, as in the reference)
    // products of the row-block kernel: odd ones walk the blocks in descending order (see SellPlan::products)
    mutable std::atomic<unsigned> sweeps{0};
    // the same for csrmm: every second product of a handle runs its blocks in descending order (csrmm_kernels.hip: mm_block_index)
    mutable std::atomic<unsigned> mm_products{0};
};

// Direction of the NEXT csrmm launches of the calling thread (set by csrmm_api.cpp right before it dispatches; the launchers put it
// into bit 30 of the kernels' XCD-chunk word).  0: ascending.
constexpr int MM_DESCENDING = 0x40000000;
constexpr int MM_DEAL       = 0x20000000; // the chunk of the word counts blocks per XCD TURN (chunks dealt round-robin), not per XCD
int  &mm_direction_word();

// TRSV plan of one (triangle, op) pair (trsv_plan.cpp / trsv_kernels.hip): the strict triangle
// re-laid out in LEVEL ORDER.  Position k holds row rowmap[k]; its entries sit at
// [pptr[k], pptr[k+1]) of pind/pval already in the order the reference's chain consumes them, so
// a level is one contiguous slab of HBM and every kernel walks forward.
struct TrsvSegment
{
    aoclsparse_int l0, l1; // levels [l0, l1)
    bool           narrow; // true: one single-workgroup launch loops over the levels
};
// Supernodal variant of the plan (trsv_block_kernel; all four (fill, op) triangles of real types): rows consecutive in
// SOLVE order where each depends on exactly its predecessor's dependencies plus the predecessor (the dofs of a mesh node
// in an ILU(0) factor) form a BLOCK that ONE lane solves back to back -- the block's external dependencies are waited for
// once, the rows inside it hand their results on in registers -- so the dependency DAG is levelled per block (shell-like
// factor: 1,101 block levels instead of 5,505 row levels).  Own level-ordered copy of the triangle (positions = rows in
// block-level order, in solve order inside a block; entries in chain order).
constexpr int TRSV_BLK_ROWS = 8; // rows per block at most
constexpr int TRSV_BLK_EXT  = 24; // external dependencies of a multi-row block at most
// entries of a multi-row block at most: 5 rows on 20 external dependencies (a mesh node of 5 unknowns below 4 neighbours: 5 x 20 + 10).
// (96 until round 6: such a node was cut into 4 rows + 1 single row of 24 entries -- an extra block level per node, and the single rows
// put the whole solve on the (5, 24) shape of trsv_block_kernel, whose values live in LDS: 2.5 instead of 1.7 us per block level.)
constexpr int TRSV_BLK_NV   = 110;
// spare elements behind the m x nrhs position-ordered solution buffer: [0, 64) parked tag stores, [64, 128) parked x stores
// (one slot per lane), the last one (191) the slot that always holds 0 -- apart from the parked ones: a parked NaN must not reach it
constexpr int TRSV_XP_PAD = 192;
// Two-level schedule on top of the block plan (trsv_chunk_kernel; round 6; L, L^T, U^T of real types): the blocks in their
// natural (solve) order are cut into CHUNKS of consecutive blocks, one workgroup per chunk.  A chunk walks its own blocks in
// block-level order, a STEP (<= 64 / TRSV_CHUNK_LANES blocks of one level, TRSV_CHUNK_LANES lanes per block: a lane per row) per
// wavefront, steps dealt round-robin to the workgroup's wavefronts.  The chunk's x lives in LDS (NaN-tagged words, as in HBM):
// a dependency inside the chunk is polled there (~0.1 us per hand-off).  Rows of EARLIER chunks a chunk depends on are its HALO:
// one wavefront of the workgroup polls them in xp (HBM, ~1.5-2 us) in the order of their first use and copies them into LDS
// slots behind the chunk's own rows -- the wavefronts that solve only ever poll LDS.  The chunk plan shares the block plan's
// level-ordered copy of the triangle; its own data:
//   steps  nsteps x 8 words {first block (index in block-level order), position of its first row, LDS slot of that row, rows of
//          the step's blocks as nibbles; rows in front of block j as bytes (2 words), rows of the step, blocks}
//   cptr   nchunks + 1 first step of every chunk, then nchunks: rows of the chunk, nchunks: first halo entry (a multiple of 4),
//          nchunks: halo entries
//   eptr   nblocks + 1 offsets into cind (indexed like bfirst)
//   cind   the external dependencies of every block as LDS slots of its chunk (own rows first, halo behind them)
//   hind   the halos: positions in xp, per chunk in the order of first use
constexpr int TRSV_CHUNK_LANES = 8; // lanes per block = TRSV_BLK_ROWS
// wavefronts per workgroup: all but the last take steps, the last one fetches the halo.  (4 + 1: 1.144 ms on the shell-like factor, 5 + 1:
// 1.103, 7 + 1: 1.102 -- the solve is paced by the dependency chain; two staging areas fewer leave LDS for 12 % more rows per chunk,
// i.e. fewer chunk boundaries on the critical path)
constexpr int TRSV_CHUNK_WAVES = 6;
// a solving wavefront's staging area holds the values of one step: 8 blocks of bs rows with ext external + (bs - 1) / 2 internal entries
constexpr int trsv_chunk_pcap(int bs, int ext)
{
    return 8 * (bs * ext + bs * (bs - 1) / 2) + ext + 16; // (+ what a read past the last block's entries can overshoot)
}
// LDS slots (8 bytes as double) of a chunk -- own rows + halo -- at most: what the CU's 160 KB leave next to the staging areas
constexpr int trsv_chunk_slots(int bs, int ext)
{
    return ((160 * 1024 - 16 - (TRSV_CHUNK_WAVES - 1) * (trsv_chunk_pcap(bs, ext) * 8 + 9 * ext * 4) - 65 * 8) / 8) / 256 * 256;
}
constexpr int TRSV_CHUNK_ROWS = trsv_chunk_slots(5, 16); // the largest of the four shapes
// the compiled shape (rows per block, external dependencies) that holds a plan's largest block / external list
constexpr int trsv_chunk_bs(int max_rows) { return max_rows <= 5 ? 5 : TRSV_CHUNK_LANES; }
constexpr int trsv_chunk_ext(int max_ext) { return max_ext <= 16 ? 16 : TRSV_BLK_EXT; }
struct TrsvChunkPlan
{
    bool           tried = false, valid = false;
    aoclsparse_int nchunks = 0, nsteps = 0, max_rows = 0; // max_rows: LDS slots (rows + halo) of the largest chunk
    double         model_us = 0.0, model_block_us = 0.0; // plan-time estimates: this schedule / the lane-per-block one
    DeviceBuffer   steps, cptr, eptr, cind, hind;
};
struct TrsvBlockPlan
{
    double         slice_fan_in = 0.0; // producer slices a slice of 64 blocks waits for, on average (trsv_plan.cpp: the slice width)
    TrsvChunkPlan  chunk;
    bool           tried = false, valid = false;
    bool           front = false; // a row's chain starts with the rows of its own block (U), instead of ending with them
    aoclsparse_int nblocks = 0, nslices = 0, nlevels = 0;
    int            max_rows = 1, max_ext = 0; // largest block / largest external list of a multi-row block
    DeviceBuffer   rowmap, pptr, pind, pval; // as TrsvPlan, in block-level order
    DeviceBuffer   psrc; // value map (aoclsparse_mi355_keep_value_maps): per entry of pval its position in the clean value array
    DeviceBuffer   bfirst; // nblocks+1: first position of every block
    // nslices+1: first BLOCK of every slice (<= 64 blocks of one block level); then nslices: the slice's block level;
    // then nlevels+1: first slice of every level (the kernel's gate counts finished slices per level)
    DeviceBuffer   slices;
};
struct TrsvPlan
{
    TrsvBlockPlan               blk;
    aoclsparse_int              nlevels   = -1;
    aoclsparse_int              max_width = 0; // widest level
    aoclsparse_int              launches  = 0; // kernel launches of the hybrid schedule
    aoclsparse_int              nnz_tri   = 0; // entries of the strict triangle
    std::vector<aoclsparse_int> level_ptr; // host, nlevels+1
    std::vector<TrsvSegment>    segments; // hybrid schedule
    DeviceBuffer                rowmap, levels; // device: m rows in level order; level_ptr copy
    DeviceBuffer                pptr, pind, pval; // device: level-ordered strict triangle; pind = positions
    // level slices for trsv_slice_kernel: slice w = positions [slices[w], slices[w+1]), <= 64 of them, never across a
    // level boundary (so the lanes of a wavefront are independent of each other)
    aoclsparse_int              nslices = 0;
    DeviceBuffer                slices;
    bool                        valid = false;
    // the level-ordered layout above (rowmap .. slices) is on the device.  Round 3: when the triangle has a block plan the
    // automatic schedule never touches it, so it is built only when something asks for it (a forced row-level schedule, the
    // hybrid schedule, complex types, sorv): levels / nlevels / nnz_tri are always valid once `valid` is.
    bool rows_valid = false;
    // value maps, recorded only while the handle's keep_value_maps flag is set: psrc / blk.psrc = per entry of pval / blk.pval its
    // 0-based position in the clean CSR's value array; conj = the values are the conjugates (op = H).  They hold no values, but they
    // index a layout: whatever invalidates the plan releases them.
    DeviceBuffer psrc;
    bool         conj = false;
    void         drop_value_maps() { psrc.release(), blk.psrc.release(); }
    // every layout this plan holds has its map (value_mapped), large enough for the triangle's entries in values of vsz bytes
    // (follows): aoclsparse_mi355_?revalue_device can carry the plan over
    bool value_mapped() const
    {
        return valid && (rows_valid || blk.valid) && (!rows_valid || psrc.ptr) && (!blk.valid || blk.psrc.ptr);
    }
    bool follows(size_t vsz) const
    {
        const size_t ne = (size_t)std::max<aoclsparse_int>(nnz_tri, 0);
        return value_mapped() && (!rows_valid || (psrc.bytes >= sizeof(int) * ne && pval.bytes >= vsz * ne))
               && (!blk.valid || (blk.psrc.bytes >= sizeof(int) * ne && blk.pval.bytes >= vsz * ne));
    }
};

// host CSR view; owned==true when the library allocated the arrays (clean copy / transpose)
struct HostCsr
{
    aoclsparse_int        m = 0, n = 0, nnz = 0;
    aoclsparse_index_base base  = aoclsparse_index_base_zero;
    aoclsparse_int       *ptr   = nullptr;
    aoclsparse_int       *ind   = nullptr;
    void                 *val   = nullptr;
    aoclsparse_int       *idiag = nullptr; // owned whenever non-null
    aoclsparse_int       *iurow = nullptr;
    bool                  owned        = false;
    bool                  is_optimized = false;
    // owned ind / val came from host_result_alloc (sp2m results: 2 MB-aligned, huge pages asked for) and are freed with free()
    bool                  result_arrays = false;
    ~HostCsr();
};
// Host arrays a product hands back (sp2m): a copy out of HBM first-touches them, and on a fresh new[] that costs more than the
// copy -- 156 MB: 11.6-27 ms in 4 KB pages whatever the number of touching threads, 1.1 ms as 2 MB pages touched by 16 threads
// (tools/history/pagefault_probe.cpp on the GPU box).  2 MB-aligned + MADV_HUGEPAGE from 4 MB up, plain malloc below; released with free().
void *host_result_alloc(size_t bytes);
void  host_result_touch(void *p, size_t bytes); // first touch by several threads (no-op for small arrays)
constexpr size_t HOST_RESULT_BIG = (size_t)4 << 20; // ... that is, for fewer bytes than this; huge pages from here up

// A general CSR derived from the clean CSR so that the general kernels can serve a symmetric or
// triangular descriptor: key = (type, fill, diag, transposed).
struct Derived
{
    int       type = 0, fill = 0, diag = 0, trans = 0;
    HostCsr   host; // owned, 0-based, sorted rows
    DeviceCsr dev;
    SpmvPlan  plan;
    // aoclsparse_mi355_build_operator_device (device_handle_api.cpp, derived_kernels.hip) built it in HBM: host is then a copy back
    // of dev.  mapped: src holds, per entry of dev.val, where its value comes from -- the 0-based position in the clean CSR's value
    // array, DERIVED_SRC_CONJ set when the value is the conjugate of that entry, DERIVED_SRC_CONST for a constant (the one of a unit
    // diagonal) -- recorded while the handle's keep_value_maps flag is set: ?revalue_device gathers dev.val again through it.
    bool         on_device = false, mapped = false;
    DeviceBuffer src;
    void         drop_value_map() { src.release(), mapped = false; }
    // ?revalue_device can carry the operator over (together with the clean CSR its map indexes): values of vsz bytes
    bool follows(size_t vsz) const
    {
        const size_t ne = (size_t)std::max<aoclsparse_int>(host.nnz, 1);
        return mapped && src.ptr && dev.valid && dev.nnz == host.nnz && host.val && src.bytes >= sizeof(unsigned) * ne
               && dev.val.bytes >= vsz * ne;
    }
};
constexpr unsigned DERIVED_SRC_CONJ = 0x80000000u, DERIVED_SRC_CONST = 0xffffffffu;

// What a value change leaves standing, as drop_derived_state reads it: the copies that have the new values already.  A default one
// keeps nothing; anything else comes from values_kept (device_handle_api.cpp), which asks every kind of copy for its `follows` and ties
// the members together: diagonal and operators only with the clean CSR, plans only with the diagonal, SELL-64 only with the mirror.
struct ValuesKept
{
    bool     mirror    = false; // dev_user stays valid
    bool     clean = false, diag = false; // the clean CSR (and clean_src with a copy); dev_diag and diag_src
    bool     sell      = false; // the STRUCTURE of plan_user's SELL-64 copy (SellPlan::stale: the next build_sell refills its cells)
    unsigned plans     = 0; // bit i: trsv_plan[i]
    bool     operators = false; // the derived operators that follow (Derived::follows), each with the structure of its SELL-64 copy
};

} // namespace mi355

// ---- matrix handle (library/src/include/aoclsparse_mat_structures.hpp:774-859) -------------
struct _aoclsparse_matrix
{
    aoclsparse_int                m = 0, n = 0, nnz = 0;
    aoclsparse_index_base         base         = aoclsparse_index_base_zero;
    aoclsparse_matrix_data_type   val_type     = aoclsparse_dmat;
    aoclsparse_matrix_format_type input_format = aoclsparse_csr_mat;
    int                           sort         = 0; // aoclsparse_matrix_sort
    bool                          fulldiag     = false;
    aoclsparse_memory_usage       mem_policy   = aoclsparse_memory_usage_unrestricted;
    bool                          optimized    = false;
    bool                          opt_csr_full_diag = false;

    mi355::HostCsr                  user; // aliases the caller's arrays
    std::unique_ptr<mi355::HostCsr> opt_copy; // clean copy when the user arrays are not clean
    mi355::HostCsr                 *opt = nullptr; // clean CSR: &user or opt_copy.get()
    std::unique_ptr<mi355::HostCsr> trans; // A^T of the user CSR (built for gt hints / first use)

    std::vector<mi355::Hint> hints; // newest first (csr_util.cpp:47-100 prepends)

    // device side; guarded by `guard` (executors take it shared, builders exclusive)
    mi355::DeviceCsr dev_user, dev_trans;
    mi355::SpmvPlan  plan_user, plan_trans;
    mi355::TrsvPlan  trsv_plan[6]; // index: trsv_plan_index (trsv_schedule.hpp)
    mi355::DeviceBuffer dev_diag; // diagonal values of the clean CSR (length min(m,n))
    // Value maps (round 25, device_handle_api.cpp).  keep_maps: what is built from now on records where its values come from, so
    // that aoclsparse_mi355_?revalue_device can bring new values to it instead of dropping it.  clean_src: per entry of the clean
    // COPY (opt_copy) its 0-based position in the user's value array, -1 for an inserted zero -- only aoclsparse_mi355_clean_csr_device
    // records it, and it goes with the copy.  diag_src: per row the clean position dev_diag's item comes from, or -1; goes with
    // dev_diag.  The TRSV layouts' maps hang on their plans.  None of them is a copy of the values.
    bool                keep_maps = false;
    mi355::DeviceBuffer clean_src, diag_src;
    // observers (aoclsparse_mi355_get_value_map_info): builds that did work since the handle was created, successful revalues
    long long plan_builds = 0, clean_builds = 0, revalues = 0;
    int       last_kept_plans = 0;
    void      drop_value_maps()
    {
        clean_src.release(), diag_src.release();
        for(auto &p : trsv_plan)
            p.drop_value_maps();
        for(auto &d : derived)
            d->drop_value_map();
    }
    // ?revalue_device can carry over: the clean CSR, the user's arrays or a copy with its map; the diagonal (vsz bytes a value) with its map
    bool clean_follows() const
    {
        return opt && (opt == &user || (opt == opt_copy.get() && opt->val && clean_src.ptr && clean_src.bytes >= sizeof(int) * (size_t)opt->nnz));
    }
    bool diag_follows(size_t vsz) const
    {
        return dev_diag.ptr && diag_src.ptr && dev_diag.bytes >= vsz * (size_t)m
               && diag_src.bytes >= sizeof(int) * (size_t)std::max<aoclsparse_int>(m, 1);
    }
    mi355::DeviceBuffer trsv_scratch; // ticket (one per right-hand side) + timeout words of the sync-free solve
    mi355::DeviceBuffer trsv_xp; // solution(s) in level order, m x nrhs (stream-ordered reuse)
    // the stream of the last call that used the handle's workspaces (the two above, `work` below): they are reused in stream
    // order, so a call on ANOTHER stream first waits for the device -- not for that stream, which the caller may have destroyed
    // since (workspace_stream_guard; written under the runtime's stage lock)
    void              *ws_last_stream = nullptr;
    unsigned long long ws_last_uid    = 0; // hipStreamGetId: a recycled stream address is another stream
    bool               ws_ran         = false;
    // one word of pinned, device-mapped host memory THIS handle's sync-free solves set when a wait expires (round 3,
    // the process-wide word of round 2 could not say which handle had failed, and a failure surfaced on an
    // unrelated solve).  Allocated at the handle's first sync-free solve; read without a device round trip.
    volatile unsigned int *trsv_timeout_host = nullptr;
    unsigned int          *trsv_timeout_dev  = nullptr;

    // matrices derived from the clean CSR for non-general descriptors (symmetric expansion,
    // triangular slices), built on first use: see derived.cpp
    std::vector<std::unique_ptr<mi355::Derived>> derived;
    // observers (aoclsparse_mi355_get_operator_info), since the handle was created: operators built in HBM / on the host, the
    // operators the last successful ?revalue_device carried over, the operators value changes have dropped
    long long op_device_builds = 0, op_host_builds = 0, op_dropped_by_value_change = 0;
    int       op_followed = 0;

    // sp2m stage-1 state (C handles own their arrays)
    bool owns_user_arrays = false;
    // does a row of the user CSR hold a column twice?  -1: not looked at yet (sy_dense_api.cpp looks once; the pattern of a
    // handle never changes)
    std::atomic<int> repeated_cols{-1};

    // other input formats (formats_api.cpp): the caller's CSC arrays of a handle created from CSC (its CSR
    // lives in `user`, owned), or the caller's COO arrays (input_format == aoclsparse_coo_mat, no CSR)
    aoclsparse_int *csc_ptr = nullptr, *csc_ind = nullptr;
    void           *csc_val = nullptr;
    int             csc_sort = 0; // sort class of those CSC arrays (`sort` is the class of the CSR in `user`)
    aoclsparse_int *coo_row = nullptr, *coo_col = nullptr;
    void           *coo_val = nullptr;
    // the map of the triplet sort, kept on request (aoclsparse_mi355_coo_keep_map; device_handle_api.cpp): coo_pos[q] = the triplet
    // that sorted entry q came from (coo_map_triplets ints), in `sum` mode coo_runs[o] = where the run of CSR entry o starts among
    // the sorted entries (nnz + 1 ints).  They index the handle's value array as it was created: aoclsparse_order_mat releases them;
    // value changes leave them alone.  Not a copy of the values, so drop_derived_state does not come here.
    mi355::DeviceBuffer coo_pos, coo_runs;
    bool                coo_map_kept = false;
    aoclsparse_int      coo_map_mode = 0, coo_map_triplets = 0;
    void                drop_coo_map()
    {
        coo_pos.release(), coo_runs.release();
        coo_map_kept = false, coo_map_mode = coo_map_triplets = 0;
    }
    // TCSR (input_format == aoclsparse_tcsr_mat, no CSR in `user`): [0] = L, [1] = U, each a CSR handle of its own that aliases the
    // caller's three arrays of that triangle (L: the diagonal ends every row, U: it starts every row).  Every copy of the values --
    // device mirrors, TRSV plans, symmetric / triangular expansions -- hangs on these two (drop_derived_state walks them)
    aoclsparse_matrix tcsr_tri[2] = {nullptr, nullptr};
    // BSR (input_format == aoclsparse_bsr_mat, no CSR in `user`): the block pattern as a CSR of bM x bN blocks (`bsr`: m = bM,
    // n = bN, nnz = blocks) whose value array holds bsr_dim^2 values per block in bsr_order.  The arrays are the caller's
    // (aoclsparse_create_?bsr) or owned (aoclsparse_convert_bsr: bsr.owned).  dev_bsr is their one mirror in HBM, uploaded at the
    // first product and dropped by drop_derived_state
    mi355::HostCsr   bsr;
    aoclsparse_int   bsr_dim   = 0;
    aoclsparse_order bsr_order = aoclsparse_order_column;
    mi355::DeviceCsr dev_bsr;

    // composite solvers (solvers_api.cpp): vector workspaces in HBM, and the ILU(0) factors
    // (solvers/aoclsparse_ilu.hpp:94-104, analysis.cpp:390-425): values on the user's pattern, kept
    // on the host for *precond_csr_val and mirrored by a factor handle whose TRSV plans do the solves
    mi355::DeviceBuffer work[6];
    bool                ilu_ready = false, ilu_factorized = false;
    void               *ilu_val = nullptr; // nnz values, library-owned (malloc)
    aoclsparse_matrix   ilu_factor = nullptr; // aliases user.ptr / user.ind / ilu_val
    // What the factorisation computes from the PATTERN, kept from the first factorisation on (the smoother's or
    // aoclsparse_mi355_?ilu0_refactor_device's) for every later one: the rows in level order (in HBM), where each level starts,
    // the longest row, and the two choices made from them -- one launch per level or the sync-free launch, and the row routine
    // that finds the updated position by a scan or by a binary search (ilu_kernels.hip).  Value changes leave it alone; whatever
    // changes the pattern or its order releases it (aoclsparse_order_mat, order_mat_device, aoclsparse_mi355_invalidate).
    struct IluSchedule
    {
        bool                        valid = false;
        mi355::DeviceBuffer         rows; // n row numbers, level by level
        std::vector<aoclsparse_int> level_ptr; // nlevels + 1
        aoclsparse_int              nlevels = 0, max_row = 0;
        bool                        syncfree = false, search = false;
        void                        release()
        {
            valid = false, rows.release(), level_ptr.clear(), level_ptr.shrink_to_fit();
            nlevels = max_row = 0, syncfree = search = false;
        }
    } ilu_sched;
    // observers (aoclsparse_mi355_get_ilu_info): times the levels were computed, successful factorisations, and the TRSV plans of
    // the factor handle the last refactorisation carried over
    long long ilu_analyses = 0, ilu_factorizations = 0;
    int       ilu_plans_kept_last = 0;
    // What aoclsparse_mi355_sp2m_numeric_device computes from this handle's ROW POINTER when the handle is the C of a product
    // (spg_product.cpp: sp2m_plan_build): the rows binned by their exact length, as the fill pass of spgemm_hash_kernel bins them.
    // In HBM, in buffers of its own: the row order (absent when one LDS bin holds every row) and the records of the rows of the
    // global slab; on the host what the launches need, the bin bounds, the batch list and the slab's sizes.  Structure only: value
    // changes leave it alone, and it is released exactly where ilu_sched is.  Written under the runtime's stage lock.
    struct Sp2mPlan
    {
        bool                        valid = false;
        aoclsparse_int              bounds[5 + 1] = {}; // SPGEMM_BINS + 1
        mi355::DeviceBuffer         order, heavy; // m row numbers bin by bin; SpgHeavy records in batches
        std::vector<aoclsparse_int> batch; // batch b = records [batch[b], batch[b + 1])
        long long                   slots = 0, entries = 0; // table slots / list entries of the largest batch
        void                        release()
        {
            valid = false, order.release(), heavy.release(), batch.clear(), batch.shrink_to_fit();
            std::fill(bounds, bounds + 6, 0), slots = entries = 0;
        }
        void adopt(Sp2mPlan &o)
        {
            valid = o.valid, std::copy(o.bounds, o.bounds + 6, bounds), order.adopt(o.order), heavy.adopt(o.heavy);
            batch = std::move(o.batch), slots = o.slots, entries = o.entries;
            o.release();
        }
        long long bytes() const
        {
            return valid ? (long long)(order.bytes + heavy.bytes + sizeof(aoclsparse_int) * batch.size() + sizeof(bounds)) : 0;
        }
    } sp2m_plan;
    // observers (aoclsparse_mi355_get_sp2m_plan_info): times the plan was built, successful numeric calls, calls the verdict stopped
    long long sp2m_plan_builds = 0, sp2m_numeric_runs = 0, sp2m_refused = 0;

    // multi-device calls (aoclsparse_mi355_?csrmm_multi): replica[i] = a handle over the SAME host arrays whose device copy
    // and plans live on the device of runtime slot i (slot 0 is this handle itself); built on first use, dropped by
    // aoclsparse_mi355_invalidate / ?set_value / ?update_values and by aoclsparse_destroy
    std::vector<aoclsparse_matrix> replicas;
    int                            replicas_cloned = 0; // of them: device state copied device to device instead of re-analysed

    mutable std::shared_mutex guard;
};

namespace mi355
{
// identity of a stream beyond its address (the runtime reuses the address of a destroyed stream for a new one): hipStreamGetId
// where the loaded HIP runtime has it (ROCm >= 7.1; looked up at run time -- the process may run on the older runtime a
// framework bundles), else 0 for every stream (the address alone decides, as in rounds 1-5)
unsigned long long stream_uid(hipStream_t s);
// call with the runtime's stage lock held, before a handle's workspaces are touched on stream s
inline aoclsparse_status workspace_stream_guard(_aoclsparse_matrix *A, hipStream_t s)
{
    const unsigned long long uid = stream_uid(s);
    if(A->ws_ran && (A->ws_last_stream != (void *)s || A->ws_last_uid != uid))
        MI355_HIP_TRY(hipDeviceSynchronize());
    A->ws_last_stream = (void *)s, A->ws_last_uid = uid, A->ws_ran = true;
    return aoclsparse_status_success;
}
} // namespace mi355

namespace mi355
{

// ---- staging buffers by name -------------------------------------------------------------------
// Who owns which of the runtime's staging buffers (Runtime::staging).  A number that several families use has ONE primary name;
// the others are aliases declared right under it, each with the reason why the two are never live together on one thread.  The
// entry points of the aliases are leaves: each stages, launches and finishes inside one CallScope and calls no other entry point
// while its views are live, unless its line says otherwise.  (Composite routines -- symgs, the ILU smoother, the iterative
// solvers -- run the executors inside a DeviceScope, where nothing is staged.)  No nesting was found in which one number is live
// twice on a thread.
enum StageSlot : int
{
    // -- 0-2: the three CSR arrays of a raw-array call
    STAGE_CSR_VAL = 0, // ?csrmv: val
    STAGE_TRSV_B  = STAGE_CSR_VAL, // ?trsv / ?trsm b: a solve runs on a handle and calls no raw-array product
    STAGE_L1_X    = STAGE_CSR_VAL, // level 1 x: leaf
    STAGE_C2D_PTR = STAGE_CSR_VAL, // csr2dense row_ptr: leaf
    STAGE_CSR_COL, // ?csrmv: col_ind
    STAGE_L1_IND  = STAGE_CSR_COL, // level 1 indx: leaf
    STAGE_C2D_COL = STAGE_CSR_COL, // csr2dense col_ind: leaf
    STAGE_CSR_PTR, // ?csrmv: row_ptr
    STAGE_TRSV_X  = STAGE_CSR_PTR, // ?trsv / ?trsm x: as STAGE_TRSV_B
    STAGE_L1_Y    = STAGE_CSR_PTR, // level 1 y: leaf
    STAGE_C2D_VAL = STAGE_CSR_PTR, // csr2dense val: leaf
    // -- 3-4: the dense operands of a product
    STAGE_MV_X, // x of ?mv, ?csrmv, ?dotmv, ell / ellt / ellthyb / blkcsr mv and the BSR handle product
    STAGE_CSRMM_B = STAGE_MV_X, // ?csrmm B: csrmm calls no mv
    STAGE_L1_DOT  = STAGE_MV_X, // ?doti partial sums and result: leaf.  (Not a nesting, but noted: in device-pointer mode ?doti takes
                                // no stage lock, so two THREADS calling it at once share this buffer; as before this enum.)
    STAGE_MV_Y, // y of the same products; ?dotmv stages y here again AFTER its ?mv has finished (copied back and synchronised)
    STAGE_CSRMM_C = STAGE_MV_Y, // ?csrmm C: csrmm calls no mv
    STAGE_DENSE_C = STAGE_MV_Y, // C of ?syrkd / ?syprd / ?sp2md / ?spmmd, A of csr2dense: their kernels are their own, no mv inside
    // -- 5-7
    STAGE_CSRMM_BT, // the csrmm detour's row-major copy of B (taken under the stage lock whatever the pointer mode)
    STAGE_SYPRD_B = STAGE_CSRMM_BT, // ?syprd B: syprd runs launch_syprd only, never csrmm
    STAGE_CSRMM_CT, // the csrmm detour's row-major copy of C
    STAGE_SYPRD_SCRATCH = STAGE_CSRMM_CT, // ?syprd's m_c x n_in intermediate: as STAGE_SYPRD_B
    STAGE_DOTMV_PART    = STAGE_CSRMM_CT, // ?dotmv partial sums: taken after its ?mv has finished; mv never takes the detour
    STAGE_DOTMV_D, // ?dotmv: the result scalar of a host d
    // -- 8-15: the raw-array formats (ELL family, BLKCSR, DIA, BSR): all leaves
    STAGE_ELL_VAL,
    STAGE_BLK_MASKS = STAGE_ELL_VAL,
    STAGE_DIA_VAL   = STAGE_ELL_VAL,
    STAGE_BSR_VAL   = STAGE_ELL_VAL,
    STAGE_ELL_COL,
    STAGE_BLK_VAL    = STAGE_ELL_COL,
    STAGE_DIA_OFFSET = STAGE_ELL_COL,
    STAGE_BSR_COL    = STAGE_ELL_COL,
    STAGE_HYB_CSR_VAL, // ellthybmv: the CSR part of the long rows (val, col, row, row map)
    STAGE_BLK_COL = STAGE_HYB_CSR_VAL,
    STAGE_FMT_X   = STAGE_HYB_CSR_VAL, // x of diamv / bsrmv (the ELL family and BLKCSR stage x and y in STAGE_MV_X / _Y)
    STAGE_HYB_CSR_COL,
    STAGE_BLK_PTR = STAGE_HYB_CSR_COL,
    STAGE_FMT_Y   = STAGE_HYB_CSR_COL, // y of diamv / bsrmv
    STAGE_HYB_CSR_PTR,
    STAGE_BSR_PTR = STAGE_HYB_CSR_PTR,
    STAGE_HYB_ROWMAP,
    STAGE_HYB_YTMP, // ellthybmv: the long rows' y across the ELL pass
    STAGE_BLK_VALOFF = STAGE_HYB_YTMP,
    STAGE_BLK_PARTS,
    // -- 16-39: one first-touch product D = X * Y (sp2m, syrk, sypr; SpgProduct in spg_product.cpp).  The caller holds the stage
    // lock from analyse() to the last pass.
    SPG_SLOT_XP, // operands that no handle keeps resident: X (ptr, ind, val), then Y
    SPG_SLOT_XI,
    SPG_SLOT_XV,
    SPG_SLOT_YP,
    SPG_SLOT_YI,
    SPG_SLOT_YV,
    SPG_SLOT_CNT, // the list size of every row: the counts themselves
    SPG_SLOT_ORDER_COUNT,
    SPG_SLOT_ORDER_FILL,
    SPG_SLOT_HEAVY_COUNT,
    SPG_SLOT_HEAVY_FILL,
    SPG_SLOT_G_KEY,
    SPG_SLOT_G_POS,
    SPG_SLOT_G_LIST,
    SPG_SLOT_G_ACC,
    SPG_SLOT_CAP,
    SPG_SLOT_SMALL,
    SPG_SLOT_SCAN,
    SPG_SLOT_HEAVY_KEYS,
    SPG_SLOT_TP, // sypr: the intermediate product T = sym(B) * A (ptr, ind, val), which never leaves HBM
    SPG_SLOT_TI,
    SPG_SLOT_TV,
    SPG_SLOT_CP, // syrk / sypr: the result before it goes to the handle's host arrays (ptr, ind; val: SPG_SLOT_CV)
    SPG_SLOT_CI,
    // -- 40-45: the temporaries of the device transpose (transpose_kernels.hip).  Names of their own because they ARE live inside
    // another family: sp2m / syrk / sypr transpose operands while the SPG slots are in use.
    STAGE_TR_CNT,
    STAGE_TR_SMALL,
    STAGE_TR_CURSOR,
    STAGE_TR_TPOS,
    STAGE_TR_SCAN,
    STAGE_TR_ORDER,
    SPG_SLOT_CV, // 46: the values of the syrk / sypr result
    STAGE_UNUSED_47,
    // -- 48-58: the triplet sort (coo_sort_kernels.hip); a handle is created from triplets outside every product
    COO_SLOT_KEY_A,
    COO_SLOT_POS_A,
    COO_SLOT_KEY_B,
    COO_SLOT_POS_B,
    COO_SLOT_HIST,
    COO_SLOT_OFFS,
    COO_SLOT_SCAN,
    COO_SLOT_SMALL,
    COO_SLOT_CNT,
    COO_SLOT_FLAG,
    COO_SLOT_RUNS,
    STAGE_SLOT_COUNT
};
// every site keeps the buffer it has always used (what aoclsparse_mi355_release_staging reports depends on it)
static_assert(STAGE_MV_Y == 4 && STAGE_DOTMV_D == 7 && STAGE_BLK_PARTS == 15 && SPG_SLOT_XP == 16 && STAGE_TR_CNT == 40
                  && SPG_SLOT_CV == 46 && COO_SLOT_KEY_A == 48 && STAGE_SLOT_COUNT == 59,
              "StageSlot: a slot moved");
// The row sort of aoclsparse_mi355_order_mat_device (order_kernels.hip) under names of its own.  A handle is ordered outside every
// product, under the stage lock from its first slot to the drain, so slots of the product family serve; the long rows go through the
// COO_SLOT_* of the triplet sort, which is not running either.
constexpr StageSlot ORD_SLOT_KEY   = SPG_SLOT_XP; // per row: its length when it has to be sorted, 0 otherwise
constexpr StageSlot ORD_SLOT_ORDER = SPG_SLOT_XI; // the rows by bin
constexpr StageSlot ORD_SLOT_SMALL = SPG_SLOT_XV; // histogram, cursors, flags
constexpr StageSlot ORD_SLOT_SCAN  = SPG_SLOT_YP;
constexpr StageSlot ORD_SLOT_LEN   = SPG_SLOT_YI; // the lengths of the long rows, in list order
constexpr StageSlot ORD_SLOT_OFF   = SPG_SLOT_YV; // ... and their prefix sum: where a long row starts among the compacted entries
constexpr StageSlot ORD_SLOT_MAJOR = SPG_SLOT_CNT; // per compacted entry: its long row's place in the list; behind the sort its sorted column
constexpr StageSlot ORD_SLOT_MINOR = SPG_SLOT_ORDER_COUNT; // per compacted entry: its column
constexpr StageSlot ORD_SLOT_VAL   = SPG_SLOT_ORDER_FILL; // the sorted values of the long rows before they go back
// The per-row temporaries of aoclsparse_mi355_clean_csr_device (clean_csr_kernels.hip) under names of their own.  device_order_rows
// runs INSIDE that call (on a copy of an unsorted handle's columns and values), so these are product slots that ORD_SLOT_* and the
// triplet sort's COO_SLOT_* do not name; a clean copy is built outside every product, under the stage lock to the drain.
constexpr StageSlot CLN_SLOT_AT   = SPG_SLOT_HEAVY_COUNT; // per row: the offset of its first entry at or right of the diagonal
constexpr StageSlot CLN_SLOT_MISS = SPG_SLOT_HEAVY_FILL; // per row: 1 when a diagonal entry is inserted
constexpr StageSlot CLN_SLOT_CNT  = SPG_SLOT_G_KEY; // per row: the clean row length
constexpr StageSlot CLN_SLOT_SCAN = SPG_SLOT_G_POS;
// the k-th slot after a named one (the ptr / ind / val triples of an operand; the A / B pair of the sort)
constexpr StageSlot operator+(StageSlot s, int k)
{
    return static_cast<StageSlot>(static_cast<int>(s) + k);
}

// ---- runtime (one process per GPU; uses the current HIP device) ----------------------------
class Runtime
{
public:
    // The calling thread's runtime: the primary one (the process's GPU), unless a RuntimeScope put a secondary slot in
    // charge (in-library multi-device calls, csrmm_api.cpp: one worker thread per device).
    static Runtime &get();
    static Runtime &primary();
    // secondary slot idx >= 1 bound to HIP device `dev` (created on first use; own stream, staging buffers and pinned words).
    // Two slots may name the same device: that is how the multi-device control flow is tested on a one-GPU box.
    static Runtime *slot(int idx, int dev);
    static std::vector<Runtime *> secondary(); // the slots created so far
    aoclsparse_status init(); // lazy; internal_error when no device; binds the calling thread to `device`
    void              bind_thread();
    hipStream_t       stream() const
    {
        return stream_;
    }
    void set_stream(hipStream_t s)
    {
        stream_ = s;
    }
    aoclsparse_mi355_pointer_mode pointer_mode = aoclsparse_mi355_pointer_auto;
    // TRSV schedule: -1 = chosen from the plan (default); 0..5 force one (aoclsparse_mi355_set_trsv_schedule; trsv_api.cpp)
    int trsv_schedule = -1;
    // true when p is memory the device can dereference (device or managed allocation)
    bool is_device_pointer(const void *p);
    int  device = -1, cus = 0;
    char name[256] = {0};
    // scratch staging buffers for host-pointer calls (grown on demand, reused)
    aoclsparse_status staging(StageSlot slot, size_t bytes, void **out);
    size_t            release_staging(); // frees every slot (after the stream has drained); bytes freed
    // Host <-> device copies of PAGEABLE caller memory on the library's stream (plain stream-ordered copies: the runtime's own
    // staging runs at 56 GB/s on these boxes; h2d returns once enqueued, d2h likewise -- callers synchronise the stream)
    aoclsparse_status h2d(void *dev, const void *host, size_t bytes);
    aoclsparse_status d2h(void *host, const void *dev, size_t bytes);
    hipEvent_t        ev0 = nullptr, ev1 = nullptr;
    // per-iteration timing: a ring of events recorded by aoclsparse_mi355_timer_mark (runtime.cpp)
    std::vector<hipEvent_t> marks;
    size_t                  marks_used = 0;
    // sync-free TRSV: one word of pinned, device-mapped host memory a kernel sets when a wait expires.  The host reads
    // it without a device round trip: right after the stream sync of a host-pointer solve, and at the START of the next
    // solve for device-pointer callers (which therefore stay asynchronous).
    volatile unsigned int *trsv_timeout_host = nullptr;
    unsigned int          *trsv_timeout_dev  = nullptr;
    // second word of the same pinned line: "cached raw-csrmv plan does not match this row_ptr" (spmv_api.cpp)
    volatile unsigned int *plan_stale_host = nullptr;
    unsigned int          *plan_stale_dev  = nullptr;
    std::mutex        lock;
    std::recursive_mutex stage_lock; // serialises calls that stage host buffers

    int forced_device = -1; // secondary slots: the device to bind to (the primary honours AOCLSPARSE_MI355_DEVICE / the current device)

private:
    std::atomic<bool> inited_{false}; // set (release) after init_status_ / device / events are written
    aoclsparse_status init_status_ = aoclsparse_status_success;
    hipStream_t  stream_ = nullptr;
    DeviceBuffer stage_[STAGE_SLOT_COUNT]; // one per StageSlot, which says who owns it
};

// While one of these is alive on a thread, Runtime::get() on that thread is the given slot: its device is current, its
// stream / staging buffers are used and handles built under it live on its device.  Settings of the primary runtime
// (pointer mode, csrmm beta = 0 policy) are inherited at entry.
struct RuntimeScope
{
    explicit RuntimeScope(Runtime *r);
    ~RuntimeScope();
    RuntimeScope(const RuntimeScope &)            = delete;
    RuntimeScope &operator=(const RuntimeScope &) = delete;
    Runtime          *prev;
    aoclsparse_status status;
};

// While one of these is alive on a thread, every pointer handed to the executors by that thread is
// taken as device memory: composite routines (symgs, ilu smoother, iterative solvers) chain the
// executors on their own HBM workspaces whatever pointer mode the caller selected.
struct DeviceScope
{
    DeviceScope();
    ~DeviceScope();
    DeviceScope(const DeviceScope &)            = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
};

} // namespace mi355

#include "staging.hpp" // CallScope: the host-pointer arguments of one call

namespace mi355
{

// ---- host analysis (matrix.cpp) --------------------------------------------------------------
aoclsparse_status mat_check(aoclsparse_int maj, aoclsparse_int mind, aoclsparse_int nnz,
                            const aoclsparse_int *ptr, const aoclsparse_int *ind, const void *val,
                            int shape, aoclsparse_index_base base, int &sort, bool &fulldiag);
aoclsparse_status check_sort_diag(aoclsparse_int m, aoclsparse_int n, aoclsparse_index_base base,
                                  const aoclsparse_int *ptr, const aoclsparse_int *ind, bool &sorted,
                                  bool &fulldiag);
aoclsparse_status csr_indices(aoclsparse_int m, aoclsparse_index_base base,
                              const aoclsparse_int *ptr, const aoclsparse_int *ind,
                              aoclsparse_int **idiag, aoclsparse_int **iurow);
// builds A->opt (clean CSR + idiag/iurow) if absent; thread-safe (double-checked)
aoclsparse_status csr_optimize(aoclsparse_matrix A);
// forget every copy derived from the user's arrays (clean CSR, transposes, device mirrors, SELL, TRSV plans) except what `kept` names,
// each value map with its holder; dev_user.valid ends as kept.mirror.  -> the operators that went (a value change counts them)
size_t drop_derived_state(aoclsparse_matrix A, const ValuesKept &kept = {});
// drop_derived_state, and with it what indexes the entries in their order within the rows (the triplet map, the ILU(0) schedule):
// for whoever has sorted the rows (kept: the mirror alone, when it was sorted in place and IS the handle's CSR now)
void drop_order_dependent_state(aoclsparse_matrix A, const ValuesKept &kept = {});
// the statuses of aoclsparse_?update_values, in its order, all decided before the handle is locked (matrix.cpp);
// aoclsparse_mi355_?update_values_device / ?revalue_device append theirs (device_handle_api.cpp)
aoclsparse_status update_values_status(const _aoclsparse_matrix *A, aoclsparse_int len, const void *val, aoclsparse_matrix_data_type vt);
// value mutation on handles created from CSC / COO arrays (formats_api.cpp): the caller's arrays are the first
// representation there; csc_refresh_csr rebuilds the handle's CSR values from the CSC arrays
aoclsparse_status coo_set_value(aoclsparse_matrix A, aoclsparse_int row_idx, aoclsparse_int col_idx, const void *val);
void              csc_set_value(aoclsparse_matrix A, aoclsparse_int row_idx, aoclsparse_int col_idx, const void *val);
aoclsparse_status csc_refresh_csr(aoclsparse_matrix A);
// a handle over the caller's CSR arrays, nothing checked (the creators check first)
aoclsparse_status alias_csr(aoclsparse_matrix *mat, aoclsparse_index_base base, aoclsparse_int M, aoclsparse_int N, aoclsparse_int nnz,
                            aoclsparse_int *row_ptr, aoclsparse_int *col_idx, void *val, aoclsparse_matrix_data_type vt, int sort,
                            bool fulldiag);
// the triangle of a TCSR handle that serves descriptors of this fill mode (L also for anything that is not `upper`)
inline aoclsparse_matrix tcsr_triangle(const _aoclsparse_matrix *A, aoclsparse_fill_mode fill)
{
    return A->tcsr_tri[fill == aoclsparse_fill_mode_upper ? 1 : 0];
}
// TCSR and BSR handles hold valid arrays of their own format and no CSR in `user`: a null user.ptr is no missing pointer there,
// the format checks that follow decide
inline bool holds_no_csr(const _aoclsparse_matrix *A)
{
    return A->input_format == aoclsparse_tcsr_mat || A->input_format == aoclsparse_bsr_mat;
}
// allocates the ILU(0) value array as a copy of A's values (solvers_api.cpp; analysis.cpp:390-425)
aoclsparse_status ilu_prepare(aoclsparse_matrix A);
// aoclsparse_mi355_?revalue_device on a handle of whatever value type it has (device_handle_api.cpp): `val` = nnz values in HBM.
// The route a new ILU(0) factor takes into its factor handle (solvers_api.cpp)
aoclsparse_status revalue_device_any(aoclsparse_matrix A, aoclsparse_int len, const void *val);
// builds A->trans (host transpose of the user CSR, 0-based) if absent
aoclsparse_status build_transpose(aoclsparse_matrix A);
// B = A^T of a device CSR in the reference's counting-sort order (transpose_kernels.hip), into buffers it allocates once the matrix
// is accepted; aoclsparse_status_not_implemented when a column is too long for the device sort (the caller sorts on the host; the
// three buffers are then empty)
aoclsparse_status device_transpose(hipStream_t s, aoclsparse_int m, aoclsparse_int n, aoclsparse_int nnz, int base,
                                   const aoclsparse_int *d_ptr, const aoclsparse_int *d_ind, const void *d_val, size_t vsize,
                                   DeviceBuffer &tptr, DeviceBuffer &tind, DeviceBuffer &tval);
// The operator build_derived (derived.cpp) makes of a clean CSR, built in HBM (derived_kernels.hip): the clean CSR of an m x n matrix
// with its idiag / iurow (positions in `base`, as the host arrays hold them) and nnz values of vsize bytes (cplx: a pair of reals),
// all in HBM, and the operator's key.
struct DerivedDeviceIn
{
    aoclsparse_int          m = 0, n = 0, nnz = 0;
    int                     base = 0;
    const aoclsparse_int   *ptr = nullptr, *ind = nullptr, *idiag = nullptr, *iurow = nullptr;
    const void             *val   = nullptr;
    size_t                  vsize = 0;
    bool                    cplx  = false;
    aoclsparse_matrix_type  type  = aoclsparse_matrix_type_symmetric;
    bool                    upper = false, transposed = false;
    aoclsparse_diag_type    diag  = aoclsparse_diag_type_non_unit;
};
// optr (rows + 1), oind, oval and osrc (the source map, Derived::src; nnz items each, one at least): the 0-based operator, bit for
// bit build_derived's, ALLOCATED HERE once the matrix is accepted.  aoclsparse_status_not_implemented when a mirrored row segment is
// longer than the segment sort takes (the caller leaves the operator to the host); on any failure the four buffers are empty.
// The caller holds the stage lock; returns with the stream drained.
aoclsparse_status device_build_derived(hipStream_t s, const DerivedDeviceIn &in, DeviceBuffer &optr, DeviceBuffer &oind,
                                       DeviceBuffer &oval, DeviceBuffer &osrc, aoclsparse_int *nnz_out);
// CSR arrays (in the triplets' base) from nnz unordered triplets in HBM by a stable radix sort (coo_sort_kernels.hip), into buffers
// it allocates once every index is known to be in range (invalid_index_value otherwise; the buffers are then empty).  sum == false:
// the reference's coo2csr, *nnz_out = nnz; sum == true: sorted by (row, column), equal coordinates added left to right in triplet
// order, *nnz_out = the distinct coordinates.  vsize / cplx: bytes of a value, and whether it is a pair of reals.
// map != nullptr: the sort's map leaves the staging slots too, in buffers allocated here -- map[0] = the final positions (nnz ints),
// in `sum` mode map[1] = the run starts (*nnz_out + 1 ints); both empty again on failure.
aoclsparse_status device_coo_to_csr(hipStream_t s, aoclsparse_int M, aoclsparse_int N, aoclsparse_int nnz, int base,
                                    const aoclsparse_int *row, const aoclsparse_int *col, const void *val, size_t vsize, bool cplx,
                                    bool sum, DeviceBuffer &ptr, DeviceBuffer &ind, DeviceBuffer &valb, aoclsparse_int *nnz_out,
                                    DeviceBuffer *map = nullptr);
// The values of a CSR built by device_coo_to_csr, again, from `triplets` new values in the triplets' order and the map kept then:
// out[q] = val[pos[q]] (sum == false, entries == triplets), or per entry the left-to-right chain over its run (sum == true).
// Enqueued on s, not waited for; reads pos, runs and val, writes `entries` values.
aoclsparse_status device_coo_refresh_values(hipStream_t s, aoclsparse_int triplets, aoclsparse_int entries, bool sum, const int *pos,
                                            const int *runs, const void *val, size_t vsize, bool cplx, void *out);
// The triplet sort's radix passes on their own: `count` (major, minor) pairs in HBM, 0 <= major[i] < major_range and
// 0 <= minor[i] < minor_range, in; *perm out: count ints in a staging slot, perm[q] = the pair that comes q-th in the stable order by
// (major, minor).  The caller holds the stage lock and drains the stream before it lets go (COO_SLOT_KEY_A .. COO_SLOT_SCAN are
// taken); enqueued on s, not waited for.
aoclsparse_status device_sort_pairs(hipStream_t s, aoclsparse_int count, const aoclsparse_int *major, aoclsparse_int major_range,
                                    const aoclsparse_int *minor, aoclsparse_int minor_range, const int **perm);
// Every row of a device CSR into ascending column order, stably, IN PLACE (order_kernels.hip): rows that are ascending already are
// not touched.  ptr is read only.  Takes the stage lock, returns with the stream drained.  On failure the arrays may be half sorted:
// the caller gives them up.  moved (optional): the rows that were sorted.
aoclsparse_status device_order_rows(hipStream_t s, aoclsparse_int m, aoclsparse_int n, aoclsparse_int nnz, int base,
                                    const aoclsparse_int *d_ptr, aoclsparse_int *d_ind, void *d_val, size_t vsize,
                                    long long *moved = nullptr);

// The clean copy of a device CSR (clean_csr_kernels.hip; any base in, 0-based out).  All three are enqueued on s, not waited for.
// mark: per row at / miss / cnt (m ints each) -- the offset of the first entry with column >= i, whether a diagonal entry is to be
// inserted, the clean row length.  expand: the `total` entries of the clean copy to cind / cval, cptr = the exclusive scan of cnt.
// finish: idiag / iurow (positions in cptr; cptr == nullptr: in d_ptr itself, keeping its base) and diag, m items of vsize bytes.
aoclsparse_status launch_clean_mark(hipStream_t s, aoclsparse_int m, aoclsparse_int n, aoclsparse_int nnz, int base,
                                    const aoclsparse_int *d_ptr, const aoclsparse_int *d_ind, int *at, int *miss, int *cnt);
aoclsparse_status launch_clean_expand(hipStream_t s, aoclsparse_int m, aoclsparse_int nnz, aoclsparse_int total, int base,
                                      const aoclsparse_int *d_ptr, const aoclsparse_int *d_ind, const void *d_val, size_t vsize,
                                      const aoclsparse_int *cptr, const int *at, const int *miss, aoclsparse_int *cind, void *cval,
                                      int *csrc = nullptr);
aoclsparse_status launch_clean_finish(hipStream_t s, aoclsparse_int m, aoclsparse_int n, aoclsparse_int nnz, int base,
                                      const aoclsparse_int *d_ptr, const void *d_val, size_t vsize, const aoclsparse_int *cptr,
                                      const int *at, const int *miss, aoclsparse_int *idiag, aoclsparse_int *iurow, void *diag);

// Values through a value map (revalue_kernels.hip; all enqueued on s, not waited for).  gather: out[k] = in[map[k]] for k < count,
// the all-zero item where map[k] < 0, conjugated when conj (items of 8 or 16 bytes only); nsrc = items of `in`.  iota: out[k] = k.
// compose: map[k] = perm[map[k]] where map[k] >= 0, in place.  diag_map: per row the 0-based clean position of its diagonal entry
// (idiag - base where iurow == idiag + 1 and the row is < min(m, n)), else -1.
aoclsparse_status launch_revalue_gather(hipStream_t s, long long count, long long nsrc, const int *map, const void *in, void *out,
                                        size_t vsize, bool conj);
// gather_flagged: the same through a derived operator's map (Derived::src): out[k] = in[map[k] & ~DERIVED_SRC_CONJ], conjugated where
// DERIVED_SRC_CONJ is set (never for items of 4 bytes); out[k] is LEFT AS IT IS where map[k] == DERIVED_SRC_CONST
aoclsparse_status launch_revalue_gather_flagged(hipStream_t s, long long count, long long nsrc, const unsigned *map, const void *in,
                                                void *out, size_t vsize);
aoclsparse_status launch_revalue_iota(hipStream_t s, aoclsparse_int count, int *out);
aoclsparse_status launch_revalue_compose(hipStream_t s, aoclsparse_int count, aoclsparse_int nperm, const int *perm, int *map);
aoclsparse_status launch_revalue_diag_map(hipStream_t s, aoclsparse_int m, aoclsparse_int n, int base, aoclsparse_int total,
                                          const aoclsparse_int *idiag, const aoclsparse_int *iurow, int *out);

// ---- device mirrors / plans (spmv_plan.cpp, sell_plan.cpp) ------------------------------------------
size_t            val_size(aoclsparse_matrix_data_type t);
aoclsparse_status upload_csr(const HostCsr &h, size_t vsize, DeviceCsr &d);
aoclsparse_status ensure_spmv(aoclsparse_matrix A, bool transposed, DeviceCsr *&dcsr,
                              SpmvPlan *&plan);
// symmetric expansion / triangular slice of the clean CSR as a general device CSR (derived.cpp)
aoclsparse_status ensure_derived(aoclsparse_matrix A, aoclsparse_matrix_type type, aoclsparse_fill_mode fill,
                                 aoclsparse_diag_type diag, bool transposed, Derived *&out);
// clean CSR on the device + level sets of one triangle (trsv_plan.cpp)
// need_rows: also the level-ordered row layout (TrsvPlan::rows_valid); false = only what the automatic schedule needs
aoclsparse_status ensure_trsv(aoclsparse_matrix A, bool upper, bool transposed, bool conj = false, bool need_rows = true);
// SELL-64 copy of d (row_ptr_host = the host row pointer d mirrors); leaves plan.sell.valid false when the
// padding would exceed the budget (aoclsparse_mi355_set_option(aoclsparse_mi355_option_sell, 0 / 1): never / always)
aoclsparse_status build_sell(const aoclsparse_int *row_ptr_host, const DeviceCsr &d, size_t vsize, SpmvPlan &plan, bool complex_values = false);
// merge-path tiling (host binary searches over row_ptr_host); built when the longest row spans >= 32 LDS tiles, or when
// aoclsparse_mi355_set_option(aoclsparse_mi355_option_spmv_kernel, ...) asks for it
aoclsparse_status build_merge_plan(aoclsparse_int m, aoclsparse_int nnz, aoclsparse_index_base base,
                                   const aoclsparse_int *row_ptr_host, size_t vsize, SpmvPlan &plan);
aoclsparse_status build_spmv_plan(aoclsparse_int m, aoclsparse_int nnz, aoclsparse_index_base base,
                                  const aoclsparse_int *row_ptr_host, SpmvPlan &plan, size_t vsize = 8);

// ---- kernel launchers (HIP translation units) --------------------------------------------------
// order: 0 scalar, 1 lane4, 2 lane8
template <typename T>
aoclsparse_status launch_csrmv(hipStream_t s, int order, bool strict, int tile, int base, T alpha,
                               aoclsparse_int m, const T *val, const aoclsparse_int *col,
                               const aoclsparse_int *row_ptr, const aoclsparse_int *blocks,
                               aoclsparse_int nblocks, const T *x, T beta, T *y, const aoclsparse_int *blocks4 = nullptr,
                               aoclsparse_int max_row_nnz = 1 << 30, unsigned int *stale = nullptr);
// (stale != nullptr: the block table is a cached plan of a raw-array call -- every workgroup validates its own entry against
// the live row_ptr, computes its rows from the live arrays on a mismatch and sets *stale, a pinned host word)
// SELL-64 plan kernels (sell_build_kernels.hip)
// fills the cells, columns and row lengths of the copy v describes from d (values of vsize bytes; cells / col / rowlen are v's
// arrays, writable); with a table (v.ntab > 0) the cells get one-byte indices into it instead of the values, or (v.pbits > 0) one
// packed word per row (zero words behind m, 0 in the padding cells); ucol (nullable; preset to -1) gets the list of every mode
// 1 / 2 slice.  col == nullptr: the values stage on a KEPT structure -- the cells from d's values alone, neither col nor rowlen
// is written.
aoclsparse_status launch_sell_fill(hipStream_t s, const DeviceCsr &d, size_t vsize, const SellView &v, void *cells, aoclsparse_int *col,
                                   aoclsparse_int *rowlen, aoclsparse_int *ucol);
// behind launch_sell_fill on the same stream, for a copy with uniform lists and one-byte packed words: sets SELL_DESC_UWORD /
// SELL_DESC_EXCEPT in the device records (desc, nslices of them) and writes the canonical list of an exception slice to ucol;
// counts (device, two words, zeroed here) receives how many slices got each flag.  d = the CSR the copy mirrors.
aoclsparse_status launch_sell_records(hipStream_t s, const DeviceCsr &d, const SellView &v, SellSliceDesc *desc, aoclsparse_int *ucol,
                                      unsigned *counts);
// behind launch_sell_records: *verdict (device, zeroed here) becomes 1 when the nslices records or the nslices x SELL_SHORT_WMAX list
// entries of set a differ from those of set b anywhere, and stays 0 when they are equal
aoclsparse_status launch_sell_compare(hipStream_t s, aoclsparse_int nslices, const SellSliceDesc *desc_a, const SellSliceDesc *desc_b,
                                      const aoclsparse_int *ucol_a, const aoclsparse_int *ucol_b, unsigned *verdict);
// distinct bit patterns of n values of vsize (4 / 8) bytes on the device: *ntab of them; table = SELL_VTAB_MAX entries of vsize
// bytes ready to upload, ascending by bit pattern, the unused ones 0; *ntab = 0 when there are more than SELL_VTAB_MAX
constexpr int     SELL_VTAB_MAX = 256;
aoclsparse_status sell_value_table(hipStream_t s, size_t vsize, long long n, const void *val, void *table, int *ntab);
aoclsparse_status launch_sell_leaders(hipStream_t s, aoclsparse_int m, int base, const aoclsparse_int *row_ptr, const aoclsparse_int *col,
                                      aoclsparse_int nslices, unsigned short *lead, aoclsparse_int *nl);
// y = alpha op(A) x + beta y on the SELL-64 copy (sell_kernels.hip): double, float, cdouble, cfloat.  conj: complex T only;
// complex copies are pack 1 without a table and run order 0.  Order 0 on a plan with slice records runs the short-row kernel.
template <typename T>
aoclsparse_status launch_sellmv(hipStream_t s, const SellView &v, int order, bool conj, T alpha, const T *x, T beta, T *y, int rev);
// BLKCSR (blk_kernels.hip): value offset of every block (three small launches: per-chunk popcount scan, scan of
// the chunk totals in part[], add), then the product
constexpr int     BLK_PART_SHIFT = 10;
aoclsparse_status launch_blk_valoff(hipStream_t s, aoclsparse_int nblk, int rows, const uint8_t *masks,
                                    aoclsparse_int *valoff, aoclsparse_int *part);
aoclsparse_status launch_blkcsrmv(hipStream_t s, int base, double alpha, aoclsparse_int m, int rows, const uint8_t *masks,
                                  const double *val, const aoclsparse_int *col, const aoclsparse_int *row_ptr,
                                  const aoclsparse_int *valoff, const double *x, double beta, double *y);
// y = alpha (L + U - D) x + beta y of a TCSR handle in the order of the reference's aoclsparse_dtcsrmv_avx2 (tcsr_kernels.hip)
aoclsparse_status launch_tcsrmv(hipStream_t s, int base, double alpha, aoclsparse_int m, const double *val_l, const aoclsparse_int *col_l,
                                const aoclsparse_int *ptr_l, const double *val_u, const aoclsparse_int *col_u, const aoclsparse_int *ptr_u,
                                const double *x, double beta, double *y);
// y = alpha A x + beta y for BSR arrays with column-major blocks, one lane per scalar row in the reference's chain order: real
// values (dia_bsr_kernels.hip) and complex ones (bsr_complex_kernels.hip)
template <typename T>
aoclsparse_status launch_bsrmv(hipStream_t s, T alpha, aoclsparse_int mb, aoclsparse_int dim, int base, const T *val,
                               const aoclsparse_int *col, const aoclsparse_int *row_ptr, const T *x, T beta, T *y);
template <typename R>
aoclsparse_status launch_cbsrmv(hipStream_t s, cplx<R> alpha, aoclsparse_int mb, aoclsparse_int dim, int base, const cplx<R> *val,
                                const aoclsparse_int *col, const aoclsparse_int *row_ptr, const cplx<R> *x, cplx<R> beta,
                                cplx<R> *y);
// the mirror of a BSR handle's arrays in HBM, uploaded if absent (formats_api.cpp); call without A->guard held
aoclsparse_status ensure_bsr_mirror(aoclsparse_matrix A);
// y = alpha A x + beta y on a BSR handle with column-major blocks (dia_bsr_api.cpp): T = float / double / cfloat / cdouble, x and y
// host or device memory, the matrix read from the handle's mirror.  The caller has initialised the runtime and holds its stage lock
template <typename T>
aoclsparse_status bsr_handle_mv(CallScope &cs, aoclsparse_matrix A, T alpha, const T *x, T beta, T *y);
template <typename T>
aoclsparse_status launch_mergepath(hipStream_t s, int base, T alpha, aoclsparse_int ntiles, const aoclsparse_int *starts,
                                   const aoclsparse_int *first, const T *val, const aoclsparse_int *col,
                                   const aoclsparse_int *row_ptr, const T *x, T beta, T *y, void *pieces);
template <typename T>
aoclsparse_status launch_scale(hipStream_t s, T *y, aoclsparse_int n, T beta);
// w = a*x + b*y elementwise (w may alias x or y); a == 1, b == -1 is an exact subtraction
template <typename T>
aoclsparse_status launch_waxpby(hipStream_t s, aoclsparse_int n, T a, const T *x, T b, const T *y, T *w);
// d = x . y; partial must hold 1024 elements (spmv_kernels.hip)
template <typename T>
aoclsparse_status launch_dot(hipStream_t s, aoclsparse_int n, const T *x, const T *y, T *partial, T *d);
template <typename T>
aoclsparse_status launch_strided_gather(hipStream_t s, const T *src, aoclsparse_int inc,
                                        aoclsparse_int n, T *dst);
template <typename T>
aoclsparse_status launch_strided_scatter(hipStream_t s, const T *src, aoclsparse_int n, T *dst,
                                         aoclsparse_int inc);

// complex SpMV on a device CSR (complex_kernels.hip); conj multiplies by the conjugated matrix values
template <typename R>
aoclsparse_status launch_cspmv(hipStream_t s, int base, bool conj, cplx<R> alpha, aoclsparse_int m, aoclsparse_int nnz,
                               const cplx<R> *val, const aoclsparse_int *col, const aoclsparse_int *row_ptr,
                               const cplx<R> *x, cplx<R> beta, cplx<R> *y);
template <typename R>
aoclsparse_status launch_cscale(hipStream_t s, cplx<R> *y, aoclsparse_int n, cplx<R> beta);
template <typename R>
aoclsparse_status launch_ccsrmm(hipStream_t s, aoclsparse_order order, int base, bool conj, cplx<R> alpha,
                                aoclsparse_int m, const cplx<R> *val, const aoclsparse_int *col,
                                const aoclsparse_int *row_ptr, const cplx<R> *B, aoclsparse_int n, aoclsparse_int ldb,
                                cplx<R> beta, cplx<R> *C, aoclsparse_int ldc);
template <typename R>
aoclsparse_status launch_cscale_dense(hipStream_t s, aoclsparse_order order, cplx<R> *C, aoclsparse_int m,
                                      aoclsparse_int n, aoclsparse_int ld, cplx<R> beta);

// ELL family (ell_kernels.hip).  ellmv: row-major ELL, padding = column -1, double in the reference's
// 4-lane order (ellmv.hpp:90-208), float in its scalar order (:34-85).  elltmv: column-major ELL, one
// FMA chain per row (:316-444).  csr_rows: the CSR part of ELLT-HYB, rows listed in `map`, 4-lane
// order, beta term taken from ysrc[i] (:660-757).
template <typename T>
aoclsparse_status launch_ellmv(hipStream_t s, int base, T alpha, aoclsparse_int m, const T *val,
                               const aoclsparse_int *col, aoclsparse_int width, const T *x, T beta, T *y);
template <typename T>
aoclsparse_status launch_elltmv(hipStream_t s, int base, T alpha, aoclsparse_int m, const T *val,
                                const aoclsparse_int *col, aoclsparse_int width, const T *x, T beta, T *y);
template <typename T>
aoclsparse_status launch_csr_rows(hipStream_t s, int base, T alpha, aoclsparse_int nrows,
                                  const aoclsparse_int *map, const T *val, const aoclsparse_int *col,
                                  const aoclsparse_int *row_ptr, const T *x, T beta, const T *ysrc, T *y);
template <typename T>
aoclsparse_status launch_gather_rows(hipStream_t s, aoclsparse_int n, const aoclsparse_int *map, const T *src,
                                     T *dst);

// one dependency level of the in-place ILU(0) factorisation (ilu_kernels.hip): rows[0..nrows) of the level,
// diag[] = position of each finished row's diagonal, *error set on a bad pivot / missing diagonal.  search: the position of row
// i that an entry of row k updates is found by a binary search of the row's columns instead of a scan -- for rows in ascending
// column order (sort class 1) ONLY; the factor's bits are the same either way
template <typename T>
aoclsparse_status launch_ilu0_level(hipStream_t s, int base, aoclsparse_int nrows, const aoclsparse_int *rows,
                                    const aoclsparse_int *row_ptr, const aoclsparse_int *col, T *val,
                                    aoclsparse_int *diag, int maxlen, int *error, bool search);
template <typename T>
aoclsparse_status launch_ilu0_syncfree(hipStream_t s, int base, aoclsparse_int n, const aoclsparse_int *rows,
                                       const aoclsparse_int *row_ptr, const aoclsparse_int *col, T *val, aoclsparse_int *diag,
                                       int maxlen, int *error, unsigned int *ticket, bool search);

// dense-vector steps of the iterative solvers (itsol_kernels.hip); `partial` holds
// vec_reduce_scratch_elems(k) elements, reduction results land in device memory
int vec_reduce_scratch_elems(int k);
template <typename T>
aoclsparse_status launch_cg_init(hipStream_t s, aoclsparse_int n, const T *b, const T *x, T *r, T *p);
template <typename T>
aoclsparse_status launch_vec_copy(hipStream_t s, aoclsparse_int n, const T *src, T *dst);
template <typename T>
aoclsparse_status launch_vec_add(hipStream_t s, aoclsparse_int n, const T *src, T *dst);
template <typename T>
aoclsparse_status launch_vec_mul(hipStream_t s, aoclsparse_int n, const T *src, T *dst);
template <typename T>
aoclsparse_status launch_vec_fill(hipStream_t s, aoclsparse_int n, T *dst, T value);
template <typename T>
aoclsparse_status launch_cg_direction(hipStream_t s, aoclsparse_int n, T beta, T *p, const T *z);
template <typename T>
aoclsparse_status launch_cg_step_dev(hipStream_t s, aoclsparse_int n, T rz, T tiny, const T *p, const T *q, T *x, T *r,
                                     T *partial, T *out2);
template <typename T>
aoclsparse_status launch_multidot(hipStream_t s, aoclsparse_int n, int k, const T *V, long long ld, const T *w,
                                  T *partial, T *out);
template <typename T>
aoclsparse_status launch_lincomb(hipStream_t s, int sign, aoclsparse_int n, int k, const T *c, const T *V,
                                 long long ld, T *w);

// TRSV on the level-ordered layout (trsv_kernels.hip).
// schedule 0: one launch per level; 1: hybrid (narrow level runs inside one workgroup); 2: sync-free, a lane per
// position; 3: sync-free, a level slice per wavefront (single right-hand side); 4: sync-free, a lane per BLOCK of chained
// rows (plan.blk, real types); 5: chunks of blocks (plan.blk.chunk).  The schedule is the one resolve_trsv_schedule
// (trsv_schedule.hpp) returned: the launcher replaces nothing, what the plan cannot serve is an internal error.
// csrmm with beta == 0: false (default) = C is read and multiplied by zero as in every reference kernel (NaN / Inf in C
// propagate); true = C is overwritten without being read (BLAS semantics, a third less traffic at 256 columns).  One word for the
// process (aoclsparse_mi355_set_csrmm_beta0_overwrite; AOCLSPARSE_MI355_CSRMM_BETA0_OVERWRITE seeds it once, on first touch).
std::atomic<bool> &csrmm_beta0_overwrite_flag();
// process-wide plan options (aoclsparse_mi355_set_option; read when a plan is built): tests and measurements only
int plan_option(aoclsparse_mi355_option option);
inline int SellPlan::next_direction() const
{
    if(plan_option(aoclsparse_mi355_option_alternate_sweeps) == 0)
        return 0;
    return (int)(products.fetch_add(1u, std::memory_order_relaxed) & 1u);
}
// does a csrmm kernel read C?  always for beta != 0; for beta == 0 unless the overwrite mode is on
bool csrmm_reads_c(bool beta_nonzero);
// timeout_word: where a sync-free kernel reports an expired wait (pinned host memory, Runtime::trsv_timeout_dev).
constexpr int TRSV_NARROW = 1024; // a level this narrow is solved by one workgroup (one row per lane)
template <typename T>
aoclsparse_status launch_trsv(hipStream_t s, int schedule, bool unit, T alpha, aoclsparse_int m,
                              const TrsvPlan &plan, const T *diag, const T *b, T *x, T *xp,
                              unsigned int *scratch, aoclsparse_int nrhs, long long b_off, aoclsparse_int incb,
                              long long x_off, aoclsparse_int incx, unsigned int *timeout_word = nullptr, int kt_bits = 0);

template <typename R>
aoclsparse_status launch_cvec_mul(hipStream_t s, aoclsparse_int n, const cplx<R> *d, cplx<R> *y);
template <typename R>
aoclsparse_status launch_cdiff(hipStream_t s, aoclsparse_int n, const cplx<R> *x, const cplx<R> *y, cplx<R> *w);
// d = sum conj(x_i) y_i; partial holds 1024 elements
template <typename R>
aoclsparse_status launch_cdot(hipStream_t s, aoclsparse_int n, const cplx<R> *x, const cplx<R> *y, cplx<R> *partial,
                              cplx<R> *d, bool conj_x = true);
template <typename R>
aoclsparse_status launch_caxpby(hipStream_t s, aoclsparse_int n, cplx<R> a, const cplx<R> *x, cplx<R> b, const cplx<R> *y,
                                cplx<R> *w);
// row bins of spgemm_hash_kernel (spgemm_kernels.hip): list capacity 32 / 256 / 2048 / 8192 in LDS; the last bin keeps its tables
// in a global slab.  The fill pass has no 8192 bin (values and slots would not fit the LDS): rows with more than 2048 entries of
// C go to the last bin there.
constexpr int SPGEMM_BINS = 5;
int           spgemm_bin_of(long long entries, bool fill);
// one row of the last bin: its hash table of 2^logh slots starts at h_off (g_key / g_pos), its list at c_off (g_list / g_acc)
struct SpgHeavy
{
    int       row, logh;
    long long h_off, c_off;
};
// the analysis around the two passes, on the device (spgemm_kernels.hip): upper bounds, bin histogram (+ a validity word), the
// rows of every bin, the prefix sum of the counts
aoclsparse_status launch_spg_bounds(hipStream_t s, aoclsparse_int m, aoclsparse_int n, int base_a, const aoclsparse_int *ptr_a,
                                    const aoclsparse_int *ind_a, const aoclsparse_int *ptr_b, int *cap);
aoclsparse_status launch_spg_diff(hipStream_t s, aoclsparse_int m, const aoclsparse_int *ptr, int *key);
aoclsparse_status launch_spg_hist(hipStream_t s, aoclsparse_int m, const int *key, const int *limit, bool fill, unsigned int *hist);
aoclsparse_status launch_spg_order(hipStream_t s, aoclsparse_int m, const int *key, bool fill, const aoclsparse_int *bounds,
                                   unsigned int *cursor, aoclsparse_int *order);
aoclsparse_status launch_spg_gather(hipStream_t s, aoclsparse_int count, const aoclsparse_int *ids, const int *key, int *out);
size_t            spg_scan_scratch_bytes(aoclsparse_int m);
aoclsparse_status launch_spg_scan(hipStream_t s, aoclsparse_int m, const int *cnt, aoclsparse_int *ptr, long long *scratch,
                                  long long **total_dev);
// complex triangular solve (complex_kernels.hip): the hybrid schedule of the plan (runs of narrow levels inside one
// workgroup, one launch per wide level); conj_diag for op = H (the plan's values are stored conjugated)
template <typename R>
aoclsparse_status launch_ctrsv(hipStream_t s, bool unit, bool conj_diag, cplx<R> alpha, aoclsparse_int m,
                               const TrsvPlan &plan, const cplx<R> *diag, const cplx<R> *b, cplx<R> *x, cplx<R> *xp,
                               aoclsparse_int nrhs, long long b_off, aoclsparse_int incb, long long x_off,
                               aoclsparse_int incx);

template <typename T>
aoclsparse_status launch_csrmm(hipStream_t s, aoclsparse_order order, int base, T alpha,
                               aoclsparse_int m, aoclsparse_int k, const T *val,
                               const aoclsparse_int *col, const aoclsparse_int *row_ptr, const T *B,
                               aoclsparse_int n, aoclsparse_int ldb, T beta, T *C,
                               aoclsparse_int ldc, const aoclsparse_int *grp = nullptr, aoclsparse_int ngroups = 0,
                               int group_rows = 0, bool row_runs = false,
                               const aoclsparse_int *run_order = nullptr, int kt_lanes = 0, aoclsparse_int band = 0);
// column-major detour, handles with row groups: row-major B scratch in, column-major C written directly (no C copies)
template <typename T>
bool csrmm_groups_ccol_applies(aoclsparse_int n, aoclsparse_int ldb, const T *B);
template <typename T>
aoclsparse_status launch_csrmm_groups_ccol(hipStream_t s, int base, T alpha, const T *val, const aoclsparse_int *col,
                                           const aoclsparse_int *row_ptr, const T *B, aoclsparse_int n, aoclsparse_int ldb,
                                           T beta, T *C, aoclsparse_int ldc, const aoclsparse_int *grp, aoclsparse_int ngroups,
                                           int group_rows, aoclsparse_int m = 0, aoclsparse_int band = 0);
// row-major, n < 128: workgroup per row block of the handle's SpMV plan, A staged in LDS (csrmm_tile_kernel)
template <typename T>
bool csrmm_tiled_applies(aoclsparse_int n, aoclsparse_int ldb, aoclsparse_int ldc, const T *B, const T *C);
template <typename T>
aoclsparse_status launch_csrmm_tiled(hipStream_t s, int base, T alpha, const T *val, const aoclsparse_int *col,
                                     const aoclsparse_int *row_ptr, const aoclsparse_int *blocks, aoclsparse_int nblocks,
                                     int tile, aoclsparse_int max_row_nnz, const T *B, aoclsparse_int n, aoclsparse_int ldb,
                                     T beta, T *C, aoclsparse_int ldc, int kt_lanes = 0, bool launch_order = false);
// column-major: a lane owns a row PAIR; 16-byte loads where the second row is the first shifted by one column
template <typename T>
aoclsparse_status launch_csrmm_colpair(hipStream_t s, int base, T alpha, aoclsparse_int npairs,
                                       const aoclsparse_int *pair_first, aoclsparse_int nsingles,
                                       const aoclsparse_int *single_rows, const T *val, const aoclsparse_int *col,
                                       const aoclsparse_int *row_ptr, aoclsparse_int max_row_nnz, const T *B, aoclsparse_int n,
                                       aoclsparse_int ldb, T beta, T *C, aoclsparse_int ldc);
// all csrmm plans of the untransposed matrix, built from the host arrays now (csrmm_api.cpp)
aoclsparse_status prepare_mm_plans(aoclsparse_matrix A);
// row-major, block-dense matrices: blocked-ELL copy + v_mfma_f64_16x16x4_f64 (csrmm_bell_kernels.hip)
aoclsparse_status build_bell(const HostCsr &h, const DeviceCsr &d, SpmvPlan &plan, aoclsparse_matrix_data_type vt);
aoclsparse_status launch_bell_fill(hipStream_t s, aoclsparse_int m, int base, const aoclsparse_int *ptr, const aoclsparse_int *ind,
                                   const double *val, aoclsparse_int nbr, aoclsparse_int width, const aoclsparse_int *bcol, double *out);
// (base / rp / ci / cv: the device CSR the copy was built from -- an element whose tile sum is not finite is recomputed from it)
aoclsparse_status launch_csrmm_bell(hipStream_t s, double alpha, aoclsparse_int m, aoclsparse_int k, const BellPlan &bell,
                                    int base, const aoclsparse_int *rp, const aoclsparse_int *ci, const double *cv,
                                    const double *B, aoclsparse_int n, aoclsparse_int ldb, double beta, double *C,
                                    aoclsparse_int ldc, bool column_major = false);
// column-major, banded: a workgroup stages the stretch of a B column its rows can touch in LDS (csrmm_window_kernels.hip)
int csrmm_window_rows(aoclsparse_int max_row_nnz, size_t elem); // rows per workgroup the kernel will use
int csrmm_window_max_pieces(); // 16-byte pieces a window may hold
template <typename T>
bool csrmm_window_applies(aoclsparse_int n, aoclsparse_int ldb, const T *B);
template <typename T>
aoclsparse_status launch_csrmm_window(hipStream_t s, int base, T alpha, aoclsparse_int m, const T *val, const aoclsparse_int *col,
                                      const aoclsparse_int *row_ptr, const aoclsparse_int *win, int win_rows,
                                      aoclsparse_int max_row_nnz, const T *B, aoclsparse_int n, aoclsparse_int ldb, T beta, T *C,
                                      aoclsparse_int ldc);
// aoclsparse_?csrmm_kid with kid 1/2/3: the reference's KT kernels' arithmetic (csrmm_kt.cpp:31-363), lanes = 4 / 8 (double), 8 / 16 (float)
template <typename T>
aoclsparse_status launch_csrmm_kt(hipStream_t s, aoclsparse_order order, int lanes, int base, T alpha, aoclsparse_int m,
                                  const T *val, const aoclsparse_int *col, const aoclsparse_int *row_ptr, const T *B,
                                  aoclsparse_int n, aoclsparse_int ldb, T beta, T *C, aoclsparse_int ldc);
template <typename T>
aoclsparse_status launch_relayout(hipStream_t s, bool to_row_major, const T *src, T *dst, aoclsparse_int R, aoclsparse_int N,
                                  aoclsparse_int ld);
template <typename T>
aoclsparse_status launch_scale_dense(hipStream_t s, aoclsparse_order order, T *C, aoclsparse_int m,
                                     aoclsparse_int n, aoclsparse_int ld, T beta);

// sp2md_kernels.hip: dense-result product, CSR -> dense, sparse sum
template <typename T>
aoclsparse_status launch_dense_scale(hipStream_t s, T *C, aoclsparse_int inner, aoclsparse_int outer, long long ld,
                                     T beta, bool zero);
template <typename T>
aoclsparse_status launch_sp2md(hipStream_t s, aoclsparse_int m, int base_a, const aoclsparse_int *ptr_a,
                               const aoclsparse_int *ind_a, const T *val_a, bool conj_a, int base_b,
                               const aoclsparse_int *ptr_b, const aoclsparse_int *ind_b, const T *val_b, bool conj_b,
                               T alpha, T *C, long long rs, long long cs);
template <typename T>
aoclsparse_status launch_csr2dense(hipStream_t s, aoclsparse_int m, int base, const aoclsparse_int *ptr,
                                   const aoclsparse_int *ind, const T *val, T *A, long long rs, long long cs, int mode,
                                   int fill, int diag);
template <typename T>
aoclsparse_status launch_csradd(hipStream_t s, bool fill, aoclsparse_int m, int base_a, const aoclsparse_int *ptr_a,
                                const aoclsparse_int *ind_a, const T *val_a, bool conj_a, T alpha, int base_b,
                                const aoclsparse_int *ptr_b, const aoclsparse_int *ind_b, const T *val_b, int base_c,
                                const aoclsparse_int *ptr_c, aoclsparse_int *cnt_or_ind_c, T *val_c);
// sy_dense_kernels.hip: the symmetric products with a dense result (?syrkd, ?syprd); only C's upper triangle is touched
constexpr int    SY_SERIAL  = 1; // syrkd: a row of the handle repeats a column -- one lane walks the rows of W
constexpr int    SY_ORDERED = 2; // syrkd: walk X's rows by ascending column (op = none on rows that are not sorted)
constexpr size_t SY_LDS_MAX = 128 * 1024; // syprd stage 2 keeps a row of the scratch in LDS up to this size
template <typename T>
aoclsparse_status launch_sy_scale_upper(hipStream_t s, T *C, aoclsparse_int n, long long ld, bool rowmajor, T beta,
                                        bool zero);
// X = the CSR whose row i lists the rows of M that hold column i (M's transpose), W = M
template <typename T>
aoclsparse_status launch_syrkd(hipStream_t s, aoclsparse_int mc, int base_x, const aoclsparse_int *ptr_x,
                               const aoclsparse_int *ind_x, const T *val_x, bool conj_x, int base_w,
                               const aoclsparse_int *ptr_w, const aoclsparse_int *ind_w, const T *val_w, bool conj_w,
                               T alpha, T *C, long long rs, long long cs, int flags);
// scratch: mc x nin values; beta_mode: 0 C starts at zero, 1 at C, 2 at beta*C
template <typename T>
aoclsparse_status launch_syprd(hipStream_t s, aoclsparse_int mc, aoclsparse_int nin, int base, const aoclsparse_int *ptr,
                               const aoclsparse_int *ind, const T *val, bool conj_1, bool conj_2, T alpha, const T *B,
                               long long ldb, bool rowmajor, T *scratch, T beta, int beta_mode, T *C, long long rs, long long cs);
// a new handle that owns host CSR arrays (spg_product.cpp); row_ptr copied when given, else filled with `base`
aoclsparse_status new_csr_result(aoclsparse_matrix *C, aoclsparse_int m, aoclsparse_int n, aoclsparse_int nnz,
                                 aoclsparse_matrix_data_type vt, const aoclsparse_int *row_ptr,
                                 aoclsparse_index_base base = aoclsparse_index_base_zero);

// ---- one first-touch product D = X * Y on the device (spg_product.cpp; kernels: spgemm_kernels.hip; host side: spg_host.hpp) ------
// What aoclsparse_sp2m, aoclsparse_syrk and aoclsparse_sypr share: the upper bound of every row's list, the bins, the count pass
// with its prefix sum and the fill pass.  X and Y are CSR arrays in HBM (any base), D is 0-based.  The SPG_SLOT_* staging slots (StageSlot) of the
// runtime belong to these three entry points; the caller holds the runtime's stage lock from analyse() to the last pass.
struct SpgDevOp
{
    const aoclsparse_int *ptr = nullptr, *ind = nullptr;
    const void           *val = nullptr;
    int                   base = 0;
};
template <typename T>
struct SpgProduct
{
    Runtime       &rt;
    aoclsparse_int m = 0, n = 0; // D is m x n
    SpgDevOp       x, y;
    bool           conj_x = false, conj_y = false;
    bool           upper  = false; // row i of D keeps the columns >= i only (spgemm_hash_kernel, UPPER)
    std::function<void(const char *)> phase; // diagnostic hook: called after every step with its name

    explicit SpgProduct(Runtime &r)
        : rt(r)
    {
    }
    // the upper bound of every row's list; clears the word the passes raise when a row does not fit what it was given
    aoclsparse_status analyse();
    // count pass and prefix sum: d_ptr[0..m] (device) = D's row pointer, *d_total (device) = its last entry in 64 bits
    aoclsparse_status count(aoclsparse_int *d_ptr, long long **d_total);
    // instead of count(): the counts that a row pointer from elsewhere (a finalize call) implies
    aoclsparse_status counts_from(const aoclsparse_int *d_ptr);
    // fill pass; the counts of count() / counts_from() are checked against the upper bounds first (invalid_value)
    aoclsparse_status fill(const aoclsparse_int *d_ptr, aoclsparse_int *d_ind, T *d_val);
    // device word, nonzero once a row ended short of, or beyond, its segment
    const unsigned int *bad_word() const
    {
        return d_bad;
    }

private:
    struct Binned;
    int          *d_cap = nullptr, *d_key = nullptr;
    unsigned int *d_hist = nullptr, *d_cursor = nullptr, *d_bad = nullptr;
    aoclsparse_status bin_rows(Binned &bn, bool for_fill, const int *key, const int *limit);
    aoclsparse_status run_pass(bool pass_fill, Binned &bn, const aoclsparse_int *ptr_c, aoclsparse_int *out_i, T *out_v);
};
// ---- the values of D = X * Y again on a structure that is kept (aoclsparse_mi355_sp2m_numeric_device; spg_product.cpp, kernels:
// spgemm_numeric_kernels.hip).  sp2m_plan_build: the bins of C's rows by their exact length, from C's row pointer in HBM (any base)
// alone, in buffers of the plan's own (two host waits at most: the histogram, and the rows of the global slab).  spg_numeric: one
// launch per populated bin and per batch of the slab; C = (ptr, ind) in HBM in base c.base, `out` = the new values in C's order,
// *d_bad (zeroed by the caller) raised when C's structure is not the product's.  The slab's tables are staging slots
// (SPG_SLOT_G_*): the caller holds the stage lock.
static_assert(SPGEMM_BINS == 5, "Sp2mPlan::bounds");
aoclsparse_status sp2m_plan_build(Runtime &rt, aoclsparse_int m, const aoclsparse_int *d_ptr_c, _aoclsparse_matrix::Sp2mPlan &plan);
template <typename T>
aoclsparse_status spg_numeric(Runtime &rt, const _aoclsparse_matrix::Sp2mPlan &plan, const SpgDevOp &x, const SpgDevOp &y, bool conj_x,
                              bool conj_y, const SpgDevOp &c, T *out, unsigned int *d_bad);
// the dense-row path of aoclsparse_syrk (spgemm_kernels.hip: aat_dense_row_kernel): the upper triangle of A * A^H for a short, wide
// A (syrk.hpp:46-113).  (ptr_s, ind_s, val_s): A with every row sorted by column and one entry per column (repeats
// summed), 0-based -- the searchable form of the reference's dense row.  Count pass: cnt[i]; fill pass: ind_c (in base_c) / val_c
// at the 0-based ptr_c.
template <typename T>
aoclsparse_status launch_aat_dense_row(hipStream_t s, bool fill, aoclsparse_int m, int base_a, const aoclsparse_int *ptr_a,
                                       const aoclsparse_int *ind_a, const T *val_a, const aoclsparse_int *ptr_s,
                                       const aoclsparse_int *ind_s, const T *val_s, const aoclsparse_int *ptr_c, int *cnt,
                                       int base_c, aoclsparse_int *ind_c, T *val_c);

// level1_kernels.hip: sparse-vector operations
constexpr int L1_DOT_PARTIALS = 1024;
template <typename T>
aoclsparse_status launch_axpyi(hipStream_t s, aoclsparse_int nnz, T a, const T *x, const aoclsparse_int *indx, T *y);
template <typename T>
aoclsparse_status launch_gather_scatter(hipStream_t s, aoclsparse_int nnz, T *x, const aoclsparse_int *indx,
                                        long long stride, T *y, int mode);
template <typename T>
aoclsparse_status launch_roti(hipStream_t s, aoclsparse_int nnz, T *x, const aoclsparse_int *indx, T *y, T c, T sn);
template <typename T>
aoclsparse_status launch_doti(hipStream_t s, aoclsparse_int nnz, const T *x, const aoclsparse_int *indx, const T *y,
                              bool conj, T *partial, T *out);

// sorv_kernels.hip: one level of the forward SOR sweep
template <typename T>
aoclsparse_status launch_sorv_level(hipStream_t s, const aoclsparse_int *rows, aoclsparse_int count, int base,
                                    const aoclsparse_int *ptr, const aoclsparse_int *ind, const T *val, T omega, T *x,
                                    const T *xold, const T *b);

// SpMV plan constants shared by host planner and kernels
// LDS tile = non-zeros staged per workgroup: 512 (128 threads), 1024 or 2048 (256 threads);
// rows per stream block (their row_ptr slice is kept in LDS)
// csr_adaptive_kernel, auto mode (scalar order, no pinned kid): rows of an LDS tile with at least this many entries are summed by a
// whole wavefront (64 strided FMA chains + a fixed-order tree) instead of one lane's chain
constexpr int SPMV_TREE_MIN = 32;
constexpr int spmv_maxrows(int tile)
{
    return tile / 2 < 512 ? tile / 2 : 512;
}

} // namespace mi355
