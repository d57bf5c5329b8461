// spg_product.cpp -- what aoclsparse_sp2m, aoclsparse_syrk and aoclsparse_sypr (and the other makers of result handles) share:
// new_csr_result, the first-touch product D = X * Y on the device (SpgProduct<T>: analyse, bin, count, scan, fill; kernels in
// spgemm_kernels.hip) and the host pieces around it (spg_host.hpp).
#include "spg_host.hpp"
#include "device_handle.hpp"

#include <cstring>
#include <thread>

using namespace mi355;

namespace mi355
{
template <typename T>
aoclsparse_status launch_spgemm_heavy(hipStream_t s, bool fill, aoclsparse_int nrows, const SpgHeavy *heavy, int *g_key, int *g_pos,
                                      int *g_list, T *g_acc, int base_a, const aoclsparse_int *ptr_a, const aoclsparse_int *ind_a,
                                      const T *val_a, int base_b, const aoclsparse_int *ptr_b, const aoclsparse_int *ind_b,
                                      const T *val_b, const aoclsparse_int *ptr_c, aoclsparse_int *cnt_or_ind_c, T *val_c,
                                      bool conj_a, bool conj_b, bool upper, unsigned int *bad);
template <typename T>
aoclsparse_status launch_spgemm_bin(hipStream_t s, bool fill, int bin, aoclsparse_int nrows, const aoclsparse_int *rows, int base_a,
                                    const aoclsparse_int *ptr_a, const aoclsparse_int *ind_a, const T *val_a, int base_b,
                                    const aoclsparse_int *ptr_b, const aoclsparse_int *ind_b, const T *val_b,
                                    const aoclsparse_int *ptr_c, aoclsparse_int *cnt_or_ind_c, T *val_c, bool conj_a, bool conj_b,
                                    bool upper, unsigned int *bad);
// spgemm_numeric_kernels.hip
template <typename T>
aoclsparse_status launch_spg_numeric_bin(hipStream_t s, int bin, aoclsparse_int nrows, const aoclsparse_int *rows, int base_a,
                                         const aoclsparse_int *ptr_a, const aoclsparse_int *ind_a, const T *val_a, int base_b,
                                         const aoclsparse_int *ptr_b, const aoclsparse_int *ind_b, const T *val_b, int base_c,
                                         const aoclsparse_int *ptr_c, const aoclsparse_int *ind_c, T *out, bool conj_a, bool conj_b,
                                         unsigned int *bad);
template <typename T>
aoclsparse_status launch_spg_numeric_heavy(hipStream_t s, aoclsparse_int nrows, const SpgHeavy *heavy, int *g_key, int *g_pos,
                                           unsigned char *g_touched, int base_a, const aoclsparse_int *ptr_a,
                                           const aoclsparse_int *ind_a, const T *val_a, int base_b, const aoclsparse_int *ptr_b,
                                           const aoclsparse_int *ind_b, const T *val_b, int base_c, const aoclsparse_int *ptr_c,
                                           const aoclsparse_int *ind_c, T *out, bool conj_a, bool conj_b, unsigned int *bad);

aoclsparse_status new_csr_result(aoclsparse_matrix *C, aoclsparse_int m, aoclsparse_int n, aoclsparse_int nnz,
                                 aoclsparse_matrix_data_type vt, const aoclsparse_int *row_ptr, aoclsparse_index_base base)
{
    _aoclsparse_matrix *c = new(std::nothrow) _aoclsparse_matrix;
    if(!c)
        return aoclsparse_status_memory_error;
    const size_t vs = val_size(vt);
    c->m = m, c->n = n, c->nnz = nnz, c->base = base, c->val_type = vt;
    c->user.m = m, c->user.n = n, c->user.nnz = nnz, c->user.base = base;
    c->user.ptr = new(std::nothrow) aoclsparse_int[(size_t)m + 1];
    c->user.ind = static_cast<aoclsparse_int *>(host_result_alloc(sizeof(aoclsparse_int) * (size_t)std::max(nnz, 1)));
    c->user.val = host_result_alloc(vs * (size_t)std::max(nnz, 1));
    c->user.owned = c->user.result_arrays = true; // freed by the handle
    c->owns_user_arrays = true;
    if(!c->user.ptr || !c->user.ind || !c->user.val)
    {
        delete c;
        return aoclsparse_status_memory_error;
    }
    if(row_ptr)
        std::memcpy(c->user.ptr, row_ptr, sizeof(aoclsparse_int) * ((size_t)m + 1));
    else
        std::fill(c->user.ptr, c->user.ptr + m + 1, (aoclsparse_int)base);
    *C = c;
    return aoclsparse_status_success;
}

// the rows of a product grouped by the bin of spgemm_hash_kernel that serves them (device arrays: staging slots of the runtime,
// grown on demand and reused by the next product -- a hipMalloc / hipFree pair per temporary cost more than the kernels)
template <typename T>
struct SpgProduct<T>::Binned
{
    aoclsparse_int        bounds[SPGEMM_BINS + 1] = {};
    const aoclsparse_int *d_order = nullptr; // null: one bin holds every row (no list needed)
    // the rows of the last bin (tables in a global slab), in batches whose tables fit SPG_SLAB_SLOTS: batch b = records
    // [batch[b], batch[b + 1]) with offsets that start at 0
    std::vector<SpgHeavy>       heavy;
    std::vector<aoclsparse_int> batch;
    long long                   slots = 0, entries = 0; // of the largest batch
    const SpgHeavy             *d_heavy = nullptr;
};
constexpr long long SPG_SLAB_SLOTS = 1LL << 28; // 1 GiB of keys (and of slots in the fill pass) per batch

// the rows of the last bin, (row, list size) in any order -> their records by ascending row, in batches whose tables fit
// SPG_SLAB_SLOTS; slots / entries: of the largest batch
static aoclsparse_status spg_heavy_layout(std::vector<std::pair<aoclsparse_int, int>> &rows, std::vector<SpgHeavy> &heavy,
                                          std::vector<aoclsparse_int> &batch, long long &slots, long long &entries)
{
    std::sort(rows.begin(), rows.end()); // (the device appends them in arrival order)
    heavy.reserve(rows.size());
    long long hs = 0, cs = 0;
    batch.push_back(0);
    for(const auto &r : rows)
    {
        const long long cap = r.second;
        if(cap > (1LL << 29))
            return aoclsparse_status_memory_error;
        int logh = 6;
        while((1LL << logh) < 2 * cap)
            logh++;
        if(hs + (1LL << logh) > SPG_SLAB_SLOTS && hs > 0)
        {
            batch.push_back((aoclsparse_int)heavy.size());
            hs = cs = 0;
        }
        heavy.push_back(SpgHeavy{r.first, logh, hs, cs});
        hs += 1LL << logh, cs += cap;
        slots = std::max(slots, hs), entries = std::max(entries, cs);
    }
    batch.push_back((aoclsparse_int)heavy.size());
    return aoclsparse_status_success;
}

// ---- analysis on the device: the upper bound of every row's list, the bins, the rows of every bin (spgemm_kernels.hip) ----
template <typename T>
aoclsparse_status SpgProduct<T>::analyse()
{
    void             *p_cap = nullptr, *p_key = nullptr, *p_small = nullptr;
    aoclsparse_status st    = rt.staging(SPG_SLOT_CAP, sizeof(int) * (size_t)m, &p_cap);
    if(st == aoclsparse_status_success)
        st = rt.staging(SPG_SLOT_CNT, sizeof(int) * (size_t)m, &p_key);
    if(st == aoclsparse_status_success)
        st = rt.staging(SPG_SLOT_SMALL, 256, &p_small);
    if(st == aoclsparse_status_success)
        st = launch_spg_bounds(rt.stream(), m, n, x.base, x.ptr, x.ind, y.ptr, static_cast<int *>(p_cap));
    if(st != aoclsparse_status_success)
        return st;
    d_cap = static_cast<int *>(p_cap), d_key = static_cast<int *>(p_key);
    d_hist = static_cast<unsigned int *>(p_small), d_cursor = d_hist + 16, d_bad = d_hist + 32;
    MI355_HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(unsigned int), rt.stream())); // raised by a row whose list does not fit what it was given
    return aoclsparse_status_success;
}

// key = the size of every row's list (count pass: d_cap; fill pass: the exact counts, checked against d_cap)
template <typename T>
aoclsparse_status SpgProduct<T>::bin_rows(Binned &bn, bool for_fill, const int *key, const int *limit)
{
    hipStream_t       s  = rt.stream();
    aoclsparse_status rc = launch_spg_hist(s, m, key, limit, for_fill, d_hist);
    if(rc != aoclsparse_status_success)
        return rc;
    unsigned int hist[SPGEMM_BINS + 1];
    MI355_HIP_TRY(hipMemcpyAsync(hist, d_hist, sizeof(hist), hipMemcpyDeviceToHost, s));
    MI355_HIP_TRY(hipStreamSynchronize(s));
    if(hist[SPGEMM_BINS])
        return aoclsparse_status_invalid_value; // a row_ptr that is not this product's (csr2m.cpp:397-399 checks dimensions only)
    bn.bounds[0] = 0;
    bool one_bin = false;
    for(int b = 0; b < SPGEMM_BINS; b++)
    {
        bn.bounds[b + 1] = bn.bounds[b] + (aoclsparse_int)hist[b];
        one_bin |= (aoclsparse_int)hist[b] == m;
    }
    const aoclsparse_int nheavy = (aoclsparse_int)hist[SPGEMM_BINS - 1];
    if(one_bin && nheavy == 0)
        return aoclsparse_status_success; // (no list: workgroup g serves row g)
    void *po = nullptr;
    rc       = rt.staging(for_fill ? SPG_SLOT_ORDER_FILL : SPG_SLOT_ORDER_COUNT, sizeof(aoclsparse_int) * (size_t)m, &po);
    if(rc == aoclsparse_status_success)
        rc = launch_spg_order(s, m, key, for_fill, bn.bounds, d_cursor, static_cast<aoclsparse_int *>(po));
    if(rc != aoclsparse_status_success)
        return rc;
    bn.d_order = static_cast<const aoclsparse_int *>(po);
    if(nheavy == 0)
        return rc;
    // the rows of the last bin: ids and list sizes to the host, slab offsets back (few rows: the dense ones of a power-law matrix)
    void *pk = nullptr;
    rc       = rt.staging(SPG_SLOT_HEAVY_KEYS, sizeof(int) * (size_t)nheavy, &pk);
    if(rc == aoclsparse_status_success)
        rc = launch_spg_gather(s, nheavy, bn.d_order + bn.bounds[SPGEMM_BINS - 1], key, static_cast<int *>(pk));
    if(rc != aoclsparse_status_success)
        return rc;
    std::vector<aoclsparse_int> ids((size_t)nheavy);
    std::vector<int>            caps((size_t)nheavy);
    MI355_HIP_TRY(hipMemcpyAsync(ids.data(), bn.d_order + bn.bounds[SPGEMM_BINS - 1], sizeof(aoclsparse_int) * (size_t)nheavy,
                                 hipMemcpyDeviceToHost, s));
    MI355_HIP_TRY(hipMemcpyAsync(caps.data(), pk, sizeof(int) * (size_t)nheavy, hipMemcpyDeviceToHost, s));
    MI355_HIP_TRY(hipStreamSynchronize(s));
    std::vector<std::pair<aoclsparse_int, int>> rows((size_t)nheavy);
    for(aoclsparse_int j = 0; j < nheavy; j++)
        rows[(size_t)j] = {ids[(size_t)j], caps[(size_t)j]};
    rc = spg_heavy_layout(rows, bn.heavy, bn.batch, bn.slots, bn.entries);
    if(rc != aoclsparse_status_success)
        return rc;
    void *ph = nullptr;
    rc       = rt.staging(for_fill ? SPG_SLOT_HEAVY_FILL : SPG_SLOT_HEAVY_COUNT, sizeof(SpgHeavy) * bn.heavy.size(), &ph);
    if(rc == aoclsparse_status_success)
        rc = rt.h2d(ph, bn.heavy.data(), sizeof(SpgHeavy) * bn.heavy.size());
    bn.d_heavy = static_cast<const SpgHeavy *>(ph);
    return rc;
}

template <typename T>
aoclsparse_status SpgProduct<T>::run_pass(bool pass_fill, Binned &bn, const aoclsparse_int *ptr_c, aoclsparse_int *out_i, T *out_v)
{
    hipStream_t       s  = rt.stream();
    const T          *xv = static_cast<const T *>(x.val), *yv = static_cast<const T *>(y.val);
    aoclsparse_status rc = aoclsparse_status_success;
    for(int b = 0; b < SPGEMM_BINS - 1 && rc == aoclsparse_status_success; b++)
        rc = launch_spgemm_bin<T>(s, pass_fill, b, bn.bounds[b + 1] - bn.bounds[b], bn.d_order ? bn.d_order + bn.bounds[b] : nullptr,
                                  x.base, x.ptr, x.ind, xv, y.base, y.ptr, y.ind, yv, ptr_c, out_i, out_v, conj_x, conj_y, upper,
                                  d_bad);
    if(rc != aoclsparse_status_success || bn.heavy.empty())
        return rc;
    void *gk = nullptr, *gp = nullptr, *gl = nullptr, *ga = nullptr;
    rc       = rt.staging(SPG_SLOT_G_KEY, sizeof(int) * (size_t)bn.slots, &gk);
    if(pass_fill)
    {
        if(rc == aoclsparse_status_success)
            rc = rt.staging(SPG_SLOT_G_POS, sizeof(int) * (size_t)bn.slots, &gp);
        if(rc == aoclsparse_status_success)
            rc = rt.staging(SPG_SLOT_G_LIST, sizeof(int) * (size_t)bn.entries, &gl);
        if(rc == aoclsparse_status_success)
            rc = rt.staging(SPG_SLOT_G_ACC, sizeof(T) * (size_t)bn.entries, &ga);
    }
    for(size_t b = 0; b + 1 < bn.batch.size() && rc == aoclsparse_status_success; b++) // (stream order: a batch reuses the slab)
        rc = launch_spgemm_heavy<T>(s, pass_fill, bn.batch[b + 1] - bn.batch[b], bn.d_heavy + bn.batch[b], static_cast<int *>(gk),
                                    static_cast<int *>(gp), static_cast<int *>(gl), static_cast<T *>(ga), x.base, x.ptr, x.ind, xv,
                                    y.base, y.ptr, y.ind, yv, ptr_c, out_i, out_v, conj_x, conj_y, upper, d_bad);
    return rc;
}

template <typename T>
aoclsparse_status SpgProduct<T>::count(aoclsparse_int *d_ptr, long long **d_total)
{
    Binned            by_bound;
    aoclsparse_status st = bin_rows(by_bound, false, d_cap, nullptr);
    if(phase)
        phase("count: bins");
    if(st == aoclsparse_status_success)
        st = run_pass(false, by_bound, nullptr, d_key, nullptr);
    if(st != aoclsparse_status_success)
        return st;
    if(phase)
        phase("count: kernels");
    // row_ptr of D = prefix sum of the counts, on the device (64-bit sums: a product of more than 2^31 - 1 entries is refused by the
    // caller, csr2m.cpp:221-236)
    void *p_scan = nullptr;
    st           = rt.staging(SPG_SLOT_SCAN, spg_scan_scratch_bytes(m), &p_scan);
    if(st == aoclsparse_status_success)
        st = launch_spg_scan(rt.stream(), m, d_key, d_ptr, static_cast<long long *>(p_scan), d_total);
    return st;
}

template <typename T>
aoclsparse_status SpgProduct<T>::counts_from(const aoclsparse_int *d_ptr)
{
    return launch_spg_diff(rt.stream(), m, d_ptr, d_key);
}

template <typename T>
aoclsparse_status SpgProduct<T>::fill(const aoclsparse_int *d_ptr, aoclsparse_int *d_ind, T *d_val)
{
    // rows binned by their exact count, checked against the upper bounds on the device (bin_rows)
    Binned            by_count;
    aoclsparse_status st = bin_rows(by_count, true, d_key, d_cap);
    if(phase)
        phase("fill: bins");
    if(st == aoclsparse_status_success)
        st = run_pass(true, by_count, d_ptr, d_ind, d_val);
    return st;
}

// ---- the numeric phase on a kept structure (aoclsparse_mi355_sp2m_numeric_device) ----------------------------------------------
// The bins of C's rows by their exact length: bin_rows(for_fill) without an upper bound to check against and in buffers of the
// plan's own -- the staging slots are overwritten by the next product, the plan outlives the call.
aoclsparse_status sp2m_plan_build(Runtime &rt, aoclsparse_int m, const aoclsparse_int *d_ptr_c, _aoclsparse_matrix::Sp2mPlan &plan)
{
    hipStream_t  s = rt.stream();
    DeviceBuffer key, small, hkeys; // per row: its length; histogram (at 0) and cursors (at 16); the lengths of the slab's rows
    StreamDrain  drain{s}; // (declared after the buffers: the stream finishes before they are released)
    plan.release();
    MI355_TRY(key.alloc(sizeof(int) * (size_t)std::max<aoclsparse_int>(m, 1)));
    MI355_TRY(small.alloc(256));
    unsigned int *d_hist = small.as<unsigned int>(), *d_cursor = d_hist + 16;
    MI355_TRY(launch_spg_diff(s, m, d_ptr_c, key.as<int>()));
    MI355_TRY(launch_spg_hist(s, m, key.as<int>(), nullptr, true, d_hist));
    unsigned int hist[SPGEMM_BINS + 1];
    MI355_HIP_TRY(hipMemcpyAsync(hist, d_hist, sizeof(hist), hipMemcpyDeviceToHost, s));
    MI355_HIP_TRY(hipStreamSynchronize(s));
    if(hist[SPGEMM_BINS])
        return aoclsparse_status_invalid_value; // a row pointer that descends
    bool one_bin = false;
    for(int b = 0; b < SPGEMM_BINS; b++)
    {
        plan.bounds[b + 1] = plan.bounds[b] + (aoclsparse_int)hist[b];
        one_bin |= (aoclsparse_int)hist[b] == m;
    }
    const aoclsparse_int nheavy = (aoclsparse_int)hist[SPGEMM_BINS - 1];
    if(!(one_bin && nheavy == 0)) // (otherwise no list: workgroup g serves row g)
    {
        MI355_TRY(plan.order.alloc(sizeof(aoclsparse_int) * (size_t)m));
        MI355_TRY(launch_spg_order(s, m, key.as<int>(), true, plan.bounds, d_cursor, plan.order.as<aoclsparse_int>()));
    }
    if(nheavy > 0)
    {
        const aoclsparse_int *d_ids = plan.order.as<aoclsparse_int>() + plan.bounds[SPGEMM_BINS - 1];
        MI355_TRY(hkeys.alloc(sizeof(int) * (size_t)nheavy));
        MI355_TRY(launch_spg_gather(s, nheavy, d_ids, key.as<int>(), hkeys.as<int>()));
        std::vector<aoclsparse_int> ids((size_t)nheavy);
        std::vector<int>            lens((size_t)nheavy);
        MI355_HIP_TRY(hipMemcpyAsync(ids.data(), d_ids, sizeof(aoclsparse_int) * (size_t)nheavy, hipMemcpyDeviceToHost, s));
        MI355_HIP_TRY(hipMemcpyAsync(lens.data(), hkeys.ptr, sizeof(int) * (size_t)nheavy, hipMemcpyDeviceToHost, s));
        MI355_HIP_TRY(hipStreamSynchronize(s));
        std::vector<std::pair<aoclsparse_int, int>> rows((size_t)nheavy);
        for(aoclsparse_int j = 0; j < nheavy; j++)
            rows[(size_t)j] = {ids[(size_t)j], lens[(size_t)j]};
        std::vector<SpgHeavy> heavy;
        MI355_TRY(spg_heavy_layout(rows, heavy, plan.batch, plan.slots, plan.entries));
        MI355_TRY(plan.heavy.upload(heavy.data(), sizeof(SpgHeavy) * heavy.size(), s));
    }
    MI355_HIP_TRY(hipStreamSynchronize(s)); // (the order kernel has read `key`; an upload from pageable memory has left the host)
    drain.dismiss();
    plan.valid = true;
    return aoclsparse_status_success;
}

template <typename T>
aoclsparse_status spg_numeric(Runtime &rt, const _aoclsparse_matrix::Sp2mPlan &plan, const SpgDevOp &x, const SpgDevOp &y, bool conj_x,
                              bool conj_y, const SpgDevOp &c, T *out, unsigned int *d_bad)
{
    hipStream_t           s  = rt.stream();
    const T              *xv = static_cast<const T *>(x.val), *yv = static_cast<const T *>(y.val);
    const aoclsparse_int *order = plan.order.as<const aoclsparse_int>();
    for(int b = 0; b < SPGEMM_BINS - 2; b++) // (rows binned by their exact length: the 8,192 bin of the count pass stays empty)
        MI355_TRY(launch_spg_numeric_bin<T>(s, b, plan.bounds[b + 1] - plan.bounds[b], order ? order + plan.bounds[b] : nullptr, x.base,
                                            x.ptr, x.ind, xv, y.base, y.ptr, y.ind, yv, c.base, c.ptr, c.ind, out, conj_x, conj_y, d_bad));
    if(plan.batch.size() < 2)
        return aoclsparse_status_success;
    void *gk = nullptr, *gp = nullptr, *gt = nullptr;
    MI355_TRY(rt.staging(SPG_SLOT_G_KEY, sizeof(int) * (size_t)plan.slots, &gk));
    MI355_TRY(rt.staging(SPG_SLOT_G_POS, sizeof(int) * (size_t)plan.slots, &gp));
    MI355_TRY(rt.staging(SPG_SLOT_G_LIST, (size_t)plan.entries, &gt));
    for(size_t b = 0; b + 1 < plan.batch.size(); b++) // (stream order: a batch reuses the slab)
        MI355_TRY(launch_spg_numeric_heavy<T>(s, plan.batch[b + 1] - plan.batch[b], plan.heavy.as<const SpgHeavy>() + plan.batch[b],
                                              static_cast<int *>(gk), static_cast<int *>(gp), static_cast<unsigned char *>(gt), x.base,
                                              x.ptr, x.ind, xv, y.base, y.ptr, y.ind, yv, c.base, c.ptr, c.ind, out, conj_x, conj_y,
                                              d_bad));
    return aoclsparse_status_success;
}

// ---- the host side (spg_host.hpp) ---------------------------------------------------------------------------------------------
aoclsparse_status spg_resident(const aoclsparse_matrix H, const aoclsparse_int *ptr, size_t vsize, SpgDevOp &dv)
{
    std::unique_lock<std::shared_mutex> w(H->guard);
    const bool own = ptr == H->user.ptr, own_t = H->trans && ptr == H->trans->ptr;
    if(!own && !own_t)
        return aoclsparse_status_not_implemented;
    DeviceCsr &dc = own ? H->dev_user : H->dev_trans;
    if(!dc.valid)
    {
        const aoclsparse_status rc = upload_csr(own ? H->user : *H->trans, vsize, dc);
        if(rc != aoclsparse_status_success)
            return rc;
    }
    dv = SpgDevOp{dc.ptr.as<aoclsparse_int>(), dc.ind.as<aoclsparse_int>(), dc.val.ptr, (int)dc.base}; // (the base of the host copy)
    return aoclsparse_status_success;
}

aoclsparse_status spg_count_to_host(Runtime &rt, const long long *d_total, const aoclsparse_int *d_ptr, aoclsparse_int m,
                                    aoclsparse_index_base base, std::vector<aoclsparse_int> *cptr, aoclsparse_int &total)
{
    hipStream_t s  = rt.stream();
    long long   t64 = 0;
    MI355_HIP_TRY(hipMemcpyAsync(&t64, d_total, sizeof(long long), hipMemcpyDeviceToHost, s));
    if(cptr)
    {
        cptr->resize((size_t)m + 1);
        MI355_HIP_TRY(hipMemcpyAsync(cptr->data(), d_ptr, sizeof(aoclsparse_int) * ((size_t)m + 1), hipMemcpyDeviceToHost, s));
    }
    MI355_HIP_TRY(hipStreamSynchronize(s));
    if(t64 > 2147483647LL - base)
        return aoclsparse_status_invalid_size;
    total = (aoclsparse_int)t64;
    if(cptr && base)
        for(aoclsparse_int &p : *cptr)
            p += base;
    return aoclsparse_status_success;
}

template <typename T>
aoclsparse_status spg_fill_to_host(SpgProduct<T> &prod, bool finalize_only, aoclsparse_int *d_ptr, aoclsparse_int *d_ind, T *d_val,
                                   HostCsr &dst, const std::function<void()> &before_write)
{
    Runtime             &rt = prod.rt;
    hipStream_t          s  = rt.stream();
    const aoclsparse_int m  = prod.m;
    const size_t         ib = sizeof(aoclsparse_int) * (size_t)(dst.ptr[m] - dst.base), vb = sizeof(T) * (size_t)(dst.ptr[m] - dst.base);
    std::vector<aoclsparse_int> zero_based; // (dst's row pointer; lives until the last sync)
    aoclsparse_status           st = aoclsparse_status_success;
    if(finalize_only)
    {
        // rows are binned by their exact count: after a count pass the counts are still in HBM, a finalize call sends the row pointer
        zero_based.assign(dst.ptr, dst.ptr + m + 1);
        for(aoclsparse_int &p : zero_based)
            p -= dst.base;
        st = rt.h2d(d_ptr, zero_based.data(), sizeof(aoclsparse_int) * ((size_t)m + 1));
        if(st == aoclsparse_status_success)
            st = prod.counts_from(d_ptr);
    }
    if(st == aoclsparse_status_success)
        st = prod.fill(d_ptr, d_ind, d_val);
    if(st != aoclsparse_status_success)
        return st;
    unsigned int bad = 0;
    if(finalize_only)
    {
        MI355_HIP_TRY(hipMemcpyAsync(&bad, prod.bad_word(), sizeof(bad), hipMemcpyDeviceToHost, s));
        MI355_HIP_TRY(hipStreamSynchronize(s));
        if(bad)
            return aoclsparse_status_invalid_value;
    }
    before_write();
    // while the kernels run: the result's host arrays are first-touched by several threads (faulted in by the copy itself they cost
    // more than the copy: 7-13 ms for 156 MB against ~3); the values' pages while the column indices already travel
    host_result_touch(dst.ind, ib);
    if(prod.phase)
        prod.phase("fill: kernels (+ host pages of col_ind)");
    std::thread toucher;
    if(vb >= HOST_RESULT_BIG) // (below it host_result_touch does nothing: no thread)
    {
        try
        {
            toucher = std::thread([&] { host_result_touch(dst.val, vb); });
        }
        catch(const std::system_error &)
        {
            host_result_touch(dst.val, vb);
        }
    }
    const hipError_t e1 = hipMemcpyAsync(dst.ind, d_ind, ib, hipMemcpyDeviceToHost, s);
    if(toucher.joinable())
        toucher.join();
    MI355_HIP_TRY(e1);
    MI355_HIP_TRY(hipMemcpyAsync(dst.val, d_val, vb, hipMemcpyDeviceToHost, s));
    if(!finalize_only)
        MI355_HIP_TRY(hipMemcpyAsync(&bad, prod.bad_word(), sizeof(bad), hipMemcpyDeviceToHost, s));
    MI355_HIP_TRY(hipStreamSynchronize(s));
    if(bad) // the row pointer is not the one the count pass of THIS product returned (a row ended short of, or beyond, its segment)
        return aoclsparse_status_invalid_value;
    if(prod.phase)
        prod.phase("fill: result to host");
    return aoclsparse_status_success;
}

#define MI355_SPG_INSTANTIATE(T)   \
    template struct SpgProduct<T>; \
    template aoclsparse_status spg_fill_to_host<T>(SpgProduct<T> &, bool, aoclsparse_int *, aoclsparse_int *, T *, HostCsr &, \
                                                   const std::function<void()> &);                                            \
    template aoclsparse_status spg_numeric<T>(Runtime &, const _aoclsparse_matrix::Sp2mPlan &, const SpgDevOp &, const SpgDevOp &, \
                                              bool, bool, const SpgDevOp &, T *, unsigned int *)
MI355_SPG_INSTANTIATE(double);
MI355_SPG_INSTANTIATE(float);
MI355_SPG_INSTANTIATE(cdouble);
MI355_SPG_INSTANTIATE(cfloat);
#undef MI355_SPG_INSTANTIATE
} // namespace mi355
