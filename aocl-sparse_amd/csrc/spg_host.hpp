// spg_host.hpp -- the host side that aoclsparse_sp2m, aoclsparse_syrk and aoclsparse_sypr share around SpgProduct (spg_product.cpp).
// The transpose core also serves the handles' kept transpose (matrix.cpp) and aoclsparse_?csr2csc.
#pragma once
#include "internal.hpp"

#include <algorithm>
#include <functional>
#include <vector>

namespace mi355
{

// B = A^T by the stable counting sort of conversion/aoclsparse_convert.hpp:552-655.  The column histogram runs flat over
// ind[0 .. nnz), as the reference's does; the scatter walks the rows.  The two agree whenever ptr[0] == base_in and
// ptr[m] - base_in == nnz: mat_check (every create_?csr / create_?csc / alias_csr) and its device twin (matcheck.hpp) refuse
// anything else, and a result handle's row pointer is a prefix sum from base to nnz -- except in the C of a count-only sp2m(T, T),
// which holds nnz with a row pointer still all base and ind unwritten.  So callers that hold a handle pass the count the row
// pointer spans; aoclsparse_?csr2csc on raw arrays checks nothing and passes the caller's nnz, as the reference does.
template <typename T>
void host_transpose(aoclsparse_int m, aoclsparse_int n, aoclsparse_int nnz, aoclsparse_int base_in, aoclsparse_int base_out,
                    const aoclsparse_int *ptr, const aoclsparse_int *ind, const T *val, aoclsparse_int *optr, aoclsparse_int *oind,
                    T *oval)
{
    std::fill(optr, optr + n + 1, 0);
    for(aoclsparse_int p = 0; p < nnz; p++)
        ++optr[ind[p] - base_in + 1];
    for(aoclsparse_int j = 0; j < n; j++)
        optr[j + 1] += optr[j];
    for(aoclsparse_int i = 0; i < m; i++)
        for(aoclsparse_int p = ptr[i] - base_in; p < ptr[i + 1] - base_in; p++)
        {
            const aoclsparse_int q = optr[ind[p] - base_in]++; // (optr[j] runs up to the start of column j + 1 ...)
            oind[q] = i + base_out, oval[q] = val[p];
        }
    for(aoclsparse_int j = n; j > 0; j--) // (... so the array is shifted up by one afterwards)
        optr[j] = optr[j - 1] + base_out;
    optr[0] = base_out;
}

// a host CSR: a view (of a handle's arrays) or owned
template <typename T>
struct HostCsrOp
{
    aoclsparse_int              m = 0, n = 0, nnz = 0, base = 0;
    const aoclsparse_int       *ptr = nullptr, *ind = nullptr;
    const T                    *val = nullptr;
    std::vector<aoclsparse_int> optr, oind;
    std::vector<T>              oval;
    void own()
    {
        ptr = optr.data(), ind = oind.data(), val = oval.data();
    }
};

template <typename T>
void view_of(const HostCsr &h, HostCsrOp<T> &o)
{
    o.m = h.m, o.n = h.n, o.nnz = h.nnz, o.base = h.base;
    o.ptr = h.ptr, o.ind = h.ind, o.val = static_cast<const T *>(h.val);
}

// t = a^T in a's base, owned
template <typename T>
void transpose_of(const HostCsrOp<T> &a, HostCsrOp<T> &t)
{
    t.m = a.n, t.n = a.m, t.nnz = a.nnz, t.base = a.base;
    t.optr.resize((size_t)t.m + 1);
    t.oind.resize((size_t)std::max(a.nnz, 1));
    t.oval.resize((size_t)std::max(a.nnz, 1));
    host_transpose(a.m, a.n, a.ptr[a.m] - a.base, a.base, a.base, a.ptr, a.ind, a.val, t.optr.data(), t.oind.data(), t.oval.data());
    t.own();
}

// host CSR -> three staging slots starting at `first` (ptr, ind, val; the values only when asked for: a count pass reads none)
template <typename T>
aoclsparse_status spg_send(Runtime &rt, const HostCsrOp<T> &o, StageSlot first, bool with_values, SpgDevOp &dv)
{
    void             *pp = nullptr, *pi = nullptr, *pv = nullptr;
    const size_t      np = (size_t)o.m + 1, nz = (size_t)std::max<aoclsparse_int>(o.nnz, 1);
    aoclsparse_status rc = rt.staging(first, sizeof(aoclsparse_int) * np, &pp);
    if(rc == aoclsparse_status_success)
        rc = rt.staging(first + 1, sizeof(aoclsparse_int) * nz, &pi);
    if(rc == aoclsparse_status_success && with_values)
        rc = rt.staging(first + 2, sizeof(T) * nz, &pv);
    if(rc == aoclsparse_status_success)
        rc = rt.h2d(pp, o.ptr, sizeof(aoclsparse_int) * np);
    if(rc == aoclsparse_status_success)
        rc = rt.h2d(pi, o.ind, sizeof(aoclsparse_int) * (size_t)o.nnz);
    if(rc == aoclsparse_status_success && with_values)
        rc = rt.h2d(pv, o.val, sizeof(T) * (size_t)o.nnz);
    dv = SpgDevOp{static_cast<const aoclsparse_int *>(pp), static_cast<const aoclsparse_int *>(pi), pv, (int)o.base};
    return rc;
}

// Arrays that ARE the handle's user arrays or its kept transpose are used from the handle's own device copy, made here when
// nothing has made it yet (the next product with this handle sends nothing); anything else: not_implemented.  Takes the handle's
// guard exclusively for its own duration; the caller holds the stage lock already (CallScope), which comes first.
aoclsparse_status spg_resident(const aoclsparse_matrix H, const aoclsparse_int *ptr, size_t vsize, SpgDevOp &dv);

// resident when it is the handle's own, sent otherwise
template <typename T>
aoclsparse_status spg_to_device(Runtime &rt, const aoclsparse_matrix H, const HostCsrOp<T> &o, StageSlot first, bool with_values,
                                SpgDevOp &dv)
{
    const aoclsparse_status rc = spg_resident(H, o.ptr, sizeof(T), dv);
    return rc == aoclsparse_status_not_implemented ? spg_send(rt, o, first, with_values, dv) : rc;
}

// After a count pass (or a scan of counts): the total and, when cptr is given, the row pointer to the host in index base `base`;
// invalid_size when the total does not fit the index type in that base (csr2m.cpp:221-236, sypr.hpp:391-396, :512-525).
aoclsparse_status spg_count_to_host(Runtime &rt, const long long *d_total, const aoclsparse_int *d_ptr, aoclsparse_int m,
                                    aoclsparse_index_base base, std::vector<aoclsparse_int> *cptr, aoclsparse_int &total);

// The fill pass of `prod` into dst (prod.m rows, any base) through the 0-based device arrays.  finalize_only: d_ptr does not hold
// the row pointer yet: dst's is sent and turned into counts, and the verdict of the device checks is read BEFORE before_write()
// runs and anything of dst is written (a refused call leaves the caller's handle as it was); otherwise the verdict is read with
// the result.  The column indices arrive 0-based: a caller whose result has another base shifts them.
template <typename T>
aoclsparse_status spg_fill_to_host(SpgProduct<T> &prod, bool finalize_only, aoclsparse_int *d_ptr, aoclsparse_int *d_ind, T *d_val,
                                   HostCsr &dst, const std::function<void()> &before_write);

} // namespace mi355
