// spgemm_numeric_kernels.hip -- the values of C = A * B again, on the structure C already has (aoclsparse_mi355_sp2m_numeric_device).
//
// C's rows list their columns in the first-touch order of the reference's walk (spgemm_kernels.hip, the comment at the top), so the
// numeric phase needs no list and no insertion: the columns C holds go into the hash table once, each with its slot, and every
// product is a lookup.  The arithmetic is the fill pass's -- first product stored, later ones added with a contracted multiply-add,
// in the same walk order -- so the values are its values bit for bit.
//
// The kernel also proves that C's structure IS the product's, row by row, and raises *bad otherwise (nothing of C is written: the
// values go to a buffer of the call's, and the host reads the word first):
//   (a) a product's column is not in C's row                  -- a lookup ends at an empty slot;
//   (b) a slot of C's row receives no product                 -- the columns first touched are fewer than the row holds;
//   (c) C's row holds a column twice                          -- the insert finds its key present;
//   (d) the columns are not first touched in slot order       -- the k-th distinct column the walk meets is not in slot k.
// With (c) and (d) the row's first `len` slots are exactly the first `len` distinct columns of the walk, with (b) len is the row's
// length, with (a) there is no further column: the row is the one the fill pass would write.
//
// Geometry and bins are the fill pass's: 16 lanes and a 64-slot table for rows of up to 32 columns, 64 lanes and 512 / 4,096 slots
// up to 256 / 2,048, the global slab above that (agent-scope loads and fences as explained in spgemm_kernels.hip).  Per group:
// hkey[H], hpos[H] (the slot of the key), acc[H / 2] and touched[H / 2]; in the slab acc is the row's segment of the output itself.
//
// Bound: as the fill pass, latency / instruction bound; 12 B per entry of A and of the touched B rows, 4 B per entry of C read and
// sizeof(T) written.
#include "spgemm_device.hpp"

namespace mi355
{

template <typename T, int G, int LOGH, int NG, bool GLOBAL>
__global__ __launch_bounds__(G *NG) void spg_numeric_kernel(aoclsparse_int nrows, const aoclsparse_int *__restrict__ rows,
                                                           const SpgHeavy *__restrict__ heavy, int *g_key, int *g_pos,
                                                           unsigned char *g_touched, int base_a,
                                                           const aoclsparse_int *__restrict__ ptr_a,
                                                           const aoclsparse_int *__restrict__ ind_a,
                                                           const T *__restrict__ val_a, int base_b,
                                                           const aoclsparse_int *__restrict__ ptr_b,
                                                           const aoclsparse_int *__restrict__ ind_b,
                                                           const T *__restrict__ val_b, int base_c,
                                                           const aoclsparse_int *__restrict__ ptr_c,
                                                           const aoclsparse_int *__restrict__ ind_c, T *out, bool conj_a,
                                                           bool conj_b, unsigned int *bad)
{
    constexpr int EMPTY = -1;
    constexpr int LH    = GLOBAL ? 1 : (1 << LOGH); // (LDS arrays of the global mode: one dummy element)
    using PosT          = typename std::conditional<GLOBAL, int, unsigned short>::type;
    __shared__ int            s_key[NG][LH];
    __shared__ unsigned short s_pos[NG][LH];
    __shared__ unsigned char  s_touched[NG][GLOBAL ? 1 : LH / 2];
    __shared__ T              s_acc[NG][GLOBAL ? 1 : LH / 2];
    const int                 grp = threadIdx.x / G, gl = threadIdx.x % G;
    const int                 wgrp = (threadIdx.x & 63) / G; // group inside its wavefront (ballots are per wavefront)
    const long long           g    = (long long)blockIdx.x * NG + grp;
    if(g >= nrows)
        return;
    int            i, logh = LOGH;
    int           *hkey;
    PosT          *hpos;
    unsigned char *touched;
    T             *acc;
    if constexpr(GLOBAL)
    {
        const SpgHeavy r = heavy[g];
        i = r.row, logh = r.logh;
        hkey = g_key + r.h_off, hpos = reinterpret_cast<PosT *>(g_pos) + r.h_off, touched = g_touched + r.c_off;
    }
    else
    {
        i    = rows ? rows[g] : (int)g; // (no list: every row of the matrix is in this bin)
        hkey = s_key[grp], hpos = reinterpret_cast<PosT *>(s_pos[grp]), touched = s_touched[grp], acc = s_acc[grp];
    }
    const int      H     = 1 << logh;
    const unsigned hmask = (unsigned)H - 1u;
    const int      dst = ptr_c[i] - base_c, nc = ptr_c[i + 1] - ptr_c[i]; // the row's segment of C
    if constexpr(GLOBAL)
        acc = out + dst;
    // (the bins are C's own row lengths: nc <= H / 2 always; a row for which that did not hold would never end a probe)
    bool dead = nc < 0 || nc > H / 2;
    if(dead)
    {
        if(gl == 0)
            atomicOr(bad, 1u);
        return;
    }
    for(int t = gl; t < H; t += G)
        hkey[t] = EMPTY;
    for(int t = gl; t < nc; t += G)
        touched[t] = 0;
    spg_sync<GLOBAL>();
    const unsigned long long lt     = (1ull << gl) - 1ull;
    const int                hshift = 32 - logh;
    auto                     hash   = [&](int c) { return (unsigned)c * 2654435761u >> hshift; };
    // ---- phase 1: C's own columns into the table, value = slot; a key found present: the row holds the column twice ----
    bool twice = false;
    for(int t = gl; t < nc; t += G)
    {
        const int c = ind_c[dst + t] - base_c;
        if(c < 0) // (not a column: it would pass for an empty slot)
        {
            twice = true;
            continue;
        }
        unsigned h = hash(c);
        for(;;)
        {
            const int old = atomicCAS(&hkey[h], EMPTY, c);
            if(old == EMPTY)
            {
                hpos[h] = (PosT)t;
                break;
            }
            if(old == c)
            {
                twice = true;
                break;
            }
            h = (h + 1) & hmask;
        }
    }
    dead = spg_group_bits<G>(__ballot(twice), wgrp) != 0;
    spg_sync<GLOBAL>();
    // ---- phase 2: the walk of the fill pass; every entry a lookup ----
    int       len = 0; // distinct columns met so far
    const int ja = ptr_a[i] - base_a, je = ptr_a[i + 1] - base_a;
    for(int j0 = ja; j0 < je && !dead; j0 += G)
    {
        // this round's entries of A's row, one per lane: value and the extent of the matching B row
        const bool have = j0 + gl < je;
        int        my_kb = 0, my_ke = 0;
        T          my_va = T(0);
        if(have)
        {
            const int ca = ind_a[j0 + gl] - base_a;
            my_kb = ptr_b[ca] - base_b, my_ke = ptr_b[ca + 1] - base_b;
            my_va = sp_conj(val_a[j0 + gl], conj_a);
        }
        const int nj = min(G, je - j0);
        for(int jj = 0; jj < nj && !dead; jj++)
        {
            const int kb = __shfl(my_kb, jj, G), ke = __shfl(my_ke, jj, G);
            const T   va = spg_shfl(my_va, jj, G);
            int       carry = -1;
            for(int k0 = kb; k0 < ke && !dead; k0 += G)
            {
                const int  k     = k0 + gl;
                const bool valid = k < ke;
                const int  c     = valid ? ind_b[k] - base_b : 0x7fffffff;
                T          vb    = T(0);
                if(valid)
                    vb = sp_conj(val_b[k], conj_b);
                int prev = __shfl_up(c, 1, G);
                if(gl == 0)
                    prev = carry;
                carry = __shfl(c, G - 1, G);
                const unsigned long long unsorted = spg_group_bits<G>(__ballot(valid && c <= prev), wgrp);
                if(!unsorted)
                {
                    // distinct columns: looked up together; the new ones must sit in the next slots, in lane order
                    int pos = -1;
                    if(valid)
                    {
                        unsigned h = hash(c);
                        for(;;)
                        {
                            const int key = spg_key<GLOBAL>(&hkey[h]);
                            if(key == EMPTY)
                                break;
                            if(key == c)
                            {
                                pos = (int)hpos[h];
                                break;
                            }
                            h = (h + 1) & hmask;
                        }
                    }
                    const bool               isnew = valid && pos >= 0 && !touched[pos];
                    const unsigned long long nm    = spg_group_bits<G>(__ballot(isnew), wgrp);
                    const bool               wrong = valid && (pos < 0 || (isnew && pos != len + __popcll(nm & lt)));
                    if(spg_group_bits<G>(__ballot(wrong), wgrp)) // (a) or (d)
                    {
                        dead = true;
                        break;
                    }
                    if(isnew)
                    {
                        touched[pos] = 1;
                        acc[pos]     = sp_mul(va, vb); // first touch: the product itself (csr2m.cpp:489-496)
                    }
                    else if(valid)
                        acc[pos] = sp_fma(va, vb, acc[pos]); // csr2m.cpp:498, contracted
                    len += __popcll(nm);
                }
                else
                {
                    // unsorted or repeated columns inside this chunk: one entry at a time, in order (every lane the same lookup)
                    const int nv = min(G, ke - k0);
                    for(int q = 0; q < nv; q++)
                    {
                        const int cq  = __shfl(c, q, G);
                        const T   vq  = spg_shfl(vb, q, G);
                        unsigned  h   = hash(cq);
                        int       pos = -1;
                        for(;;)
                        {
                            const int key = spg_key<GLOBAL>(&hkey[h]);
                            if(key == EMPTY)
                                break;
                            if(key == cq)
                            {
                                pos = (int)hpos[h];
                                break;
                            }
                            h = (h + 1) & hmask;
                        }
                        const bool fresh = pos >= 0 && !touched[pos];
                        if(pos < 0 || (fresh && pos != len)) // (a) or (d); uniform inside the group
                        {
                            dead = true;
                            break;
                        }
                        if(gl == 0)
                        {
                            if(fresh)
                            {
                                touched[pos] = 1;
                                acc[pos]     = sp_mul(va, vq);
                            }
                            else
                                acc[pos] = sp_fma(va, vq, acc[pos]);
                        }
                        len += fresh;
                        spg_sync<GLOBAL>();
                    }
                }
                spg_sync<GLOBAL>();
            }
        }
    }
    dead |= len != nc; // (b)
    if(dead)
    {
        if(gl == 0)
            atomicOr(bad, 1u);
        return;
    }
    // ---- phase 3: the accumulators to the row's segment (the slab's rows have accumulated there) ----
    if constexpr(!GLOBAL)
        for(int t = gl; t < nc; t += G)
            out[dst + t] = acc[t];
}

template <typename T>
aoclsparse_status launch_spg_numeric_bin(hipStream_t s, int bin, aoclsparse_int nrows, const aoclsparse_int *rows, int base_a,
                                         const aoclsparse_int *ptr_a, const aoclsparse_int *ind_a, const T *val_a, int base_b,
                                         const aoclsparse_int *ptr_b, const aoclsparse_int *ind_b, const T *val_b, int base_c,
                                         const aoclsparse_int *ptr_c, const aoclsparse_int *ind_c, T *out, bool conj_a, bool conj_b,
                                         unsigned int *bad)
{
    if(nrows <= 0)
        return aoclsparse_status_success;
#define MI355_SPG_NUM(G, LOGH, NG)                                                                                                  \
    hipLaunchKernelGGL((spg_numeric_kernel<T, G, LOGH, NG, false>), dim3((unsigned)((nrows + NG - 1) / NG)), dim3(G * NG), 0, s,      \
                       nrows, rows, (const SpgHeavy *)nullptr, (int *)nullptr, (int *)nullptr, (unsigned char *)nullptr, base_a,     \
                       ptr_a, ind_a, val_a, base_b, ptr_b, ind_b, val_b, base_c, ptr_c, ind_c, out, conj_a, conj_b, bad)
    switch(bin) // (the fill pass's geometry: launch_spgemm_bin)
    {
    case 0: MI355_SPG_NUM(16, 6, 16); break;
    case 1: MI355_SPG_NUM(64, 9, 4); break;
    case 2: MI355_SPG_NUM(64, 12, 1); break;
    default: return aoclsparse_status_internal_error;
    }
#undef MI355_SPG_NUM
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

// the rows above the largest LDS bin: g_key / g_pos hold the tables (SpgHeavy::h_off), g_touched the flags (c_off)
template <typename T>
aoclsparse_status launch_spg_numeric_heavy(hipStream_t s, aoclsparse_int nrows, const SpgHeavy *heavy, int *g_key, int *g_pos,
                                           unsigned char *g_touched, int base_a, const aoclsparse_int *ptr_a,
                                           const aoclsparse_int *ind_a, const T *val_a, int base_b, const aoclsparse_int *ptr_b,
                                           const aoclsparse_int *ind_b, const T *val_b, int base_c, const aoclsparse_int *ptr_c,
                                           const aoclsparse_int *ind_c, T *out, bool conj_a, bool conj_b, unsigned int *bad)
{
    if(nrows <= 0)
        return aoclsparse_status_success;
    hipLaunchKernelGGL((spg_numeric_kernel<T, 64, 0, 1, true>), dim3((unsigned)nrows), dim3(64), 0, s, nrows,
                       (const aoclsparse_int *)nullptr, heavy, g_key, g_pos, g_touched, base_a, ptr_a, ind_a, val_a, base_b, ptr_b,
                       ind_b, val_b, base_c, ptr_c, ind_c, out, conj_a, conj_b, bad);
    MI355_HIP_TRY(hipGetLastError());
    return aoclsparse_status_success;
}

#define MI355_SPG_NUMERIC_INST(T)                                                                                                    \
    template aoclsparse_status launch_spg_numeric_bin<T>(hipStream_t, int, aoclsparse_int, const aoclsparse_int *, int,             \
                                                         const aoclsparse_int *, const aoclsparse_int *, const T *, int,            \
                                                         const aoclsparse_int *, const aoclsparse_int *, const T *, int,            \
                                                         const aoclsparse_int *, const aoclsparse_int *, T *, bool, bool,           \
                                                         unsigned int *);                                                           \
    template aoclsparse_status launch_spg_numeric_heavy<T>(hipStream_t, aoclsparse_int, const SpgHeavy *, int *, int *,             \
                                                           unsigned char *, int, const aoclsparse_int *, const aoclsparse_int *,    \
                                                           const T *, int, const aoclsparse_int *, const aoclsparse_int *, const T *, \
                                                           int, const aoclsparse_int *, const aoclsparse_int *, T *, bool, bool,    \
                                                           unsigned int *);
MI355_SPG_NUMERIC_INST(double)
MI355_SPG_NUMERIC_INST(float)
MI355_SPG_NUMERIC_INST(cdouble)
MI355_SPG_NUMERIC_INST(cfloat)

} // namespace mi355
