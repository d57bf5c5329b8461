/*
 * aoclsparse_mi355.h -- MI355X-specific additions next to the aoclsparse_* drop-in ABI.
 *
 * Nothing here exists in the reference (a CPU library has no device boundary).  Two groups:
 *   1. aoclsparse_mi355_*: runtime control and introspection of a handle's device plan.
 *   2. mi355_*: the thin HIP C-ABI the host layer itself calls -- plain device pointers,
 *      sizes and a hipStream_t (passed as void*), no handles, asynchronous.  These are the
 *      entry points a benchmark or a solver that keeps x/y resident in HBM binds directly.
 */
#ifndef AOCLSPARSE_MI355_H_
#define AOCLSPARSE_MI355_H_

#include "aoclsparse.h"

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- runtime control ------------------------------------------------------------------ */
typedef enum aoclsparse_mi355_pointer_mode_
{
    aoclsparse_mi355_pointer_auto   = 0, /* classify x/y/B/C per call (hipPointerGetAttributes) */
    aoclsparse_mi355_pointer_host   = 1, /* reference semantics: host pointers, staged, synchronous */
    aoclsparse_mi355_pointer_device = 2 /* device pointers, stream-ordered, no query */
} aoclsparse_mi355_pointer_mode;

DLL_PUBLIC aoclsparse_status aoclsparse_mi355_set_pointer_mode(aoclsparse_mi355_pointer_mode mode);
/* Plan options: ONE hook for the tests and measurements that must reach a kernel the automatic choice would not pick for
 * their (small) input.  Process-wide, read when a handle's plan is built (so: set before aoclsparse_optimize / the first
 * product, reset afterwards).  Everything else the library chooses by itself; the selection switches of rounds 1-3
 * (environment variables) are gone -- their measurements are under profiles/.
 *   spmv_kernel  0 automatic (default: CSR-Adaptive, merge-path once the longest row spans 16 LDS tiles = 8,192 entries for
 *                matrices below 4 M non-zeros), 1 CSR-Adaptive, 2 merge-path whenever it can serve the request.  Since round 5 both
 *                CSR kernels sum rows of >= spmv_info.tree_min (32) entries with a wavefront tree in their automatic mode: such
 *                rows are within the stated bound, no longer the reference's bits -- spmv_strict = 1 or a pinned kid restores them
 *   sell         -1 automatic (default: SELL-64 copy for an mv hint when its padding is <= 1.35 x), 0 never, 1 always
 *   spmv_strict  0 (default): without a pinned kid, CSR-Adaptive sums a row of >= spmv_info.tree_min entries with a wavefront tree
 *                (componentwise bound (2 ceil(log2 n) + 4) eps sum|a||x|; shorter rows are the reference's chain, bit for bit);
 *                1: every row of every product in the reference's order, as a pinned kid does -- bit-exact everywhere, at the
 *                price of one lane's serial chain per long row.  Read at every product (not a plan option).
 *   alternate_sweeps  1 (default): consecutive products of a handle (SpMV on the SELL-64 copy or on the row blocks, row-major
 *                csrmm) walk the matrix in alternating directions, so the end of one sweep -- what the 256 MB Infinity Cache still
 *                holds -- is where the next one starts; 0: always ascending.  Same bits either way (a row's chain does not depend
 *                on when the row is visited); a measurement of HBM throughput sets 0 or flushes the cache between products.
 *                Read at every product.
 *   trsv_chunks  -1 (default): the two-level TRSV schedule (chunks of consecutive blocks, hand-offs inside a chunk through LDS;
 *                schedule 5) is built when the plan-time model of the triangle's DAG predicts a gain over the lane-per-block
 *                schedule (deep, narrow DAGs: a mesh numbered line by line); 0 never; 1 whenever the triangle has the shape the
 *                kernel serves.  Read when a TRSV plan is built.  Same bits on every schedule.
 *   sell_values  -1 (default): a SELL-64 copy of a real matrix with >= 2^17 non-zeros whose values take at most 256 distinct bit
 *                patterns stores indices into a table of those patterns instead (aoclsparse_mi355_get_sell_values): one byte
 *                per cell, or -- a copy of short rows, where the indices of a row fit 32 bits -- one packed word of 1 / 2 / 4
 *                bytes per row (aoclsparse_mi355_get_sell_packing);
 *                0 never (the values in the cells); 1 whenever there are at most 256 patterns, whatever the size.  Read when the
 *                SELL-64 copy is built.  Same bits either way: the table holds the values' exact bit patterns.
 *   ilu_search   -1 (default): the ILU(0) factorisation finds the position of row i that an entry of row k updates by a binary
 *                search of the row's columns, instead of a scan of the row, when the handle's rows are fully sorted (sort class 1)
 *                and its longest row has at least AOCLSPARSE_MI355_ILU_SEARCH_MIN entries; 0 always the scan; 1 the search whenever
 *                the sort class is 1 (never for class 2: rows there are only grouped lower / diagonal / upper).  Read when a
 *                handle's ILU(0) schedule is built (aoclsparse_mi355_get_ilu_info).  Same bits either way.  Its number lies
 *                outside 0 .. option_count - 1: that block and its count stay as they are (callers and tests rely on both). */
typedef enum aoclsparse_mi355_option_
{
    aoclsparse_mi355_option_spmv_kernel = 0,
    aoclsparse_mi355_option_sell        = 1,
    aoclsparse_mi355_option_spmv_strict = 2,
    aoclsparse_mi355_option_alternate_sweeps = 3,
    aoclsparse_mi355_option_trsv_chunks = 4,
    aoclsparse_mi355_option_sell_values = 5,
    aoclsparse_mi355_option_count       = 6,
    aoclsparse_mi355_option_ilu_search  = 16
} aoclsparse_mi355_option;
/* the automatic ilu_search rule: the smallest longest row from which the search was measured to win (profiles/r26/ilu_refactor.txt:
 * by 40 % at 21 entries, a tie at 5; nothing in between was measured) */
#define AOCLSPARSE_MI355_ILU_SEARCH_MIN 21
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_set_option(aoclsparse_mi355_option option, aoclsparse_int value);
/* aoclsparse_?csrmm with beta == 0.  Default (0): C is read and multiplied by zero, exactly as every kernel of the reference
 * does (level3/aoclsparse_csrmm.hpp:83,129; aoclsparse_csrmm_kt.cpp:176-191,246), so a NaN / Inf already in C propagates.
 * 1: C is overwritten without being read (BLAS convention; identical results for every finite C, including the sign of
 * exact zeros; saves the read of C: ~15 % at 256 columns).  Also AOCLSPARSE_MI355_CSRMM_BETA0_OVERWRITE=1. */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_set_csrmm_beta0_overwrite(int overwrite);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_set_stream(void *hip_stream);
DLL_PUBLIC void             *aoclsparse_mi355_get_stream(void);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_synchronize(void);
/* device ordinal in use, CU count and name; status internal_error when no HIP device exists */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_device_info(aoclsparse_int *device,
                                                          aoclsparse_int *compute_units,
                                                          char            name[256]);
/* Path of the HIP runtime (libamdhip64) this library's calls are bound to, as the dynamic loader resolved them.  A process can
 * hold two copies (a framework that ships its own next to /opt/rocm's): streams and events are objects of ONE runtime, so a
 * stream handed to aoclsparse_mi355_set_stream must come from the copy named here.  Writes at most `capacity` bytes including
 * the terminating zero; invalid_pointer / invalid_size for a null or empty buffer, internal_error when the loader cannot tell. */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_hip_runtime_path(char *path, size_t capacity);
/* hipEvent pair on the library's stream: start, run work, stop -> elapsed milliseconds */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_timer_start(void);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_timer_stop(float *elapsed_ms);
/* per-iteration timing (the reference harness reports min / quartiles / max of its iterations,
 * tests/include/aoclsparse_stats.hpp:41-129): mark() records one event on the library's stream (at most 65536 between
 * two laps() calls); laps() waits for the last mark, writes min(*count, capacity) elapsed times between consecutive
 * marks (milliseconds) and resets the ring. */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_timer_mark(void);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_timer_laps(float *laps_ms, aoclsparse_int capacity, aoclsparse_int *count);

/* ---- column shards of csrmm: one process per GPU ------------------------------------------ */
/* The reference splits B's columns over its worker threads inside the library
 * (library/src/level3/aoclsparse_csrmm_kt.cpp:68-82: start = n*t/T rounded up to a multiple of 4, capped at n).
 * column_shard applies that rule with (world, rank) in place of (threads, thread id); ?csrmm_shard computes the slab
 * C[:, j0:j1) of rank `rank` from the FULL B / C arrays (same arguments as aoclsparse_?csrmm otherwise).  There is no
 * communication on the data path: a rank needs A and its own columns of B only. */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_column_shard(aoclsparse_int n, aoclsparse_int world, aoclsparse_int rank,
                                                           aoclsparse_int *j0, aoclsparse_int *j1);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_dcsrmm_shard(aoclsparse_operation op, const double alpha,
                                                           const aoclsparse_matrix A, const aoclsparse_mat_descr descr,
                                                           aoclsparse_order order, const double *B, aoclsparse_int n,
                                                           aoclsparse_int ldb, const double beta, double *C,
                                                           aoclsparse_int ldc, aoclsparse_int world, aoclsparse_int rank);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_scsrmm_shard(aoclsparse_operation op, const float alpha,
                                                           const aoclsparse_matrix A, const aoclsparse_mat_descr descr,
                                                           aoclsparse_order order, const float *B, aoclsparse_int n,
                                                           aoclsparse_int ldb, const float beta, float *C,
                                                           aoclsparse_int ldc, aoclsparse_int world, aoclsparse_int rank);

/* ---- one process, several GPUs (round 3) ----------------------------------------------------
 * C = alpha * op(A) * B + beta * C with the columns of B and C split over `ndev` devices by the rule above; the GPU takes
 * the place of the reference's worker thread (aoclsparse_csrmm_kt.cpp:68-82).  devices[0] must be the library's own device
 * (AOCLSPARSE_MI355_DEVICE, else the caller's current device); devices == NULL means that device and the next ndev - 1
 * ordinals.  The first call builds a replica of the handle on every other device (same host arrays, hints copied,
 * aoclsparse_optimize there), later calls reuse it; ?set_value / ?update_values / aoclsparse_mi355_invalidate drop the
 * replicas.  No collective on the data path.  Returns when every device has finished.
 *   ?csrmm_multi        B, C = the FULL operands in HOST memory (the reference's calling convention): each device stages
 *                       and returns its own slab over its own PCIe link.  AOCLSPARSE_MI355_DEVICES=N makes plain
 *                       aoclsparse_?csrmm take this path for host operands.
 *   dcsrmm_multi_slabs  B_slabs[i] / C_slabs[i] = device i's slab, resident in ITS memory (column-major: columns
 *                       [j0_i, j1_i) with leading dimension ldb / ldc; row-major: rows of j1_i - j0_i columns); n is the
 *                       TOTAL column count.  The path for operands that already live on the GPUs. */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_dcsrmm_multi(aoclsparse_operation op, const double alpha,
                                                           const aoclsparse_matrix A, const aoclsparse_mat_descr descr,
                                                           aoclsparse_order order, const double *B, aoclsparse_int n,
                                                           aoclsparse_int ldb, const double beta, double *C,
                                                           aoclsparse_int ldc, aoclsparse_int ndev,
                                                           const aoclsparse_int *devices);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_scsrmm_multi(aoclsparse_operation op, const float alpha,
                                                           const aoclsparse_matrix A, const aoclsparse_mat_descr descr,
                                                           aoclsparse_order order, const float *B, aoclsparse_int n,
                                                           aoclsparse_int ldb, const float beta, float *C,
                                                           aoclsparse_int ldc, aoclsparse_int ndev,
                                                           const aoclsparse_int *devices);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_dcsrmm_multi_slabs(aoclsparse_operation op, const double alpha,
                                                                 const aoclsparse_matrix A, const aoclsparse_mat_descr descr,
                                                                 aoclsparse_order order, const double *const *B_slabs,
                                                                 aoclsparse_int n, aoclsparse_int ldb, const double beta,
                                                                 double *const *C_slabs, aoclsparse_int ldc,
                                                                 aoclsparse_int ndev, const aoclsparse_int *devices);

/* Operands of the two calls above must be COMPLETE on every device before the call (work in flight on a device's null stream
 * is ordered before the product: the slot streams are blocking streams; work on other non-blocking streams is not).
 * multi_last_ms: wall time each device spent on its share in the last multi-device call of the process (its launches and the
 * wait for its stream), ms[i] for i < min(returned count, capacity); returns the device count of that call (0: none yet). */
DLL_PUBLIC aoclsparse_int aoclsparse_mi355_multi_last_ms(float *ms, aoclsparse_int capacity);

/* replicas of the handle currently alive on other runtime slots (0 before the first multi-device call); -1 for NULL */
DLL_PUBLIC aoclsparse_int aoclsparse_mi355_replica_count(const aoclsparse_matrix A);
/* ... of which built by copying the primary handle's device format device to device (peer copy over xGMI) instead of analysing
 * the host arrays again: the case when the handle was optimized (or used) before its first multi-device call; -1 for NULL */
DLL_PUBLIC aoclsparse_int aoclsparse_mi355_replicas_cloned(const aoclsparse_matrix A);

/* ---- one process per GPU: shipping the ANALYSED device state of a handle (round 4) ----------------------------------------
 * The column shards of csrmm need A on every rank.  What travels is the device format: the CSR arrays in HBM and every csrmm
 * plan (row blocks, row groups, row runs, column windows, row pairs, the blocked-ELL copy), so that the receiving ranks do no
 * analysis (the reference has nothing to ship: its column split is a thread split inside one call,
 * library/src/level3/aoclsparse_csrmm_kt.cpp:68-82, and A is shared memory).
 *   export  builds every csrmm plan of A that is still missing, then fills `state` (sizes + scalars, a POD that can be sent as
 *           bytes) and buffers[i] = device pointer of buffer i (owned by A, valid until A is modified or destroyed; NULL where
 *           state->bytes[i] == 0).
 *   adopt   creates a NEW handle (*R, to be destroyed by the caller) from `state` and device copies of the buffers that the caller
 *           has placed in THIS process's device memory (received over whatever wire it uses): the buffers are copied device to
 *           device, the CSR arrays are copied back once to give the handle its host view, no analysis runs.  Every
 *           aoclsparse_* call works on the new handle; it carries an optimized mm hint. */
#define AOCLSPARSE_MI355_MM_STATE_BUFFERS 14
#define AOCLSPARSE_MI355_MM_STATE_SCALARS 40
typedef struct aoclsparse_mi355_mm_state_
{
    long long scalars[AOCLSPARSE_MI355_MM_STATE_SCALARS];
    long long bytes[AOCLSPARSE_MI355_MM_STATE_BUFFERS];
} aoclsparse_mi355_mm_state;
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_mm_state_export(aoclsparse_matrix A, aoclsparse_mi355_mm_state *state,
                                                              const void *buffers[AOCLSPARSE_MI355_MM_STATE_BUFFERS]);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_mm_state_adopt(aoclsparse_matrix *R, const aoclsparse_mi355_mm_state *state,
                                                             const void *const buffers[AOCLSPARSE_MI355_MM_STATE_BUFFERS]);

/* ---- the matrix is already on the GPU: CSR handles from, to and updated by arrays in HBM (round 7) --------------------------
 * aoclsparse_create_?csr takes host arrays, which the first product uploads; ?update_values and aoclsparse_export_?csr speak host
 * arrays too.  For a matrix that was assembled on the device (a sparse_csr tensor, a time-stepping code that refreshes its values)
 * the three groups below do the same work from and to device arrays.  aoclsparse_int is 32-bit, here as everywhere.
 *
 *   create_?csr_device   The arguments of aoclsparse_create_?csr, with row_ptr (M + 1 entries), col_idx and val (nnz entries each)
 *           in device memory.  The arrays are COPIED: on return the handle owns a device copy (resident: spmv_info.device_resident
 *           is 1 before any product) and an owned host view made by one copy back, so every aoclsparse_* entry point works on the
 *           handle as on a host-created one and gives the same bits.  The caller may overwrite or free its arrays afterwards.
 *           The caller's arrays must be COMPLETE before the call (the work that fills them on other streams has finished: the
 *           library reads them on its own stream and does not wait for anyone else's); the call synchronises the library's stream
 *           before it returns.
 *           Validity, the sort class and the full-diagonal flag are decided on the device and are exactly what
 *           aoclsparse_create_?csr decides for the same arrays on the host: invalid_value for a row_ptr that does not start at
 *           base, does not end at base + nnz or decreases (col_idx is then never read); otherwise the status of the first
 *           offending row -- invalid_index_value for a column outside [base, base + N), invalid_value for a second diagonal
 *           entry, whichever comes first in that row.
 *           Decided before the device is touched, in the host call's order: invalid_pointer for a null mat or a null array,
 *           invalid_size for a negative M, N or nnz.  A base other than 0 / 1 is not refused as such (aoclsparse_create_?csr does
 *           not either): the arrays are checked against it like against any base.  An array that is not device (or managed)
 *           memory in the current pointer mode: invalid_pointer.  M == 0 and nnz == 0 are valid, as on the host; the arrays must
 *           still be non-null device allocations.
 *   ?update_values_device   aoclsparse_?update_values with a device array of len = nnz values in the order of the handle's CSR
 *           arrays.  Same statuses in the same order (invalid_pointer, invalid_size, wrong_type, not_implemented for TCSR / BSR
 *           handles); in addition not_implemented for a COO handle and a handle created from CSC arrays, whose values follow the
 *           order of host arrays.  The values are copied into the host view (for a host-created handle that is the caller's own
 *           val array, as with ?update_values) and, when the handle's CSR is resident, device to device into the resident copy,
 *           which stays resident: the next product uploads nothing.  Everything derived from the values (SELL-64 and blocked-ELL
 *           copies, TRSV plans, derived operators, replicas) is dropped and rebuilt on first use, as after the host call.
 *           `val` must be complete before the call; the library's stream is synchronised before return.
 *   export_csr_device   The device pointers of the handle's resident CSR arrays (uploaded first when they are not resident):
 *           the arrays the handle was created from / holds as `user` arrays, in their base -- not the clean copy
 *           aoclsparse_export_?csr prefers after aoclsparse_optimize.  Works on every CSR-format handle: host-created,
 *           device-created, a result of sp2m / syrk / sypr, an adopted one.  COO, TCSR and BSR handles: invalid_value.  The
 *           pointers are READ-ONLY and valid until the handle is modified (?update_values*, ?set_value, aoclsparse_order_mat,
 *           aoclsparse_mi355_order_mat_device, aoclsparse_mi355_invalidate) or destroyed; val points to values of the handle's
 *           type.  The library's stream is synchronised before return.
 *
 *   create_?csr_from_coo_device   (round 19) The arguments of aoclsparse_create_?coo plus `duplicates`, with row_ind, col_ind and val
 *           (nnz entries each) in device memory, in ANY order: the triplets a finite-element assembly, a graph construction or a
 *           sparse_coo tensor leaves behind.  The result is an ordinary CSR-format handle of the kind create_?csr_device returns:
 *           a resident device copy (spmv_info.device_resident is 1 before any product), an owned host view, and every
 *           aoclsparse_* entry point works on it.  The caller's arrays are copied and may be overwritten or freed on return; they
 *           must be COMPLETE before the call (the library reads them on its own stream and waits for nobody else's); the call
 *           synchronises the library's stream before it returns.
 *           The triplets are sorted on the device by a stable least-significant-digit radix sort of (key, position) pairs
 *           (coo_sort_kernels.hip) that never looks at the length of a row: one row or column may hold any share of the entries.
 *           A workgroup takes AOCLSPARSE_MI355_COO_SORT_TILE entries per pass.
 *           duplicates = aoclsparse_mi355_coo_keep: the CSR is exactly what aoclsparse_create_?coo + aoclsparse_convert_csr
 *           (op = none) give for the same triplets on the host -- the reference's stable counting sort by row.  The entries of a
 *           row keep their triplet order, repeated coordinates stay separate entries, values are moved and never touched.  The
 *           sort class and the full-diagonal flag are what aoclsparse_create_?csr decides on the converted arrays.
 *           duplicates = aoclsparse_mi355_coo_sum: the entries are ordered by (row, column), stably, and every run of equal
 *           coordinates becomes ONE entry whose value is the left-to-right chain ((v0 + v1) + v2) + ... in triplet order, in the
 *           value type (complex values component by component).  A sum that comes out zero stays an explicit entry.  The handle's
 *           nnz is the number of distinct coordinates; its rows are fully sorted.  No float atomics take part: the result is a
 *           pure function of the input arrays, and two calls on one input give the same bytes.
 *           Statuses, in this order.  Before the device is touched, in aoclsparse_create_?coo's order: invalid_pointer for a null
 *           mat (otherwise *mat is cleared first), invalid_size for a negative M, N or nnz, invalid_pointer for a null array,
 *           invalid_value for a `duplicates` other than 0 / 1.  Then: invalid_pointer for an array that is not device (or managed)
 *           memory in the current pointer mode; invalid_index_value for any row outside [base, base + M) or column outside
 *           [base, base + N) -- decided on the device before any output is allocated, nothing is ever written out of range; in
 *           `keep` mode whatever create_?csr_device answers for the converted arrays, in practice invalid_value for a second
 *           diagonal entry in a row.  nnz == 0 and M == 0 are valid; the arrays must still be non-null device allocations.
 *           duplicates | aoclsparse_mi355_coo_keep_map (16; the valid values of `duplicates` are 0, 1, 16 and 17, every other one
 *           is invalid_value at the place named above): the CSR is byte for byte what the call without the flag gives, and the
 *           handle also keeps the sort's map in device memory -- for every sorted entry the triplet it came from (one int per
 *           triplet), in `sum` mode also where every run of equal coordinates starts (distinct + 1 ints).  aoclsparse_destroy frees
 *           it.  Without the flag nothing is kept.
 *   ?refresh_values_from_coo_device   (round 22) New values for a handle created with aoclsparse_mi355_coo_keep_map, from the SAME
 *           triplets with other values: what a time step or a Newton iteration of the assembly that made them produces.  `val`
 *           holds len values in device memory in the order of the triplets the handle was created from; the handle's values
 *           become exactly -- bit for bit -- what create_?csr_from_coo_device on (the same rows, the same columns, val, the same
 *           mode) would hold.  `keep`: entry q gets the value of the triplet it came from.  `sum`: per run the left-to-right chain
 *           ((v0 + v1) + v2) + ... in triplet order, in the value type, complex values component by component, by the very device
 *           function the creation adds with; a run that sums to zero stays an entry; no float atomics.  Nothing is sorted again:
 *           one kernel reads the map and val and writes the values.
 *           The values go where ?update_values_device puts them: into the resident copy when the handle's CSR is resident, which
 *           stays resident (the next product uploads nothing), and into the host view; everything derived from the values is
 *           dropped and rebuilt on first use.  The work is ordered behind the products on the library's stream, which is
 *           synchronised before return.  `val` must be complete before the call and must not overlap the handle's own arrays
 *           (those export_csr_device returns): that is not detected.
 *           Statuses, in this order, all decided before the device is touched: invalid_pointer for a null A or val;
 *           invalid_value for a handle that holds no map (created without the flag, created any other way, or whose map was
 *           dropped); invalid_size for len other than the triplet count of the creation (in `sum` mode that is not the handle's
 *           nnz); wrong_type for another value type.  Then invalid_pointer for a val that is not device (or managed) memory in the
 *           current pointer mode.  len == 0 on a handle created from 0 triplets is valid; val must still be a non-null device
 *           allocation.
 *           The map survives ?set_value, ?update_values, ?update_values_device, aoclsparse_optimize and
 *           aoclsparse_mi355_invalidate (none changes the structure, and the next refresh overwrites every value).
 *           aoclsparse_order_mat drops it: it reorders the arrays the map points into.  aoclsparse_copy, mm_state_export / adopt
 *           and the replicas of the multi-device calls do not carry it: their handles hold no map.
 *   get_coo_map_info   Whether a handle holds a map, and how large.  The caller sets info->struct_size to sizeof(*info); the
 *           library writes no more than that many bytes (a caller compiled against a shorter struct stays intact) and leaves
 *           struct_size as it is.  kept = 1 with the creation's mode (0 / 1), its triplet count, the handle's entries and the
 *           bytes of device memory the map occupies; kept = 0 and zeros for every handle without one, which is no error.
 *           invalid_pointer for a null A or info, invalid_size for a struct_size that does not hold struct_size itself.
 *
 *   order_mat_device   (round 23) aoclsparse_order_mat on the device: every row of the handle's CSR into ascending column order,
 *           entries with equal columns keeping their relative order (the host call's std::stable_sort).  One entry point for all four
 *           value types: values are moved as items of 4, 8 or 16 bytes and never computed with.  The handle ends up exactly as
 *           aoclsparse_order_mat leaves it, bit for bit -- row_ptr, base, nnz and every value's bits untouched; sort class and
 *           full-diagonal flag decided again over the sorted arrays (on the device, mat_check's answer); a kept triplet map
 *           dropped; everything derived from the arrays (clean copy, SELL-64 and blocked-ELL copies, kept transpose, TRSV plans,
 *           derived operators, replicas) dropped and rebuilt on first use -- with two differences: the work is done in HBM, and the
 *           handle is RESIDENT afterwards (spmv_info.device_resident is 1 on return, the next product uploads nothing).  The
 *           sorted columns and values also go into the host view by one copy back; for a host-created handle those are the
 *           caller's own col_idx and val arrays, sorted in place as by the host call.  A mirror that is not resident or not valid
 *           is uploaded from the host view first, so the call works on every CSR-format handle: host-created, device-created,
 *           triplet-created, a result of sp2m / syrk / sypr, an adopted one.
 *           The sort is segmented (a row is a segment) with key (column, position in the row); rows that are ascending already
 *           are found by one pass over col_idx and not touched -- on a fully sorted handle that pass is all the sort costs, and
 *           nothing is copied back.  Rows of up to AOCLSPARSE_MI355_ORDER_SHORT_MAX entries are sorted by one lane each, rows of
 *           up to AOCLSPARSE_MI355_ORDER_LDS_MAX entries by a workgroup in LDS (bitonic network over 64-bit keys), the entries of
 *           longer rows go, compacted, through the radix passes of the triplet sort: a row may hold any share of the entries.  No
 *           float atomics: the result is a pure function of the input.
 *           Statuses, in aoclsparse_order_mat's order, all decided before the device is touched: invalid_pointer for a null A;
 *           invalid_value for a negative m, n or nnz; not_implemented for a handle whose format is not CSR (COO, TCSR, BSR);
 *           success at once, nothing touched, for m == 0, n == 0 or nnz == 0; invalid_pointer for a handle without CSR arrays;
 *           and in addition not_implemented for a handle created from CSC arrays (the host call sorts the caller's host CSC
 *           arrays there).
 *           The work is ordered behind the products on the library's stream, which is synchronised before return.  Pointers
 *           that export_csr_device returned earlier become invalid (the arrays behind them are rewritten in place).
 *           Failure (allocation, HIP): the mirror is sorted in place and the host view is committed only by the copy back, after
 *           all device work has succeeded.  Before the mirror is touched the handle is unchanged; after that, a failure leaves
 *           the host view as it was, the mirror invalid (the next product uploads the host view again) and derived state dropped.
 *           A failure of the copy back itself is reported as internal_error: the two host arrays may then hold rows of both
 *           orders, so the sort class and the full-diagonal flag stay those of the unsorted arrays, and the mirror, which is
 *           sorted in every row, stays the handle's resident CSR (no product uploads that host view).  Destroy such a handle.
 *           Peak extra device memory: 8 bytes per row (the row's key and its place in the bins), and for the entries of rows
 *           longer than AOCLSPARSE_MI355_ORDER_LDS_MAX only: 24 + sizeof(value) bytes per entry (two 4-byte keys, the sort's two
 *           (key, position) pairs, the sorted value) plus 2 KiB per 4,096 of them for the digit counts.  Nothing per entry
 *           otherwise.  The temporaries are staging slots: aoclsparse_mi355_release_staging frees them.
 *
 *   clean_csr_device   (round 24) The clean CSR aoclsparse_optimize, every ?trsv / ?trsm, symgs, the ILU smoother and the iterative
 *           solvers build on first use (csr_optimize), built in HBM.  Afterwards the handle holds exactly what csr_optimize would
 *           have given it, bit for bit -- the clean arrays with idiag / iurow, the full-diagonal flag of the ORIGINAL arrays (the
 *           non-unit solves refuse on it), `optimized` -- so every later caller finds the clean CSR present and does nothing;
 *           aoclsparse_export_?csr and aoclsparse_mi355_export_diag show it.  No plan option chooses this route: it is taken through
 *           this call only.  One entry point for all four value types: values are moved as items of 4, 8 or 16 bytes and never
 *           computed with.  The three cases are csr_optimize's, decided by the check kernels over the handle's mirror:
 *           (1) rows in L | D | U group order (sort class 1 or 2) and a full diagonal: no copy, the clean CSR is the handle's own
 *           arrays; only idiag / iurow are computed, in the matrix's base (idiag[i] = the first position of row i whose column is
 *           >= i, or the row end; iurow[i] = idiag[i] + 1 when that entry is the diagonal), and come back as 2 x 4 bytes per row;
 *           export_diag reports is_internal = 0.  (2) group order, a diagonal entry missing: a 0-based copy with every row's entries
 *           in their GIVEN order (a class-2 row is not sorted, as on the host) and, in every row i < min(m, n) without a diagonal
 *           entry, an explicit zero -- the all-zero bit pattern -- in front of the row's first entry whose column is >= i, at the
 *           row's end when there is none.  (3) any other order: every row first into ascending column order, stably
 *           (order_mat_device's sort, run on a device copy of the columns and values, never on the mirror), then as (2).  In (2)
 *           and (3) idiag / iurow are those of the copy, 0-based, and is_internal = 1.  m == 0 and nnz == 0 behave as on the host:
 *           a matrix of empty rows with n > 0 gets its diagonal of zeros.
 *           The mirror is uploaded from the host view first when it is not resident or not valid, stays valid and untouched, and
 *           the handle is resident on return; the caller's host arrays are not written; a kept triplet map, SELL-64 copies, the
 *           transpose and the plans stay.  The diagonal's values (what the TRSV launchers read: m items, zero where a row has no
 *           diagonal entry or got an inserted one) are written on the device in the same pass and stay there.
 *           Rows of up to AOCLSPARSE_MI355_CLEAN_ROW_WAVE entries are searched by one lane each, longer ones by their wavefront;
 *           the copy is balanced over entries, not rows: one row may hold every entry.  No atomics, no workgroup waits for another.
 *           Statuses, in csr_optimize's order, all decided before the device is touched: invalid_pointer for a null A; success at
 *           once, nothing touched, when the handle has its clean CSR already; not_implemented for TCSR and BSR handles;
 *           invalid_pointer for a handle without CSR arrays (COO).  After those a failure of the runtime's initialisation is
 *           returned as it is (a machine without a GPU), then what mat_check answers for arrays it refuses.  invalid_size when
 *           nnz + the inserted entries exceed 2^31 - 1 (the host route overflows there); the handle is unchanged.
 *           Failure (allocation, HIP): everything is built in fresh buffers and committed only after the one copy back has
 *           synchronised successfully; on any failure the handle is as it was before the call, except that its mirror may have
 *           gone from "not uploaded" to "uploaded".  The library's stream is synchronised before return.
 *           Peak extra device memory: 20 bytes + sizeof(value) per row (three 4-byte temporaries in staging slots, idiag, iurow,
 *           the diagonal's value, of which only the last stays) plus 8 bytes per 1,024 rows for the scan; in cases (2) and (3)
 *           4 bytes per row + (4 + sizeof(value)) per entry of the copy, released after the copy back (nothing consumes a resident
 *           clean copy yet); in case (3) also (4 + sizeof(value)) per entry for the sorted copy, and what order_mat_device needs.
 *
 *   keep_value_maps    (round 25) Sets (on != 0) or clears a flag on a CSR-format handle, at any time.  While it is set, what is
 *           built records where its values come from: every TRSV layout (the level-ordered rows and the blocked layout of each of
 *           the six (fill, op) plans) one int per entry, its position in the clean CSR's value array; the diagonal the solves
 *           read one int per row; and the clean COPY that clean_csr_device makes one int per entry, its position in the handle's
 *           own value array (-1 for an inserted zero; for unsorted rows the position goes through the row sort, which is run a
 *           second time over the positions as its 4-byte items).  What was built before the flag was set has no map; the clean
 *           copy csr_optimize builds on the host never has one.  on == 0 releases every map and clears the flag.  The maps hold
 *           no values, but they index a layout: whatever invalidates a plan or the clean copy (?set_value, ?update_values,
 *           ?update_values_device, ?refresh_values_from_coo_device, aoclsparse_order_mat, order_mat_device,
 *           aoclsparse_mi355_invalidate) releases its maps.  Without the flag nothing is recorded and every path allocates and
 *           computes what it did before.  invalid_pointer for a null A, not_implemented for TCSR and BSR handles.
 *
 *   ?revalue_device    (round 25) ?update_values_device -- same arguments, same statuses in the same order, all decided before the
 *           device is touched; it writes what that call writes (the resident mirror's values while the mirror is valid, the host
 *           view by one copy back) and drops what that call drops (SELL-64 / blocked-ELL copies, host and device transposes,
 *           derived operators, replicas) -- except for what can follow the new values through a map: (1) the clean CSR stays
 *           when it is the handle's own arrays (sorted rows, full diagonal: nothing to do) or a copy that holds its map: the copy's
 *           values are gathered in HBM (revalue_kernels.hip; the all-zero item for an inserted diagonal entry) and copied back
 *           into the host copy; its row pointer, columns, idiag / iurow and the `optimized` state are untouched.  A clean copy
 *           without a map is dropped.  (2) The diagonal in HBM stays and is gathered again when it has its map (and the clean CSR
 *           stayed).  (3) Every valid TRSV plan whose layouts all hold maps stays valid -- levels, segments, block and chunk plans
 *           and every index buffer untouched -- and its value arrays are gathered again from the clean values, conjugated for a
 *           plan built with op = H; the chunk plan holds no values of its own.  A plan survives only if the clean CSR and the
 *           diagonal it was built from survive; a plan without maps is invalidated as ?update_values_device invalidates it.
 *           The gathers move items of 4, 8 or 16 bytes and never compute with them (the conjugate flips one sign bit): a solve
 *           afterwards gives the bits a freshly created handle with the new values gives.  All device work goes on the library's
 *           stream, behind earlier solves, with no host synchronisation between the gathers; the stream is synchronised once
 *           before return.  Locking as ?update_values_device.  Failure: an allocation that fails before the first write leaves
 *           the handle as it was; after any failure behind the first device write the handle is left with everything dropped and
 *           all maps released (never plans with some old and some new values) and an invalid mirror (the next product uploads the
 *           host view), and the status is reported.  Peak extra device memory: sizeof(value) per entry of a clean copy, during
 *           the call.  Not kept (rebuilt lazily as ever): blocked-ELL copies, the SELL-64 copies of op(A), derived operators
 *           without a source map (see build_operator_device), transposes, replicas.  (4, round 28) With the keep_value_maps flag set, the STRUCTURE
 *           of the handle's own SELL-64 copy stays -- slice widths, shared column lists, columns, row lengths, the records
 *           before their device flags -- when the copy was valid (or already kept) and the mirror it was built from followed the
 *           commit.  The call itself launches and waits for nothing more: the copy is marked stale, no product runs it, and the
 *           next product, aoclsparse_optimize or hinted complex product runs the VALUES stage alone (a value-only fill kernel that
 *           reads row_ptr and the new values -- no map is needed: cell p of row i is entry row_ptr[i] + p --, the table pass, the
 *           records kernel on a spare set of records and lists, and a compare kernel; when the new records and lists equal the
 *           current ones and the cell encoding is the same, the periodic range and the stacking facts are carried over and no
 *           host search runs).  The copy is then what a fresh handle over the new values holds, bit for bit.  A different
 *           aoclsparse_mi355_option_sell at that time means a full build; a failure in the values stage releases the structure
 *           and leaves the product on CSR-Adaptive.  Every other value change drops the structure with the copy.
 *           The ILU(0) factor is neither dropped nor recomputed: it stays the factor of the values it was made from until
 *           ?ilu0_refactor_device is called.  ?update_values, ?set_value, ?update_values_device and
 *           ?refresh_values_from_coo_device do not take this route; a caller with a triplet map refreshes, exports the device
 *           values, and passes them here.
 *
 *   get_value_map_info What a handle holds of the above (struct_size as for get_coo_map_info).  plan_builds and clean_builds count
 *           the times a TRSV plan / the clean CSR was actually built or extended since the handle was created, flag or no flag:
 *           they show whether a solve after a value change analysed anything.
 *
 *   build_operator_device  (round 30) A product with a symmetric, Hermitian or triangular descriptor (?mv, ?csrmm, the complex
 *           products, the iterative solvers) runs on a derived operator: the strict triangle, D' (D, I or nothing for non_unit /
 *           unit / zero) and, for symmetric and Hermitian, the mirrored triangle (conjugated for Hermitian) -- or, for triangular
 *           with op = T / H, the transpose of triangle + D' -- as a general CSR with its own device copy, row-block plan and
 *           SELL-64 copy, keyed by (type, fill, diag, transposed): H folds to T where the products fold it, symmetric and
 *           Hermitian ignore the operation.  At first use a product builds it by a serial host loop and uploads it.  This call
 *           builds the operator of (descr, op) in HBM instead (derived_kernels.hip) and registers it on the handle: every later
 *           product with a matching descriptor finds it, and none knows where it was built.  An operator that exists already,
 *           however it was built, makes the call succeed and do nothing.  The clean CSR is made first as a product makes it
 *           (csr_optimize), or is clean_csr_device's copy when there is one; it reaches the device through the resident mirror
 *           (uploaded when absent) when it is the handle's own arrays, through buffers of the call when it is a copy; idiag /
 *           iurow are uploaded.  The result is bit for bit the host loop's: every row in ascending column order, mirrored entries
 *           of a row in ascending source position, the unit diagonal stored as ones.  The host view comes by one copy back; the
 *           row-block plan and the SELL-64 copy are built as a product builds them.  A product never takes this route by itself.
 *           Statuses, all decided before the device is touched, in this order: invalid_pointer for a null A or descr;
 *           invalid_value for a base that is not the handle's or an invalid type or operation; not_implemented for a general
 *           descriptor; not_implemented for handles that are no plain CSR (COO- or CSC-created, TCSR, BSR: ?revalue_device's set);
 *           not_implemented for a Hermitian descriptor on a real value type; invalid_size for symmetric or Hermitian with
 *           m != n.  An empty matrix (m, n or nnz zero) succeeds and builds nothing.  Declined: not_implemented, nothing
 *           registered, when a row of the result would get more than 2,048 mirrored entries (the device segment sort's cap; the
 *           verdict comes from the counters, before the operator's arrays are allocated): the next product builds on the host as
 *           ever.  Failed: the allocation or HIP status, the stream drained, the error cleared.  Either way the handle is as it
 *           was (a mirror upload aside).  Locking: the runtime's stage lock, then the handle's guard.  Peak extra device memory,
 *           during the call: 16 bytes per row of the result and 8 per row of the clean CSR, and for a clean copy its three
 *           arrays; the operator keeps 8 + sizeof(value) bytes per entry, 4 of them the source map below.
 *           With keep_value_maps set at build time the operator keeps its source map, 4 bytes per entry: the clean position the
 *           value comes from, one bit for the conjugate, one word for a constant (the unit diagonal's ones).  ?revalue_device
 *           then brings the new values to every mapped operator -- exactly when the clean CSR itself follows -- by one gather from
 *           the clean values into the operator's device values in place (revalue_kernels.hip; constants are left alone), next to
 *           the TRSV plans' gathers, and one copy back into the host view; row pointer, columns, row-block plan and map stay.
 *           The operator's SELL-64 copy keeps its structure as the handle's own does (stale; the next product runs the values
 *           stage alone), its blocked-ELL copy is rebuilt lazily.  Operators without a map are dropped as before; so is every
 *           operator, with the maps, on any failure behind the first write, when the clean CSR does not follow (a clean copy
 *           built on the host has no map), and on ?update_values_device, ?set_value and ?update_values: never a mix of old and
 *           new values.  The map is released by keep_value_maps(A, 0) (the operator stays and no longer follows) and, with the
 *           operator, by aoclsparse_order_mat, order_mat_device, aoclsparse_mi355_invalidate and destroy; nothing is carried
 *           through aoclsparse_copy, exported state or replicas.  get_value_map_info does not count these maps.
 *
 *   get_operator_info  What the handle holds for the key of (descr, op) -- present, built_on_device, mapped, rows, cols, nnz,
 *           sell_copy, sell_value_fills (refills of its kept SELL-64 structure), map_bytes -- and the handle's counters, which
 *           survive a drop: device_builds, host_builds, followed (operators the last successful ?revalue_device carried),
 *           dropped_by_value_change.  struct_size as for get_coo_map_info; works without a device.  invalid_pointer for a null
 *           argument, invalid_value as above.
 *
 *   export_operator    The host view of an existing operator, on whichever route it was built: 0-based arrays, valid until the
 *           operator is dropped; invalid_value when the handle holds none for the key.  Works without a device.
 *
 *   ?ilu0_refactor_device  (round 26) The ILU(0) factor of A again, from the values the handle holds NOW: the resident mirror
 *           while it is valid, otherwise the host view, uploaded as every product uploads it.  In the reference and here the
 *           smoother factorises once per handle, from the values it saw first, and a value update leaves that factor in force
 *           (it still does); after this call aoclsparse_?ilu_smoother and the iterative solvers with "ILU0" use the new one.
 *           precond_csr_val may be null; otherwise it receives what the smoother hands out, the factor's nnz values on A's
 *           pattern in library-owned host memory.  That array keeps its address once it exists: a pointer handed out earlier
 *           shows the new factor.  The call may also be the handle's first factorisation.
 *           What the factorisation computes from the pattern alone -- the rows in level order (resident in HBM), the level
 *           pointer, the longest row, the choice between one launch per level and the sync-free launch, and the choice of option
 *           ilu_search -- is the handle's ILU schedule: built by the first factorisation on either route, reused by every later
 *           one, untouched by value updates, released by aoclsparse_order_mat, order_mat_device, aoclsparse_mi355_invalidate
 *           and destroy.  A refactorisation therefore runs no host loop over the rows and uploads nothing but, behind an invalid
 *           mirror, the values: the factorisation runs in a fresh device buffer seeded by a device-to-device copy of the mirror's
 *           values.  On success the factor handle (a CSR handle over A's pattern and the factor values, whose TRSV plans are the
 *           smoother's solves) is brought up to date by ?revalue_device's own code: its host view -- the array above -- by one
 *           copy back, its mirror, its diagonal, and its TRSV plans through their value maps.  A factor handle created while A's
 *           keep_value_maps flag is set has the flag too; without maps its plans are invalidated as ?update_values_device
 *           invalidates plans, and the next solve builds them again.  A factor handle that does not exist yet is created as the
 *           smoother creates it; one from before the schedule was released is made anew.
 *           Statuses, in the smoother's order, all decided before the device is touched: invalid_pointer for a null A or a
 *           handle without CSR arrays (COO); not_implemented for TCSR and BSR handles; unsorted_input for a sort class other than
 *           1 or 2; numerical_error without a full diagonal; wrong_type; invalid_size for a matrix that is not square; success at
 *           once for m == 0.  After those a failure of the runtime's initialisation is returned as it is, and not_implemented
 *           for a row that does not fit LDS.  A zero or near-zero pivot, or a row whose diagonal does not follow its lower part,
 *           returns numerical_error and leaves the handle exactly as it was: the previous factor, its handle and its plans stay
 *           in use.  A failure behind the first write into the factor handle (allocation, HIP) leaves A unfactorised -- the
 *           factor handle destroyed, the value array a copy of the current values, as ilu_prepare makes it -- never a mix of
 *           old and new; the status is reported and the next smoother call factorises from scratch.
 *           The library's stream is synchronised before return.  Peak extra device memory: sizeof(value) per entry + 4 bytes per
 *           row during the call; the schedule keeps 4 bytes per row.
 *
 *   get_ilu_info       What a handle holds of the above (struct_size as for get_coo_map_info).
 *
 *   sp2m_numeric_device  (round 29) The values of C = op(A) * op(B) again, from the values A and B hold NOW, on the structure C
 *           already has; one entry point for the four value types, as aoclsparse_sp2m.  C is a CSR handle whose structure is the
 *           product's as aoclsparse_sp2m builds it -- every row's columns in first-touch order, one slot per column: the result
 *           handle of an earlier aoclsparse_sp2m / ?csr2m of these operands, or a handle created (in either base) over arrays
 *           that hold such a product.  Its mirror is uploaded when absent, as every product does.  After the call C's values are
 *           bit for bit what aoclsparse_sp2m(stage_finalize) would have written: first product stored, later ones added with the
 *           contracted multiply-add, in the reference's walk order.  C's row_ptr and col_ind, on the host and in HBM, are not
 *           written.  The operands reach the device as in aoclsparse_sp2m: the resident mirrors where they are valid, one
 *           transposed operand through the handle's kept transpose, conjugation applied at load.
 *           Statuses, all decided before the device is touched, in this order: everything aoclsparse_sp2m returns for
 *           stage_finalize before it looks at C (the quick return of an empty product succeeds and does nothing); invalid_pointer
 *           for a null C; not_implemented when both operations transpose (C = D^T would need a map); not_implemented for a C
 *           that is no plain CSR handle (COO- or CSC-created, TCSR, BSR); wrong_type when C's value type is not the operands';
 *           invalid_size when C's dimensions are not the product's; invalid_value when C is A or B.
 *           The new values are computed into a fresh device buffer, and the kernel (spgemm_numeric_kernels.hip) proves row by
 *           row that C's structure is the product's: it raises one verdict word when a product's column is not in C's row, a
 *           slot of C's row receives no product, C's row holds a column twice, or the k-th distinct column the walk meets does
 *           not sit in slot k.  The word is read back before anything of C is written: a refused call returns invalid_value and
 *           leaves C, everything derived from it and the plan exactly as they were.  No generation counter on A or B is needed.
 *           On a good verdict the buffer goes to C by ?revalue_device's own code: one copy of the values to the host view, the
 *           mirror updated device to device, and for a C with keep_value_maps set the clean CSR, the diagonal, the mapped TRSV
 *           plans and the SELL-64 structure kept; failure semantics as documented there.  Limitation: a product's rows are in
 *           first-touch order, so C's clean CSR is a copy, and only the copy aoclsparse_mi355_clean_csr_device builds holds the
 *           value map that carries it and the TRSV plans through the commit; with the copy a solve builds on the host they are
 *           dropped and analysed again by the next solve, as after any ?revalue_device.
 *           What the call computes from C's ROW POINTER alone -- the rows binned by their exact length (at most 32 / 256 / 2,048
 *           entries: tables in LDS; longer: the global slab), the row order bin by bin and the slab's row records in HBM, the
 *           bin bounds, the batch list and the slab's sizes -- is the handle's sp2m plan: built by the first numeric call in
 *           buffers of its own, kept only when that call succeeded, reused by every later call with any operands whose product
 *           has C's structure, untouched by value changes of C, released by aoclsparse_order_mat, order_mat_device,
 *           aoclsparse_mi355_invalidate (which aoclsparse_sp2m(stage_finalize) into C calls) and destroy; not carried through
 *           aoclsparse_copy, exported state or replicas.  No upper-bound kernel, histogram or row sort runs with a kept plan: such
 *           a call waits for the device twice, for the verdict and inside the commit.  Locking: the runtime's stage lock, then
 *           the handles' guards one at a time.  Peak extra device memory: sizeof(value) per entry of C, and for rows of the slab
 *           8 bytes per table slot and 1 per entry, during the call; the plan keeps 4 bytes per row.
 *           Out of scope: both operands transposed; aoclsparse_syrk / sypr on a kept structure; a numeric ?add; keeping an
 *           operand's transpose through its own revalue; a C without a host view; aoclsparse_sp2m(stage_finalize) taking this
 *           route by itself.
 *
 *   get_sp2m_plan_info What a handle holds of the above (struct_size as for get_coo_map_info); works without a device.
 *
 * Out of scope: aliasing the caller's device arrays without a copy; handles without a host view; 64-bit indices; creating CSC,
 * TCSR or BSR handles from device arrays; a transposing variant of create_?csr_from_coo_device (the caller swaps the two index
 * arrays); a refresh that changes the set of coordinates; carrying the triplet map through aoclsparse_copy, exported state or
 * replicas; a host-pointer twin of ?refresh_values_from_coo_device; sorting
 * the long columns of ?csr2csc and of the handles' transposes with the triplet sort (transpose_kernels.hip declines them still);
 * aoclsparse_order_mat itself taking the device route; adding repeated columns while ordering; ordering CSC-created, TCSR or BSR
 * handles on the device; csr_optimize / aoclsparse_optimize choosing the device route for the clean copy by themselves; keeping the
 * clean copy resident and building TRSV plans or ILU factors from it on the device; ensure_derived / aoclsparse_optimize choosing
 * build_operator_device's route by themselves, mirrored row segments beyond the segment sort's cap, source maps for operators built
 * on the host, carrying operators or their maps through aoclsparse_copy, exported state or replicas; value maps for clean copies
 * built on the host, and keeping blocked-ELL copies, the SELL-64 copies of op(A),
 * transposes or replicas through a ?revalue_device; keeping the SELL-64 structure through any other value change, carrying it
 * through aoclsparse_copy, exported state or replicas, and searching the periodic range on the device; computing the ILU(0) levels on the device; refactorising inside an update call by itself; a device-only ILU
 * factor without its host array; carrying the ILU schedule through aoclsparse_copy, exported state or replicas; carrying value maps through aoclsparse_copy, exported state or replicas; clean copies of the transpose; a host view that is filled on first use instead of by
 * order_mat_device's copy back. */
#define AOCLSPARSE_MI355_COO_SORT_TILE 4096 /* entries a workgroup of the triplet sort takes per pass */
#define AOCLSPARSE_MI355_ORDER_SHORT_MAX 32 /* order_mat_device: rows of up to this many entries are sorted by one lane */
#define AOCLSPARSE_MI355_ORDER_LDS_MAX 2048 /* ... of up to this many by a workgroup in LDS; longer ones by the radix sort */
#define AOCLSPARSE_MI355_CLEAN_ROW_WAVE 64 /* clean_csr_device: rows of up to this many entries are searched by one lane */
typedef enum
{
    aoclsparse_mi355_coo_keep = 0, /* repeated coordinates stay separate entries, in triplet order */
    aoclsparse_mi355_coo_sum  = 1, /* repeated coordinates are added, left to right in triplet order */
    aoclsparse_mi355_coo_keep_map = 16 /* flag, ORed to either: the handle keeps the sort's map for ?refresh_values_from_coo_device */
} aoclsparse_mi355_coo_duplicates;
typedef struct
{
    size_t         struct_size; /* in: sizeof(aoclsparse_mi355_coo_map_info) as the caller knows it */
    aoclsparse_int kept; /* 1: the handle holds a map; 0: none, and everything below is 0 */
    aoclsparse_int mode; /* aoclsparse_mi355_coo_keep or aoclsparse_mi355_coo_sum */
    aoclsparse_int triplets; /* the len ?refresh_values_from_coo_device expects */
    aoclsparse_int entries; /* the handle's nnz */
    long long      map_bytes; /* device memory allocated for the map */
} aoclsparse_mi355_coo_map_info;
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_create_scsr_device(aoclsparse_matrix *mat, aoclsparse_index_base base, aoclsparse_int M,
                                                                 aoclsparse_int N, aoclsparse_int nnz, const aoclsparse_int *row_ptr,
                                                                 const aoclsparse_int *col_idx, const float *val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_create_dcsr_device(aoclsparse_matrix *mat, aoclsparse_index_base base, aoclsparse_int M,
                                                                 aoclsparse_int N, aoclsparse_int nnz, const aoclsparse_int *row_ptr,
                                                                 const aoclsparse_int *col_idx, const double *val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_create_ccsr_device(aoclsparse_matrix *mat, aoclsparse_index_base base, aoclsparse_int M,
                                                                 aoclsparse_int N, aoclsparse_int nnz, const aoclsparse_int *row_ptr,
                                                                 const aoclsparse_int *col_idx, const aoclsparse_float_complex *val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_create_zcsr_device(aoclsparse_matrix *mat, aoclsparse_index_base base, aoclsparse_int M,
                                                                 aoclsparse_int N, aoclsparse_int nnz, const aoclsparse_int *row_ptr,
                                                                 const aoclsparse_int *col_idx, const aoclsparse_double_complex *val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_create_scsr_from_coo_device(aoclsparse_matrix *mat, aoclsparse_index_base base,
                                                                          aoclsparse_int M, aoclsparse_int N, aoclsparse_int nnz,
                                                                          const aoclsparse_int *row_ind, const aoclsparse_int *col_ind,
                                                                          const float *val, aoclsparse_int duplicates);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_create_dcsr_from_coo_device(aoclsparse_matrix *mat, aoclsparse_index_base base,
                                                                          aoclsparse_int M, aoclsparse_int N, aoclsparse_int nnz,
                                                                          const aoclsparse_int *row_ind, const aoclsparse_int *col_ind,
                                                                          const double *val, aoclsparse_int duplicates);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_create_ccsr_from_coo_device(aoclsparse_matrix *mat, aoclsparse_index_base base,
                                                                          aoclsparse_int M, aoclsparse_int N, aoclsparse_int nnz,
                                                                          const aoclsparse_int *row_ind, const aoclsparse_int *col_ind,
                                                                          const aoclsparse_float_complex *val,
                                                                          aoclsparse_int duplicates);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_create_zcsr_from_coo_device(aoclsparse_matrix *mat, aoclsparse_index_base base,
                                                                          aoclsparse_int M, aoclsparse_int N, aoclsparse_int nnz,
                                                                          const aoclsparse_int *row_ind, const aoclsparse_int *col_ind,
                                                                          const aoclsparse_double_complex *val,
                                                                          aoclsparse_int duplicates);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_supdate_values_device(aoclsparse_matrix A, aoclsparse_int len, const float *val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_dupdate_values_device(aoclsparse_matrix A, aoclsparse_int len, const double *val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_cupdate_values_device(aoclsparse_matrix A, aoclsparse_int len,
                                                                    const aoclsparse_float_complex *val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_zupdate_values_device(aoclsparse_matrix A, aoclsparse_int len,
                                                                    const aoclsparse_double_complex *val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_srefresh_values_from_coo_device(aoclsparse_matrix A, aoclsparse_int len, const float *val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_drefresh_values_from_coo_device(aoclsparse_matrix A, aoclsparse_int len, const double *val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_crefresh_values_from_coo_device(aoclsparse_matrix A, aoclsparse_int len,
                                                                              const aoclsparse_float_complex *val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_zrefresh_values_from_coo_device(aoclsparse_matrix A, aoclsparse_int len,
                                                                              const aoclsparse_double_complex *val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_get_coo_map_info(aoclsparse_matrix A, aoclsparse_mi355_coo_map_info *info);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_order_mat_device(aoclsparse_matrix A);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_clean_csr_device(aoclsparse_matrix A);
typedef struct
{
    size_t         struct_size; /* in: sizeof(aoclsparse_mi355_value_map_info) as the caller knows it */
    aoclsparse_int enabled; /* the keep_value_maps flag */
    aoclsparse_int clean_map; /* 1: the clean CSR can follow a ?revalue_device (the handle's own arrays, or a copy with its map) */
    aoclsparse_int plans_mapped; /* the valid TRSV plans, of the six, whose layouts all hold maps */
    aoclsparse_int last_kept_plans; /* plans the last successful ?revalue_device carried over */
    long long      plan_builds; /* times a TRSV plan was built or extended since the handle was created (flag or no flag) */
    long long      clean_builds; /* the same for the clean CSR (csr_optimize / clean_csr_device doing work) */
    long long      revalues; /* successful ?revalue_device calls */
    long long      map_bytes; /* device memory the maps occupy */
} aoclsparse_mi355_value_map_info;
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_keep_value_maps(aoclsparse_matrix A, aoclsparse_int on);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_srevalue_device(aoclsparse_matrix A, aoclsparse_int len, const float *val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_drevalue_device(aoclsparse_matrix A, aoclsparse_int len, const double *val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_crevalue_device(aoclsparse_matrix A, aoclsparse_int len,
                                                              const aoclsparse_float_complex *val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_zrevalue_device(aoclsparse_matrix A, aoclsparse_int len,
                                                              const aoclsparse_double_complex *val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_get_value_map_info(aoclsparse_matrix A, aoclsparse_mi355_value_map_info *info);
typedef struct
{
    size_t         struct_size; /* in: sizeof(aoclsparse_mi355_operator_info) as the caller knows it */
    aoclsparse_int present; /* 1: the handle holds the operator of this (type, fill, diag, op) */
    aoclsparse_int built_on_device; /* 1: build_operator_device built it; 0: a product built it on the host */
    aoclsparse_int mapped; /* 1: it holds its source map and follows a ?revalue_device */
    aoclsparse_int rows, cols, nnz; /* of the operator (0 without one) */
    aoclsparse_int followed; /* handle: operators the last successful ?revalue_device carried over */
    aoclsparse_int sell_copy; /* 1: it holds a SELL-64 copy, valid or kept stale for the next product to refill */
    long long      sell_value_fills; /* times the values stage refilled this operator's kept SELL-64 structure */
    long long      map_bytes; /* device memory this operator's source map occupies */
    long long      device_builds; /* handle, since creation: operators built in HBM */
    long long      host_builds; /* handle, since creation: operators built on the host */
    long long      dropped_by_value_change; /* handle, since creation: operators a value change dropped */
} aoclsparse_mi355_operator_info;
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_build_operator_device(aoclsparse_matrix A, const aoclsparse_mat_descr descr,
                                                                    aoclsparse_operation op);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_get_operator_info(aoclsparse_matrix A, const aoclsparse_mat_descr descr,
                                                                aoclsparse_operation op, aoclsparse_mi355_operator_info *info);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_export_operator(aoclsparse_matrix A, const aoclsparse_mat_descr descr,
                                                              aoclsparse_operation op, aoclsparse_int *rows, aoclsparse_int *cols,
                                                              aoclsparse_int *nnz, const aoclsparse_int **row_ptr,
                                                              const aoclsparse_int **col_ind, const void **val);
typedef struct
{
    size_t         struct_size; /* in: sizeof(aoclsparse_mi355_ilu_info) as the caller knows it */
    aoclsparse_int factorized; /* 1: the handle holds an ILU(0) factor (the smoother's first call or a refactorisation made it) */
    aoclsparse_int levels; /* the kept schedule: dependency levels of the strictly lower pattern; 0 (as the next four) without one */
    aoclsparse_int max_row; /* ... entries of the longest row */
    aoclsparse_int syncfree; /* ... 1: one sync-free launch over all rows; 0: one launch per level */
    aoclsparse_int search; /* ... 1: the updated position is found by binary search; 0: by a scan (option ilu_search) */
    aoclsparse_int plans_kept_last; /* TRSV plans of the factor handle the last ?ilu0_refactor_device carried over */
    long long      analyses; /* times the levels were computed since the handle was created */
    long long      factorizations; /* successful factorisations, the smoother's first call included */
    long long      schedule_bytes; /* memory the schedule occupies: the level order in HBM, the level pointer on the host */
    long long      factor_plan_builds; /* plan_builds (get_value_map_info) of the factor handle: did a solve analyse anything? */
} aoclsparse_mi355_ilu_info;
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_silu0_refactor_device(aoclsparse_matrix A, float **precond_csr_val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_dilu0_refactor_device(aoclsparse_matrix A, double **precond_csr_val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_cilu0_refactor_device(aoclsparse_matrix A, aoclsparse_float_complex **precond_csr_val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_zilu0_refactor_device(aoclsparse_matrix A, aoclsparse_double_complex **precond_csr_val);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_get_ilu_info(aoclsparse_matrix A, aoclsparse_mi355_ilu_info *info);
typedef struct
{
    size_t         struct_size; /* in: sizeof(aoclsparse_mi355_sp2m_plan_info) as the caller knows it */
    aoclsparse_int kept; /* 1: the handle holds the plan of aoclsparse_mi355_sp2m_numeric_device; 0 (as the next two) without one */
    aoclsparse_int heavy_rows; /* ... rows longer than 2,048 entries: their tables live in the global slab (= rows_in_bin[4]) */
    aoclsparse_int rows_in_bin[5]; /* ... rows of at most 32 / 256 / 2,048 entries, (unused: always 0), longer rows */
    long long      plan_builds; /* times the plan was built since the handle was created */
    long long      numeric_runs; /* successful numeric calls */
    long long      refused; /* numeric calls stopped by the verdict: C's structure was not the product's */
    long long      plan_bytes; /* memory the plan occupies: row order and slab records in HBM, bounds and batch list on the host */
} aoclsparse_mi355_sp2m_plan_info;
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_sp2m_numeric_device(aoclsparse_operation opA, const aoclsparse_mat_descr descrA,
                                                                  const aoclsparse_matrix A, aoclsparse_operation opB,
                                                                  const aoclsparse_mat_descr descrB, const aoclsparse_matrix B,
                                                                  aoclsparse_matrix C);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_get_sp2m_plan_info(aoclsparse_matrix C, aoclsparse_mi355_sp2m_plan_info *info);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_export_csr_device(aoclsparse_matrix A, aoclsparse_index_base *base, aoclsparse_int *M,
                                                                aoclsparse_int *N, aoclsparse_int *nnz, const aoclsparse_int **row_ptr,
                                                                const aoclsparse_int **col_idx, const void **val);

/* ---- the same over a communicator the LIBRARY owns: RCCL (librccl.so, loaded with dlopen at the first call) ---------------
 * One communicator per process, on the library's device.  Rank 0 calls comm_unique_id and hands the 128 bytes to the other
 * ranks by any means (MPI, a file, torch.distributed's store); every rank then calls comm_init -- a collective, like all calls
 * below.  Collectives are enqueued on the library's stream (aoclsparse_mi355_get_stream) and must be issued by one thread at a
 * time, in the same order on every rank.
 *   comm_broadcast_matrix  rank `root` passes its handle, every other rank passes *A == NULL and receives a new handle (to be
 *                          destroyed by the caller) holding root's device CSR and csrmm plans: ncclBroadcast of a header, then
 *                          one grouped ncclBroadcast per buffer straight into the new handle's device buffers.
 *   comm_allgather         bytes_per_rank bytes from `send` of every rank, concatenated in rank order in `recv` (column-major C
 *                          slabs of equal width: the whole C, in place when send == recv + rank * bytes_per_rank).
 *   comm_broadcast         a device buffer from `root` to everyone.
 * status not_implemented: librccl.so could not be loaded; invalid_operation: no communicator (or a second comm_init). */
typedef struct aoclsparse_mi355_comm_id_
{
    char internal[128];
} aoclsparse_mi355_comm_id;
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_comm_unique_id(aoclsparse_mi355_comm_id *id);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_comm_init(aoclsparse_int world, aoclsparse_int rank, const aoclsparse_mi355_comm_id *id);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_comm_destroy(void);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_comm_info(aoclsparse_int *world, aoclsparse_int *rank, aoclsparse_int *rccl_version);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_comm_broadcast(void *device_buffer, size_t bytes, aoclsparse_int root);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_comm_allgather(const void *send, void *recv, size_t bytes_per_rank);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_comm_broadcast_matrix(aoclsparse_matrix *A, aoclsparse_int root);

/* ---- introspection of a handle --------------------------------------------------------- */
/* idiag / iurow of the clean CSR (host arrays owned by the handle, length m, matrix base);
 * the counterpart of the reference-internal csr::idiag / csr::iurow the unit tests inspect
 * (tests/unit_tests/hint_tests.cpp:172-192).  Requires a prior optimize/trsv. */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_export_diag(const aoclsparse_matrix A,
                                                          aoclsparse_int        **idiag,
                                                          aoclsparse_int        **iurow,
                                                          aoclsparse_int         *is_internal);
/* The arrays of a BSR handle as it holds them (aoclsparse_create_?bsr: the caller's own, is_internal = 0; aoclsparse_convert_bsr:
 * owned by the handle, is_internal = 1), read-only: the counterpart of the reference-internal aoclsparse::bsr the unit tests
 * inspect (tests/unit_tests/bsr_convert_tests.cpp).  invalid_value for a handle of another format. */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_export_bsr(const aoclsparse_matrix A, aoclsparse_index_base *base,
                                                         aoclsparse_order *order, aoclsparse_int *bM, aoclsparse_int *bN,
                                                         aoclsparse_int *block_dim, aoclsparse_int **row_ptr,
                                                         aoclsparse_int **col_idx, void **val, aoclsparse_int *is_internal);
typedef struct aoclsparse_mi355_spmv_info_
{
    aoclsparse_int kernel; /* 0 none yet, 1 csr-adaptive stream, 2 merge-path (scalar order, no pinned kid; else 1), 3 SELL-64 (mv hint + optimize), 4 SELL-64 with one column list per run of rows that share it, 5 TCSR handle: four lanes per row over both triangles (double, op = none), 6 BSR handle: one lane per scalar row (column-major blocks, op = none) */
    aoclsparse_int order; /* 0 scalar chain (kid 0), 1 4-lane (kid 1/2), 2 8-lane (kid 3) */
    aoclsparse_int row_blocks; /* workgroups per launch */
    aoclsparse_int tile; /* non-zeros staged in LDS per workgroup */
    aoclsparse_int long_rows; /* rows longer than one LDS tile */
    aoclsparse_int max_row_nnz;
    aoclsparse_int device_resident; /* 1 once the CSR arrays (the BSR arrays of a BSR handle) are in HBM */
    aoclsparse_int sell_slices; /* SELL-64: 64-row slices (0 otherwise) */
    long long      stored_cells; /* SELL-64: value cells stored, padding included (kernel 4 stores fewer column cells) */
    aoclsparse_int mm_groups; /* row-major csrmm: row groups (runs of rows with one column pattern) in use, else 0 */
    aoclsparse_int mm_window_rows; /* column-major csrmm: rows per workgroup of the LDS-window kernel (banded matrices), else 0 */
    aoclsparse_int mm_bell_width; /* csrmm: 16 x 16 block slots per block row of the blocked-ELL copy (MFMA kernel), else 0 */
    aoclsparse_int mm_bell_fill_permille; /* ... and 1000 * nnz / (256 * stored blocks) */
    aoclsparse_int tree_min; /* CSR-Adaptive, scalar order, no pinned kid, spmv_strict 0: rows with at least this many entries are summed
                                by a wavefront tree (stated bound) instead of the reference's chain; 0: every row is the reference's order */
    aoclsparse_int mm_bell_xcd_chunk; /* blocked-ELL csrmm, which XCD works through which block rows: chunks of this many consecutive block
                                         rows dealt to the XCDs in turn (1 = launch order); 0: no copy, or the lattice sweep below */
    aoclsparse_int mm_bell_model_fetches_permille; /* ... 1000 * modelled fabric fetches per B block row in that order ... */
    aoclsparse_int mm_bell_model_fetches_launch_order_permille; /* ... and in launch order */
    aoclsparse_int mm_bell_lattice_line, mm_bell_lattice_lines; /* lattice sweep (block columns at offsets 1, n1, n1 n2): n1, n2; else 0 */
    aoclsparse_int mm_bell_region_a, mm_bell_region_b; /* ... the a x b block rows of the cross-section an XCD follows through the planes */
} aoclsparse_mi355_spmv_info;
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_get_spmv_info(const aoclsparse_matrix     A,
                                                            aoclsparse_operation        op,
                                                            aoclsparse_mi355_spmv_info *info);
/* entries of the value table of op(A)'s SELL-64 copy (aoclsparse_mi355_option_sell_values): 1..256 when the cells hold one-byte
 * indices into it, 0 when they hold the values (or there is no SELL-64 copy).  Derived (symmetric / triangular) operators are not
 * reported. */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_get_sell_values(const aoclsparse_matrix A, aoclsparse_operation op,
                                                              aoclsparse_int *table_entries);
/* How op(A)'s SELL-64 copy stores its table indices and its columns.  A copy with slice records (widest row <= 8 cells, >= 4096
 * slices) packs the indices of a ROW into one word where they fit: fields of index_bits = 1 / 2 / 4 / 8 bits (the smallest that
 * holds table_entries - 1), cell q of the row at bit q * index_bits, in a word of word_bytes = 1 / 2 / 4 bytes (the smallest
 * that holds widest row * index_bits <= 32 bits); row i's word at i * word_bytes.  Both are 0 when the cells hold one byte per
 * cell or the values.  uniform_slices = slices (64 full rows that share one column list, as it is or shifted by one per row) whose
 * columns the short-row kernel reads as one scalar list per slice; 0 without packed words or shared lists.  Derived operators
 * are not reported. */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_get_sell_packing(const aoclsparse_matrix A, aoclsparse_operation op,
                                                               aoclsparse_int *index_bits, aoclsparse_int *word_bytes,
                                                               aoclsparse_int *uniform_slices);
/* What the slice records of op(A)'s SELL-64 copy say beyond offsets, width and mode (copies with uniform lists and one-byte
 * words only; 0, 0 otherwise).  uniform_word_slices = full slices with one column list whose 64 rows share ONE packed word: the
 * record holds the word and the short-row kernel does not read the rows' words.  exception_slices = those among them that are
 * "one list shifted by one per row" in which at most two rows omit cells of it (the first and last slice of a stencil's grid
 * line): the record names the two rows and the cells they have, and the slice runs as a shifted one.  Both are recounted
 * whenever the copy is rebuilt (a value change).  Derived operators are not reported. */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_get_sell_records(const aoclsparse_matrix A, aoclsparse_operation op,
                                                               aoclsparse_int *uniform_word_slices,
                                                               aoclsparse_int *exception_slices);
/* The periodic range of the slice records and uniform column lists of op(A)'s SELL-64 copy (copies with uniform lists and
 * one-byte words only; all 0 otherwise, or when there is none).  The records and lists of slice s in [first_slice + period_slices,
 * end_slice) are those of slice s - period_slices with every column moved by column_stride -- a stencil's grid lines -- and the
 * short-row kernel reads the first period's records and lists for every slice of the range.  period_slices is the smallest
 * multiple of 4 (at most 4096) for which such a range holds two periods and half of the slices; first_slice and end_slice are
 * multiples of 4; column_stride = 64 * period_slices.  What is reported is what the kernel is handed: a range the kernel's 32-bit
 * arithmetic could not serve is not kept.  Found again whenever the copy is rebuilt (a value change).  Derived
 * operators are not reported. */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_get_sell_period(const aoclsparse_matrix A, aoclsparse_operation op,
                                                              aoclsparse_int *first_slice, aoclsparse_int *end_slice,
                                                              aoclsparse_int *period_slices, aoclsparse_int *column_stride);
/* The same search on the caller's host arrays (no device involved): records = nslices slice records of four 32-bit words
 * {cell_lo, col_lo, hi, wsm} (wsm: bits 0-7 width, 16-23 mode, bit 24 "one word, in cell_lo bits 0-7", bit 25 "exception lanes,
 * in cell_lo and hi bits 0-7"), lists = nslices x 8 columns (-1: unused), max_period in slices.  range = {first_slice, end_slice,
 * period_slices, column_stride}.  comparisons (may be null) receives the pairs of slices the search compared: it makes 8 x nslices
 * at most and reports no range when that does not suffice. */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_sell_find_period(aoclsparse_int nslices, const void *records,
                                                               const aoclsparse_int *lists, aoclsparse_int max_period,
                                                               aoclsparse_int range[4], long long *comparisons);
/* STACKED PERIODS of op(A)'s SELL-64 copy: what the short-row launcher will do with the periodic range.  Slices [first_slice,
 * end_slice) run stacked -- one wavefront takes `periods` consecutive periods of its strip of slices, reads the first period's
 * records once and issues all gathers before its first wait -- and alias_map says which gathers it shares between periods:
 * four bits per cell, nibble q = a(q) + 1 where cell q of a slice in period k + 1 is cell a(q) of the same slice in period k
 * (its column + column_stride), 0 = none (0x503: the 5-point stencil; 0x6040: a 7-offset stencil whose period is one line).
 * end_slice - first_slice is a whole number of `periods` periods and of workgroups; what is left of the range runs with the
 * slices outside it, in the same launch.  All 0 whenever the product runs the kernel without stacking: no range, a group of 4
 * slices of the first period that is not a run of shifted slices with their words in the records, an alias map the kernel is
 * not built for, a float plan, fewer than 60,000 slices.  Decided again whenever the copy is rebuilt (a value change). */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_get_sell_march(const aoclsparse_matrix A, aoclsparse_operation op,
                                                             aoclsparse_int *first_slice, aoclsparse_int *end_slice,
                                                             aoclsparse_int *periods, aoclsparse_int *alias_map);
/* What the handle's SELL-64 copy keeps through a value change (aoclsparse_mi355_?revalue_device with the keep_value_maps flag) and
 * what its builds have done.  struct_size as for aoclsparse_mi355_get_coo_map_info: the caller sets it to sizeof(*info) and the
 * library writes no more than that.  For op other than none and for handles without a copy (TCSR, BSR, no GPU) every field is 0 and
 * the status is success; derived operators are not reported.  invalid_pointer for a null A or info, invalid_size for a struct_size
 * that does not hold itself. */
typedef struct
{
    size_t         struct_size; /* in: sizeof(aoclsparse_mi355_sell_keep_info) as the caller knows it */
    aoclsparse_int kept; /* 1: a structure is held now (behind a valid copy, or stale after a ?revalue_device) */
    aoclsparse_int valid; /* 1: the copy can serve a product now */
    aoclsparse_int last_route; /* 0 nothing yet, 1 structure + values, 2 values with the search (or nothing to search), 3 values with the range carried over */
    aoclsparse_int reserved;
    long long      structure_builds; /* times the structure stage ran since creation, flag or no flag */
    long long      value_fills; /* times the values stage ran */
    long long      searches_skipped; /* times the values stage ran and the periodic range was carried over */
    long long      kept_bytes; /* device and host memory the kept state adds over the copy itself */
} aoclsparse_mi355_sell_keep_info;
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_get_sell_keep_info(const aoclsparse_matrix A, aoclsparse_operation op,
                                                                 aoclsparse_mi355_sell_keep_info *info);
/* The two plan rules behind aoclsparse_mi355_get_sell_march on the caller's host arrays (no device involved; records and lists as for
 * aoclsparse_mi355_sell_find_period, range = what that search reported, word_bytes = bytes per packed row word):
 * out = {1 if the range can be stacked else 0, the alias map of its first period}. */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_sell_find_march(aoclsparse_int nslices, const void *records,
                                                              const aoclsparse_int *lists, const aoclsparse_int range[4],
                                                              aoclsparse_int word_bytes, aoclsparse_int out[2]);
/* ... and the launcher's rule on them: max_width = the widest slice, stack / alias_map = the two results above, value_bytes = 4
 * or 8, slices_per_wavefront = what the launcher chose.  out = {first_slice, end_slice, periods, alias_map}, all 0: no stacking. */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_sell_march_rule(aoclsparse_int nslices, aoclsparse_int max_width,
                                                              const aoclsparse_int range[4], aoclsparse_int stack,
                                                              aoclsparse_int alias_map, aoclsparse_int value_bytes,
                                                              aoclsparse_int slices_per_wavefront, aoclsparse_int out[4]);
/* The plan behind mm_bell_xcd_chunk / the lattice sweep, computed from host arrays (no device involved; what aoclsparse_optimize runs on the
 * blocked-ELL copy's block columns): bcol = nbr x width block columns, ascending per block row, empty slots (-1) last; nbc = block columns of
 * the matrix.  forced: -2 automatic, -1 the lattice sweep whenever a lattice is found, 0 launch order, c >= 1 chunks of c block rows.
 * order (room for order_capacity entries; 8 * nbr always suffices) receives order[8 p + x] = the p-th block row of XCD x, -1 past the end of
 * its list; *order_len = list positions per XCD (0: launch order, nothing written).  info = {xcd chunk (0: lattice sweep), block rows per
 * line, lines per plane, planes, region a, region b, 1000 * modelled fetches per B block row, the same in launch order}. */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_plan_block_row_order(aoclsparse_int nbr, aoclsparse_int width, aoclsparse_int nbc,
                                                                   const aoclsparse_int *bcol, aoclsparse_int forced, aoclsparse_int *order,
                                                                   aoclsparse_int order_capacity, aoclsparse_int *order_len,
                                                                   aoclsparse_int info[8]);
/* number of dependency levels of the triangle a trsv with (fill, op) walks; -1 before analysis */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_get_trsv_levels(const aoclsparse_matrix A,
                                                              aoclsparse_fill_mode    fill,
                                                              aoclsparse_operation    op,
                                                              aoclsparse_int         *levels);
/* the TRSV plan of (fill, op) in numbers (zeros before analysis): what the automatic schedule will run and why */
typedef struct aoclsparse_mi355_trsv_info_
{
    aoclsparse_int levels; /* dependency levels of the rows */
    aoclsparse_int blocks, block_levels; /* blocks of chained rows (0: no block plan) and their dependency levels */
    aoclsparse_int chunks, steps, lds_slots; /* two-level schedule (0: not built): chunks of consecutive blocks, steps, LDS words of the largest chunk */
    aoclsparse_int model_chunk_us, model_block_us; /* plan-time estimates of the two-level / the lane-per-block schedule */
    /* what a single-RHS, unit-stride, kid-0 solve runs now (set_trsv_schedule included): the schedule the solve itself resolves,
     * every fallback applied (4 forced on a triangle without a block plan reads 3 or 2); other strides, right-hand sides or kids
     * may run another one */
    aoclsparse_int schedule;
    aoclsparse_int slices, slice_fan_in_permille; /* lane-per-block schedule: wavefronts (slices of <= 64 blocks of one level; 32 where
                                                     1000 * the producer slices a slice of 64 waits for, on average, exceeds 8000) */
} aoclsparse_mi355_trsv_info;
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_get_trsv_info(const aoclsparse_matrix     A,
                                                            aoclsparse_fill_mode        fill,
                                                            aoclsparse_operation        op,
                                                            aoclsparse_mi355_trsv_info *info);
/* Asynchronous (device-pointer) aoclsparse_?trsv / ?trsm calls return before the solve has run.  Should one of the
 * sync-free kernels ever give up a wait (5 s of wall time: a lost dependency, never seen in testing), it leaves x untouched
 * and sets a word owned by the handle.  Call this AFTER synchronising your stream: internal_error if a solve of THIS handle
 * expired since the last query (the word is cleared), success otherwise.  Host-pointer solves report it themselves. */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_trsv_status(aoclsparse_matrix A);
/* TRSV / TRSM schedule.  -1 (default): chosen from the plan -- one launch per level for <= 32 levels, else a single
 * sync-free launch (a lane per block of chained rows where the triangle has them, else a level slice per wavefront or a
 * lane per position).  0: one launch per level, 1: hybrid (narrow level runs inside one workgroup), 2: sync-free, lane per
 * position, 3: sync-free, level slice per wavefront, 4: sync-free, lane per block.  Every schedule returns the same bits;
 * the `kid` of aoclsparse_?trsv_kid selects the arithmetic (0: ref_trsv_*; 1/2: 256-bit KT kernels; 3: 512-bit KT kernels), as
 * in the reference (library/src/level2/aoclsparse_trsv.cpp:321-353).  Process-wide; for tests and measurements. */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_set_trsv_schedule(aoclsparse_int schedule);
/* Call after writing into the VALUES of the arrays the handle aliases (on a handle created with aoclsparse_create_?csc: the
 * caller's CSC arrays, from which the handle's own CSR is refreshed first).  Drops every copy the handle holds of them -- the clean
 * copy of unsorted / diagonal-less arrays, the host transpose, the derived symmetric / triangular matrices, the device CSRs,
 * the SELL-64 and blocked-ELL copies, the TRSV plans (row, block and chunk), the device diagonal and the multi-device replicas:
 * the list ?set_value / ?update_values drop -- and the structural plans of the device CSR (row blocks, merge-path tiles, csrmm
 * row groups, row runs, row pairs and windows).  Each is rebuilt from the arrays on first use.  The ILU(0) factor is kept, as
 * after ?update_values (it is computed once, from the values seen at the first factorisation).  The caller's ptr / ind arrays
 * must be unchanged. */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_invalidate(aoclsparse_matrix A);
/* free the library's staging buffers in HBM (process-wide: the primary device's and those of every device a multi-device call has
 * used; each device's stream is synchronised first): the grow-only scratch that host-pointer calls (?csrmv, ?mv, ?trsv, the ELL
 * family) and sp2m (operands that are not a handle's own arrays, bin lists, the global slabs of very long rows) keep between calls
 * so that the next call allocates nothing.  The next call that needs one allocates it again.  Returns the number of bytes freed
 * through *bytes_freed (may be NULL).  No reference counterpart (the reference has no device). */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_release_staging(size_t *bytes_freed);

/* trsv with strides AND a kernel id in one call: what the reference offers only through its C++ template
 * aoclsparse::trsv<T> (library/include/aoclsparse.hpp); include/aoclsparse.hpp forwards to these. */
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_strsv_full(aoclsparse_operation trans, float alpha, aoclsparse_matrix A,
                                                         const aoclsparse_mat_descr descr, const float *b,
                                                         aoclsparse_int incb, float *x, aoclsparse_int incx,
                                                         aoclsparse_int kid);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_dtrsv_full(aoclsparse_operation trans, double alpha, aoclsparse_matrix A,
                                                         const aoclsparse_mat_descr descr, const double *b,
                                                         aoclsparse_int incb, double *x, aoclsparse_int incx,
                                                         aoclsparse_int kid);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_ctrsv_full(aoclsparse_operation trans, aoclsparse_float_complex alpha,
                                                         aoclsparse_matrix A, const aoclsparse_mat_descr descr,
                                                         const aoclsparse_float_complex *b, aoclsparse_int incb,
                                                         aoclsparse_float_complex *x, aoclsparse_int incx,
                                                         aoclsparse_int kid);
DLL_PUBLIC aoclsparse_status aoclsparse_mi355_ztrsv_full(aoclsparse_operation trans, aoclsparse_double_complex alpha,
                                                         aoclsparse_matrix A, const aoclsparse_mat_descr descr,
                                                         const aoclsparse_double_complex *b, aoclsparse_int incb,
                                                         aoclsparse_double_complex *x, aoclsparse_int incx,
                                                         aoclsparse_int kid);

/* ---- thin HIP C-ABI: device pointers, explicit stream ---------------------------------- */
/* Row-block table for mi355_?csrmv, built on the HOST from a host row_ptr: nblocks+1 entries
 * {first row, first non-zero (0-based)}, i.e. 2*(nblocks+1) ints; blocks_host must hold
 * mi355_csrmv_plan_bound(m, nnz) ints.  tile = non-zeros staged in LDS per workgroup: 512, 1024 or 2048.
 * Returns the number of blocks, <0 on error. */
DLL_PUBLIC aoclsparse_int mi355_csrmv_plan_bound(aoclsparse_int m, aoclsparse_int nnz);
DLL_PUBLIC aoclsparse_int mi355_csrmv_plan_host(aoclsparse_int        m,
                                                aoclsparse_int        base,
                                                aoclsparse_int        tile,
                                                const aoclsparse_int *row_ptr_host,
                                                aoclsparse_int       *blocks_host);
/* The slice records of a SELL-64 copy as aoclsparse_optimize packs them for the short-row SpMV kernel, from host arrays (no device
 * involved): slice_ptr = nslices + 1 cell offsets (64 x width each); leaders[s] = column lists of slice s | mode << 8 (mode 0: a table
 * says which list a row follows and with which column shift, 1: one list, shift = row within the slice, 2: one list, no shift), or NULL
 * when every row keeps its own list (mode 3: a cell's column entry sits at the cell's offset); column_entries = column entries in all.
 * A record is four 32-bit words {cell offset bits 0-31, column offset bits 0-31, cell offset bits 32-47 | column offset bits 32-47 << 16,
 * width | column stride << 8 | mode << 16}.  Returns the number of records written, nslices + the padding (empty slices that start
 * at the end of both arrays); records == NULL only returns that number; < 0 on error. */
DLL_PUBLIC aoclsparse_int mi355_sell_slice_records(aoclsparse_int nslices, const long long *slice_ptr, const aoclsparse_int *leaders,
                                                   long long column_entries, unsigned int *records);
/* y = alpha*A*x + beta*y; order: 0 scalar chain, 1 4-lane, 2 8-lane (reference kid 0 / 1,2 / 3);
 * strict != 0 keeps the reference order for rows longer than one LDS tile too; tile must be the
 * value the plan was built with; blocks is the DEVICE copy of the plan. */
DLL_PUBLIC aoclsparse_status mi355_dcsrmv(void                 *stream,
                                          aoclsparse_int        order,
                                          aoclsparse_int        strict,
                                          aoclsparse_int        tile,
                                          aoclsparse_int        base,
                                          double                alpha,
                                          aoclsparse_int        m,
                                          const double         *val,
                                          const aoclsparse_int *col,
                                          const aoclsparse_int *row_ptr,
                                          const aoclsparse_int *blocks,
                                          aoclsparse_int        nblocks,
                                          const double         *x,
                                          double                beta,
                                          double               *y);
DLL_PUBLIC aoclsparse_status mi355_scsrmv(void                 *stream,
                                          aoclsparse_int        order,
                                          aoclsparse_int        strict,
                                          aoclsparse_int        tile,
                                          aoclsparse_int        base,
                                          float                 alpha,
                                          aoclsparse_int        m,
                                          const float          *val,
                                          const aoclsparse_int *col,
                                          const aoclsparse_int *row_ptr,
                                          const aoclsparse_int *blocks,
                                          aoclsparse_int        nblocks,
                                          const float          *x,
                                          float                 beta,
                                          float                *y);
/* C = alpha*A*B + beta*C (op none), dense B/C device pointers; order as aoclsparse_order. */
DLL_PUBLIC aoclsparse_status mi355_dcsrmm(void                 *stream,
                                          aoclsparse_int        order,
                                          aoclsparse_int        base,
                                          double                alpha,
                                          aoclsparse_int        m,
                                          aoclsparse_int        k,
                                          const double         *val,
                                          const aoclsparse_int *col,
                                          const aoclsparse_int *row_ptr,
                                          const double         *B,
                                          aoclsparse_int        n,
                                          aoclsparse_int        ldb,
                                          double                beta,
                                          double               *C,
                                          aoclsparse_int        ldc);

#ifdef __cplusplus
}
#endif
#endif /* AOCLSPARSE_MI355_H_ */
