// trsv_schedule.hpp -- which TRSV schedule runs: the one place that decides it (host only, no HIP calls).
//
// The solve (trsv_api.cpp: solve_core), the info call (aoclsparse_mi355_get_trsv_info) and the launcher (trsv_kernels.hip, which
// only checks that it can serve what it is handed) all go by resolve_trsv_schedule; a handle's plan of one (fill, op) is found by
// trsv_plan_index.
#pragma once

#include "internal.hpp"

namespace mi355
{

// index of a (fill, op) variant in _aoclsparse_matrix::trsv_plan: L, L^T, U, U^T; op = H of a complex type: L^H, U^H
inline int trsv_plan_index(bool upper, bool transposed, bool conj)
{
    return conj ? 4 + (upper ? 1 : 0) : (upper ? 2 : 0) + (transposed ? 1 : 0);
}

struct TrsvChoice
{
    int  schedule; // the schedule that runs, 0-5 (launch_trsv; complex types: 1, served by launch_ctrsv)
    bool needs_rows; // the level-ordered row layout (TrsvPlan::rows_valid) has to exist before the solve
    bool syncfree; // the kernel can report an expired wait: the timeout word has to be looked at
};

// forced: aoclsparse_mi355_set_trsv_schedule (-1 = automatic); unit_stride: incb == 1 && incx == 1; kt_bits: 0 = the reference
// chain, 256 / 512 = the order of the KT kernels (kid 1 / 2, kid 3).
// While needs_rows holds and the layout has not been built, `schedule` is the request: the solve builds the layout on demand
// (ensure_trsv) and resolves again.
inline TrsvChoice resolve_trsv_schedule(const TrsvPlan &plan, aoclsparse_int m, bool is_complex, bool upper, bool transposed,
                                        bool conj, int forced, aoclsparse_int nrhs, bool unit_stride, int kt_bits)
{
    const TrsvBlockPlan &blk = plan.blk;
    // the level-ordered row layout is needed by the per-level, hybrid and slice schedules (and by complex types); the
    // lane-per-position kernel runs on the block plan's layout too (any topological order of the rows will do).  Decided on the
    // REQUEST, not on the schedule that runs in the end: it settles which layout the lane-per-position kernel walks.
    const bool needs_rows = is_complex || !blk.valid || forced == 0 || forced == 1 || forced == 3 || (forced < 0 && plan.nlevels <= 32);
    // (complex handles always run the hybrid schedule: their 8 / 16-byte x cannot be the one-word ready flag)
    if(is_complex)
        return {1, needs_rows, false};

    // 1. the request.  Every one of the schedules gives the same bits.  A shallow DAG of wide levels is cheapest as plain launches;
    // otherwise sync-free, which measured fastest on both the 2-D Laplacian and the shell-like ILU(0) factors.
    // The sync-free choice is the slice-per-wavefront kernel (3) for one right-hand side -- unless the level slices
    // would leave most lanes idle (average level narrower than 16 rows: deep chains), where the lane-per-position
    // kernel (2) packs better; aoclsparse_mi355_set_trsv_schedule forces one of them.
    // measured (profiles/r2/trsv_schedules.txt): the slice kernel wins on short rows (ILU(0) of the 2-D Laplacian:
    // 1.69 vs 2.09 ms), the lane-per-position kernel on rows of ~17 entries (shell-like factor)
    // -- except when a row's chain STARTS with the row solved last (U, upper && !transposed): there every entry behind
    // the first would be polled one round trip at a time (45 ms), and the slice kernel's batch re-read wins (17.9 ms)
    const bool packed = nrhs == 1 && plan.nslices > 0 && (long long)plan.nslices * 16 <= (long long)m;
    const int  sf     = (packed && ((long long)plan.nnz_tri <= 10LL * m || (upper && !transposed && !conj))) ? 3 : 2;
    // chained rows (the dofs of a node) solved back to back by one lane: one hop per BLOCK level instead of per row level
    // ... and, where the plan-time model says it pays, the two-level schedule: chunks of consecutive blocks, hand-offs inside a
    // chunk through LDS (schedule 5; the reference chain only)
    const int sfb = blk.valid ? (blk.chunk.valid ? 5 : 4) : sf; // (trsm too: one grid column per right-hand side)
    int       s   = (forced >= 0 && forced <= 5) ? forced : (plan.nlevels <= 32 ? 0 : sfb);
    if(needs_rows && !plan.rows_valid)
        return {s, true, s >= 2};

    // 2. what the kernels cannot serve, in this order.
    // kt_bits: served by trsv_block_kt_kernel when the triangle has a block plan (schedule 4), else by the per-level launches
    // and the lane-per-position sync-free kernel (the two-level kernel serves the reference chain only)
    if(kt_bits != 0 && s == 5)
        s = 4;
    if(kt_bits != 0 && s != 0 && !(s == 4 && blk.valid))
        s = 2;
    if(s == 1 && (nrhs != 1 || !unit_stride))
        s = 2; // the single-workgroup runs of the hybrid schedule are single-RHS, unit stride
    // (several right-hand sides: the column is grid dimension x, the chunk / slice y <= 65,535; index arithmetic in int)
    const bool wide_rhs = nrhs > 1 && (long long)m * nrhs + TRSV_XP_PAD >= (1LL << 31);
    if(s == 5 && (!blk.valid || !blk.chunk.valid || kt_bits != 0 || (nrhs > 1 && blk.chunk.nchunks > 65535) || wide_rhs))
        s = 4;
    if(s == 4 && (!blk.valid || (nrhs > 1 && blk.nslices > 65535) || wide_rhs))
        s = 3;
    if(s == 3 && (nrhs != 1 || plan.nslices <= 0 || !plan.rows_valid))
        s = 2; // the slice kernel is single-RHS; trsm keeps the lane-per-position kernel
    // syncfree: schedules 2-5 wait on tagged words.  This is what solve_core used to spell out as
    //   request >= 2 || (request == 1 && (nrhs != 1 || !unit_stride || kt_bits != 0)):
    // no rule above leaves the schedules >= 2 (the targets are 4, 2, 4, 3, 2), 0 matches none of them, and 1 becomes 2 exactly
    // under the second rule (kt_bits != 0) or the third (nrhs != 1 or a stride).
    return {s, needs_rows, s >= 2};
}

} // namespace mi355
