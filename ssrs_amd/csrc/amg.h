// Internal interface of the aggregation-AMG preconditioner (amg.hip) used by
// the potential solver (potential.hip).
#pragma once
#include <vector>

#include "common.h"

namespace ssrs {

// Vectors of the V-cycle are f64.  An f32 cycle was measured in round 4 and does not work on this operator: a conductive
// cluster that floats in dead terrain is tied to its surroundings 1e-8 .. 1e-10 times more weakly than its cells are tied
// to each other, so the net residual of the cluster -- what the coarse levels need in order to set its level -- cancels to
// that relative size, below f32's resolution, and the outer iteration stalls at |r|/|b| ~ 1e-8 (profiles/r04_k5.md).

struct AmgLevel {
    int n = 0, nnz = 0, nc = 0;
    int *rowptr = nullptr, *col = nullptr;
    double *val = nullptr, *dinv = nullptr;
    float *val32 = nullptr;    // the same entries rounded to f32 for the cycle's sweeps (levels >= 1)
    // the same entries once more in sliced ELL form (slices of 64 rows, entry k of row 64 s + l at sell_ptr[s] + 64 k + l,
    // short rows padded with (own column, 0)): a wave reads 64 consecutive entries per load and its 64 gathers of x go to
    // neighbouring rows' neighbours -- the large levels' sweeps (amg.hip: k_sweep_sell)
    int *sell_ptr = nullptr, *sell_col = nullptr;
    float *sell_val = nullptr;
    int *agg = nullptr;        // fine node -> coarse node (-1: isolated row), NULL on the last level
    int *memptr = nullptr;     // coarse node I -> its fine nodes memidx[memptr[I] .. memptr[I+1])
    int *memidx = nullptr;
    double *x = nullptr, *xt = nullptr, *b = nullptr, *r = nullptr;
    // K-cycle scratch (levels 1 .. kdepth)
    double *kb = nullptr, *c1 = nullptr, *v1 = nullptr, *v2 = nullptr;
    void *kscal = nullptr;
};

struct AmgHierarchy {
    std::vector<AmgLevel> levels;
    double *dense_inv = nullptr;   // inverse of the last level when it is small
    size_t workspace_used = 0;
    void *graph_exec[2] = {nullptr, nullptr};   // hipGraphExec_t of the captured fast / robust cycle (NULL: direct launches)
    bool graph_tried[2] = {false, false};
    bool robust = false;           // the cycle being run / captured: V(2,2) everywhere instead of (nu0, nuc)
    bool symmetric = true;         // symmetric strength of connection (amg.hip: strong_link)
    int strong_rounds = 4;         // matching rounds restricted to strong couplings (of 8)
    int kdepth = 0;                // coarse levels 1..kdepth use the K-cycle (0 = V-cycle)
    int sweeps = 1;                // pairs of Jacobi sweeps before and after the coarse correction
    int nu0 = 1, nuc = 1;          // Jacobi sweeps before / after the coarse correction on level 0 / on the coarser levels:
                                   // 1 (default since round 4: V(1,1), 430 iterations x 5.2 ms at C2) or 2 (rounds 1-3: V(2,2),
                                   // 385 x 8.1 ms); SSRS_AMG_NU=a,b
    bool blocks0 = true;           // level 1 from the 2 x 2 raster blocks (amg.hip: k_block_agg); SSRS_AMG_NO_BLOCKS: pairwise matching
    bool fuse = true;              // level 0 of the V(1,1) cycle in two fused passes when it applies; SSRS_AMG_NO_FUSE: six kernels
    bool progress = false;         // SSRS_PROGRESS: the hierarchy and the graph capture on stderr
    // level 0 applied matrix-free (amg.hip: L0Stencil)
    const double *l0_rinv = nullptr;   // +-1 / cond: the cycle and the outer operator (potential.hip) read it
    // level 0 of the V(1,1) cycle fused into two stencil passes that read the caller's right-hand side and write the
    // caller's result directly (amg.hip: k_l0_pre2 / k_l0_post2); the two pointers travel through a device slot
    // so that the captured graph serves every (rhs, out) pair
    void *l0_slots = nullptr;
    bool fuse0 = false;            // `fuse` and the hierarchy allows it (set by amg_setup)
    bool l0_blocks = false;        // level 1 = parts of aligned 2 x 2 raster blocks (k_block_agg): the two-row level-0 kernels restrict in place
    const uint8_t *l0_fixed = nullptr;
    int l0_rows = 0, l0_cols = 0;
};

size_t amg_workspace_bytes(int rows, int cols);
// Builds the hierarchy inside `workspace` (device memory, 256-byte aligned).
int amg_setup(AmgHierarchy &h, const double *cond, const uint8_t *fixed, int rows, int cols,
              void *workspace, size_t workspace_bytes, hipStream_t st);
// out = M rhs (one V-cycle); rhs/out: f64 vectors on the raster numbering.
// robust: the V(2,2) cycle of rounds 1-3 whatever nu0 / nuc say (BiCGStab takes it when it stagnates under V(1,1))
void amg_apply(AmgHierarchy &h, const double *rhs, double *out, hipStream_t st, bool robust = false);
// Frees host-side resources (the captured graph); device memory is the caller's.
void amg_release(AmgHierarchy &h);

}  // namespace ssrs
