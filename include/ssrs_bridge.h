/* ssrs_bridge.h -- the gap score of libssrs_hip.so (K23): a public header beside ssrs_hip.h, ssrs_score.h and their
 * companions, whose conventions (caller-owned device memory, row-major rasters, `stream` a hipStream_t passed as void*,
 * SSRS_OK or a negative SSRS_ERR_* code with ssrs_last_error()) and error codes it shares.  The export is an addition to the
 * library: SSRS_VERSION does not change with it.  (The name stays outside ssrs_hip*.h, which the stream-contract test
 * globs: tests/test_gpu_bridge.py pins the stream of this export itself.) */
#ifndef SSRS_BRIDGE_H_
#define SSRS_BRIDGE_H_

#include "ssrs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The status of a gap, tested in the order TOO_LONG, OUT; an evaluated gap gets SCORED, ZERO or UNDEFINED from P. */
#define SSRS_BRIDGE_SCORED 0      /* P > 0 and finite */
#define SSRS_BRIDGE_ZERO 1        /* P == 0: no path of n moves the model allows; includes cheb(A, B) > n */
#define SSRS_BRIDGE_TOO_LONG 2    /* moves outside [1, SSRS_BRIDGE_MAX_MOVES]; nothing else of the job is read */
#define SSRS_BRIDGE_OUT 3         /* A is not an interior cell, or B lies outside the raster, or incoming outside 0..8 */
#define SSRS_BRIDGE_UNDEFINED 4   /* P is NaN or inf (inf x 0 or inf / inf in the reference's own sequence) */
#define SSRS_BRIDGE_MAX_MOVES 32
#define SSRS_BRIDGE_JOB 6         /* int32 per job: row_a, col_a, incoming, row_b, col_b, moves */

/* K23 -- sparse telemetry: "the bird was at cell A, and n moves later at cell B".  Under the movement model with memory 1
 * (ssrs_tracks_simulate, ssrs_tracks_score) the probability of that is the n-step transition probability, the sum over
 * EVERY path of n moves from A to B (the forward algorithm), not the probability of one line between them.
 *
 * Definition.  A state is (cell, last move k), k = 3 (dr + 1) + (dc + 1) in 0..8, delta_k = (k / 3 - 1, k % 3 - 1); k = 4 is
 * "no last move": a start, a rest, or a memory that a gap has reset.  A job is (A, s, B, n): the start cell, the state in
 * which the bird is at A, the target cell, the number of moves.
 *   alpha_0(A, s) = 1, every other state 0
 *   alpha_{t+1}(x, k) = sum over d = 0..8 of alpha_t(y, d) * p_k(y, d),  y = x - delta_k,
 *            taken in ascending d, sequentially, from 0.0; a source state with alpha_t == 0 is skipped (the NaN probability
 *            of an unoccupied state never enters); y must be an INTERIOR cell (0 < row < rows - 1, 0 < col < cols - 1): a rim
 *            cell emits nothing, as the simulated track ends there after the burn-in.  The burn-in relocation is never
 *            applied inside a gap.  x may be any cell of the raster, so B may lie on the rim
 *   p(y, d)[9]   ssrs_score.h's p[9] at base y under the mask "all but the centre AND the restriction of delta_d", with the
 *            same weights, prior and nu: the same device function on the same operands as ssrs_tracks_score
 *   g[k]     = alpha_n(B, k): the probability of being at B after n moves, by the move that arrived there
 *   P        = ((g0 + g1) + (g2 + g3)) + ((g4 + g5) + (g6 + g7)) + g8, numpy's pairwise order
 *   arrivals[t - 1] = the same sum of alpha_t(B, .), t = 1..n: the probability of being at B after t moves, so
 *            arrivals[n - 1] == P bit for bit.  Mass that is at B before move n moves on like any other
 *   status   TOO_LONG when n lies outside [1, 32]; else OUT when A is not interior, B is outside the raster or s is outside
 *            0..8; else SCORED if 0 < P < inf, ZERO if P == 0 (always when the Chebyshev distance of A and B exceeds n),
 *            UNDEFINED otherwise
 *   s        = (uint64) rint(-log2(P) * 2^32) of a SCORED gap, 0 otherwise: ssrs_score.h's unit, so gap and move
 *            surprisals add
 * The recursion above is UNCONFINED.  A cell x lies on a path only if cheb(A, x) + cheb(x, B) <= n, and its mass at time t
 * reaches B only if cheb(x, B) <= n - t; the kernel propagates inside the bounding box of those cells (a side of at most
 * n + 1), and every value that reaches B is bit-identical to the unconfined one, because the sum of each such target keeps
 * all its non-zero sources and their order.
 *
 *   params     rows, cols, scaling_parameter (nu), prior are read as ssrs_tracks_score reads them; memory_parameter must
 *              be 1; every other field is ignored
 *   updraft    f64 (rows, cols) or NULL;  potential  f32 (rows, cols) or NULL.  Both NULL = 'drw'
 *   jobs       int32 (ngaps, SSRS_BRIDGE_JOB): row_a, col_a, incoming, row_b, col_b, moves
 *   g          f64 (ngaps, 9);  status  uint8 (ngaps,);  surprisal  uint64 (ngaps,).  All three WRITTEN for every job (g
 *              and the surprisal 0 where the job is not evaluated).  surprisal[0] is used as scratch before it is written
 *   arrivals   f64 (ngaps, SSRS_BRIDGE_MAX_MOVES), WRITTEN, the entries past n (all of them where the job is not
 *              evaluated) 0; NULL = not wanted
 *
 * The pass.  One workgroup per gap (a grid-stride loop over them), the states of the gap's window ping-ponged in LDS in
 * f64: two buffers of nine planes of at most 33 x 33 cells.  One lane per SOURCE cell y sums, over its occupied incoming
 * states in ascending order, alpha times the nine probabilities -- all nine sums of the targets y + delta_k have their
 * only source cell in y, so there is no atomic and no dependence on lane or launch order -- and stores them under (y, k);
 * the next step reads alpha(x, d) at (x - delta_d, d).  One __syncthreads() per step.  Only the cells within t of A and
 * n - t of B are visited in step t, and only occupied states evaluate their probabilities, which are recomputed every
 * step (no table, no workspace).  The LDS is dynamic, 144 (N + 1)^2 bytes for the largest valid `moves` N of the call
 * (156 816 bytes at N = 32, of a CU's 160 KiB): N is found by a first small launch and read back, so the call waits for
 * `stream` once; workgroups are 512 lanes when the window has more than 512 cells, 256 otherwise.
 *
 * Errors, all SSRS_ERR_INVALID: a NULL params, jobs, g, status or surprisal; a potential without an updraft; ngaps outside
 * [0, 2^31); rows or cols outside [3, 32767]; a memory_parameter other than 1 (refused by name); a negative or NaN
 * scaling_parameter; jobs that is not 4-byte aligned; g, surprisal or arrivals that is not 8-byte aligned -- all before any
 * GPU work -- and a device whose hipDeviceAttributeMaxSharedMemoryPerBlock is less than the call needs, before the
 * gaps are launched.  ngaps == 0 returns SSRS_OK and touches nothing. */
int ssrs_tracks_bridge(const SsrsTrackParams *params, const double *updraft, const float *potential, const int32_t *jobs,
                       int64_t ngaps, double *g, uint8_t *status, uint64_t *surprisal, double *arrivals, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SSRS_BRIDGE_H_ */
