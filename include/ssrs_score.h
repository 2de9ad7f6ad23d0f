/* ssrs_score.h -- the track score of libssrs_hip.so (K21): a public header beside ssrs_hip.h and its four companions,
 * whose conventions (caller-owned device memory, row-major rasters, `stream` a hipStream_t passed as void*, SSRS_OK or a
 * negative SSRS_ERR_* code with ssrs_last_error()) and error codes it shares.  The export is an addition to the library:
 * SSRS_VERSION does not change with it. */
#ifndef SSRS_SCORE_H_
#define SSRS_SCORE_H_

#include "ssrs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The status of the move that leaves a point.  Tested in the order LAST, OUT, NOT_A_MOVE; an evaluated move gets SCORED,
 * ZERO or UNDEFINED from its probability. */
#define SSRS_SCORE_SCORED 0       /* p > 0 and finite */
#define SSRS_SCORE_ZERO 1         /* p == 0: the model forbids the move */
#define SSRS_SCORE_NOT_A_MOVE 2   /* a component of the move lies outside {-1, 0, 1}: a gap in the observations */
#define SSRS_SCORE_OUT 3          /* the move's base is not an interior cell */
#define SSRS_SCORE_UNDEFINED 4    /* p is NaN (inf x 0 or inf / inf in the reference's own sequence) */
#define SSRS_SCORE_LAST 5         /* the track's last point: no move leaves it */
#define SSRS_SCORE_MAX_MEMORY 8
#define SSRS_SCORE_ROW 6          /* uint64 per track: S, scored, zero, not_a_move, out, undefined */

/* K21 -- the movement model read backwards: the probability the stepper (ssrs_tracks_simulate) gives to every move of
 * OBSERVED tracks, and its surprisal summed per track.  Nothing is drawn; every move is independent of every other once
 * the points are known.
 *
 * Definition.  A track is points P_0 .. P_{n-1}, int16 (row, col); move j (0 <= j <= n - 2) leaves point j.
 *   base_j   = P_j when j > burnin, else move_away_from_boundary(P_j): row <= 1 -> row + 2, else row >= rows - 2 ->
 *              row - 2; col <= 0 -> col + 2, else col >= cols - 2 -> col - 2 (movmodel.py:205-217; the reference relocates
 *              before it moves while k <= burnin and records relocated + delta)
 *   delta_j  = P_{j+1} - base_j, in int32
 *   status   LAST for point n - 1; else OUT unless 0 < base row < rows - 1 and 0 < base col < cols - 1; else NOT_A_MOVE
 *            when a component of delta_j lies outside {-1, 0, 1}; else the move is evaluated
 *   mask     the restriction of (0, 0) (all but the centre) ANDed with the restrictions (movmodel.py:185-202) of
 *            delta_{j-1}, delta_{j-2}, ..., at most memory_parameter of them, each measured against its own base, walking
 *            back until the track's start or the first delta with a component outside {-1, 0, 1}: a gap in the
 *            observations resets the memory, as the start does
 *   weights  with updraft: 2 / (1 / max(u_c, 1e-6) + 1 / max(u_k, 1e-6)) over the 3 x 3 window of base_j, times, with a
 *            potential, f64(f32(f32(pot_c - pot_k) * norm_inv_k)) (movmodel.py:292-306); without fields the prior
 *   p[9]     generate_move_probabilities (movmodel.py:220-244) on them: a NaN weight -> the prior; clip at 0; centre zeroed;
 *            times the mask (inf x 0 = NaN); all zero -> the masked prior; all zero again -> the prior; divided by their
 *            pairwise-8 sum; pow(., nu) only if nu != 1; divided by their pairwise-8 sum
 *   p_j      = p[3 (dr + 1) + (dc + 1)]; SCORED if 0 < p_j < inf, ZERO if p_j == 0, UNDEFINED otherwise.  A rest (0, 0) is
 *            evaluated like any other cell: ZERO unless nu == 0, where every cell gets exactly 1 / 9
 *   s_j      = (uint64) rint(-log2(p_j) * 2^32) of a SCORED move: its surprisal in units of 2^-32 bit, at most ~2^42.1
 * Sums of s_j are integer sums: exact, independent of the launch order and of how tracks are cut over calls, and they add
 * over chunks and ranks.  The log-likelihood of a track is -ln 2 * S / 2^32.
 *
 *   params     rows, cols, burnin, memory_parameter (1 .. SSRS_SCORE_MAX_MEMORY), scaling_parameter (nu), prior are read;
 *              every other field is ignored
 *   updraft    f64 (rows, cols) or NULL;  potential  f32 (rows, cols) or NULL.  Both NULL = 'drw'
 *   traj, traj_offsets, ntracks     as ssrs_track_time takes them: int16 (row, col) pairs, ntracks + 1 int64 offsets into
 *              them (the first need not be 0)
 *   p          f64, parallel to traj: entry i is the probability of the move that LEAVES point i; 0.0 where the status is
 *              LAST, OUT or NOT_A_MOVE.  WRITTEN for every point of the chunk; NULL = not wanted
 *   status     uint8, parallel to traj, SSRS_SCORE_*.  WRITTEN; NULL = not wanted
 *   rows       uint64 (ntracks, SSRS_SCORE_ROW): per track the sum S of s_j and the numbers of moves by status.  WRITTEN
 *              (zeroed by the call, then added to)
 *   surprisal_map   uint64 (rows, cols): s_j ADDED at the base cell of each SCORED move; NULL = not wanted
 *   scored_map      uint32 (rows, cols): 1 ADDED at the same cell; NULL = not wanted
 *
 * The pass.  One launch, one lane per point.  A block takes 256 consecutive points and stages them with the 8 behind and
 * the 4 ahead in LDS (16-byte loads where traj is 16-byte aligned, point by point otherwise and at the chunk's ends); the
 * look-back of a lane reads its neighbours' points there.  A lane finds its track by binary search in the offsets between
 * the tile's first and last track.  The per-track sums are a segmented scan over the block in LDS and one 64-bit add per
 * (block, track) segment and column; the maps take one 64-bit and one 32-bit add per SCORED move.  The chunk's first and
 * last offset are read back first (the launch is sized from its points), so the call waits for `stream` once.
 *
 * Errors, all SSRS_ERR_INVALID before any GPU work: a NULL params, traj, traj_offsets or rows; a potential without an
 * updraft; ntracks outside [0, 2^31); rows or cols outside [3, 32767]; a memory_parameter outside [1, 8] (0, the whole
 * history, needs a running AND along the track and is refused by name); a negative or NaN scaling_parameter; a traj that
 * is not 4-byte aligned, a p, rows or surprisal_map that is not 8-byte aligned, a scored_map that is not 4-byte aligned.
 * ntracks == 0, or no points, returns SSRS_OK and touches nothing. */
int ssrs_tracks_score(const SsrsTrackParams *params, const double *updraft, const float *potential, const int16_t *traj,
                      const int64_t *traj_offsets, int64_t ntracks, double *p, uint8_t *status, uint64_t *rows,
                      uint64_t *surprisal_map, uint32_t *scored_map, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SSRS_SCORE_H_ */
