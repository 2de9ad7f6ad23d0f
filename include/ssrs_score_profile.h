/* ssrs_score_profile.h -- the likelihood profile of observed tracks of libssrs_hip.so (K22): a public header beside
 * ssrs_score.h (K21), whose conventions, error codes, statuses and row layout it shares.  The export is an addition to the
 * library: SSRS_VERSION does not change with it. */
#ifndef SSRS_SCORE_PROFILE_H_
#define SSRS_SCORE_PROFILE_H_

#include "ssrs_hip.h"
#include "ssrs_score.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SSRS_PROFILE_MAX_MEMORIES 8
#define SSRS_PROFILE_MAX_NUS 32

/* K22 -- K21's per-track rows over a grid of memories x nus in one pass, for calibrating the two on telemetry.
 *
 * Definition.  rows[t, a, b, :] is, integer for integer, the row that ssrs_tracks_score writes for track t with
 * memory_parameter = memories[a] and scaling_parameter = nus[b]: S, scored, zero, not_a_move, out, undefined.  Everything
 * else -- the base, the statuses, the mask, the weights, the probability sequence and s_j -- is defined in ssrs_score.h.
 *
 *   params     rows, cols, burnin and prior are read; memory_parameter and scaling_parameter are IGNORED
 *   updraft, potential, traj, traj_offsets, ntracks     as ssrs_tracks_score takes them
 *   memories   HOST int32 [nmem], 1 <= nmem <= SSRS_PROFILE_MAX_MEMORIES: each in 1 .. SSRS_SCORE_MAX_MEMORY, strictly
 *              ascending.  Copied into the kernel's arguments, like prior
 *   nus        HOST f64 [nnu], 1 <= nnu <= SSRS_PROFILE_MAX_NUS: each not negative and not NaN (what ssrs_tracks_score
 *              accepts), in any order, repeats allowed.  Copied likewise
 *   rows       DEVICE uint64 (ntracks, nmem, nnu, SSRS_SCORE_ROW).  WRITTEN (zeroed by the call, then added to)
 * Not offered: the per-point p and status and the two maps.  They come from ssrs_tracks_score at the fitted values.
 *
 * The pass.  One launch, one lane per point, staged and searched as K21's.  Per lane ONCE: the base, the status tests, the
 * raw window weights, and one walk back over memories[nmem - 1] deltas that yields the mask of every requested memory (the
 * masks are running ANDs of one another).  Per DISTINCT mask: the half of the probability sequence that does not depend on
 * nu, through the first nine divisions; a memory whose mask equals the one before -- behind a start or a gap -- reuses
 * it.  Per nu: nine pow (none for nu = 1), one pairwise sum, one division, one log2.  The block's segmented scan in LDS
 * takes four combinations at a time; the last lane of a (block, track) segment adds its non-zero totals with 64-bit adds.
 *
 * Errors, all SSRS_ERR_INVALID before any GPU work: those of ssrs_tracks_score for the arguments the two share; a NULL
 * memories or nus; nmem outside [1, 8], a memory outside [1, 8], memories that do not ascend strictly; nnu outside
 * [1, 32], a negative or NaN nu; rows not 8-byte aligned.  ntracks == 0, or no points, returns SSRS_OK
 * and touches nothing.  Every launch, the memset and the read-back of the two end offsets go to `stream`, which the call
 * waits for once. */
int ssrs_tracks_score_profile(const SsrsTrackParams *params, const double *updraft, const float *potential,
                              const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks,
                              const int32_t *memories, int32_t nmem, const double *nus, int32_t nnu,
                              uint64_t *rows, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SSRS_SCORE_PROFILE_H_ */
