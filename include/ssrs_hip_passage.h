/* ssrs_hip_passage.h -- the passage map of libssrs_hip.so (K17): a second public header beside ssrs_hip.h, whose
 * conventions (caller-owned device memory, row-major rasters, `stream` a hipStream_t passed as void*, SSRS_OK or a
 * negative SSRS_ERR_* code with ssrs_last_error()) and error codes it shares.  The two exports are additions to the
 * library: SSRS_VERSION does not change with them. */
#ifndef SSRS_HIP_PASSAGE_H_
#define SSRS_HIP_PASSAGE_H_

#include "ssrs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* K17 -- how many DISTINCT tracks came within a radius of each cell, from the trajectories on the device: K8's
 * tracks_per_turbine evaluated at every cell centre, for sites that are not in the turbine table yet.
 * Definition, all integers.  r2 >= 0 is the largest squared distance, in cells, that counts as "within";
 * D = {(dr, dc) : dr*dr + dc*dc <= r2}.  For one call over the tracks 0..ntracks-1:
 *   counts[r, c]       += #{tracks k : some in-raster point p of k has (r, c) - p in D}, for every cell of the raster;
 *   cells_per_track[k] += #{in-raster cells (r, c) : some in-raster point p of k has (r, c) - p in D}.
 * Points outside [0, rows) x [0, cols) are not positions and are ignored, as in ssrs_track_occupancy; the cells of a disk
 * outside the raster are clipped.  Sum(cells_per_track) == Sum(counts) of one call: the caller's checksum.  With r2 = 0
 * both outputs are exactly ssrs_track_occupancy's.  From metres: radius_cells = R / resolution in f64 and
 * r2 = floor(radius_cells * radius_cells), no epsilon -- a turbine on a cell centre is then counted by
 * ssrs_turbine_encounters' f64 test dx*dx + dy*dy <= R*R for exactly the tracks this call counts at that cell.
 *   traj, traj_offsets  exactly what ssrs_track_occupancy takes: int16 (row, col) pairs, 4-byte aligned (16-byte aligned
 *                       buffers are read 16 bytes a lane); int64 offsets (ntracks + 1), the first need not be 0, equal
 *                       consecutive offsets are an empty track
 *   r2                  0..SSRS_PASSAGE_MAX_RADIUS^2.  The library derives the disk's half-widths per row,
 *                       w(dy) = isqrt(r2 - dy*dy), from it
 *   planes              1..SSRS_PASSAGE_MAX_PLANES: tracks are taken in rounds of 32 * planes, track k of a round owning
 *                       bit k & 31 of plane k >> 5.  The result does not depend on it
 *   counts              uint32 (rows, cols), ADDED to, so that chunks, sub-batches and calls accumulate in one raster
 *   cells_per_track     uint32 (ntracks) or NULL, ADDED to
 *   stats               two uint64 or NULL, ADDED to: [0] the mask words the set kernels tested, [1] the bits they won.
 *                       stats[1] grows by the call's Sum(counts); stats[0] is the work: a whole disk for a track's first
 *                       point (and after a jump or an out-of-raster point), a crescent for a unit move, nothing for a rest
 *                       or for a move the lane has just made (it remembers its last two within a track)
 *   workspace           `planes` uint32 rasters, ssrs_track_passage_workspace_bytes = rows * cols * 4 * planes rounded up
 *                       to 256.  Plain scratch: its contents before a call mean nothing, and they are unspecified after
 *                       it.  The call clears a round's planes itself before that round's set kernel: the first round's
 *                       by a memset, a later round's by whichever moves fewer bytes, a memset of its planes or an "unset"
 *                       kernel that walks the round before once more and stores 0 to every word it tested.  The result
 *                       does not depend on the choice
 * Per round one "set" kernel over the round's points.  What a point sets depends on the point and its predecessor in the
 * track only -- the whole disk, the crescent (p + D) \ (q + D) after a unit move from q, or nothing -- so the union over
 * a track is the union of its disks under any launch order and any race; each cell of such a set is tested with an L2
 * load and set with atomicOr otherwise, and the one lane that is handed the old value without the bit counts it.  Exact.
 * The offsets at the round borders are read back first (each launch is sized from its round's points), so the call
 * waits for `stream` once; its launches go to `stream` in order.
 * NULL traj / traj_offsets / counts / workspace, planes outside [1, SSRS_PASSAGE_MAX_PLANES], rows / cols outside
 * [1, 32767], r2 outside [0, SSRS_PASSAGE_MAX_RADIUS^2], ntracks outside [0, 2^31), a misaligned traj, a workspace that
 * is too small -> SSRS_ERR_INVALID before any GPU work.  ntracks == 0, or no points, returns SSRS_OK and touches
 * nothing. */
#define SSRS_PASSAGE_MAX_PLANES 8
#define SSRS_PASSAGE_MAX_RADIUS 255          /* cells: r2 <= 255 * 255 */
size_t ssrs_track_passage_workspace_bytes(int rows, int cols, int planes);
int ssrs_track_passage(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks,
                       int rows, int cols, int64_t r2, int planes,
                       uint32_t *counts, uint32_t *cells_per_track, uint64_t *stats,
                       void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SSRS_HIP_PASSAGE_H_ */
