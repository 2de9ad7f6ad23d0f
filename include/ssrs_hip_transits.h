/* ssrs_hip_transits.h -- rotor transits of libssrs_hip.so (K18): a public header beside ssrs_hip.h and
 * ssrs_hip_passage.h, whose conventions (caller-owned device memory, row-major rasters, `stream` a hipStream_t passed as
 * void*, SSRS_OK or a negative SSRS_ERR_* code with ssrs_last_error()) and error codes it shares.  The export is an
 * addition to the library: SSRS_VERSION does not change with it. */
#ifndef SSRS_HIP_TRANSITS_H_
#define SSRS_HIP_TRANSITS_H_

#include "ssrs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* K18 -- transits per turbine and direction: the flights through each turbine's rotor DISK, a circle of radius reach_t
 * around the hub that stands across the wind, from the trajectories, K14's heights and the {climb, elev} raster on the
 * device.  It is the count a collision-risk model starts from; it is NOT a collision probability (no blade passage, no
 * avoidance).  Exact and independent of the launch order.
 *
 * Definition.  The frame is ssrs_turbine_encounters': x = column, y = row, in cell units.  A turbine t is
 *   (xt, yt)   f64, turbines[2 t], turbines[2 t + 1]: ssrs_turbine_encounters' numbers
 *   reach_t    f64, cells: (t_rd / 2 + rotor_clearance) / resolution
 *   hub_t      int32, millimetres above the DEM's datum: base + rint(1000 t_hh), base as for ssrs_rotor_encounters' zband,
 *              the int64 sum clipped to int32
 *   (ax_t, ay_t)  f64, axis[2 t], axis[2 t + 1]: the upwind unit step along +col and +row.  The host makes it; the
 *              kernel never evaluates a trigonometric function.
 * mm_per_cell is one f64 scalar: 1000 * resolution.
 * A MOVE is a pair of consecutive points k, k + 1 of one track: off[j] <= k and k + 1 < off[j + 1].  The last point of a
 * track and the first of the next are not a move, and nothing outside [off[0], off[ntracks]) is read as a point of a move.
 * A move is TESTABLE iff both points lie inside the raster, `elev` of both cells is not the nodata sentinel INT32_MIN,
 * and max(|r1 - r0|, |c1 - c0|) <= 1: a burn-in jump is no real flight (as for ssrs_track_altitude and ssrs_track_time),
 * and a rest never crosses.  For a testable move and turbine t, with i = 0, 1 for its two ends:
 *   dx_i = (double)c_i - xt          dy_i = (double)r_i - yt
 *   s_i  = ax*dx_i + ay*dy_i         u_i  = ax*dy_i - ay*dx_i
 *   z_i  = (int64)elev_i + alt_i     h_i  = (double)(z_i - hub_t) / mm_per_cell
 *   crossing  iff  (s_0 < 0) != (s_1 < 0)
 *   d = s_0 - s_1     U = s_0*u_1 - s_1*u_0     H = s_0*h_1 - s_1*h_0
 *   transit   iff  crossing  and  reach_t >= 0  and  U*U + H*H <= (reach_t*reach_t) * (d*d)
 *   direction = 0 ("with the wind", upwind side to downwind side) if !(s_0 < 0), else 1 ("against the wind")
 * Every product, sum and difference is rounded on its own (no contraction; the kernel writes them with __dmul_rn,
 * __dadd_rn and __dsub_rn as ssrs_turbine_encounters' d2 is), and the one division is IEEE.
 * What this implies: the test has no division by d.  It is the straight segment between the two points, heights
 * interpolated linearly, against the circle of radius reach_t around the hub in the plane through the hub whose normal is
 * the axis; U / d and H / d are the crossing point's lateral and vertical offsets.  A point exactly on the plane belongs
 * to the upwind side: a track that goes through the plane is counted once, whichever of its points lie on the plane, and
 * a move along the plane is not counted.  A NaN in xt, yt, ax or ay never crosses; a NaN or negative reach never hits.
 *
 * Outputs, accumulated like ssrs_rotor_encounters':
 *   hits       ssrs_turbine_encounters' bitmap (ntracks, ceil(nturb / 32)), ORed: bit t of row j is set iff track j has
 *              a transit of turbine t.  ssrs_turbine_encounter_counts serves it unchanged
 *   transits   uint64 (nturb, 2), ADDED to: column 0 with the wind, column 1 against the wind
 *
 * The cull.  bin_start / bin_items are ssrs_turbine_encounters' lists (bins of SSRS_TURBINE_BIN cells).  The bin of the
 * move's FIRST point decides which turbines are tested, so the caller builds the lists from reach_t + 1.5: a transit's
 * crossing point is within reach_t of the turbine in the plane, the first point within sqrt(2) of the crossing point, and
 * the 0.086 left over covers the rounding of the test.  A list that omits a turbine loses its transits; a list that names
 * it twice counts them twice.  Entries outside [0, nturb) are skipped.
 *
 *   traj, traj_offsets, alt, cellinfo   exactly what ssrs_rotor_encounters takes: int16 (row, col) pairs and int32
 *              heights above ground in mm, indexed alike, 4-byte aligned (read 16 bytes a lane when both are 16-byte
 *              aligned, point by point otherwise and at the chunk's ends); int64 offsets (ntracks + 1), the first need
 *              not be 0, equal consecutive offsets are an empty track; {climb, elev} int32 pairs per cell, 8-byte aligned
 *   turbines, reach, hub, axis          (nturb, 2) f64, (nturb) f64, (nturb) int32, (nturb, 2) f64
 *
 * One streaming pass of 8 bytes a point.  The common point costs one lookup in a bit-per-bin mask in LDS; only a move
 * whose first point lies in an occupied bin gathers the two elevations and walks the bin's list, and the plane test comes
 * first.  No global atomic per transit: a lane keeps one pending (2 * turbine + direction, count) and hands it to uint32
 * counters in the block's LDS when the key changes and at its end; the block adds its non-zero counters to `transits`
 * once, as 64-bit adds.  The LDS rule: mask (one bit per bin) and counters (8 bytes a turbine) share 60 KB of dynamic
 * LDS, sized by the call.  The mask stays while it has at most 8192 words (262 144 bins) and both fit; without it the
 * turbines [0, SSRS_ROTOR_TRANSIT_LDS_TURBINES) keep their counters in LDS and the hand-overs of the others go to
 * `transits` as 64-bit global adds, still one per change of key.  The result does not depend on any of it.
 * The chunk's first and last offset are read back first (the launch is sized from its points), so the call waits for
 * `stream` once.
 *
 * Argument errors are ssrs_rotor_encounters': NULL traj / traj_offsets / alt / cellinfo / turbines / reach / bin_start /
 * bin_items / hits, ntracks outside [0, 2^31), nturb outside [1, SSRS_TURBINE_MAX], rows / cols outside [1, 32767],
 * a misaligned traj, alt or cellinfo; and a NULL hub, axis or transits, a misaligned hub, axis or transits, an
 * mm_per_cell that is not finite and > 0 -> SSRS_ERR_INVALID before any GPU work.  ntracks == 0, or no points, returns
 * SSRS_OK and touches nothing. */
#define SSRS_ROTOR_TRANSIT_LDS_TURBINES 7680
int ssrs_rotor_transits(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks, const int32_t *alt,
                        const int32_t *cellinfo, int rows, int cols, const double *turbines, const double *reach,
                        const int32_t *hub, const double *axis, double mm_per_cell, int nturb,
                        const int32_t *bin_start, const int32_t *bin_items,
                        uint32_t *hits, uint64_t *transits, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SSRS_HIP_TRANSITS_H_ */
