/* ssrs_hip_sites.h -- the site collision-risk map of libssrs_hip.so (K20): a public header beside ssrs_hip.h,
 * ssrs_hip_passage.h, ssrs_hip_transits.h and ssrs_hip_collision.h, whose conventions (caller-owned device memory,
 * row-major rasters, `stream` a hipStream_t passed as void*, SSRS_OK or a negative SSRS_ERR_* code with
 * ssrs_last_error()) and error codes it shares.  The export is an addition to the library: SSRS_VERSION does not change
 * with it. */
#ifndef SSRS_HIP_SITES_H_
#define SSRS_HIP_SITES_H_

#include "ssrs_hip_collision.h"

#ifdef __cplusplus
extern "C" {
#endif

/* K20 -- the collision risk of ONE candidate turbine class standing on EVERY cell of the raster: K19 turned inside out,
 * for the siting question "where would a turbine of this class do the least harm?".  The result is what
 * ssrs_rotor_collision_risk would give for rows x cols turbines of class 0 on the cell centres (its nturb stops at
 * SSRS_TURBINE_MAX; this call has no such limit), in `transits` and `risk`; there is no bitmap and no per-track sum.
 *
 * Definition.  A SITE is a cell (r, c) of the raster.  Its turbine is
 *   (xt, yt)   = ((double)c, (double)r)
 *   reach_t    = reach                                             f64, cells, one scalar for all sites
 *   hub_t      = clip_int32((int64)elev[r, c] + hub_mm)            elev: cellinfo's second plane, mm above the datum
 *   (ax_t, ay_t) = axis[2 (r cols + c)], axis[2 (r cols + c) + 1]  if axis_per_cell != 0, else axis[0], axis[1]
 * and a site whose elev is INT32_MIN (nodata) is transited by nothing.  For every TESTABLE move of every track
 * (ssrs_hip_transits.h: both ends inside the raster, neither on nodata, max(|r1 - r0|, |c1 - c0|) <= 1) and every site:
 *   the transit test is ssrs_rotor_transits', the same operations in the same order, giving the direction dir;
 *   the ring k is ssrs_rotor_collision_risk's, from the test's own lhs and rhs;
 *   on a transit:   transits[2 (r cols + c) + dir] += 1      risk[2 (r cols + c) + dir] += table[dir * 256 + k]
 * The sums are 64-bit integer adds: exact, and independent of the launch order, the chunking and the alignment of the
 * buffers.
 *
 *   traj, traj_offsets, alt, cellinfo, mm_per_cell   exactly what ssrs_rotor_transits takes
 *   reach      0 .. SSRS_SITE_MAX_REACH cells
 *   hub_mm     the hub's height above the ground of its cell, mm
 *   axis       f64: (rows, cols, 2) if axis_per_cell != 0 (16 bytes a cell), else 2 values.  The upwind unit step along
 *              +col and +row, made by the host; a NaN axis never crosses, nor does a zero axis
 *   table      uint32 (2, 256): ONE class's rows of ssrs_rotor_collision_risk's table, [with the wind, against the wind]
 *   transits   uint64 (rows, cols, 2), ADDED to; NULL = not wanted
 *   risk       uint64 (rows, cols, 2), ADDED to, units of 2^-32
 *
 * The window.  A move is tested against the sites with |r - r0| <= W and |c - c0| <= W, clipped to the raster, where
 * (r0, c0) is the move's FIRST point and W = (int)floor(reach + 1.5).  Proof (ssrs_rotor_transits' cull proof with integer
 * site coordinates): on a transit the crossing point lies within reach of the hub in the disk's plane, so its horizontal
 * distance from (c, r) is at most reach; the first point lies on the move's segment, whose length is at most sqrt(2), so
 * it is within sqrt(2) of the crossing point; hence the first point is within reach + 1.4143 of the site, and the 0.0857
 * left to reach + 1.5 covers the rounding of the test, as there.  |r - r0| and |c - c0| are
 * integers below reach + 1.5, so they are at most floor(reach + 1.5) = W.  No pair the definition accepts lies outside the
 * window; inside it every site is tested, the plane test first.
 *
 * The pass.  One launch; a block takes a tile of 2048 consecutive points of the chunk, a lane eight of them and the one
 * behind (16-byte loads when traj and alt are 16-byte aligned, point by point otherwise and at the chunk's ends).  Every
 * point is looked at as the first point of a move: there is no occupied-bin mask, every cell is a site.  The tile's first
 * and last track come from two binary searches of the offsets, every lane searches between them and walks the offsets
 * from there (ssrs_track_time's way).  The 2 KB of `table` are staged in LDS; a transit goes to `transits` and `risk` as
 * two 64-bit global adds (a table of sites in LDS in front of them was measured and did not pay:
 * profiles/site_collision_risk.md).
 * The chunk's first and last offset are read back first (the launch is sized from its points), so the call waits for
 * `stream` once.
 *
 * Errors, all SSRS_ERR_INVALID before any GPU work: a NULL traj, traj_offsets, alt, cellinfo, axis, table or risk;
 * ntracks outside [0, 2^31); rows or cols outside [1, 32767]; a traj, alt or table that is not 4-byte aligned, a cellinfo,
 * axis, transits or risk that is not 8-byte aligned; an mm_per_cell that is not finite and > 0;
 * reach > SSRS_SITE_MAX_REACH.  A NaN or negative reach returns SSRS_OK and touches nothing (nothing transits such a
 * turbine); so does ntracks == 0, or no points. */
#define SSRS_SITE_MAX_REACH 62.0          /* cells */
int ssrs_site_collision_risk(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks, const int32_t *alt,
                             const int32_t *cellinfo, int rows, int cols, double reach, int hub_mm,
                             const double *axis, int axis_per_cell, double mm_per_cell, const uint32_t *table,
                             uint64_t *transits, uint64_t *risk, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SSRS_HIP_SITES_H_ */
