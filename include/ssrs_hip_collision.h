/* ssrs_hip_collision.h -- collision risk per turbine of libssrs_hip.so (K19): a public header beside ssrs_hip.h,
 * ssrs_hip_passage.h and ssrs_hip_transits.h, whose conventions (caller-owned device memory, row-major rasters, `stream` a
 * hipStream_t passed as void*, SSRS_OK or a negative SSRS_ERR_* code with ssrs_last_error()) and error codes it shares.
 * The export is an addition to the library: SSRS_VERSION does not change with it. */
#ifndef SSRS_HIP_COLLISION_H_
#define SSRS_HIP_COLLISION_H_

#include "ssrs_hip_transits.h"

#ifdef __cplusplus
extern "C" {
#endif

/* K19 -- collision risk per turbine, direction and track: every transit of ssrs_rotor_transits (K18) weighted with the
 * single-transit collision probability of the place in the disk it goes through, looked up in a table the HOST makes
 * (Band's model, turbines.band_collision_table; the kernel evaluates no trigonometric function, sqrt or exp), and summed
 * exactly in 64-bit integers.  `hits` and `transits` come out exactly as ssrs_rotor_transits gives them, so a caller that
 * wants both makes this one pass.
 *
 * Definition.  A transit is ssrs_rotor_transits', unchanged: the same operations in the same order (ssrs_hip_transits.h),
 * so the same moves count, in the same direction dir.  The test's own two numbers are kept,
 *   lhs = U*U + H*H        rhs = (reach_t*reach_t) * (d*d)          (transit iff ... lhs <= rhs)
 * and lhs / rhs is the crossing point's squared distance from the hub over reach_t squared.  The disk is cut into
 * SSRS_COLLISION_RINGS = 256 rings of EQUAL AREA, ring k holding k/256 <= rho^2 / reach_t^2 < (k + 1)/256.  For a transit of
 * turbine t by a move of track j:
 *   k   = 0                                        if rhs == 0          (a zero reach, or a move along a degenerate axis)
 *       = 255                                      if !(lhs < rhs)      (on the rim: lhs == rhs)
 *       = min(255, (int)((lhs / rhs) * 256.0))     otherwise            (one IEEE division; the product is exact; truncation)
 *   if 0 <= cls[t] < nclass:
 *       q32 = table[(cls[t] * 2 + dir) * 256 + k]
 *       risk[2 t + dir] += q32            track_risk[j] += q32
 * A turbine whose class lies outside [0, nclass) (the host's -1: a NaN in one of its parameters) still counts in `hits`
 * and `transits` and adds nothing to `risk` and `track_risk`.  The sums are 64-bit integer adds of uint32 values: exact,
 * and independent of the launch order, the chunking, the alignment of the buffers and the LDS rule below.
 *
 *   cls        int32 (nturb): the turbine's row of `table`
 *   table      uint32 (nclass, 2, 256): the probability of a collision in one transit of ring k in direction dir (0 with
 *              the wind, 1 against it), in units of 2^-32: min(2^32 - 1, rint(p * 2^32)).  It stays in global memory: it is
 *              read once per transit, and transits are rare
 *   nclass     >= 1
 *   risk       uint64 (nturb, 2), ADDED to, units of 2^-32: column 0 with the wind, column 1 against the wind
 *   track_risk uint64 (ntracks), ADDED to, units of 2^-32; NULL = not wanted
 * Every other argument, the cull lists and their contract, and the outputs `hits` and `transits` are
 * ssrs_rotor_transits'.
 *
 * The pass is ssrs_rotor_transits' own walk with one more compile-time switch: 8 bytes a point, the bit-per-bin mask in
 * LDS for the common point, the plane test first, no cross-lane step, and no global atomic per transit.  A lane keeps one
 * pending (2 * turbine + direction, count, q32 sum) and hands it to the block's LDS counters -- the uint32 count and a
 * uint64 sum beside it -- when the key changes and at its end; the block adds its non-zero counters to `transits` and `risk`
 * once.  It also keeps one pending (track, q32 sum) and hands it to `track_risk` with one 64-bit global add when its track
 * changes and at its end.  The LDS rule: mask (one bit per bin, padded to an even number of words so that the sums are
 * 8-byte aligned) and counters (24 bytes a turbine: two uint32 counts, two uint64 sums) share the same 60 KB of dynamic
 * LDS as ssrs_rotor_transits, sized by the call: at 256 lanes a block that keeps two blocks a CU inside the 160 KB of a
 * gfx950 CU, and a typical call (a few hundred turbines) asks for a tenth of it.  The mask stays while it has at most 8192
 * words and both fit; without it the turbines [0, SSRS_ROTOR_COLLISION_LDS_TURBINES) keep their counters in LDS and the
 * hand-overs of the others go to `transits` and `risk` as 64-bit global adds, still one pair per change of key.  The
 * result does not depend on any of it.
 *
 * Argument errors are ssrs_rotor_transits'; and a NULL cls, table or risk, nclass < 1, a cls or table that is not
 * 4-byte aligned, a risk or track_risk that is not 8-byte aligned -> SSRS_ERR_INVALID before any GPU work.  ntracks == 0,
 * or no points, returns SSRS_OK and touches nothing.  Like ssrs_rotor_transits the call reads the chunk's first and
 * last offset back and so waits for `stream` once; its launch goes to `stream`. */
#define SSRS_COLLISION_RINGS 256
#define SSRS_ROTOR_COLLISION_LDS_TURBINES 2560
int ssrs_rotor_collision_risk(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks, const int32_t *alt,
                              const int32_t *cellinfo, int rows, int cols, const double *turbines, const double *reach,
                              const int32_t *hub, const double *axis, double mm_per_cell, int nturb,
                              const int32_t *bin_start, const int32_t *bin_items,
                              uint32_t *hits, uint64_t *transits,
                              const int32_t *cls, const uint32_t *table, int nclass, uint64_t *risk, uint64_t *track_risk,
                              void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SSRS_HIP_COLLISION_H_ */
