// The one statement of the rotor-disk test (include/ssrs_hip_transits.h "Definition", include/ssrs_hip_collision.h for the
// ring): K18 and K19 (rotor_transits.hip) and K20 (site_risk.hip) all call it.  Plain values in, no memory read: the caller
// decides where the turbine's numbers come from -- K18's arrays, K20's cell -- and what it loads only behind the plane test.
// Every product, sum and difference rounds on its own (__dmul_rn, __dadd_rn, __dsub_rn); the divisions are IEEE.
#pragma once
#include "common.h"
#include "../../include/ssrs_hip_collision.h"

namespace ssrs {

// what the plane test leaves for the disk test
struct RotorPlane {
    double dx0, dy0, dx1, dy1;     // the move's two ends from the turbine
    double s0, s1;                 // their signed distances along the axis
};

// The plane test of the move (r0, c0) -> (r1, c1) against a turbine at (xt, yt) with the axis (ax, ay): true iff the move
// crosses the plane.  A NaN in xt, yt, ax or ay never crosses.
__device__ __forceinline__ bool rotor_plane_test(double xt, double yt, double ax, double ay, int r0, int c0, int r1, int c1,
                                                 RotorPlane &p)
{
    p.dx0 = __dsub_rn(static_cast<double>(c0), xt), p.dy0 = __dsub_rn(static_cast<double>(r0), yt);
    p.dx1 = __dsub_rn(static_cast<double>(c1), xt), p.dy1 = __dsub_rn(static_cast<double>(r1), yt);
    p.s0 = __dadd_rn(__dmul_rn(ax, p.dx0), __dmul_rn(ay, p.dy0));
    p.s1 = __dadd_rn(__dmul_rn(ax, p.dx1), __dmul_rn(ay, p.dy1));
    return (p.s0 < 0.0) != (p.s1 < 0.0);
}

// The rest of the test for a move that crosses the plane: -1 for no transit, else the direction.  z0, z1: the ends'
// heights above the datum in mm; hub likewise.  kRing (K19, K20): `ring` gets the equal-area ring of the crossing point,
// from the two numbers the test compares.
template <bool kRing>
__device__ __forceinline__ int rotor_disk_test(const RotorPlane &p, double ax, double ay, double reach, long long hub,
                                               long long z0, long long z1, double mm_per_cell, int &ring)
{
    if (!(reach >= 0.0)) return -1;
    const double u0 = __dsub_rn(__dmul_rn(ax, p.dy0), __dmul_rn(ay, p.dx0));
    const double u1 = __dsub_rn(__dmul_rn(ax, p.dy1), __dmul_rn(ay, p.dx1));
    const double h0 = static_cast<double>(z0 - hub) / mm_per_cell;
    const double h1 = static_cast<double>(z1 - hub) / mm_per_cell;
    const double d = __dsub_rn(p.s0, p.s1);
    const double U = __dsub_rn(__dmul_rn(p.s0, u1), __dmul_rn(p.s1, u0));
    const double H = __dsub_rn(__dmul_rn(p.s0, h1), __dmul_rn(p.s1, h0));
    const double lhs = __dadd_rn(__dmul_rn(U, U), __dmul_rn(H, H));
    const double rhs = __dmul_rn(__dmul_rn(reach, reach), __dmul_rn(d, d));
    if (!(lhs <= rhs)) return -1;
    if constexpr (kRing) {
        if (rhs == 0.0) ring = 0;
        else if (!(lhs < rhs)) ring = SSRS_COLLISION_RINGS - 1;
        else {
            const int k = static_cast<int>((lhs / rhs) * static_cast<double>(SSRS_COLLISION_RINGS));
            ring = k < SSRS_COLLISION_RINGS - 1 ? k : SSRS_COLLISION_RINGS - 1;
        }
    }
    return p.s0 < 0.0 ? 1 : 0;
}

}  // namespace ssrs
