// Device arithmetic shared by the raster kernels (raster.hip: K1, shelter.hip: K9): the thresholded
// updraft, the reciprocal square root and the degree-argument sine / cosine.  One definition, so that
// kernels which promise equal bits evaluate the very same expressions.
#pragma once
#include "common.h"

namespace ssrs {

constexpr double kPi = 3.141592653589793;  // np.pi

// ----------------------------------------------------------------------------
// XCD-aware tile order: blocks are dealt round-robin over the 8 XCDs, so give
// block b the tile (b % 8) * ceil(n/8) + b / 8 (bijective form): each XCD then
// walks one contiguous band of tiles and finds its halo rows in its own L2.
__device__ __forceinline__ int xcd_tile(int b, int n)
{
    const int q = n / 8, r = n % 8, x = b % 8, j = b / 8;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;
}

// layers.py:171-185 on one value already rounded to f32 and widened again
__device__ __forceinline__ double usable_updraft(double v, double thr, double em1)
{
    double f = 0.0;
    if (v > 1e-02) {
        if (v > thr) {
            f = v;
        } else {
            const double y = v / thr;
            const double y2 = y * y;
            const double y5 = (y2 * y2) * y;       // (v/thr)**5
            f = thr * (exp(y5) - 1.0) / em1;       // em1 = e - 1 (host libm)
        }
    }
    return f;
}

// Thresholded updraft with the two divisions folded into host constants
// (v / thr -> v * inv_thr, . / (e - 1) -> . * scale) and exp(x) - 1 on x = (v/thr)^5 in (0, 1] as
// its Taylor polynomial to x^17 (truncation 1.6e-16 relative; libm's exp(x) - 1 carries 1.1e-16
// ABSOLUTE, so the two agree to 1e-16 absolute and the polynomial is the more accurate one for
// small x): 17 fused multiply-adds instead of ocml's exp (range reduction, ldexp and three
// branches).  Inside the rtol 1e-12 / atol 1e-15 the tests state.
__device__ __forceinline__ double expm1_unit(double x)
{
    constexpr double c[17] = {
        1.00000000000000000e+00,
        5.00000000000000000e-01,
        1.66666666666666657e-01,
        4.16666666666666644e-02,
        8.33333333333333322e-03,
        1.38888888888888894e-03,
        1.98412698412698413e-04,
        2.48015873015873016e-05,
        2.75573192239858925e-06,
        2.75573192239858883e-07,
        2.50521083854417202e-08,
        2.08767569878681002e-09,
        1.60590438368216133e-10,
        1.14707455977297245e-11,
        7.64716373181981641e-13,
        4.77947733238738525e-14,
        2.81145725434552060e-15};
    double p = c[16];
#pragma unroll
    for (int k = 15; k >= 0; --k) p = __builtin_fma(p, x, c[k]);
    return x * p;
}

__device__ __forceinline__ double usable_updraft_fast(double v, double thr, double inv_thr,
                                                      double scale)
{
    double f = 0.0;
    if (v > 1e-02) {
        if (v > thr) {
            f = v;
        } else {
            const double y = v * inv_thr;
            const double y2 = y * y;
            f = scale * expm1_unit((y2 * y2) * y);          // thr (exp((v/thr)^5) - 1) / (e - 1)
        }
    }
    return f;
}

// 1 / sqrt(s) for a normal positive s: the hardware estimate and two Newton steps (ocml's rsqrt
// adds scaling for denormals and special cases these sums of squares never need)
__device__ __forceinline__ double rsqrt_pos(double s)
{
    double r = __builtin_amdgcn_rsq(s);
    const double h = 0.5 * s;
#pragma unroll
    for (int k = 0; k < 2; ++k) r = r * __builtin_fma(-h, r * r, 1.5);
    return r;
}

// sin / cos of an angle given in DEGREES.  The reference converts to radians
// first ((a - w) * pi / 180, two roundings) and calls libm; ocml's f64 sin/cos
// carry a Payne-Hanek path these bounded arguments never need and made
// k_orographic ALU-bound (170-180 us at C2).  Here the quadrant is removed
// exactly in degrees (x - 90 k is exact for |x| < 2^52), the remainder
// |r| <= 45 deg goes through the classic minimax kernels on [-pi/4, pi/4]
// (fdlibm k_sin / k_cos coefficients, < 1-2 ulp).  Result within ~1e-15 of the
// reference's value, far inside the 1-f32-ulp tolerance of the orograph.
__device__ __forceinline__ void sincos_deg(double x, double &sn, double &cs)
{
    const double kq = rint(x * (1.0 / 90.0));
    const double r = x - 90.0 * kq;                    // exact
    const double t = r * (kPi / 180.0);
    const double z = t * t;
    const double ps = -1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 +
                      z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10))));
    const double pc = 4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 +
                      z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11))));
    const double s0 = t + (t * z) * ps;
    const double c0 = 1.0 - (0.5 * z - (z * z) * pc);
    const int q = static_cast<int>(kq) & 3;
    sn = (q == 0) ? s0 : (q == 1) ? c0 : (q == 2) ? -s0 : -c0;
    cs = (q == 0) ? c0 : (q == 1) ? -s0 : (q == 2) ? -c0 : s0;
}

}  // namespace ssrs
