// K10 -- Albers Equal Area Conic on an ellipsoid (Snyder, USGS PP 1395, eqs. 14-12 ... 14-21, 3-12, 3-16): the scalar
// arithmetic that the host (ssrs_projection_init_albers), the warp kernel (georef.hip) and the NumPy restatement
// (ssrs_amd/georef.py) share, expression by expression and in the same order.  No HIP runtime here: tests/
// georef_driver.cpp includes this header in a plain C++ program.  The library is built with -ffp-contract=off, so the
// device evaluates the operations below one by one, as a CPU does.
#pragma once
#include <cmath>

#include "../../include/ssrs_hip.h"

#ifndef SSRS_HD
#if defined(__HIP__) || defined(__HIPCC__)
#define SSRS_HD __host__ __device__
#else
#define SSRS_HD
#endif
#endif

namespace ssrs {

// Iterations of eq. 3-16 for the latitude, fixed: one more than the smallest count that holds the round trip
// inverse(forward(.)) within 1e-11 degrees (tests/test_georef_host.py measures it: 2 iterations leave 6.4e-9 degrees,
// 3 leave 1.4e-13 and 4 leave 1.1e-13, which is the rounding of the formulas themselves).
constexpr int kAlbersIterations = 4;

constexpr double kDegToRad = 3.14159265358979323846 / 180.0;
constexpr double kRadToDeg = 180.0 / 3.14159265358979323846;

// eq. 3-12
SSRS_HD inline double albers_q(double e2, double e, double sinphi)
{
    const double es = e * sinphi;
    return (1.0 - e2) * (sinphi / (1.0 - e2 * (sinphi * sinphi)) - (1.0 / (2.0 * e)) * log((1.0 - es) / (1.0 + es)));
}

// eq. 14-15
SSRS_HD inline double albers_m(double e2, double sinphi, double cosphi)
{
    return cosphi / sqrt(1.0 - e2 * (sinphi * sinphi));
}

SSRS_HD inline bool albers_finite(double v) { return v - v == 0.0; }

// Fills n, C, rho0, e from the inputs; false (nothing usable written) when the inputs do not define a cone.
SSRS_HD inline bool albers_init(SsrsProjection *p)
{
    const double in[8] = {p->a, p->e2, p->lat_1, p->lat_2, p->lat_0, p->lon_0, p->x_0, p->y_0};
    for (int k = 0; k < 8; ++k)
        if (!albers_finite(in[k])) return false;
    if (!(p->a > 0.0) || !(p->e2 > 0.0 && p->e2 < 1.0)) return false;
    const double e = sqrt(p->e2);
    const double phi1 = p->lat_1 * kDegToRad, phi2 = p->lat_2 * kDegToRad, phi0 = p->lat_0 * kDegToRad;
    const double s1 = sin(phi1), s2 = sin(phi2), s0 = sin(phi0);
    const double m1 = albers_m(p->e2, s1, cos(phi1)), m2 = albers_m(p->e2, s2, cos(phi2));
    const double q1 = albers_q(p->e2, e, s1), q2 = albers_q(p->e2, e, s2), q0 = albers_q(p->e2, e, s0);
    // eq. 14-14; one standard parallel (q2 == q1) is its limit sin(lat_1)
    const double n = q2 != q1 ? (m1 * m1 - m2 * m2) / (q2 - q1) : s1;
    if (!albers_finite(n) || fabs(n) < 1e-12) return false;
    const double C = m1 * m1 + n * q1;
    const double rho0 = p->a * sqrt(C - n * q0) / n;
    if (!albers_finite(C) || !albers_finite(rho0)) return false;
    p->e = e;
    p->n = n;
    p->C = C;
    p->rho0 = rho0;
    return true;
}

// eqs. 14-1 ... 14-4, 14-12: degrees -> metres
SSRS_HD inline void albers_forward(const SsrsProjection &p, double lon, double lat, double &x, double &y)
{
    const double phi = lat * kDegToRad;
    const double rho = p.a * sqrt(p.C - p.n * albers_q(p.e2, p.e, sin(phi))) / p.n;
    const double theta = p.n * ((lon - p.lon_0) * kDegToRad);
    x = p.x_0 + rho * sin(theta);
    y = p.y_0 + p.rho0 - rho * cos(theta);
}

// eqs. 14-9 ... 14-11, 14-19, 3-16: metres -> degrees.  A point the cone does not reach comes back with whatever
// the clamped arcsine and the iteration make of it (possibly NaN); the warp kernel then finds it outside the source.
SSRS_HD inline void albers_inverse(const SsrsProjection &p, double x, double y, double &lon, double &lat)
{
    double X = x - p.x_0;
    double Y = p.rho0 - (y - p.y_0);
    const double rho = sqrt(X * X + Y * Y);
    if (p.n < 0.0) {
        X = -X;
        Y = -Y;
    }
    const double theta = atan2(X, Y);
    const double rn = rho * p.n / p.a;
    const double qv = (p.C - rn * rn) / p.n;
    lon = p.lon_0 + (theta / p.n) * kRadToDeg;
    double h = qv / 2.0;
    h = h > 1.0 ? 1.0 : (h < -1.0 ? -1.0 : h);
    double phi = asin(h);
    const double qe = qv / (1.0 - p.e2), inv2e = 1.0 / (2.0 * p.e);
#pragma unroll
    for (int it = 0; it < kAlbersIterations; ++it) {
        const double s = sin(phi), c = cos(phi);
        const double es = p.e * s;
        const double w = 1.0 - p.e2 * (s * s);
        phi = phi + (w * w) / (2.0 * c) * (qe - s / w + inv2e * log((1.0 - es) / (1.0 + es)));
    }
    lat = phi * kRadToDeg;
}

}  // namespace ssrs
