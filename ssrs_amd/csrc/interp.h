// Per-cell evaluation of scipy griddata's three methods on the device, shared by the wind kernels (raster.hip) and
// the scalar / WTK thermal kernels (wtk_thermals.hip), and the host-side launchers of the geometry kernels that
// raster.hip owns (cell ownership, Clough-Tocher ordinates).  Every helper is the expression the wind kernels have
// always evaluated, in the same order: the library is built with -ffp-contract=off, so a caller of these helpers gets
// the same bits wherever it sits.
#pragma once
#include "common.h"

namespace ssrs {

constexpr int kCT = 19;                       // Bezier ordinates of one Clough-Tocher macro-triangle and field
constexpr int32_t kNoOwner = 0x7f7f7f7f;      // owner raster: outside the hull (hipMemsetAsync 0x7f)

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

// barycentric coordinates of the centre of cell (r, c) in the triangle whose transform is T = [T00 T01; T10 T11; r0 r1]
// (scipy.spatial.Delaunay.transform)
__device__ __forceinline__ void tri_barycentric(const double *__restrict__ T, int r, int c, double cell, double &b0,
                                                double &b1, double &b2)
{
    const double dx = static_cast<double>(c) * cell - T[4], dy = static_cast<double>(r) * cell - T[5];
    b0 = T[0] * dx + T[1] * dy;
    b1 = T[2] * dx + T[3] * dy;
    b2 = 1.0 - b0 - b1;
}

// LinearNDInterpolator on one field (left to right, as scipy sums them)
__device__ __forceinline__ double tri_linear(double b0, double b1, double b2, const double *__restrict__ val, int32_t v0,
                                             int32_t v1, int32_t v2)
{
    return b0 * val[v0] + b1 * val[v1] + b2 * val[v2];
}

// the 19 monomials of the four shifted barycentric coordinates (scipy's _clough_tocher_2d_single), in the order of
// k_ct_coefficients' ordinates
__device__ __forceinline__ void ct_monomials(double b0, double b1, double b2, double (&mono)[kCT])
{
    const double m = fmin(b0, fmin(b1, b2));
    const double a1 = b0 - m, a2 = b1 - m, a3 = b2 - m, a4 = 3 * m;
    const double a11 = a1 * a1, a22 = a2 * a2, a33 = a3 * a3, a44 = a4 * a4;
    mono[0] = a11 * a1;       mono[1] = 3 * a11 * a2;   mono[2] = 3 * a11 * a3;       mono[3] = 3 * a11 * a4;
    mono[4] = 3 * a1 * a22;   mono[5] = 6 * a1 * a2 * a4; mono[6] = 3 * a1 * a33;     mono[7] = 6 * a1 * a3 * a4;
    mono[8] = 3 * a1 * a44;   mono[9] = a22 * a2;       mono[10] = 3 * a22 * a3;      mono[11] = 3 * a22 * a4;
    mono[12] = 3 * a2 * a33;  mono[13] = 6 * a2 * a3 * a4; mono[14] = 3 * a2 * a44;   mono[15] = a33 * a3;
    mono[16] = 3 * a33 * a4;  mono[17] = 3 * a3 * a44;  mono[18] = a44 * a4;
}

// CloughTocher2DInterpolator on one field: cf = its 19 ordinates in the owner triangle
__device__ __forceinline__ double ct_eval(const double (&mono)[kCT], const double *__restrict__ cf)
{
    double v = mono[0] * cf[0];
#pragma unroll
    for (int k = 1; k < kCT; ++k) v += mono[k] * cf[k];
    return v;
}

static inline size_t align256(size_t n) { return (n + 255) / 256 * 256; }

// blocks of a grid-stride launch over `nthreads_needed` work items (common.h: kMaxStreamBlocks)
static inline int stream_grid(size_t nthreads_needed)
{
    size_t b = (nthreads_needed + kBlock - 1) / kBlock;
    if (b < 1) b = 1;
    if (b > static_cast<size_t>(kMaxStreamBlocks)) b = kMaxStreamBlocks;
    return static_cast<int>(b);
}

// owner (rows, cols) int32: per cell the lowest index of a triangle that contains its centre by scipy's test (eps =
// 100 DBL_EPSILON), kNoOwner outside the hull.  Asynchronous on st.
int launch_tri_owner(const double *points, const int32_t *triangles, const double *transform, int ntri, double cell,
                     int rows, int cols, int32_t *owner, hipStream_t st);

// coef [triangle][nfield][19]: field f reads its samples at (f & 1 ? val_odd : val_even) + (f >> 1) * pair_stride and
// its vertex gradients at (f & 1 ? grad_odd : grad_even) + (f >> 1) * pair_stride * 2.  The wind call passes east /
// north with pair_stride = npts; consecutive fields of one (nfield, npts) array are val, val + npts, 2 * npts.
int launch_ct_coefficients(const double *points, const int32_t *triangles, const int32_t *neighbors,
                           const double *transform, const double *val_even, const double *val_odd,
                           const double *grad_even, const double *grad_odd, size_t pair_stride, int ntri, int nfield,
                           double *coef, hipStream_t st);

}  // namespace ssrs
