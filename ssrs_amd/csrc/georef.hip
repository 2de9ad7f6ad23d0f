// K10 -- a longitude / latitude raster onto the projected grid (the reference's get_raster_in_projected_crs,
// ssrs/raster.py:12-49, which goes through GDAL): per destination cell the exact Albers inverse of georef.h in f64
// and one bilinear gather from the source.  One streaming pass: a lane owns kWarpCells consecutive cells of a
// destination row and stores them at once; neighbouring lanes read neighbouring source pixels, straight from
// global memory (no LDS: a wave's footprint in the source is a few rows of a few hundred bytes).
#include <initializer_list>

#include "common.h"
#include "georef.h"
#include "interp.h"

namespace ssrs {

constexpr int kWarpCells = 4;

template <typename T>
struct alignas(kWarpCells * sizeof(T) > 16 ? 16 : kWarpCells * sizeof(T)) WarpPack {
    T v[kWarpCells];
};

// everything but the pointers, by value in the kernel arguments
struct WarpGeometry {
    SsrsProjection proj;
    double lon0, lat0, dlon, dlat, nodata;
    double west, south, res;
    int src_rows, src_cols, rows, cols;
};

// One source pixel as f64, or NaN when it is missing.  Called only for neighbours of non-zero weight.
template <typename Tsrc>
__device__ __forceinline__ double warp_pixel(const Tsrc *__restrict__ src, size_t k, double nodata)
{
    const double v = static_cast<double>(src[k]);
    return v == nodata ? quiet_nan() : v;
}

// The bilinear rule of include/ssrs_hip.h at (fr, fc); NaN when the cell is not covered or a neighbour it needs is
// missing.  i + 1 <= src_rows - 1 and j + 1 <= src_cols - 1 hold for every load below.
template <typename Tsrc>
__device__ __forceinline__ double warp_sample(const Tsrc *__restrict__ src, const WarpGeometry &g, double fr, double fc)
{
    if (!(fr >= 0.0 && fr <= static_cast<double>(g.src_rows - 1) && fc >= 0.0 && fc <= static_cast<double>(g.src_cols - 1)))
        return quiet_nan();
    int i = static_cast<int>(floor(fr)), j = static_cast<int>(floor(fc));
    i = i > g.src_rows - 2 ? g.src_rows - 2 : i;
    j = j > g.src_cols - 2 ? g.src_cols - 2 : j;
    const double tr = fr - static_cast<double>(i), tc = fc - static_cast<double>(j);
    const double ur = 1.0 - tr, uc = 1.0 - tc;
    const size_t k = static_cast<size_t>(i) * g.src_cols + j;
    const double z00 = ur != 0.0 && uc != 0.0 ? warp_pixel(src, k, g.nodata) : 0.0;
    const double z01 = ur != 0.0 && tc != 0.0 ? warp_pixel(src, k + 1, g.nodata) : 0.0;
    const double z10 = tr != 0.0 && uc != 0.0 ? warp_pixel(src, k + g.src_cols, g.nodata) : 0.0;
    const double z11 = tr != 0.0 && tc != 0.0 ? warp_pixel(src, k + g.src_cols + 1, g.nodata) : 0.0;
    return (z00 * uc + z01 * tc) * ur + (z10 * uc + z11 * tc) * tr;
}

template <typename T>
__device__ __forceinline__ void warp_store(T *__restrict__ out, const WarpPack<T> &w, size_t i0, int ncells, bool packed)
{
    if (packed) {
        *reinterpret_cast<WarpPack<T> *>(out + i0) = w;
    } else {
#pragma unroll
        for (int j = 0; j < kWarpCells; ++j)
            if (j < ncells) out[i0 + j] = w.v[j];
    }
}

// The loop is wave-granular (lanes past the end carry no cell) so that the ballots below see whole waves.
template <typename Tsrc, typename Tdst>
__global__ __launch_bounds__(kBlock) void k_warp_lonlat(WarpGeometry g, const Tsrc *__restrict__ src, Tdst *__restrict__ dst,
                                                        double *__restrict__ lon, double *__restrict__ lat,
                                                        unsigned long long *__restrict__ uncovered, int packed)
{
    const int per_row = (g.cols + kWarpCells - 1) / kWarpCells;
    const size_t ngroup = static_cast<size_t>(g.rows) * per_row;
    const int lane = threadIdx.x & 63;
    unsigned long long missing = 0;                                   // wave-uniform: cells of this wave that got NaN
    for (size_t base = blockIdx.x * static_cast<size_t>(kBlock) + (threadIdx.x - lane); base < ngroup;
         base += static_cast<size_t>(gridDim.x) * kBlock) {
        const size_t q = base + lane;
        const bool live = q < ngroup;
        const int r = live ? static_cast<int>(q / per_row) : 0, c0 = live ? static_cast<int>(q % per_row) * kWarpCells : 0;
        const size_t i0 = static_cast<size_t>(r) * g.cols + c0;
        const int ncells = live ? (g.cols - c0 < kWarpCells ? g.cols - c0 : kWarpCells) : 0;
        const double y = g.south + static_cast<double>(r) * g.res;
        WarpPack<double> wlon, wlat;
        WarpPack<Tdst> w;
#pragma unroll
        for (int j = 0; j < kWarpCells; ++j) {
            const double x = g.west + static_cast<double>(c0 + j) * g.res;
            albers_inverse(g.proj, x, y, wlon.v[j], wlat.v[j]);
            bool bad = false;
            if (dst) {
                double v = quiet_nan();
                if (j < ncells) v = warp_sample(src, g, (wlat.v[j] - g.lat0) / g.dlat, (wlon.v[j] - g.lon0) / g.dlon);
                bad = j < ncells && v != v;
                w.v[j] = static_cast<Tdst>(v);
            }
            missing += __popcll(__ballot(bad));
        }
        if (!live) continue;
        if (dst) warp_store(dst, w, i0, ncells, packed != 0);
        if (lon) warp_store(lon, wlon, i0, ncells, packed != 0);
        if (lat) warp_store(lat, wlat, i0, ncells, packed != 0);
    }
    if (uncovered && lane == 0 && missing != 0) atomicAdd(uncovered, missing);
}

template <typename Tsrc, typename Tdst>
static void launch_warp(const WarpGeometry &g, const void *src, void *dst, double *lon, double *lat,
                        unsigned long long *uncovered, hipStream_t st)
{
    const size_t ngroup = static_cast<size_t>(g.rows) * ((g.cols + kWarpCells - 1) / kWarpCells);
    // whole lanes' worth of cells per row and 16-byte aligned bases: one 16-byte store per lane (f32), two (f64)
    const auto aligned = [](const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
    const int packed = g.cols % kWarpCells == 0 && aligned(dst) && aligned(lon) && aligned(lat);
    hipLaunchKernelGGL((k_warp_lonlat<Tsrc, Tdst>), dim3(stream_grid(ngroup)), dim3(kBlock), 0, st, g,
                       static_cast<const Tsrc *>(src), static_cast<Tdst *>(dst), lon, lat, uncovered, packed);
}

static inline bool finite_all(std::initializer_list<double> vals)
{
    for (double v : vals)
        if (!albers_finite(v)) return false;
    return true;
}

}  // namespace ssrs

using namespace ssrs;

extern "C" int ssrs_projection_init_albers(SsrsProjection *proj)
{
    SSRS_REQUIRE(proj, "ssrs_projection_init_albers: proj is NULL");
    SSRS_REQUIRE(finite_all({proj->a, proj->e2, proj->lat_1, proj->lat_2, proj->lat_0, proj->lon_0, proj->x_0, proj->y_0}),
                 "ssrs_projection_init_albers: a non-finite field");
    SSRS_REQUIRE(proj->a > 0.0, "ssrs_projection_init_albers: a = %g must be > 0", proj->a);
    SSRS_REQUIRE(proj->e2 > 0.0 && proj->e2 < 1.0, "ssrs_projection_init_albers: e2 = %g must lie in (0, 1)", proj->e2);
    SSRS_REQUIRE(albers_init(proj),
                 "ssrs_projection_init_albers: lat_1 = %g, lat_2 = %g give no cone (|n| < 1e-12: lat_1 = -lat_2 is the "
                 "cylindrical limit)", proj->lat_1, proj->lat_2);
    return SSRS_OK;
}

extern "C" int ssrs_warp_lonlat_raster(const void *src, int src_type, int src_rows, int src_cols, double lon0, double lat0,
                                       double dlon, double dlat, double nodata, const SsrsProjection *proj, double west,
                                       double south, double res, void *dst, int dst_type, double *lon, double *lat,
                                       unsigned long long *uncovered, int rows, int cols, void *stream)
{
    SSRS_REQUIRE(proj, "ssrs_warp_lonlat_raster: proj is NULL");
    SSRS_REQUIRE(dst || lon || lat, "ssrs_warp_lonlat_raster: dst, lon and lat are all NULL");
    SSRS_REQUIRE(src || !dst, "ssrs_warp_lonlat_raster: src is NULL but dst is asked for");
    SSRS_REQUIRE(rows >= 1 && rows <= 32767 && cols >= 1 && cols <= 32767,
                 "ssrs_warp_lonlat_raster: rows = %d, cols = %d must lie in [1, 32767]", rows, cols);
    SSRS_REQUIRE(src_rows >= 2 && src_cols >= 2, "ssrs_warp_lonlat_raster: the source is %d x %d, it needs 2 x 2 pixels",
                 src_rows, src_cols);
    SSRS_REQUIRE(finite_all({lon0, lat0, dlon, dlat, west, south, res}) && !std::isinf(nodata),
                 "ssrs_warp_lonlat_raster: a non-finite argument");
    SSRS_REQUIRE(dlon != 0.0 && dlat != 0.0, "ssrs_warp_lonlat_raster: dlon and dlat must not be 0");
    SSRS_REQUIRE(res > 0.0, "ssrs_warp_lonlat_raster: res = %g must be > 0", res);
    SSRS_REQUIRE((src_type == SSRS_F32 || src_type == SSRS_F64) && (dst_type == SSRS_F32 || dst_type == SSRS_F64),
                 "ssrs_warp_lonlat_raster: src_type and dst_type must be SSRS_F32 or SSRS_F64");
    SsrsProjection check = *proj;
    SSRS_REQUIRE(albers_init(&check) && check.n == proj->n && check.C == proj->C && check.rho0 == proj->rho0 &&
                     check.e == proj->e,
                 "ssrs_warp_lonlat_raster: proj was not initialised by ssrs_projection_init_albers");
    const WarpGeometry g{*proj, lon0, lat0, dlon, dlat, nodata, west, south, res, src_rows, src_cols, rows, cols};
    hipStream_t st = as_stream(stream);
    if (src_type == SSRS_F32 && dst_type == SSRS_F32)
        launch_warp<float, float>(g, src, dst, lon, lat, uncovered, st);
    else if (src_type == SSRS_F32)
        launch_warp<float, double>(g, src, dst, lon, lat, uncovered, st);
    else if (dst_type == SSRS_F32)
        launch_warp<double, float>(g, src, dst, lon, lat, uncovered, st);
    else
        launch_warp<double, double>(g, src, dst, lon, lat, uncovered, st);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}
