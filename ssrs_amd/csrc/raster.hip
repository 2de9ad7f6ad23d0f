// K1 -- updraft raster kernels for gfx950 (MI355X).
//
// Reference semantics (paths relative to /root/reference):
//   ssrs/layers.py:11-22    compute_orographic_updraft
//   ssrs/layers.py:63-128   compute_slope_degrees / compute_aspect_degrees
//   ssrs/layers.py:171-185  get_above_threshold_speed
//   ssrs/simulator.py:189-243  orographic -> np.save(f32) -> load -> threshold
//
// All arithmetic is f64 like the reference; the kernels are HBM-streaming:
//   k_orographic       12 B/cell (f32 slope+aspect in, f32 out), +8 B if the
//                      thresholded f64 raster is also written; batched over B
//                      wind cases so the terrain is read once ((8+12B)/B B)
//   k_updraft_from_dem 8..12 B/cell: DEM tile (+1-cell halo) staged in LDS,
//                      Horn gradients -> updraft with no trig at all
// Built with -ffp-contract=off (see build.py).
#include "common.h"
#include "interp.h"
#include "raster_math.h"

namespace ssrs {

// ---------------------------------------------------------------------------
// DEM tile staging: TW x TH outputs per block, (TW+2) x (TH+2) f64 in LDS.
constexpr int TW = 64;          // one wave spans a tile row: 512 B coalesced
constexpr int TH = 32;
constexpr int LW = TW + 2;
constexpr int LH = TH + 2;

template <typename T>
__device__ __forceinline__ void stage_dem_tile(const T *__restrict__ dem, int rows,
                                               int cols, int r0, int c0,
                                               double *__restrict__ tile)
{
    for (int i = threadIdx.x; i < LW * LH; i += kBlock) {
        const int lr = i / LW, lc = i - lr * LW;
        int gr = r0 - 1 + lr, gc = c0 - 1 + lc;
        gr = gr < 0 ? 0 : (gr >= rows ? rows - 1 : gr);   // clamped cells are only
        gc = gc < 0 ? 0 : (gc >= cols ? cols - 1 : gc);   // read by border outputs
        tile[i] = static_cast<double>(dem[static_cast<size_t>(gr) * cols + gc]);
    }
    __syncthreads();
}

// Horn gradients exactly in the reference's operand order (layers.py:78-90);
// "x" is the ROW axis and "y" the COLUMN axis there.
__device__ __forceinline__ void horn(const double *__restrict__ t, int lr, int lc,
                                     double res, double &dzdx, double &dzdy)
{
    const double *m = t + (lr - 1) * LW + lc;
    const double *z = t + lr * LW + lc;
    const double *p = t + (lr + 1) * LW + lc;
    const double z1 = m[1], z2 = z[1], z3 = p[1];
    const double z4 = m[0], z6 = p[0];
    const double z7 = m[-1], z8 = z[-1], z9 = p[-1];
    const double d = 8 * res;
    dzdx = ((z3 + 2 * z6 + z9) - (z1 + 2 * z4 + z7)) / d;
    dzdy = ((z1 + 2 * z2 + z3) - (z7 + 2 * z8 + z9)) / d;
}

template <typename Tin, typename Tout>
__global__ __launch_bounds__(kBlock) void k_slope_aspect(
    const Tin *__restrict__ dem, double res, Tout *__restrict__ slope,
    Tout *__restrict__ aspect, int rows, int cols, int tiles_x, int ntiles)
{
    __shared__ double tile[LW * LH];
    const int t = xcd_tile(blockIdx.x, ntiles);
    const int r0 = (t / tiles_x) * TH, c0 = (t % tiles_x) * TW;
    stage_dem_tile(dem, rows, cols, r0, c0, tile);
    const int lc = threadIdx.x % TW + 1;
    const int c = c0 + lc - 1;
    if (c >= cols) return;
    const double r2d = 180.0 / kPi;
    for (int lr = threadIdx.x / TW + 1; lr <= TH; lr += kBlock / TW) {
        const int r = r0 + lr - 1;
        if (r >= rows) break;
        double s = 0.0, a = 0.0;
        if (r > 0 && c > 0 && r < rows - 1 && c < cols - 1) {
            double dzdx, dzdy;
            horn(tile, lr, lc, res, dzdx, dzdy);
            s = atan(sqrt(dzdx * dzdx + dzdy * dzdy)) * r2d;   // np.degrees
            const double dx = dzdx == 0.0 ? 1e-10 : dzdx;
            const double ang = atan(dzdy / dx) * r2d;
            a = 180.0 - ang + 90.0 * (dx / fabs(dx));
            // a nodata (NaN) elevation in the stencil: the reference closes with np.nan_to_num
            // (layers.py:93, :128), so both layers are 0 there (+-inf elevations: out of scope)
            s = s != s ? 0.0 : s;
            a = a != a ? 0.0 : a;
        }
        const size_t i = static_cast<size_t>(r) * cols + c;
        if (slope) slope[i] = static_cast<Tout>(s);
        if (aspect) aspect[i] = static_cast<Tout>(a);
    }
}

struct FusedArgs {
    double d, d2;             // 8 res and its square
    double wspeed, cos_w, sin_w, min_val;
    double thr, inv_thr, scale;
};

template <typename Tin>
__global__ __launch_bounds__(kBlock) void k_updraft_from_dem(
    const Tin *__restrict__ dem, FusedArgs fa, float *__restrict__ orograph,
    double *__restrict__ usable, int rows, int cols, int tiles_x, int ntiles)
{
    __shared__ double tile[LW * LH];
    const int t = xcd_tile(blockIdx.x, ntiles);
    const int r0 = (t / tiles_x) * TH, c0 = (t % tiles_x) * TW;
    stage_dem_tile(dem, rows, cols, r0, c0, tile);
    const int lc = threadIdx.x % TW + 1;
    const int c = c0 + lc - 1;
    if (c >= cols) return;
    // each wave owns TH/4 consecutive rows of the tile and slides a 3 x 3 window
    // down its column: 3 new LDS reads per cell instead of 8
    constexpr int kRowsPerWave = TH / (kBlock / TW);
    const int lr0 = (threadIdx.x / TW) * kRowsPerWave + 1;
    const double *q = tile + (lr0 - 1) * LW + lc;
    double m_l = q[-1], m_c = q[0], m_r = q[1];               // row lr - 1
    double z_l = q[LW - 1], z_c = q[LW], z_r = q[LW + 1];     // row lr
    for (int lr = lr0; lr < lr0 + kRowsPerWave; ++lr) {
        const int r = r0 + lr - 1;
        if (r >= rows) break;
        const double *p = tile + (lr + 1) * LW + lc;
        const double p_l = p[-1], p_c = p[0], p_r = p[1];     // row lr + 1
        double w = 0.0;
        if (r > 0 && c > 0 && r < rows - 1 && c < cols - 1) {
            // un-normalised Horn sums X = 8 res dz_dx, Y = 8 res dz_dy in the
            // reference's operand order (layers.py:78-90; "x" = row axis)
            const double X = (p_r + 2 * p_c + p_l) - (m_r + 2 * m_c + m_l);
            const double Y = (m_r + 2 * z_r + p_r) - (m_l + 2 * z_l + p_l);
            if (X != 0.0) {
                // sin(slope) cos(aspect - wdirn) = -(dz_dy cos w + dz_dx sin w) / sqrt(1 + g^2)
                //                                 = -(Y cos w + X sin w) / sqrt(d^2 + X^2 + Y^2)
                // (sin(atan g) = g / sqrt(1 + g^2); cos(aspect - w) from aspect =
                //  180 - atan(dz_dy/dz_dx) + 90 sign(dz_dx)): no trig, no division.
                const double P = -(Y * fa.cos_w + X * fa.sin_w);
                if (P > 0.0) w = fa.wspeed * (P * rsqrt_pos(fa.d2 + (X * X + Y * Y)));
            } else {
                // dz_dx == 0: the reference substitutes 1e-10 for the aspect only
                // (layers.py:124) -- rare, evaluated in the explicit form
                const double dzdy = Y / fa.d, dx = 1e-10;
                const double g2 = dzdy * dzdy, gp2 = dx * dx + g2;
                const double proj = -(dzdy * fa.cos_w + dx * fa.sin_w);
                if (proj > 0.0 && g2 > 0.0) w = fa.wspeed * (proj * sqrt(g2 / (gp2 * (1.0 + g2))));
            }
        }
        w = w > fa.min_val ? w : fa.min_val;
        const size_t i = static_cast<size_t>(r) * cols + c;
        const float w32 = static_cast<float>(w);
        if (orograph) orograph[i] = w32;
        if (usable)
            usable[i] = usable_updraft_fast(static_cast<double>(w32), fa.thr, fa.inv_thr, fa.scale);
        m_l = z_l; m_c = z_c; m_r = z_r;
        z_l = p_l; z_c = p_c; z_r = p_r;
    }
}

// ---------------------------------------------------------------------------
// Elementwise orographic updraft, VEC consecutive cells per thread (16-byte
// accesses for f32 rasters), batched over wind cases.
constexpr int kMaxUniformBatch = 16;
struct UniformWind {
    double wspeed[kMaxUniformBatch];
    double wdirn[kMaxUniformBatch];
};

template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) Pack {
    T v[VEC];
};

template <typename Tin, typename Tw, bool UNIFORM, int VEC>
__global__ __launch_bounds__(kBlock) void k_orographic(
    const Tin *__restrict__ slope, const Tin *__restrict__ aspect,
    const Tw *__restrict__ wspeed, const Tw *__restrict__ wdirn, UniformWind uni,
    double min_val, float *__restrict__ orograph, double thr, double em1,
    double *__restrict__ usable, size_t ncells, int batch)
{
    const size_t nvec = ncells / VEC;   // host guarantees ncells % VEC == 0
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < nvec;
         i += static_cast<size_t>(gridDim.x) * kBlock) {
        const Pack<Tin, VEC> s = reinterpret_cast<const Pack<Tin, VEC> *>(slope)[i];
        const Pack<Tin, VEC> a = reinterpret_cast<const Pack<Tin, VEC> *>(aspect)[i];
        double sin_s[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j)
        {
            double unused;
            sincos_deg(static_cast<double>(s.v[j]), sin_s[j], unused);
        }
        for (int b = 0; b < batch; ++b) {
            const size_t o = static_cast<size_t>(b) * nvec + i;
            Pack<Tw, VEC> ws, wd;
            if (!UNIFORM) {
                ws = reinterpret_cast<const Pack<Tw, VEC> *>(wspeed)[o];
                wd = reinterpret_cast<const Pack<Tw, VEC> *>(wdirn)[o];
            }
            Pack<float, VEC> out;
            Pack<double, VEC> use;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const double spd = UNIFORM ? uni.wspeed[b] : static_cast<double>(ws.v[j]);
                const double dir = UNIFORM ? uni.wdirn[b] : static_cast<double>(wd.v[j]);
                double ad, unused;
                sincos_deg(static_cast<double>(a.v[j]) - dir, unused, ad);
                ad = ad > 0.0 ? ad : 0.0;                      // np.maximum(0., .)
                double w = spd * (sin_s[j] * ad);
                w = w > min_val ? w : min_val;
                out.v[j] = static_cast<float>(w);
                if (usable)
                    use.v[j] = usable_updraft(static_cast<double>(out.v[j]), thr, em1);
            }
            if (orograph) reinterpret_cast<Pack<float, VEC> *>(orograph)[o] = out;
            if (usable) reinterpret_cast<Pack<double, VEC> *>(usable)[o] = use;
        }
    }
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void k_threshold(const float *__restrict__ in,
                                                      double thr, double em1,
                                                      double *__restrict__ out, size_t n)
{
    const size_t nvec = n / VEC;
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < nvec;
         i += static_cast<size_t>(gridDim.x) * kBlock) {
        const Pack<float, VEC> v = reinterpret_cast<const Pack<float, VEC> *>(in)[i];
        Pack<double, VEC> o;
#pragma unroll
        for (int j = 0; j < VEC; ++j)
            o.v[j] = usable_updraft(static_cast<double>(v.v[j]), thr, em1);
        reinterpret_cast<Pack<double, VEC> *>(out)[i] = o;
    }
}

static inline bool aligned16(const void *p)
{   // NULL counts as aligned (optional arrays); 32 B covers Pack<double, 4>
    return (reinterpret_cast<uintptr_t>(p) & 31u) == 0;
}

template <typename Tin, typename Tw, bool UNIFORM>
static int launch_orographic(const void *slope, const void *aspect, const void *wspeed,
                             const void *wdirn, const UniformWind &uni, double min_val,
                             float *orograph, double thr, double *usable, size_t ncells,
                             int batch, hipStream_t st)
{
    const double em1 = exp(1.0) - 1.0;
    const bool vec = (ncells % 4 == 0) && aligned16(slope) && aligned16(aspect) &&
                     aligned16(wspeed) && aligned16(wdirn) && aligned16(orograph) &&
                     aligned16(usable);
    auto s = static_cast<const Tin *>(slope);
    auto a = static_cast<const Tin *>(aspect);
    auto ws = static_cast<const Tw *>(wspeed);
    auto wd = static_cast<const Tw *>(wdirn);
    if (vec) {
        hipLaunchKernelGGL((k_orographic<Tin, Tw, UNIFORM, 4>), dim3(stream_grid(ncells / 4)),
                           dim3(kBlock), 0, st, s, a, ws, wd, uni, min_val, orograph, thr,
                           em1, usable, ncells, batch);
    } else {
        hipLaunchKernelGGL((k_orographic<Tin, Tw, UNIFORM, 1>), dim3(stream_grid(ncells)),
                           dim3(kBlock), 0, st, s, a, ws, wd, uni, min_val, orograph, thr,
                           em1, usable, ncells, batch);
    }
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

}  // namespace ssrs

using namespace ssrs;

extern "C" int ssrs_slope_aspect(const void *dem, int dem_type, double res, void *slope,
                                 void *aspect, int out_type, int rows, int cols,
                                 void *stream)
{
    SSRS_REQUIRE(dem != nullptr, "ssrs_slope_aspect: dem is NULL");
    SSRS_REQUIRE(rows >= 3 && cols >= 3, "ssrs_slope_aspect: need rows, cols >= 3 (got %d x %d)",
                 rows, cols);
    SSRS_REQUIRE(res > 0.0, "ssrs_slope_aspect: res must be > 0");
    SSRS_REQUIRE((dem_type == SSRS_F32 || dem_type == SSRS_F64) &&
                     (out_type == SSRS_F32 || out_type == SSRS_F64),
                 "ssrs_slope_aspect: bad element type");
    if (!slope && !aspect) return SSRS_OK;
    const int tx = (cols + TW - 1) / TW, ty = (rows + TH - 1) / TH, nt = tx * ty;
    hipStream_t st = as_stream(stream);
#define SA_LAUNCH(TI, TO)                                                              \
    hipLaunchKernelGGL((k_slope_aspect<TI, TO>), dim3(nt), dim3(kBlock), 0, st,        \
                       static_cast<const TI *>(dem), res, static_cast<TO *>(slope),    \
                       static_cast<TO *>(aspect), rows, cols, tx, nt)
    if (dem_type == SSRS_F64 && out_type == SSRS_F64) SA_LAUNCH(double, double);
    else if (dem_type == SSRS_F64) SA_LAUNCH(double, float);
    else if (out_type == SSRS_F64) SA_LAUNCH(float, double);
    else SA_LAUNCH(float, float);
#undef SA_LAUNCH
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

extern "C" int ssrs_updraft_from_dem(const void *dem, int dem_type, double res,
                                     double wspeed, double wdirn, double min_val,
                                     float *orograph, double threshold, double *usable,
                                     int rows, int cols, void *stream)
{
    SSRS_REQUIRE(dem != nullptr, "ssrs_updraft_from_dem: dem is NULL");
    SSRS_REQUIRE(rows >= 3 && cols >= 3, "ssrs_updraft_from_dem: need rows, cols >= 3");
    SSRS_REQUIRE(res > 0.0, "ssrs_updraft_from_dem: res must be > 0");
    SSRS_REQUIRE(dem_type == SSRS_F32 || dem_type == SSRS_F64,
                 "ssrs_updraft_from_dem: bad element type");
    SSRS_REQUIRE(!(usable && !(threshold > 0.0)),
                 "ssrs_updraft_from_dem: usable requested without a positive threshold");
    if (!orograph && !usable) return SSRS_OK;
    const int tx = (cols + TW - 1) / TW, ty = (rows + TH - 1) / TH, nt = tx * ty;
    const double w = wdirn * kPi / 180.0;
    FusedArgs fa;
    fa.d = 8 * res;
    fa.d2 = fa.d * fa.d;
    fa.wspeed = wspeed;
    fa.cos_w = cos(w);
    fa.sin_w = sin(w);
    fa.min_val = min_val;
    fa.thr = threshold;
    fa.inv_thr = threshold > 0.0 ? 1.0 / threshold : 0.0;
    fa.scale = threshold > 0.0 ? threshold / (exp(1.0) - 1.0) : 0.0;
    hipStream_t st = as_stream(stream);
    if (dem_type == SSRS_F64)
        hipLaunchKernelGGL((k_updraft_from_dem<double>), dim3(nt), dim3(kBlock), 0, st,
                           static_cast<const double *>(dem), fa, orograph, usable, rows, cols, tx, nt);
    else
        hipLaunchKernelGGL((k_updraft_from_dem<float>), dim3(nt), dim3(kBlock), 0, st,
                           static_cast<const float *>(dem), fa, orograph, usable, rows, cols, tx, nt);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

extern "C" int ssrs_orographic_updraft(const void *slope, const void *aspect, int in_type,
                                       const void *wspeed, const void *wdirn, int wind_type,
                                       const double *wspeed0, const double *wdirn0,
                                       double min_val, float *orograph, double threshold,
                                       double *usable, int rows, int cols, int batch,
                                       void *stream)
{
    SSRS_REQUIRE(slope && aspect, "ssrs_orographic_updraft: slope/aspect is NULL");
    SSRS_REQUIRE(rows > 0 && cols > 0 && batch > 0,
                 "ssrs_orographic_updraft: rows, cols, batch must be > 0");
    SSRS_REQUIRE((in_type == SSRS_F32 || in_type == SSRS_F64) &&
                     (wind_type == SSRS_F32 || wind_type == SSRS_F64),
                 "ssrs_orographic_updraft: bad element type");
    SSRS_REQUIRE((wspeed == nullptr) == (wdirn == nullptr),
                 "ssrs_orographic_updraft: give both wind rasters or neither");
    SSRS_REQUIRE(!(usable && threshold < 0.0),
                 "ssrs_orographic_updraft: usable requested with threshold < 0");
    if (!orograph && !usable) return SSRS_OK;
    const size_t ncells = static_cast<size_t>(rows) * cols;
    hipStream_t st = as_stream(stream);
    UniformWind uni = {};
    if (wspeed) {
        if (in_type == SSRS_F32 && wind_type == SSRS_F32)
            return launch_orographic<float, float, false>(slope, aspect, wspeed, wdirn, uni,
                                                          min_val, orograph, threshold,
                                                          usable, ncells, batch, st);
        if (in_type == SSRS_F32)
            return launch_orographic<float, double, false>(slope, aspect, wspeed, wdirn, uni,
                                                           min_val, orograph, threshold,
                                                           usable, ncells, batch, st);
        if (wind_type == SSRS_F32)
            return launch_orographic<double, float, false>(slope, aspect, wspeed, wdirn, uni,
                                                           min_val, orograph, threshold,
                                                           usable, ncells, batch, st);
        return launch_orographic<double, double, false>(slope, aspect, wspeed, wdirn, uni,
                                                        min_val, orograph, threshold, usable,
                                                        ncells, batch, st);
    }
    SSRS_REQUIRE(wspeed0 && wdirn0, "ssrs_orographic_updraft: uniform mode needs wspeed0/wdirn0");
    for (int b0 = 0; b0 < batch; b0 += kMaxUniformBatch) {
        const int nb = batch - b0 < kMaxUniformBatch ? batch - b0 : kMaxUniformBatch;
        for (int j = 0; j < nb; ++j) {
            uni.wspeed[j] = wspeed0[b0 + j];
            uni.wdirn[j] = wdirn0[b0 + j];
        }
        float *o = orograph ? orograph + static_cast<size_t>(b0) * ncells : nullptr;
        double *u = usable ? usable + static_cast<size_t>(b0) * ncells : nullptr;
        int rc = in_type == SSRS_F32
                     ? launch_orographic<float, float, true>(slope, aspect, nullptr, nullptr,
                                                             uni, min_val, o, threshold, u,
                                                             ncells, nb, st)
                     : launch_orographic<double, float, true>(slope, aspect, nullptr, nullptr,
                                                              uni, min_val, o, threshold, u,
                                                              ncells, nb, st);
        if (rc != SSRS_OK) return rc;
    }
    return SSRS_OK;
}

extern "C" int ssrs_threshold_updraft(const float *in, double threshold, double *out,
                                      size_t n, void *stream)
{
    SSRS_REQUIRE(in && out, "ssrs_threshold_updraft: NULL pointer");
    SSRS_REQUIRE(threshold > 0.0, "ssrs_threshold_updraft: threshold must be > 0");
    if (n == 0) return SSRS_OK;
    const double em1 = exp(1.0) - 1.0;
    hipStream_t st = as_stream(stream);
    if (n % 4 == 0 && aligned16(in) && aligned16(out))
        hipLaunchKernelGGL((k_threshold<4>), dim3(stream_grid(n / 4)), dim3(kBlock), 0, st, in,
                           threshold, em1, out, n);
    else
        hipLaunchKernelGGL((k_threshold<1>), dim3(stream_grid(n)), dim3(kBlock), 0, st, in,
                           threshold, em1, out, n);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

// ---------------------------------------------------------------------------
// K6 -- wind field preparation for snapshot / seasonal modes
// (ssrs/simulator.py:778-792): speed/direction samples -> easterly/northerly
// components -> interpolation to the terrain grid -> speed and direction
// (degrees in [0, 360)).  The reference interpolates scattered WTK points with
// scipy griddata (Qhull Delaunay, 'linear'); on a regular lattice -- the shape
// of the 2-km WTK grid and of the synthetic configs -- piecewise-bilinear
// interpolation is the natural equivalent and needs no triangulation.  The
// lattice (<= a few thousand points) is read through L2; one thread per cell.
namespace ssrs {

__global__ __launch_bounds__(kBlock) void k_wind_lattice(
    const double *__restrict__ lat_speed, const double *__restrict__ lat_dirn, int nx, int ny,
    double x0, double y0, double dx, double dy, double cell, double *__restrict__ wspeed,
    double *__restrict__ wdirn, int rows, int cols, int batch)
{
    const size_t ncell = static_cast<size_t>(rows) * cols;
    const size_t total = ncell * batch;
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < total;
         i += static_cast<size_t>(gridDim.x) * kBlock) {
        const int b = static_cast<int>(i / ncell);
        const size_t c0 = i - static_cast<size_t>(b) * ncell;
        const int r = static_cast<int>(c0 / cols), c = static_cast<int>(c0 % cols);
        // cell centre in lattice units, clamped to the lattice hull
        double fx = (c * cell - x0) / dx, fy = (r * cell - y0) / dy;
        fx = fx < 0.0 ? 0.0 : (fx > nx - 1.0 ? nx - 1.0 : fx);
        fy = fy < 0.0 ? 0.0 : (fy > ny - 1.0 ? ny - 1.0 : fy);
        int ix = static_cast<int>(fx), iy = static_cast<int>(fy);
        ix = ix > nx - 2 ? (nx > 1 ? nx - 2 : 0) : ix;
        iy = iy > ny - 2 ? (ny > 1 ? ny - 2 : 0) : iy;
        const double tx = nx > 1 ? fx - ix : 0.0, ty = ny > 1 ? fy - iy : 0.0;
        const double *ls = lat_speed + static_cast<size_t>(b) * nx * ny;
        const double *ld = lat_dirn + static_cast<size_t>(b) * nx * ny;
        double east = 0.0, north = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int jx = ix + (k & 1 && nx > 1 ? 1 : 0), jy = iy + (k >> 1 && ny > 1 ? 1 : 0);
            const double w = ((k & 1) ? tx : 1.0 - tx) * ((k >> 1) ? ty : 1.0 - ty);
            const double s = ls[static_cast<size_t>(jy) * nx + jx];
            const double a = ld[static_cast<size_t>(jy) * nx + jx] * kPi / 180.0;
            east += w * (s * sin(a));       // simulator.py:784
            north += w * (s * cos(a));      // simulator.py:785
        }
        const double spd = sqrt(east * east + north * north);
        double ang = atan2(east, north);                               // :790
        ang = fmod(ang + 2.0 * kPi, 2.0 * kPi);                        // :791
        wspeed[i] = spd;
        wdirn[i] = ang * 180.0 / kPi;
    }
}

}  // namespace ssrs

namespace ssrs {

// Lattice speed / direction -> east and north components (simulator.py:784-785), once
// per lattice point instead of once per raster cell and corner.
__global__ __launch_bounds__(kBlock) void k_lattice_components(const double *__restrict__ lat_speed,
                                                              const double *__restrict__ lat_dirn,
                                                              size_t n, double *__restrict__ east,
                                                              double *__restrict__ north)
{
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < n;
         i += static_cast<size_t>(gridDim.x) * kBlock) {
        const double s = lat_speed[i], a = lat_dirn[i] * kPi / 180.0;
        east[i] = s * sin(a);
        north[i] = s * cos(a);
    }
}

// Scattered wind samples (the reference's general case, simulator.py:765-776: scipy griddata, method 'linear' =
// Delaunay triangulation + barycentric interpolation).  The triangulation is the host's (scipy.spatial.Delaunay, the
// very object griddata builds); here: (1) every triangle claims the cells of its bounding box whose centre it
// contains -- by scipy's own test, all barycentric coordinates within [-eps, 1 + eps], eps = 100 DBL_EPSILON -- and the
// LOWEST triangle index wins a cell on a shared edge (deterministic; the interpolant is continuous there);
// (2) per cell: c_j = sum_k T[j][k] (x_k - r_k), c_2 = 1 - c_0 - c_1 from the triangulation's affine transform,
// east / north = sum_j c_j value[vertex_j] in scipy's order, then the u/v recipe of simulator.py:778-792.  Cells
// outside the hull are NaN, as griddata's fill value.
__global__ __launch_bounds__(kBlock) void k_tri_owner(const double *__restrict__ pts, const int32_t *__restrict__ tri,
                                                     const double *__restrict__ transform, int ntri, double cell,
                                                     int rows, int cols, int32_t *__restrict__ owner)
{
    const int t = blockIdx.x;
    if (t >= ntri) return;
    const int32_t v0 = tri[3 * t], v1 = tri[3 * t + 1], v2 = tri[3 * t + 2];
    const double x0 = pts[2 * v0], y0 = pts[2 * v0 + 1], x1 = pts[2 * v1], y1 = pts[2 * v1 + 1], x2 = pts[2 * v2], y2 = pts[2 * v2 + 1];
    const double xmin = fmin(x0, fmin(x1, x2)), xmax = fmax(x0, fmax(x1, x2));
    const double ymin = fmin(y0, fmin(y1, y2)), ymax = fmax(y0, fmax(y1, y2));
    // cells whose centre (c cell, r cell) may lie in the box, one cell of margin for the tolerance
    long long c_lo = static_cast<long long>(floor(xmin / cell)) - 1, c_hi = static_cast<long long>(ceil(xmax / cell)) + 1;
    long long r_lo = static_cast<long long>(floor(ymin / cell)) - 1, r_hi = static_cast<long long>(ceil(ymax / cell)) + 1;
    c_lo = c_lo < 0 ? 0 : c_lo;  r_lo = r_lo < 0 ? 0 : r_lo;
    c_hi = c_hi > cols - 1 ? cols - 1 : c_hi;  r_hi = r_hi > rows - 1 ? rows - 1 : r_hi;
    if (c_lo > c_hi || r_lo > r_hi) return;
    const double *T = transform + 6 * static_cast<size_t>(t);        // [T00 T01; T10 T11; r0 r1]
    const double t00 = T[0], t01 = T[1], t10 = T[2], t11 = T[3], rx = T[4], ry = T[5];
    if (!(t00 == t00)) return;                                         // degenerate simplex (scipy: NaN transform)
    const double eps = 100.0 * 2.220446049250313e-16;
    const long long w = c_hi - c_lo + 1, n = w * (r_hi - r_lo + 1);
    for (long long q = static_cast<long long>(blockIdx.y) * kBlock + threadIdx.x; q < n; q += static_cast<long long>(gridDim.y) * kBlock) {
        const long long r = r_lo + q / w, c = c_lo + q % w;
        const double dx = static_cast<double>(c) * cell - rx, dy = static_cast<double>(r) * cell - ry;
        const double b0 = t00 * dx + t01 * dy, b1 = t10 * dx + t11 * dy, b2 = 1.0 - b0 - b1;
        const bool inside = b0 >= -eps && b0 <= 1.0 + eps && b1 >= -eps && b1 <= 1.0 + eps && b2 >= -eps && b2 <= 1.0 + eps;
        if (inside) atomicMin(&owner[static_cast<size_t>(r) * cols + static_cast<size_t>(c)], t);
    }
}

__global__ __launch_bounds__(kBlock) void k_wind_triangles(const int32_t *__restrict__ owner, const int32_t *__restrict__ tri,
                                                          const double *__restrict__ transform,
                                                          const double *__restrict__ east, const double *__restrict__ north,
                                                          int npts, double cell, double *__restrict__ wspeed,
                                                          double *__restrict__ wdirn, int rows, int cols, int batch)
{
    const size_t ncell = static_cast<size_t>(rows) * cols, total = ncell * batch;
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < total; i += static_cast<size_t>(gridDim.x) * kBlock) {
        const int b = static_cast<int>(i / ncell);
        const size_t c0 = i - static_cast<size_t>(b) * ncell;
        const int r = static_cast<int>(c0 / cols), c = static_cast<int>(c0 % cols);
        const int32_t t = owner[c0];
        double spd = quiet_nan(), ang = spd;
        if (t != kNoOwner) {
            double b0, b1, b2;
            tri_barycentric(transform + 6 * static_cast<size_t>(t), r, c, cell, b0, b1, b2);
            const double *e = east + static_cast<size_t>(b) * npts, *nn = north + static_cast<size_t>(b) * npts;
            const int32_t v0 = tri[3 * t], v1 = tri[3 * t + 1], v2 = tri[3 * t + 2];
            const double ee = tri_linear(b0, b1, b2, e, v0, v1, v2);
            const double en = tri_linear(b0, b1, b2, nn, v0, v1, v2);
            spd = sqrt(ee * ee + en * en);
            ang = fmod(atan2(ee, en) + 2.0 * kPi, 2.0 * kPi) * 180.0 / kPi;
        }
        wspeed[i] = spd;
        wdirn[i] = ang;
    }
}

// Snapshot / seasonal K1: DEM tile in LDS -> Horn sums once per cell, then for every
// snapshot b the wind at the cell (bilinear in the lattice's east / north components,
// as k_wind_lattice) and the updraft in the trig-free form of k_updraft_from_dem: with
// (cos w, sin w) = (north, east) / speed the wind speed cancels,
//     w = -(Y north + X east) / sqrt(d^2 + X^2 + Y^2),
// so neither the per-cell wind rasters (16 B per cell and snapshot written and read
// again) nor atan2 / sin / cos per cell are needed: 8 B read per cell for the whole
// batch, 4-12 B written per cell and snapshot.
struct LatticeArgs {
    const double *east, *north;       // (batch, ny, nx)
    int nx, ny, batch;
    double x0, y0, inv_dx, inv_dy, cell;
};

template <typename Tin>
__global__ __launch_bounds__(kBlock) void k_updraft_from_dem_lattice(
    const Tin *__restrict__ dem, FusedArgs fa, LatticeArgs la, float *__restrict__ orograph,
    double *__restrict__ usable, int rows, int cols, int tiles_x, int ntiles)
{
    __shared__ double tile[LW * LH];
    const int t = xcd_tile(blockIdx.x, ntiles);
    const int r0 = (t / tiles_x) * TH, c0 = (t % tiles_x) * TW;
    stage_dem_tile(dem, rows, cols, r0, c0, tile);
    const int lc = threadIdx.x % TW + 1;
    const int c = c0 + lc - 1;
    if (c >= cols) return;
    constexpr int kRowsPerWave = TH / (kBlock / TW);
    const int lr0 = (threadIdx.x / TW) * kRowsPerWave + 1;
    // lattice column of this thread's cells (the same for all its rows)
    double fx = (c * la.cell - la.x0) * la.inv_dx;
    fx = fx < 0.0 ? 0.0 : (fx > la.nx - 1.0 ? la.nx - 1.0 : fx);
    int ix = static_cast<int>(fx);
    ix = ix > la.nx - 2 ? (la.nx > 1 ? la.nx - 2 : 0) : ix;
    const double tx = la.nx > 1 ? fx - ix : 0.0;
    const int jx1 = la.nx > 1 ? 1 : 0;
    const size_t ncell = static_cast<size_t>(rows) * cols;
    for (int lr = lr0; lr < lr0 + kRowsPerWave; ++lr) {
        const int r = r0 + lr - 1;
        if (r >= rows) break;
        const double *m = tile + (lr - 1) * LW + lc, *z = tile + lr * LW + lc, *p = tile + (lr + 1) * LW + lc;
        const bool interior = r > 0 && c > 0 && r < rows - 1 && c < cols - 1;
        // un-normalised Horn sums (layers.py:78-90; "x" = row axis)
        const double X = (p[1] + 2 * p[0] + p[-1]) - (m[1] + 2 * m[0] + m[-1]);
        const double Y = (m[1] + 2 * z[1] + p[1]) - (m[-1] + 2 * z[-1] + p[-1]);
        const double rs = rsqrt_pos(fa.d2 + (X * X + Y * Y));
        double fy = (r * la.cell - la.y0) * la.inv_dy;
        fy = fy < 0.0 ? 0.0 : (fy > la.ny - 1.0 ? la.ny - 1.0 : fy);
        int iy = static_cast<int>(fy);
        iy = iy > la.ny - 2 ? (la.ny > 1 ? la.ny - 2 : 0) : iy;
        const double ty = la.ny > 1 ? fy - iy : 0.0;
        const size_t o00 = static_cast<size_t>(iy) * la.nx + ix;
        const size_t o10 = o00 + (la.ny > 1 ? la.nx : 0);
        const double w00 = (1.0 - tx) * (1.0 - ty), w01 = tx * (1.0 - ty), w10 = (1.0 - tx) * ty, w11 = tx * ty;
        const size_t i = static_cast<size_t>(r) * cols + c;
        for (int b = 0; b < la.batch; ++b) {
            const double *le = la.east + static_cast<size_t>(b) * la.nx * la.ny;
            const double *ln = la.north + static_cast<size_t>(b) * la.nx * la.ny;
            // same accumulation order as k_wind_lattice
            double east = 0.0, north = 0.0;
            east += w00 * le[o00]; north += w00 * ln[o00];
            east += w01 * le[o00 + jx1]; north += w01 * ln[o00 + jx1];
            east += w10 * le[o10]; north += w10 * ln[o10];
            east += w11 * le[o10 + jx1]; north += w11 * ln[o10 + jx1];
            double w = 0.0;
            if (interior) {
                if (X != 0.0) {
                    const double P = -(Y * north + X * east);
                    if (P > 0.0) w = P * rs;
                } else {
                    // dz_dx == 0: the reference substitutes 1e-10 for the aspect only (layers.py:124)
                    const double spd = sqrt(east * east + north * north);
                    const double dzdy = Y / fa.d, dx = 1e-10;
                    const double g2 = dzdy * dzdy, gp2 = dx * dx + g2;
                    const double proj = spd > 0.0 ? -(dzdy * north + dx * east) : 0.0;
                    if (proj > 0.0 && g2 > 0.0) w = proj * sqrt(g2 / (gp2 * (1.0 + g2)));
                }
            }
            w = w > fa.min_val ? w : fa.min_val;
            const float w32 = static_cast<float>(w);
            if (orograph) orograph[b * ncell + i] = w32;
            if (usable)
                usable[b * ncell + i] = usable_updraft_fast(static_cast<double>(w32), fa.thr, fa.inv_thr, fa.scale);
        }
    }
}

}  // namespace ssrs

extern "C" size_t ssrs_lattice_workspace_bytes(int nx, int ny, int batch)
{
    if (nx <= 0 || ny <= 0 || batch <= 0) return 0;
    return static_cast<size_t>(nx) * ny * batch * 2 * sizeof(double);
}

extern "C" int ssrs_updraft_from_dem_lattice(const void *dem, int dem_type, double res,
                                             const double *lattice_speed, const double *lattice_dirn,
                                             int nx, int ny, double x0, double y0, double dx, double dy,
                                             double min_val, float *orograph, double threshold,
                                             double *usable, int rows, int cols, int batch,
                                             void *workspace, size_t workspace_bytes, void *stream)
{
    SSRS_REQUIRE(dem && lattice_speed && lattice_dirn, "ssrs_updraft_from_dem_lattice: NULL pointer");
    SSRS_REQUIRE(rows >= 3 && cols >= 3 && nx >= 1 && ny >= 1 && batch >= 1,
                 "ssrs_updraft_from_dem_lattice: bad sizes");
    SSRS_REQUIRE(res > 0.0 && dx > 0.0 && dy > 0.0, "ssrs_updraft_from_dem_lattice: res, dx, dy must be > 0");
    SSRS_REQUIRE(dem_type == SSRS_F32 || dem_type == SSRS_F64, "ssrs_updraft_from_dem_lattice: bad element type");
    SSRS_REQUIRE(!(usable && !(threshold > 0.0)),
                 "ssrs_updraft_from_dem_lattice: usable requested without a positive threshold");
    SSRS_REQUIRE(workspace && workspace_bytes >= ssrs_lattice_workspace_bytes(nx, ny, batch),
                 "ssrs_updraft_from_dem_lattice: workspace too small");
    if (!orograph && !usable) return SSRS_OK;
    hipStream_t st = as_stream(stream);
    const size_t npts = static_cast<size_t>(nx) * ny * batch;
    double *east = static_cast<double *>(workspace), *north = east + npts;
    hipLaunchKernelGGL(k_lattice_components, dim3(stream_grid(npts)), dim3(kBlock), 0, st, lattice_speed,
                       lattice_dirn, npts, east, north);
    const int tx = (cols + TW - 1) / TW, ty = (rows + TH - 1) / TH, nt = tx * ty;
    FusedArgs fa = {};
    fa.d = 8 * res;
    fa.d2 = fa.d * fa.d;
    fa.min_val = min_val;
    fa.thr = threshold;
    fa.inv_thr = threshold > 0.0 ? 1.0 / threshold : 0.0;
    fa.scale = threshold > 0.0 ? threshold / (exp(1.0) - 1.0) : 0.0;
    LatticeArgs la = {east, north, nx, ny, batch, x0, y0, 1.0 / dx, 1.0 / dy, res / 1000.0};
    if (dem_type == SSRS_F64)
        hipLaunchKernelGGL((k_updraft_from_dem_lattice<double>), dim3(nt), dim3(kBlock), 0, st,
                           static_cast<const double *>(dem), fa, la, orograph, usable, rows, cols, tx, nt);
    else
        hipLaunchKernelGGL((k_updraft_from_dem_lattice<float>), dim3(nt), dim3(kBlock), 0, st,
                           static_cast<const float *>(dem), fa, la, orograph, usable, rows, cols, tx, nt);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

extern "C" int ssrs_wind_from_lattice(const double *lattice_speed, const double *lattice_dirn,
                                      int nx, int ny, double x0, double y0, double dx, double dy,
                                      double cell_size, double *wspeed, double *wdirn, int rows,
                                      int cols, int batch, void *stream)
{
    SSRS_REQUIRE(lattice_speed && lattice_dirn && wspeed && wdirn,
                 "ssrs_wind_from_lattice: NULL pointer");
    SSRS_REQUIRE(nx >= 1 && ny >= 1 && rows > 0 && cols > 0 && batch > 0,
                 "ssrs_wind_from_lattice: bad sizes");
    SSRS_REQUIRE(dx > 0.0 && dy > 0.0 && cell_size > 0.0,
                 "ssrs_wind_from_lattice: spacings must be > 0");
    const size_t total = static_cast<size_t>(rows) * cols * batch;
    hipLaunchKernelGGL(k_wind_lattice, dim3(stream_grid(total)), dim3(kBlock), 0,
                       as_stream(stream), lattice_speed, lattice_dirn, nx, ny, x0, y0, dx, dy,
                       cell_size, wspeed, wdirn, rows, cols, batch);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

extern "C" size_t ssrs_wind_triangles_workspace_bytes(int npts, int rows, int cols, int batch)
{
    if (npts <= 0 || rows <= 0 || cols <= 0 || batch <= 0) return 0;
    return static_cast<size_t>(rows) * cols * sizeof(int32_t) + 2 * static_cast<size_t>(npts) * batch * sizeof(double) + 512;
}

extern "C" int ssrs_wind_from_triangles(const double *points, const int32_t *triangles, const double *transform,
                                        const double *speed, const double *dirn, int npts, int ntri, double cell_size,
                                        double *wspeed, double *wdirn, int rows, int cols, int batch,
                                        void *workspace, size_t workspace_bytes, void *stream)
{
    SSRS_REQUIRE(points && triangles && transform && speed && dirn && wspeed && wdirn,
                 "ssrs_wind_from_triangles: NULL pointer");
    SSRS_REQUIRE(npts >= 3 && ntri >= 1 && rows > 0 && cols > 0 && batch > 0, "ssrs_wind_from_triangles: bad sizes");
    SSRS_REQUIRE(cell_size > 0.0, "ssrs_wind_from_triangles: cell_size must be > 0");
    SSRS_REQUIRE(workspace && workspace_bytes >= ssrs_wind_triangles_workspace_bytes(npts, rows, cols, batch),
                 "ssrs_wind_from_triangles: workspace too small");
    hipStream_t st = as_stream(stream);
    const size_t ncell = static_cast<size_t>(rows) * cols, nval = static_cast<size_t>(npts) * batch;
    int32_t *owner = static_cast<int32_t *>(workspace);
    double *east = reinterpret_cast<double *>(static_cast<char *>(workspace) + ((ncell * sizeof(int32_t) + 255) / 256) * 256);
    double *north = east + nval;
    hipLaunchKernelGGL(k_lattice_components, dim3(stream_grid(nval)), dim3(kBlock), 0, st, speed, dirn, nval, east, north);
    if (int rc = launch_tri_owner(points, triangles, transform, ntri, cell_size, rows, cols, owner, st)) return rc;
    hipLaunchKernelGGL(k_wind_triangles, dim3(stream_grid(ncell * batch)), dim3(kBlock), 0, st, owner, triangles, transform, east,
                       north, npts, cell_size, wspeed, wdirn, rows, cols, batch);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

// ---------------------------------------------------------------------------
// K6, the other two griddata methods (simulator.py:774-775 hands wtk_interp_type to scipy):
//   'nearest'  NearestNDInterpolator: every cell takes the sample nearest to its centre.  The index raster depends on
//              the points only (k_nearest_index, built once per geometry); per snapshot k_wind_nearest is two table
//              look-ups and two stores per cell.
//   'cubic'    CloughTocher2DInterpolator: a C1 piecewise cubic on the Delaunay triangulation.  The vertex gradients are
//              scipy's (a global iteration over a few thousand vertices, done on the host); k_ct_coefficients turns
//              values + gradients into the 19 Bezier ordinates of every macro-triangle, k_wind_cubic evaluates them
//              per cell.  Cell ownership is k_tri_owner, as for 'linear'.
namespace ssrs {

// simulator.py:784-785,790-791 on one sample
__device__ __forceinline__ void wind_recipe(double s, double a_deg, double &spd, double &dir)
{
    const double a = a_deg * kPi / 180.0;
    const double e = s * sin(a), n = s * cos(a);
    spd = sqrt(e * e + n * n);
    dir = fmod(atan2(e, n) + 2.0 * kPi, 2.0 * kPi) * 180.0 / kPi;
}

__device__ __forceinline__ double wave_min(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}

// One block per TW x TH tile.  With c the tile's centre, h its half diagonal and dmin the distance from c to its
// nearest sample, the nearest sample p of ANY cell x of the tile has |c - p| <= |c - x| + |x - p| <= h + (|x - c| +
// dmin) <= dmin + 2h: two passes over the samples collect those candidates in LDS and every lane scans the candidates
// only.  A list that does not fit falls back to all samples, so the cull never decides a result; a lane keeps
// (d^2, index) lexicographically smallest, so neither does the order in which candidates were collected.
constexpr int kNearCand = 1024;
static_assert(kBlock == 4 * 64 && kBlock % TW == 0 && TH % (kBlock / TW) == 0, "k_nearest_index: four waves over a TW x TH tile");

__global__ __launch_bounds__(kBlock) void k_nearest_index(const double *__restrict__ pts, int npts, double cell, int rows,
                                                         int cols, int tiles_x, int32_t *__restrict__ index,
                                                         int32_t *__restrict__ full_scans)
{
    __shared__ double cand_x[kNearCand], cand_y[kNearCand];
    __shared__ int32_t cand_i[kNearCand];
    __shared__ double wave_dmin[kBlock / 64];
    __shared__ int ncand;
    const int tid = threadIdx.x;
    const int r0 = (blockIdx.x / tiles_x) * TH, c0 = (blockIdx.x % tiles_x) * TW;
    const double xc = (c0 + 0.5 * (TW - 1)) * cell, yc = (r0 + 0.5 * (TH - 1)) * cell;
    const double h = 0.5 * sqrt(static_cast<double>((TW - 1) * (TW - 1) + (TH - 1) * (TH - 1))) * cell;
    if (tid == 0) ncand = 0;
    double dmin = __longlong_as_double(0x7FF0000000000000ll);
    for (int p = tid; p < npts; p += kBlock) {
        const double dx = pts[2 * p] - xc, dy = pts[2 * p + 1] - yc;
        dmin = fmin(dmin, dx * dx + dy * dy);
    }
    dmin = wave_min(dmin);
    if ((tid & 63) == 0) wave_dmin[tid >> 6] = dmin;
    __syncthreads();
    dmin = fmin(fmin(wave_dmin[0], wave_dmin[1]), fmin(wave_dmin[2], wave_dmin[3]));
    const double reach = sqrt(dmin) + 2.0 * h;
    const double lim = reach * reach * (1.0 + 1e-9);                // (rounding of d^2 is 1e-16 relative)
    for (int p = tid; p < npts; p += kBlock) {
        const double px = pts[2 * p], py = pts[2 * p + 1];
        const double dx = px - xc, dy = py - yc;
        if (dx * dx + dy * dy <= lim) {
            const int k = atomicAdd(&ncand, 1);
            if (k < kNearCand) {
                cand_x[k] = px;
                cand_y[k] = py;
                cand_i[k] = p;
            }
        }
    }
    __syncthreads();
    const int n = ncand;
    const bool culled = n <= kNearCand;
    if (!culled && tid == 0) atomicAdd(full_scans, 1);

    constexpr int kRowsPerLane = TH / (kBlock / TW);
    const int c = c0 + tid % TW, rl = tid / TW;
    const double x = static_cast<double>(c) * cell;
    double y[kRowsPerLane], best[kRowsPerLane];
    int32_t who[kRowsPerLane];
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) {
        y[j] = static_cast<double>(r0 + rl + j * (kBlock / TW)) * cell;
        best[j] = __longlong_as_double(0x7FF0000000000000ll);
        who[j] = 0;
    }
    auto visit = [&](double px, double py, int32_t id) {
        const double dx = x - px, dxx = dx * dx;
#pragma unroll
        for (int j = 0; j < kRowsPerLane; ++j) {
            const double dy = y[j] - py, d2 = dxx + dy * dy;
            if (d2 < best[j] || (d2 == best[j] && id < who[j])) {
                best[j] = d2;
                who[j] = id;
            }
        }
    };
    if (culled)
        for (int k = 0; k < n; ++k) visit(cand_x[k], cand_y[k], cand_i[k]);
    else
        for (int p = 0; p < npts; ++p) visit(pts[2 * p], pts[2 * p + 1], p);
    if (c < cols) {
#pragma unroll
        for (int j = 0; j < kRowsPerLane; ++j) {
            const int r = r0 + rl + j * (kBlock / TW);
            if (r < rows) index[static_cast<size_t>(r) * cols + c] = who[j];
        }
    }
}

// Snapshot blockIdx.y.  The recipe runs once per sample and block into LDS (the value set is npts wide, the raster
// 30 M cells); `table` == 0 (more samples than the LDS table holds) applies it per cell instead, same function, same
// bits.  An index outside [0, npts) gives NaN.
__global__ __launch_bounds__(kBlock) void k_wind_nearest(const int32_t *__restrict__ index, const double *__restrict__ speed,
                                                        const double *__restrict__ dirn, int npts, double *__restrict__ wspeed,
                                                        double *__restrict__ wdirn, size_t ncell, int table)
{
    extern __shared__ double sample_table[];                           // speed[npts], direction[npts]
    const size_t b = blockIdx.y;
    const double *s = speed + b * npts, *d = dirn + b * npts;
    if (table) {
        for (int p = threadIdx.x; p < npts; p += kBlock) wind_recipe(s[p], d[p], sample_table[p], sample_table[npts + p]);
        __syncthreads();
    }
    double *os = wspeed + b * ncell, *od = wdirn + b * ncell;
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < ncell; i += static_cast<size_t>(gridDim.x) * kBlock) {
        const int32_t k = index[i];
        double spd = __longlong_as_double(0x7FF8000000000000ll), dir = spd;
        if (static_cast<uint32_t>(k) < static_cast<uint32_t>(npts)) {
            if (table) {
                spd = sample_table[k];
                dir = sample_table[npts + k];
            } else {
                wind_recipe(s[k], d[k], spd, dir);
            }
        }
        os[i] = spd;
        od[i] = dir;
    }
}

// The 19 Bezier ordinates of the Clough-Tocher macro-triangle t for field f (the wind: f = 2 * snapshot + (0 east |
// 1 north); in general the pairing of interp.h's launch_ct_coefficients), as
// scipy's _clough_tocher_2d_single computes them on every evaluation; they do not depend on the evaluation point.
// Order: c3000 c2100 c2010 c2001 c1200 c1101 c1020 c1011 c1002 c0300 c0210 c0201 c0120 c0111 c0102 c0030 c0021 c0012
// c0003 (the order of the cubic's terms).  No guard scipy does not have: a neighbour whose centroid makes a
// denominator of g vanish gives what IEEE gives.
__global__ __launch_bounds__(kBlock) void k_ct_coefficients(const double *__restrict__ pts, const int32_t *__restrict__ tri,
                                                           const int32_t *__restrict__ nbr, const double *__restrict__ transform,
                                                           const double *__restrict__ east, const double *__restrict__ north,
                                                           const double *__restrict__ grad_east, const double *__restrict__ grad_north,
                                                           size_t npts, int ntri, int nfield, double *__restrict__ coef)
{
    const size_t q = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x;
    if (q >= static_cast<size_t>(ntri) * nfield) return;
    const int t = static_cast<int>(q / nfield), f = static_cast<int>(q % nfield);
    const size_t b = f >> 1;
    const double *val = ((f & 1) ? north : east) + b * npts;
    const double *grad = ((f & 1) ? grad_north : grad_east) + b * npts * 2;
    const int32_t v0 = tri[3 * t], v1 = tri[3 * t + 1], v2 = tri[3 * t + 2];
    const double x0 = pts[2 * v0], y0 = pts[2 * v0 + 1], x1 = pts[2 * v1], y1 = pts[2 * v1 + 1], x2 = pts[2 * v2], y2 = pts[2 * v2 + 1];
    const double e12x = x1 - x0, e12y = y1 - y0, e23x = x2 - x1, e23y = y2 - y1, e31x = x0 - x2, e31y = y0 - y2;
    const double f1 = val[v0], f2 = val[v1], f3 = val[v2];
    const double g0x = grad[2 * v0], g0y = grad[2 * v0 + 1], g1x = grad[2 * v1], g1y = grad[2 * v1 + 1];
    const double g2x = grad[2 * v2], g2y = grad[2 * v2 + 1];
    const double df12 = +(g0x * e12x + g0y * e12y), df21 = -(g1x * e12x + g1y * e12y);
    const double df23 = +(g1x * e23x + g1y * e23y), df32 = -(g2x * e23x + g2y * e23y);
    const double df31 = +(g2x * e31x + g2y * e31y), df13 = -(g0x * e31x + g0y * e31y);
    const double c3000 = f1, c2100 = (df12 + 3 * f1) / 3, c2010 = (df13 + 3 * f1) / 3;
    const double c0300 = f2, c1200 = (df21 + 3 * f2) / 3, c0210 = (df23 + 3 * f2) / 3;
    const double c0030 = f3, c1020 = (df31 + 3 * f3) / 3, c0120 = (df32 + 3 * f3) / 3;
    const double c2001 = (c2100 + c2010 + c3000) / 3;
    const double c0201 = (c1200 + c0300 + c0210) / 3;
    const double c0021 = (c1020 + c0120 + c0030) / 3;
    const double *T = transform + 6 * static_cast<size_t>(t);
    double g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int32_t n = nbr[3 * t + k];
        if (n < 0) {
            g[k] = -1.0 / 2;
            continue;
        }
        const int32_t n0 = tri[3 * n], n1 = tri[3 * n + 1], n2 = tri[3 * n + 2];
        const double yx = (pts[2 * n0] + pts[2 * n1] + pts[2 * n2]) / 3;          // the neighbour's centroid ...
        const double yy = (pts[2 * n0 + 1] + pts[2 * n1 + 1] + pts[2 * n2 + 1]) / 3;
        const double dx = yx - T[4], dy = yy - T[5];                                // ... in this triangle's coordinates
        double c[3];
        c[0] = T[0] * dx + T[1] * dy;
        c[1] = T[2] * dx + T[3] * dy;
        c[2] = 1.0 - c[0] - c[1];
        const double a = c[(k + 2) % 3], bb = c[(k + 1) % 3];
        g[k] = (2 * a + bb - 1) / (2 - 3 * a - 3 * bb);
    }
    const double c0111 = (g[0] * (-c0300 + 3 * c0210 - 3 * c0120 + c0030) + (-c0300 + 2 * c0210 - c0120 + c0021 + c0201)) / 2;
    const double c1011 = (g[1] * (-c0030 + 3 * c1020 - 3 * c2010 + c3000) + (-c0030 + 2 * c1020 - c2010 + c2001 + c0021)) / 2;
    const double c1101 = (g[2] * (-c3000 + 3 * c2100 - 3 * c1200 + c0300) + (-c3000 + 2 * c2100 - c1200 + c2001 + c0201)) / 2;
    const double c1002 = (c1101 + c1011 + c2001) / 3;
    const double c0102 = (c1101 + c0111 + c0201) / 3;
    const double c0012 = (c1011 + c0111 + c0021) / 3;
    const double c0003 = (c1002 + c0102 + c0012) / 3;
    double *o = coef + q * kCT;
    o[0] = c3000;  o[1] = c2100;  o[2] = c2010;  o[3] = c2001;  o[4] = c1200;  o[5] = c1101;  o[6] = c1020;
    o[7] = c1011;  o[8] = c1002;  o[9] = c0300;  o[10] = c0210; o[11] = c0201; o[12] = c0120; o[13] = c0111;
    o[14] = c0102; o[15] = c0030; o[16] = c0021; o[17] = c0012; o[18] = c0003;
}

// (east, north) of every snapshot at one cell from its 19 monomials; cf: the owner's [field][19] block
__device__ __forceinline__ void ct_store(const double *__restrict__ cf, const double (&mono)[kCT], int batch, size_t ncell,
                                         size_t i, double *__restrict__ wspeed, double *__restrict__ wdirn)
{
    for (int b = 0; b < batch; ++b, cf += 2 * kCT) {
        const double e = ct_eval(mono, cf), n = ct_eval(mono, cf + kCT);
        wspeed[b * ncell + i] = sqrt(e * e + n * n);
        wdirn[b * ncell + i] = fmod(atan2(e, n) + 2.0 * kPi, 2.0 * kPi) * 180.0 / kPi;
    }
}

// One thread per cell, all snapshots: owner -> barycentric coordinates -> the 19 monomials of the four shifted
// coordinates, once; then 2 x 19 multiply-adds per snapshot and the u/v recipe.  A triangle of a 2 km lattice covers
// some 20 000 cells at 10 m, so nearly every wave has ONE owner: its transform and coefficients are then read through
// a wave-uniform pointer (scalar loads); a wave that straddles an edge takes the same code with per-lane pointers.
__global__ __launch_bounds__(kBlock) void k_wind_cubic(const int32_t *__restrict__ owner, const double *__restrict__ transform,
                                                      const double *__restrict__ coef, double cell,
                                                      double *__restrict__ wspeed, double *__restrict__ wdirn, int rows,
                                                      int cols, int batch)
{
    const size_t ncell = static_cast<size_t>(rows) * cols;
    const size_t stride = static_cast<size_t>(2 * batch) * kCT;
    const int lane = threadIdx.x & 63;
    for (size_t base = blockIdx.x * static_cast<size_t>(kBlock) + (threadIdx.x - lane); base < ncell;
         base += static_cast<size_t>(gridDim.x) * kBlock) {
        const size_t i = base + lane;
        if (i >= ncell) continue;
        const int32_t t = owner[i];
        if (t == kNoOwner) {                                          // outside the hull: griddata's fill value
            const double nan = quiet_nan();
            for (int b = 0; b < batch; ++b) {
                wspeed[b * ncell + i] = nan;
                wdirn[b * ncell + i] = nan;
            }
            continue;
        }
        // (readfirstlane and __ballot see the lanes that reached this point: those with an owner)
        const int32_t t0 = __builtin_amdgcn_readfirstlane(t);
        const bool uniform = __ballot(t != t0) == 0ull;
        const size_t tt = static_cast<size_t>(uniform ? t0 : t);
        const int r = static_cast<int>(i / cols), c = static_cast<int>(i % cols);
        double b0, b1, b2, mono[kCT];
        tri_barycentric(transform + 6 * tt, r, c, cell, b0, b1, b2);
        ct_monomials(b0, b1, b2, mono);
        if (uniform)
            ct_store(coef + static_cast<size_t>(t0) * stride, mono, batch, ncell, i, wspeed, wdirn);
        else
            ct_store(coef + static_cast<size_t>(t) * stride, mono, batch, ncell, i, wspeed, wdirn);
    }
}

constexpr int kNearestTable = 3072;                                    // samples whose (speed, direction) fit 48 KB of LDS

int launch_tri_owner(const double *points, const int32_t *triangles, const double *transform, int ntri, double cell,
                     int rows, int cols, int32_t *owner, hipStream_t st)
{
    SSRS_HIP_CHECK(hipMemsetAsync(owner, 0x7f, static_cast<size_t>(rows) * cols * sizeof(int32_t), st));   // kNoOwner: above any index
    hipLaunchKernelGGL(k_tri_owner, dim3(static_cast<unsigned>(ntri), 64), dim3(kBlock), 0, st, points, triangles, transform, ntri,
                       cell, rows, cols, owner);
    return SSRS_OK;
}

int launch_ct_coefficients(const double *points, const int32_t *triangles, const int32_t *neighbors,
                           const double *transform, const double *val_even, const double *val_odd,
                           const double *grad_even, const double *grad_odd, size_t pair_stride, int ntri, int nfield,
                           double *coef, hipStream_t st)
{
    const size_t ncoef = static_cast<size_t>(ntri) * nfield;
    hipLaunchKernelGGL(k_ct_coefficients, dim3(static_cast<unsigned>((ncoef + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, points,
                       triangles, neighbors, transform, val_even, val_odd, grad_even, grad_odd, pair_stride, ntri, nfield, coef);
    return SSRS_OK;
}

}  // namespace ssrs

extern "C" size_t ssrs_wind_nearest_workspace_bytes(int npts, int rows, int cols)
{
    if (npts <= 0 || rows <= 0 || cols <= 0) return 0;
    return 256;
}

extern "C" int ssrs_wind_nearest_index(const double *points, int npts, double cell_size, int32_t *index, int rows, int cols,
                                       void *workspace, size_t workspace_bytes, void *stream)
{
    SSRS_REQUIRE(points && index, "ssrs_wind_nearest_index: NULL pointer");
    SSRS_REQUIRE(npts >= 1 && rows > 0 && cols > 0, "ssrs_wind_nearest_index: bad sizes");
    SSRS_REQUIRE(cell_size > 0.0, "ssrs_wind_nearest_index: cell_size must be > 0");
    SSRS_REQUIRE(workspace && workspace_bytes >= ssrs_wind_nearest_workspace_bytes(npts, rows, cols),
                 "ssrs_wind_nearest_index: workspace too small");
    const int tiles_x = (cols + TW - 1) / TW, tiles_y = (rows + TH - 1) / TH;
    hipStream_t st = as_stream(stream);
    SSRS_HIP_CHECK(hipMemsetAsync(workspace, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_nearest_index, dim3(static_cast<unsigned>(tiles_x) * tiles_y), dim3(kBlock), 0, st, points, npts,
                       cell_size, rows, cols, tiles_x, index, static_cast<int32_t *>(workspace));
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

extern "C" int ssrs_wind_from_nearest(const int32_t *index, const double *speed, const double *dirn, int npts,
                                      double *wspeed, double *wdirn, int rows, int cols, int batch, void *stream)
{
    SSRS_REQUIRE(index && speed && dirn && wspeed && wdirn, "ssrs_wind_from_nearest: NULL pointer");
    SSRS_REQUIRE(npts >= 1 && rows > 0 && cols > 0 && batch > 0 && batch <= 65535, "ssrs_wind_from_nearest: bad sizes");
    const size_t ncell = static_cast<size_t>(rows) * cols;
    const int table = npts <= kNearestTable;
    int nbx = kMaxStreamBlocks / batch;
    nbx = nbx < 64 ? 64 : nbx;
    const size_t need = (ncell + kBlock - 1) / kBlock;
    if (static_cast<size_t>(nbx) > need) nbx = static_cast<int>(need);
    hipLaunchKernelGGL(k_wind_nearest, dim3(nbx, batch), dim3(kBlock), table ? 2 * sizeof(double) * npts : 0, as_stream(stream),
                       index, speed, dirn, npts, wspeed, wdirn, ncell, table);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

extern "C" size_t ssrs_wind_cubic_workspace_bytes(int npts, int ntri, int rows, int cols, int batch)
{
    if (npts < 3 || ntri <= 0 || rows <= 0 || cols <= 0 || batch <= 0) return 0;
    return align256(static_cast<size_t>(rows) * cols * sizeof(int32_t)) +
           static_cast<size_t>(ntri) * 2 * batch * kCT * sizeof(double) + 512;
}

extern "C" int ssrs_wind_from_triangles_cubic(const double *points, const int32_t *triangles, const int32_t *neighbors,
                                              const double *transform, const double *east, const double *north,
                                              const double *grad_east, const double *grad_north, int npts, int ntri,
                                              double cell_size, double *wspeed, double *wdirn, int rows, int cols, int batch,
                                              void *workspace, size_t workspace_bytes, void *stream)
{
    SSRS_REQUIRE(points && triangles && neighbors && transform && east && north && grad_east && grad_north && wspeed && wdirn,
                 "ssrs_wind_from_triangles_cubic: NULL pointer");
    SSRS_REQUIRE(npts >= 3 && ntri >= 1 && rows > 0 && cols > 0 && batch > 0, "ssrs_wind_from_triangles_cubic: bad sizes");
    SSRS_REQUIRE(cell_size > 0.0, "ssrs_wind_from_triangles_cubic: cell_size must be > 0");
    SSRS_REQUIRE(workspace && workspace_bytes >= ssrs_wind_cubic_workspace_bytes(npts, ntri, rows, cols, batch),
                 "ssrs_wind_from_triangles_cubic: workspace too small");
    hipStream_t st = as_stream(stream);
    const size_t ncell = static_cast<size_t>(rows) * cols;
    int32_t *owner = static_cast<int32_t *>(workspace);
    double *coef = reinterpret_cast<double *>(static_cast<char *>(workspace) + align256(ncell * sizeof(int32_t)));
    launch_ct_coefficients(points, triangles, neighbors, transform, east, north, grad_east, grad_north,
                           static_cast<size_t>(npts), ntri, 2 * batch, coef, st);
    if (int rc = launch_tri_owner(points, triangles, transform, ntri, cell_size, rows, cols, owner, st)) return rc;
    hipLaunchKernelGGL(k_wind_cubic, dim3(stream_grid(ncell)), dim3(kBlock), 0, st, owner, transform, coef, cell_size, wspeed,
                       wdirn, rows, cols, batch);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}
