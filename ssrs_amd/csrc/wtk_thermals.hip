// The physical thermal model of the reference (ssrs/layers.py:25-60) and the general scalar interpolation that feeds
// it (ssrs/simulator.py:765-776), on the device:
//   a. three elementwise f64 kernels: potential temperature, Deardorff velocity, thermal updraft at height z;
//   b. k_scalar_interp: griddata's 'nearest' | 'linear' | 'cubic' of any number of scalar sample vectors;
//   c. k_wtk_thermals: b. on the four WTK layers of `batch` snapshots, then a., per cell and in registers.
// b. and c. evaluate a cell through the helpers of interp.h, which the wind kernels use too, and a. and c. share
// the three __device__ functions below: with -ffp-contract=off the fused kernel gives the bits of the chain.
#include "common.h"
#include "interp.h"

namespace ssrs {

// np.maximum / np.minimum / ndarray.clip propagate NaN; fmax / fmin would drop it
__device__ __forceinline__ double np_maximum(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
__device__ __forceinline__ double np_minimum(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }

// Which NaN an operation hands on (sign, payload) is not part of IEEE arithmetic and differs between the inlined
// copies of pow: every function below returns ONE NaN, so that NaN results too are the same bits wherever they are
// computed.
__device__ __forceinline__ double one_nan(double v) { return v != v ? quiet_nan() : v; }

// layers.py:40-48, degrees Celsius in and out
__device__ __forceinline__ double potential_temperature(double pressure, double temperature)
{
    const double temp_k = temperature + 273.15;
    const double temp_r = 1e5 / pressure;
    return one_nan(temp_k * pow(temp_r, 0.2857) - 273.15);
}

// layers.py:25-37 (np.power of a negative base is NaN, as pow; cbrt would not be)
__device__ __forceinline__ double deardorff_velocity(double pot_temperature, double blayer_height, double surface_heat_flux,
                                                     double min_updraft_val)
{
    const double fac = 9.8 / 1216.;
    const double pot_temp_kelvin = pot_temperature + 273.15;
    const double pos_heat_flux = np_maximum(surface_heat_flux, 0.);
    const double mod_blheight = np_maximum(blayer_height, 100.);
    return one_nan(np_maximum(min_updraft_val, pow(fac * ((mod_blheight * pos_heat_flux) / pot_temp_kelvin), 1. / 3.)));
}

// layers.py:51-60; blayer_height is NOT clipped here (the reference does not)
__device__ __forceinline__ double thermal_updraft(double z, double deardorff_vel, double blayer_height, double min_updraft_val)
{
    const double zbyzi = np_minimum(np_maximum(z / blayer_height, 0.), 1.);
    const double emat = 0.85 * (pow(zbyzi, 1. / 3.) * (1.3 - zbyzi));
    return one_nan(np_maximum(min_updraft_val, deardorff_vel * emat));
}

__global__ __launch_bounds__(kBlock) void k_potential_temperature(const double *__restrict__ pressure,
                                                                 const double *__restrict__ temperature,
                                                                 double *__restrict__ out, size_t n)
{
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * kBlock)
        out[i] = potential_temperature(pressure[i], temperature[i]);
}

__global__ __launch_bounds__(kBlock) void k_deardorff_velocity(const double *__restrict__ pot_temperature,
                                                              const double *__restrict__ blayer_height,
                                                              const double *__restrict__ surface_heat_flux,
                                                              double min_updraft_val, double *__restrict__ out, size_t n)
{
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * kBlock)
        out[i] = deardorff_velocity(pot_temperature[i], blayer_height[i], surface_heat_flux[i], min_updraft_val);
}

__global__ __launch_bounds__(kBlock) void k_thermal_updraft(const double *__restrict__ zmat, double z0,
                                                           const double *__restrict__ deardorff_vel,
                                                           const double *__restrict__ blayer_height,
                                                           double min_updraft_val, double *__restrict__ out, size_t n)
{
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * kBlock)
        out[i] = thermal_updraft(zmat ? zmat[i] : z0, deardorff_vel[i], blayer_height[i], min_updraft_val);
}

// ---------------------------------------------------------------------------------------------------------------
// Where a cell sits among the samples, found once per cell and used for every field: the nearest sample ('nearest'),
// the owner triangle's vertices and barycentric coordinates ('linear'), or the owner and the 19 monomials ('cubic').
// `cellmap` is the index raster of ssrs_wind_nearest_index or the owner raster of k_tri_owner.
struct SampleGeometry {
    const int32_t *cellmap;       // (rows, cols)
    const int32_t *tri;           // (ntri, 3)
    const double *transform;      // (ntri, 3, 2)
    const double *coef;           // [ntri][nfield][19], cubic
    const double *values;         // (nfield, npts)
    int npts, nfield;
    double cell;
};

template <int METHOD>
struct CellSite;

template <>
struct CellSite<SSRS_INTERP_NEAREST> {
    int32_t k;
    __device__ __forceinline__ bool locate(const SampleGeometry &g, size_t i, int, int)
    {
        k = g.cellmap[i];
        return static_cast<uint32_t>(k) < static_cast<uint32_t>(g.npts);
    }
    __device__ __forceinline__ int32_t owner() const { return k; }
    __device__ __forceinline__ double field(const SampleGeometry &g, int f, int32_t) const
    {
        return g.values[static_cast<size_t>(f) * g.npts + k];
    }
};

template <>
struct CellSite<SSRS_INTERP_LINEAR> {
    int32_t v0, v1, v2;
    double b0, b1, b2;
    __device__ __forceinline__ bool locate(const SampleGeometry &g, size_t i, int r, int c)
    {
        const int32_t t = g.cellmap[i];
        if (t == kNoOwner) return false;
        tri_barycentric(g.transform + 6 * static_cast<size_t>(t), r, c, g.cell, b0, b1, b2);
        v0 = g.tri[3 * t];
        v1 = g.tri[3 * t + 1];
        v2 = g.tri[3 * t + 2];
        return true;
    }
    __device__ __forceinline__ int32_t owner() const { return 0; }
    __device__ __forceinline__ double field(const SampleGeometry &g, int f, int32_t) const
    {
        return tri_linear(b0, b1, b2, g.values + static_cast<size_t>(f) * g.npts, v0, v1, v2);
    }
};

template <>
struct CellSite<SSRS_INTERP_CUBIC> {
    int32_t t;
    double mono[kCT];
    __device__ __forceinline__ bool locate(const SampleGeometry &g, size_t i, int r, int c)
    {
        t = g.cellmap[i];
        if (t == kNoOwner) return false;
        double b0, b1, b2;
        tri_barycentric(g.transform + 6 * static_cast<size_t>(t), r, c, g.cell, b0, b1, b2);
        ct_monomials(b0, b1, b2, mono);
        return true;
    }
    __device__ __forceinline__ int32_t owner() const { return t; }
    // `tt`: this cell's owner, handed back by the caller so that a wave with ONE owner can pass it as a wave-uniform
    // value (the ordinates then come through scalar loads, as in k_wind_cubic)
    __device__ __forceinline__ double field(const SampleGeometry &g, int f, int32_t tt) const
    {
        return ct_eval(mono, g.coef + (static_cast<size_t>(tt) * g.nfield + f) * kCT);
    }
};

// b. one thread per cell, every field: out (nfield, rows, cols) f64, NaN where the cell has no sample geometry
template <int METHOD>
__global__ __launch_bounds__(kBlock) void k_scalar_interp(SampleGeometry g, double *__restrict__ out, int rows, int cols)
{
    const size_t ncell = static_cast<size_t>(rows) * cols;
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < ncell; i += static_cast<size_t>(gridDim.x) * kBlock) {
        const int r = static_cast<int>(i / cols), c = static_cast<int>(i % cols);
        CellSite<METHOD> site;
        const bool ok = site.locate(g, i, r, c);
        for (int f = 0; f < g.nfield; ++f) out[f * ncell + i] = ok ? site.field(g, f, site.owner()) : quiet_nan();
    }
}

// c. One lane owns kLaneCells consecutive cells of a row, so that its f32 results leave as one 16-byte store.  Per
// lane: the sites of its cells once; per snapshot the four layers at each site, the three functions of a., the store.
// Layer l of snapshot b is field l * batch + b of the geometry (pressure, temperature, blheight, surfheatflux).
// The loop is wave-granular (lanes past the end carry no valid cell) so that the owner test below sees whole waves.
constexpr int kLaneCells = 4;

template <typename T>
struct alignas(kLaneCells * sizeof(T)) LanePack {
    T v[kLaneCells];
};

template <int METHOD, typename Tout>
__device__ __forceinline__ void wtk_store(const SampleGeometry &g, const CellSite<METHOD> (&site)[kLaneCells],
                                          const bool (&ok)[kLaneCells], const int32_t (&tt)[kLaneCells],
                                          const double (&z)[kLaneCells], double min_updraft_val, int batch, size_t ncell,
                                          size_t i0, int ncells, bool packed, Tout *__restrict__ out)
{
    for (int b = 0; b < batch; ++b) {
        LanePack<Tout> w;
#pragma unroll
        for (int j = 0; j < kLaneCells; ++j) {
            // a cell without sample geometry carries NaN through the same three functions, as the chain does
            double pressure = quiet_nan(), temperature = pressure, blheight = pressure, surfheatflux = pressure;
            if (ok[j]) {
                pressure = site[j].field(g, b, tt[j]);
                temperature = site[j].field(g, batch + b, tt[j]);
                blheight = site[j].field(g, 2 * batch + b, tt[j]);
                surfheatflux = site[j].field(g, 3 * batch + b, tt[j]);
            }
            const double theta = potential_temperature(pressure, temperature);
            const double wstar = deardorff_velocity(theta, blheight, surfheatflux, min_updraft_val);
            const double u = thermal_updraft(z[j], wstar, blheight, min_updraft_val);
            w.v[j] = static_cast<Tout>(u);
        }
        Tout *o = out + b * ncell + i0;
        if (packed) {
            *reinterpret_cast<LanePack<Tout> *>(o) = w;
        } else {
#pragma unroll
            for (int j = 0; j < kLaneCells; ++j)
                if (j < ncells) o[j] = w.v[j];
        }
    }
}

template <int METHOD, typename Tout>
__global__ __launch_bounds__(kBlock) void k_wtk_thermals(SampleGeometry g, const double *__restrict__ zmat, double z0,
                                                        double min_updraft_val, Tout *__restrict__ out, int rows, int cols,
                                                        int batch, int packed)
{
    const size_t ncell = static_cast<size_t>(rows) * cols;
    const int per_row = (cols + kLaneCells - 1) / kLaneCells;
    const size_t ngroup = static_cast<size_t>(rows) * per_row;
    const int lane = threadIdx.x & 63;
    for (size_t base = blockIdx.x * static_cast<size_t>(kBlock) + (threadIdx.x - lane); base < ngroup;
         base += static_cast<size_t>(gridDim.x) * kBlock) {
        const size_t q = base + lane;
        const bool live = q < ngroup;
        const int r = live ? static_cast<int>(q / per_row) : 0, c0 = live ? static_cast<int>(q % per_row) * kLaneCells : 0;
        const size_t i0 = static_cast<size_t>(r) * cols + c0;
        const int ncells = live ? (cols - c0 < kLaneCells ? cols - c0 : kLaneCells) : 0;
        CellSite<METHOD> site[kLaneCells];
        bool ok[kLaneCells];
        int32_t tt[kLaneCells];
        double z[kLaneCells];
        int32_t mine = kNoOwner;                                       // an owner among this lane's cells
#pragma unroll
        for (int j = 0; j < kLaneCells; ++j) {
            ok[j] = j < ncells && site[j].locate(g, i0 + j, r, c0 + j);
            tt[j] = ok[j] ? site[j].owner() : 0;
            z[j] = j < ncells && zmat ? zmat[i0 + j] : z0;
            if (ok[j]) mine = tt[j];
        }
        if (METHOD == SSRS_INTERP_CUBIC) {
            // a triangle of a 2 km lattice covers some 20 000 cells at 10 m: nearly every wave has ONE owner, whose
            // ordinates are then read through a wave-uniform pointer; a wave that straddles an edge takes the same
            // code with per-lane pointers.  Same loads, same sums: the bits do not depend on the path.
            const unsigned long long has = __ballot(mine != kNoOwner);
            if (has != 0ull) {
                const int32_t t0 = __builtin_amdgcn_readfirstlane(__shfl(mine, __ffsll(static_cast<long long>(has)) - 1));
                bool same = true;
#pragma unroll
                for (int j = 0; j < kLaneCells; ++j) same = same && (!ok[j] || tt[j] == t0);
                if (__ballot(!same) == 0ull) {
                    const int32_t uni[kLaneCells] = {t0, t0, t0, t0};
                    if (live) wtk_store<METHOD, Tout>(g, site, ok, uni, z, min_updraft_val, batch, ncell, i0, ncells, packed != 0, out);
                    continue;
                }
            }
        }
        if (live) wtk_store<METHOD, Tout>(g, site, ok, tt, z, min_updraft_val, batch, ncell, i0, ncells, packed != 0, out);
    }
}

static inline bool interp_method_ok(int method)
{
    return method == SSRS_INTERP_NEAREST || method == SSRS_INTERP_LINEAR || method == SSRS_INTERP_CUBIC;
}

// the geometry kernels of raster.hip into `workspace`: owner raster ('linear', 'cubic'), ordinate table ('cubic')
static int prepare_geometry(int method, const double *points, const int32_t *triangles, const int32_t *neighbors,
                            const double *transform, const int32_t *index, const double *values, const double *grad,
                            int npts, int ntri, double cell, int rows, int cols, int nfield, void *workspace,
                            hipStream_t st, SampleGeometry &g)
{
    g = SampleGeometry{index, triangles, transform, nullptr, values, npts, nfield, cell};
    if (method == SSRS_INTERP_NEAREST) return SSRS_OK;
    int32_t *owner = static_cast<int32_t *>(workspace);
    g.cellmap = owner;
    if (method == SSRS_INTERP_CUBIC) {
        double *coef = reinterpret_cast<double *>(static_cast<char *>(workspace) +
                                                  align256(static_cast<size_t>(rows) * cols * sizeof(int32_t)));
        const size_t n = static_cast<size_t>(npts);
        launch_ct_coefficients(points, triangles, neighbors, transform, values, values + n, grad, grad + 2 * n, 2 * n, ntri,
                               nfield, coef, st);
        g.coef = coef;
    }
    return launch_tri_owner(points, triangles, transform, ntri, cell, rows, cols, owner, st);
}

#define SSRS_REQUIRE_GEOMETRY(name)                                                                                     \
    do {                                                                                                                \
        SSRS_REQUIRE(interp_method_ok(method), name ": method must be SSRS_INTERP_NEAREST, _LINEAR or _CUBIC");        \
        SSRS_REQUIRE(rows > 0 && cols > 0 && cell_size > 0.0, name ": rows, cols and cell_size must be > 0");          \
        if (method == SSRS_INTERP_NEAREST) {                                                                            \
            SSRS_REQUIRE(index, name ": 'nearest' needs the index raster of ssrs_wind_nearest_index");                 \
            SSRS_REQUIRE(npts >= 1, name ": bad sizes");                                                                \
        } else {                                                                                                        \
            SSRS_REQUIRE(points && triangles && transform, name ": NULL pointer");                                     \
            SSRS_REQUIRE(npts >= 3 && ntri >= 1, name ": bad sizes");                                                   \
            SSRS_REQUIRE(method != SSRS_INTERP_CUBIC || (neighbors && grad),                                            \
                         name ": 'cubic' needs neighbors and the vertex gradients");                                   \
        }                                                                                                               \
    } while (0)

}  // namespace ssrs

using namespace ssrs;

extern "C" int ssrs_potential_temperature(const double *pressure, const double *temperature, double *out, size_t n,
                                          void *stream)
{
    SSRS_REQUIRE(pressure && temperature && out, "ssrs_potential_temperature: NULL pointer");
    SSRS_REQUIRE(n > 0, "ssrs_potential_temperature: n must be > 0");
    hipLaunchKernelGGL(k_potential_temperature, dim3(stream_grid(n)), dim3(kBlock), 0, as_stream(stream), pressure,
                       temperature, out, n);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

extern "C" int ssrs_deardorff_velocity(const double *pot_temperature, const double *blayer_height,
                                       const double *surface_heat_flux, double min_updraft_val, double *out, size_t n,
                                       void *stream)
{
    SSRS_REQUIRE(pot_temperature && blayer_height && surface_heat_flux && out, "ssrs_deardorff_velocity: NULL pointer");
    SSRS_REQUIRE(n > 0, "ssrs_deardorff_velocity: n must be > 0");
    hipLaunchKernelGGL(k_deardorff_velocity, dim3(stream_grid(n)), dim3(kBlock), 0, as_stream(stream), pot_temperature,
                       blayer_height, surface_heat_flux, min_updraft_val, out, n);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

extern "C" int ssrs_thermal_updraft(const double *zmat, double z0, const double *deardorff_vel, const double *blayer_height,
                                    double min_updraft_val, double *out, size_t n, void *stream)
{
    SSRS_REQUIRE(deardorff_vel && blayer_height && out, "ssrs_thermal_updraft: NULL pointer");
    SSRS_REQUIRE(n > 0, "ssrs_thermal_updraft: n must be > 0");
    hipLaunchKernelGGL(k_thermal_updraft, dim3(stream_grid(n)), dim3(kBlock), 0, as_stream(stream), zmat, z0, deardorff_vel,
                       blayer_height, min_updraft_val, out, n);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

extern "C" size_t ssrs_scalar_interp_workspace_bytes(int method, int ntri, int rows, int cols, int nfields)
{
    if (!interp_method_ok(method) || rows <= 0 || cols <= 0 || nfields <= 0) return 0;
    if (method == SSRS_INTERP_NEAREST) return 256;
    if (ntri <= 0) return 0;
    size_t n = align256(static_cast<size_t>(rows) * cols * sizeof(int32_t));
    if (method == SSRS_INTERP_CUBIC) n += static_cast<size_t>(ntri) * nfields * kCT * sizeof(double);
    return n + 256;
}

extern "C" int ssrs_scalar_from_samples(int method, const double *points, const int32_t *triangles, const int32_t *neighbors,
                                        const double *transform, const int32_t *index, const double *values,
                                        const double *grad, int npts, int ntri, double cell_size, double *out, int rows,
                                        int cols, int nfields, void *workspace, size_t workspace_bytes, void *stream)
{
    SSRS_REQUIRE(values && out, "ssrs_scalar_from_samples: NULL pointer");
    SSRS_REQUIRE(nfields > 0, "ssrs_scalar_from_samples: nfields must be > 0");
    SSRS_REQUIRE_GEOMETRY("ssrs_scalar_from_samples");
    SSRS_REQUIRE(workspace && workspace_bytes >= ssrs_scalar_interp_workspace_bytes(method, ntri, rows, cols, nfields),
                 "ssrs_scalar_from_samples: workspace too small");
    hipStream_t st = as_stream(stream);
    SampleGeometry g;
    if (int rc = prepare_geometry(method, points, triangles, neighbors, transform, index, values, grad, npts, ntri, cell_size,
                                  rows, cols, nfields, workspace, st, g))
        return rc;
    const dim3 grid(stream_grid(static_cast<size_t>(rows) * cols)), block(kBlock);
    if (method == SSRS_INTERP_NEAREST)
        hipLaunchKernelGGL((k_scalar_interp<SSRS_INTERP_NEAREST>), grid, block, 0, st, g, out, rows, cols);
    else if (method == SSRS_INTERP_LINEAR)
        hipLaunchKernelGGL((k_scalar_interp<SSRS_INTERP_LINEAR>), grid, block, 0, st, g, out, rows, cols);
    else
        hipLaunchKernelGGL((k_scalar_interp<SSRS_INTERP_CUBIC>), grid, block, 0, st, g, out, rows, cols);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

template <typename Tout>
static void launch_wtk_thermals(int method, const SampleGeometry &g, const double *zmat, double z0, double min_updraft_val,
                                void *out, int rows, int cols, int batch, hipStream_t st)
{
    const size_t ngroup = static_cast<size_t>(rows) * ((cols + kLaneCells - 1) / kLaneCells);
    // whole lanes' worth of cells per row and a store-aligned base: one 16-byte (f32) / 32-byte (f64) store per lane
    const int packed = cols % kLaneCells == 0 && reinterpret_cast<uintptr_t>(out) % (kLaneCells * sizeof(Tout)) == 0;
    const dim3 grid(stream_grid(ngroup)), block(kBlock);
    Tout *o = static_cast<Tout *>(out);
    if (method == SSRS_INTERP_NEAREST)
        hipLaunchKernelGGL((k_wtk_thermals<SSRS_INTERP_NEAREST, Tout>), grid, block, 0, st, g, zmat, z0, min_updraft_val, o, rows,
                           cols, batch, packed);
    else if (method == SSRS_INTERP_LINEAR)
        hipLaunchKernelGGL((k_wtk_thermals<SSRS_INTERP_LINEAR, Tout>), grid, block, 0, st, g, zmat, z0, min_updraft_val, o, rows,
                           cols, batch, packed);
    else
        hipLaunchKernelGGL((k_wtk_thermals<SSRS_INTERP_CUBIC, Tout>), grid, block, 0, st, g, zmat, z0, min_updraft_val, o, rows,
                           cols, batch, packed);
}

extern "C" int ssrs_wtk_thermal_fields(int method, const double *points, const int32_t *triangles, const int32_t *neighbors,
                                       const double *transform, const int32_t *index, const double *layers,
                                       const double *grad, int npts, int ntri, double cell_size, const double *zmat,
                                       double z0, double min_updraft_val, void *out, int out_is_f32, int rows, int cols,
                                       int batch, void *workspace, size_t workspace_bytes, void *stream)
{
    SSRS_REQUIRE(layers && out, "ssrs_wtk_thermal_fields: NULL pointer");
    SSRS_REQUIRE(batch > 0 && batch <= (1 << 20), "ssrs_wtk_thermal_fields: bad batch");
    SSRS_REQUIRE_GEOMETRY("ssrs_wtk_thermal_fields");
    SSRS_REQUIRE(workspace && workspace_bytes >= ssrs_scalar_interp_workspace_bytes(method, ntri, rows, cols, 4 * batch),
                 "ssrs_wtk_thermal_fields: workspace too small");
    hipStream_t st = as_stream(stream);
    SampleGeometry g;
    if (int rc = prepare_geometry(method, points, triangles, neighbors, transform, index, layers, grad, npts, ntri, cell_size,
                                  rows, cols, 4 * batch, workspace, st, g))
        return rc;
    if (out_is_f32)
        launch_wtk_thermals<float>(method, g, zmat, z0, min_updraft_val, out, rows, cols, batch, st);
    else
        launch_wtk_thermals<double>(method, g, zmat, z0, min_updraft_val, out, rows, cols, batch, st);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}
