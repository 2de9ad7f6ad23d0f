/* ssrs_hip.h -- C ABI of libssrs_hip.so, the MI355X (gfx950) implementation of
 * the SSRS data-parallel hot path: the updraft raster and the stochastic track
 * stepper.
 *
 * SSRS has no FFI/plugin seam of its own: the boundary this library replaces
 * is the set of module-level numeric functions that ssrs/simulator.py imports
 * by name (/root/reference/ssrs/simulator.py:21-28).  Each entry point below
 * cites the reference function it stands in for; INTEGRATION.md shows the
 * ctypes stub a maintainer of the reference would add at each call site.
 *
 * Conventions
 *  - every array pointer is CALLER-OWNED DEVICE memory (e.g. a torch tensor's
 *    data_ptr()), row-major (rows, cols), row 0 = south, unless marked [host];
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *  - raster entry points are asynchronous on `stream`; ssrs_tracks_simulate
 *    drives a launch loop and returns after the last launch has completed;
 *    every launch, memset and copy of an export goes to `stream` and nowhere else.
 *    An export whose comment says it waits for `stream` once needs a value on the
 *    host (a size, a flag, a host temporary it is about to drop); it puts its
 *    launches to `stream` in order like the others;
 *  - return value: SSRS_OK (0) or a negative SSRS_ERR_* code, with a
 *    thread-local message available from ssrs_last_error();
 *  - no hidden global state: the random stream is a pure function of
 *    (seed, global track id, step) -- see "Uniform contract" below;
 *  - thread-safe for distinct streams / devices.
 *
 * Uniform contract (replaces the reference's serial global MT19937 draw in
 * np.random.choice, movmodel.py:312, which no parallel run can reproduce):
 *   u(seed, track, step) = ((a >> 5) * 2^26 + (b >> 6)) / 2^53,
 *   (a, b) = words (0,1) [even step] or (2,3) [odd step] of
 *   Philox4x32-10(key = {seed lo, seed hi},
 *                 ctr = {blk lo, blk hi, track lo, track hi}),  blk = step >> 1,
 * i.e. exactly rocRAND's rocrand_init(seed, track, 2*step) + 2 x rocrand().
 */
#ifndef SSRS_HIP_H_
#define SSRS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSRS_VERSION 109 /* 0.1.9 */

#define SSRS_OK 0
#define SSRS_ERR_INVALID (-1) /* bad argument (message says which) */
#define SSRS_ERR_HIP (-2)     /* a HIP runtime call failed */
#define SSRS_ERR_START (-3)   /* a start cell lies outside the raster */

/* element type selectors for `const void*` rasters */
#define SSRS_F32 0
#define SSRS_F64 1

int ssrs_version(void);
/* bit 0: a timing-probe build of the library (a kernel stage is stubbed out on purpose, results are
 * wrong): product code, tests and bench.py refuse to run against it */
int ssrs_build_flags(void);
const char *ssrs_last_error(void);
/* name[] receives the device name; returns SSRS_OK or SSRS_ERR_HIP */
int ssrs_device_info(int device, char *name, size_t name_len, int *compute_units,
                     size_t *hbm_bytes);

/* ------------------------------------------------------------------ raster */

/* compute_slope_degrees + compute_aspect_degrees (ssrs/layers.py:63-128):
 * Horn 3x3 gradients on the DEM, slope = deg(atan|grad|), aspect per :124-127,
 * border cells 0.  slope or aspect may be NULL.  f64 arithmetic. */
int ssrs_slope_aspect(const void *dem, int dem_type, double res, void *slope,
                      void *aspect, int out_type, int rows, int cols, void *stream);

/* compute_orographic_updraft (ssrs/layers.py:11-22) for `batch` wind cases over
 * one terrain, optionally fused with get_above_threshold_speed
 * (ssrs/layers.py:171-185, applied to the f32-rounded orograph exactly as
 * Simulator.load_updrafts does after np.save(float32), simulator.py:198,233-242).
 *   slope, aspect   (rows, cols) of in_type
 *   wspeed, wdirn   NULL -> uniform mode, wspeed0[b] / wdirn0[b] ([host], length
 *                   batch); else (batch, rows, cols) rasters of wind_type
 *   orograph        (batch, rows, cols) f32 out, may be NULL
 *   threshold       < 0 -> `usable` is not written
 *   usable          (batch, rows, cols) f64 out (thresholded updraft), may be NULL */
int ssrs_orographic_updraft(const void *slope, const void *aspect, int in_type,
                            const void *wspeed, const void *wdirn, int wind_type,
                            const double *wspeed0, const double *wdirn0,
                            double min_updraft_val, float *orograph,
                            double threshold, double *usable, int rows, int cols,
                            int batch, void *stream);

/* get_above_threshold_speed (ssrs/layers.py:171-185) on n f32 values -> f64. */
int ssrs_threshold_updraft(const float *in, double threshold, double *out,
                           size_t n, void *stream);

/* Fused DEM -> orographic updraft (-> usable updraft): slope/aspect/orographic/
 * threshold of layers.py:11-22,63-128,171-185 in one pass over an LDS-staged
 * DEM tile, uniform wind.  Trig-free: sin(slope) cos(aspect - wdirn) is
 * evaluated from the Horn gradients directly (DESIGN.md "K1"); results agree
 * with the reference expression to a few f64 ulps before the f32 rounding.
 * orograph / usable as above (batch = 1). */
int ssrs_updraft_from_dem(const void *dem, int dem_type, double res, double wspeed,
                          double wdirn, double min_updraft_val, float *orograph,
                          double threshold, double *usable, int rows, int cols,
                          void *stream);

/* Snapshot / seasonal form of ssrs_updraft_from_dem (simulator.py:200-215 with the wind
 * preparation of :765-792 folded in): `batch` wind snapshots given as speed / direction
 * samples on a regular nx x ny lattice (as ssrs_wind_from_lattice; x0, y0, dx, dy in km,
 * the raster's cell size is res / 1000 km) -> orograph (batch, rows, cols) f32 and / or
 * usable updraft (batch, rows, cols) f64.  The DEM is read once for the whole batch and
 * no per-cell wind raster is materialised: bilinear east / north components at the cell,
 * w = -(Y north + X east) / sqrt(d^2 + X^2 + Y^2) (the wind speed cancels).
 * workspace: ssrs_lattice_workspace_bytes(nx, ny, batch) bytes of device scratch; its contents before a call mean
 * nothing and after it are unspecified. */
size_t ssrs_lattice_workspace_bytes(int nx, int ny, int batch);
int ssrs_updraft_from_dem_lattice(const void *dem, int dem_type, double res,
                                  const double *lattice_speed, const double *lattice_dirn,
                                  int nx, int ny, double x0, double y0, double dx, double dy,
                                  double min_updraft_val, float *orograph, double threshold,
                                  double *usable, int rows, int cols, int batch,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* Wind preparation of snapshot / seasonal modes (ssrs/simulator.py:778-792):
 * `batch` sets of speed/direction samples on a regular nx x ny lattice (origin
 * x0,y0 and spacings dx,dy in the raster's length unit, cell_size likewise;
 * lattice arrays (batch, ny, nx) f64) -> u/v components -> bilinear
 * interpolation to cell centres (clamped at the hull) -> per-cell speed and
 * direction in [0, 360), (batch, rows, cols) f64.  The reference triangulates
 * scattered points with scipy griddata; on a lattice bilinear is its equivalent. */
int ssrs_wind_from_lattice(const double *lattice_speed, const double *lattice_dirn,
                           int nx, int ny, double x0, double y0, double dx, double dy,
                           double cell_size, double *wspeed, double *wdirn, int rows,
                           int cols, int batch, void *stream);

/* The same for SCATTERED samples -- the reference's general case, ssrs/simulator.py:765-776:
 * scipy.interpolate.griddata(points, values, mesh, method='linear'), i.e. a Delaunay triangulation of the sample
 * points and barycentric interpolation inside each triangle, applied to the east / north components (:778-792).
 * The triangulation is the caller's: `points` (npts, 2) f64 in the raster's length unit relative to the centre of
 * cell (0, 0) (x along columns, y along rows), `triangles` (ntri, 3) int32 vertex indices and `transform` (ntri, 3, 2)
 * f64 exactly as scipy.spatial.Delaunay(points) holds them (.simplices, .transform: the 2 x 2 inverse of the edge
 * matrix and the offset r) -- griddata builds that very object.  speed / dirn (batch, npts) f64 -> wspeed / wdirn
 * (batch, rows, cols) f64, direction in [0, 360); cells outside the convex hull are NaN (griddata's fill value).  A
 * cell on an edge shared by two triangles takes the one with the lower index (the interpolant is continuous there;
 * scipy's walk picks either), so results agree with griddata to rounding, not bit for bit.
 * workspace: ssrs_wind_triangles_workspace_bytes(npts, rows, cols, batch) bytes of device scratch; its contents before a
 * call mean nothing and after it are unspecified. */
size_t ssrs_wind_triangles_workspace_bytes(int npts, int rows, int cols, int batch);
int ssrs_wind_from_triangles(const double *points, const int32_t *triangles, const double *transform,
                             const double *speed, const double *dirn, int npts, int ntri,
                             double cell_size, double *wspeed, double *wdirn, int rows, int cols,
                             int batch, void *workspace, size_t workspace_bytes, void *stream);

/* griddata's method='nearest' (NearestNDInterpolator -> cKDTree, Euclidean, no rescaling), in two steps.
 * ssrs_wind_nearest_index: `points` as above -> index (rows, cols) int32, per cell the sample nearest to its centre,
 * d^2 = dx * dx + dy * dy in f64.  A cell equally far from several samples takes the LOWEST sample index (cKDTree picks
 * either), so the raster equals cKDTree's wherever the nearest sample is unique.  It depends on the points only: build
 * it once per wind geometry.  Samples are culled per 64 x 32 cell tile by the triangle inequality; the cull never
 * decides a result (a tile with too many candidates scans all samples).
 * workspace: ssrs_wind_nearest_workspace_bytes(npts, rows, cols) bytes of device scratch; on return its first int32
 * holds the number of tiles that scanned all samples; its contents before a call mean nothing and after it are
 * otherwise unspecified.
 * ssrs_wind_from_nearest: speed / dirn (batch, npts) f64 -> per sample the u/v recipe of simulator.py:778-792
 * (speed = sqrt(e^2 + n^2), direction = mod(atan2(e, n) + 2 pi, 2 pi) in degrees) -> wspeed / wdirn (batch, rows, cols)
 * f64 gathered through `index`.  No NaN (nearest has no hull), except for an index outside [0, npts). */
size_t ssrs_wind_nearest_workspace_bytes(int npts, int rows, int cols);
int ssrs_wind_nearest_index(const double *points, int npts, double cell_size, int32_t *index, int rows,
                            int cols, void *workspace, size_t workspace_bytes, void *stream);
int ssrs_wind_from_nearest(const int32_t *index, const double *speed, const double *dirn, int npts,
                           double *wspeed, double *wdirn, int rows, int cols, int batch, void *stream);

/* griddata's method='cubic' (CloughTocher2DInterpolator: a C1 piecewise cubic on the Delaunay triangulation).
 * The caller's, from scipy: points / triangles / transform as for ssrs_wind_from_triangles, `neighbors` (ntri, 3) int32
 * = Delaunay.neighbors (-1 on the hull), the east / north components (batch, npts) f64 of the samples and their
 * gradients at the vertices grad_east / grad_north (batch, npts, 2) f64 as scipy estimates them
 * (CloughTocher2DInterpolator(tri, values, tol=1e-6, maxiter=400).grad: a global iteration over the vertices).
 * The device's: the 19 Bezier ordinates of every macro-triangle and field (a table [triangle][2 batch][19] in the
 * workspace), cell ownership exactly as ssrs_wind_from_triangles (scipy's eps, lowest triangle index on a shared edge,
 * NaN outside the hull), the cubic in the four shifted barycentric coordinates, and the u/v recipe -> wspeed / wdirn
 * (batch, rows, cols) f64.  The interpolant is C1 across edges, so the triangle chosen on an edge changes a value by
 * rounding only; sums are taken in scipy's order but agreement with griddata is to rounding, not bit for bit.
 * workspace: ssrs_wind_cubic_workspace_bytes(npts, ntri, rows, cols, batch) bytes of device scratch; its contents before
 * a call mean nothing and after it are unspecified. */
size_t ssrs_wind_cubic_workspace_bytes(int npts, int ntri, int rows, int cols, int batch);
int ssrs_wind_from_triangles_cubic(const double *points, const int32_t *triangles, const int32_t *neighbors,
                                   const double *transform, const double *east, const double *north,
                                   const double *grad_east, const double *grad_north, int npts, int ntri,
                                   double cell_size, double *wspeed, double *wdirn, int rows, int cols,
                                   int batch, void *workspace, size_t workspace_bytes, void *stream);

/* compute_thermals (ssrs/layers.py:188-214), split in its two stages.
 * ssrs_thermal_seeds: per-cell seeding inside the 10 % border with probability
 * 1/(int(wt)-1), wt = 1000 + |aspect-180|/180*2000, amplitude
 * lognormal(scale + 3, 0.5); counter-based (Philox keyed by seed and cell) --
 * statistical parity only, the reference replays a serial global RNG.
 * ssrs_gaussian_blur: scipy.ndimage.gaussian_filter(sigma, mode='constant'),
 * separable, truncated at 4 sigma.  thermals = blur(seeds, sigma = 4).
 * workspace: ssrs_blur_workspace_bytes(rows, cols, sigma) bytes of device scratch; its contents before a call mean
 * nothing and after it are unspecified.
 * ssrs_thermal_seeds is asynchronous on `stream`; ssrs_gaussian_blur copies its weights from a host temporary and
 * waits for `stream` once, before its two passes, which go to `stream` in order. */
int ssrs_thermal_seeds(const double *aspect, double thermal_intensity_scale,
                       uint64_t seed, double *seeds, int rows, int cols, void *stream);
size_t ssrs_blur_workspace_bytes(int rows, int cols, double sigma);
int ssrs_gaussian_blur(const double *in, double *out, double sigma, int rows, int cols,
                       void *workspace, size_t workspace_bytes, void *stream);

/* compute_thermals as ONE call for `count` realisations: out[k] = blur(seeds(aspect, scale, seeds[k]), sigma),
 * bit for bit what the two calls above give in f64 (the same Philox key per cell, the same sum in the same order),
 * rounded once to f32 when out_is_f32 (what the <case>_r<k>_thermals.npy files hold).  One launch per 32
 * realisations; a block draws the seeds of a 32 x 64 tile and its halo into LDS and blurs there, so neither the
 * seed raster nor the axis-0 result reaches HBM.  No workspace; asynchronous on `stream`.
 * aspect: device, (rows, cols) f64.  seeds: HOST array of `count` keys (read before the call returns).
 * out: device, (count, rows, cols) f32 or f64.  sigma: the reference's 4 is what ssrs_amd passes; a sigma whose
 * radius int(4 sigma + 0.5) exceeds 16 does not fit the tile and takes the chain above per realisation through
 * stream-ordered scratch (hipMallocAsync, 16 bytes per cell; that path synchronises `stream` once).
 * NULL pointers, count / rows / cols <= 0 or sigma <= 0 -> SSRS_ERR_INVALID before any GPU work. */
int ssrs_thermal_fields(const double *aspect, double thermal_intensity_scale, double sigma,
                        const uint64_t *seeds, int count, void *out, int out_is_f32,
                        int rows, int cols, void *stream);

/* The physical thermal model: the WTK layers pressure / temperature at wtk_thermal_height, boundary-layer height and
 * surface heat flux -> thermal updraft at height z.  Three elementwise f64 calls over n values, each the reference's
 * expression in the reference's operation order:
 * ssrs_potential_temperature (ssrs/layers.py:40-48): (T + 273.15) * pow(1e5 / p, 0.2857) - 273.15, degrees Celsius.
 * ssrs_deardorff_velocity (ssrs/layers.py:25-37): max(min, pow(9.8 / 1216 * (max(zi, 100) * max(q, 0) /
 *   (theta + 273.15)), 1/3)).
 * ssrs_thermal_updraft (ssrs/layers.py:51-60): x = clip(z / zi, 0, 1); max(min, w* * (0.85 * (pow(x, 1/3) * (1.3 - x))));
 *   z = zmat[i], or z0 everywhere when zmat is NULL; zi is not clipped here (the reference does not).
 * max / clip are numpy's: a NaN argument gives NaN (fmax / fmin would drop it).  The IEEE specials follow from plain
 * division: zi = 0 with z > 0 gives x = 1, zi < 0 gives x = 0 and so the floor `min`, p = 0 gives theta = inf and so
 * the floor, p < 0 gives NaN.  NULL pointers (zmat excepted) or n == 0 -> SSRS_ERR_INVALID before any GPU work.
 * One launch each, asynchronous on `stream`. */
int ssrs_potential_temperature(const double *pressure, const double *temperature, double *out, size_t n,
                               void *stream);
int ssrs_deardorff_velocity(const double *pot_temperature, const double *blayer_height,
                            const double *surface_heat_flux, double min_updraft_val, double *out, size_t n,
                            void *stream);
int ssrs_thermal_updraft(const double *zmat, double z0, const double *deardorff_vel, const double *blayer_height,
                         double min_updraft_val, double *out, size_t n, void *stream);

/* _interpolate_wtk_vardata (ssrs/simulator.py:765-776): scipy griddata of ANY scalar samples, method 'nearest' |
 * 'linear' | 'cubic'.  values (nfields, npts) f64 -> out (nfields, rows, cols) f64.  The geometry is the wind calls':
 * 'nearest' reads `index`, the raster of ssrs_wind_nearest_index (the other geometry pointers may be NULL); 'linear'
 * and 'cubic' take points / triangles / transform of scipy.spatial.Delaunay and find cell ownership exactly as
 * ssrs_wind_from_triangles does (scipy's eps, lowest triangle index on a shared edge, NaN outside the hull); 'cubic'
 * also takes `neighbors` and `grad` (nfields, npts, 2), the vertex gradients of scipy's estimator, and builds the
 * ordinate table of ssrs_wind_from_triangles_cubic, [triangle][nfields][19].  A cell is evaluated by the very
 * expressions of the wind kernels.  workspace: ssrs_scalar_interp_workspace_bytes(method, ntri, rows, cols, nfields)
 * bytes of device scratch (ntri is ignored for 'nearest'); 0 for arguments the call would refuse.  Its contents before a
 * call mean nothing and after it are unspecified. */
#define SSRS_INTERP_NEAREST 0
#define SSRS_INTERP_LINEAR 1
#define SSRS_INTERP_CUBIC 2
size_t ssrs_scalar_interp_workspace_bytes(int method, int ntri, int rows, int cols, int nfields);
int ssrs_scalar_from_samples(int method, const double *points, const int32_t *triangles, const int32_t *neighbors,
                             const double *transform, const int32_t *index, const double *values,
                             const double *grad, int npts, int ntri, double cell_size, double *out, int rows,
                             int cols, int nfields, void *workspace, size_t workspace_bytes, void *stream);

/* The two above as ONE call for `batch` snapshots (what compute_thermal_updraft would make of the four WTK layers the
 * reference downloads, ssrs/simulator.py:107-115).  layers (4, batch, npts) f64: pressure, temperature, blheight,
 * surfheatflux at the sample points; grad (4, batch, npts, 2), 'cubic' only.  Per cell the sample geometry is located
 * once for the whole batch; per snapshot the four values are interpolated, run through the three functions in
 * registers and stored: out (batch, rows, cols), f64 or -- out_is_f32 -- that result rounded once to f32 (what
 * <case>_r<k>_thermals.npy holds).  zmat: (rows, cols) f64 heights, or NULL for z0 everywhere.  Bit for bit the chain
 * ssrs_scalar_from_samples -> ssrs_potential_temperature -> ssrs_deardorff_velocity -> ssrs_thermal_updraft, none of
 * whose 4 + 3 rasters per snapshot reaches memory: 4 B read per cell (owner or index), 4-8 B written per cell and
 * snapshot.  A lane owns four consecutive cells of a row (one 16-byte f32 store when cols % 4 == 0).
 * workspace: ssrs_scalar_interp_workspace_bytes(method, ntri, rows, cols, 4 * batch); its contents before a call mean
 * nothing and after it are unspecified. */
int ssrs_wtk_thermal_fields(int method, const double *points, const int32_t *triangles, const int32_t *neighbors,
                            const double *transform, const int32_t *index, const double *layers,
                            const double *grad, int npts, int ntri, double cell_size, const double *zmat,
                            double z0, double min_updraft_val, void *out, int out_is_f32, int rows, int cols,
                            int batch, void *workspace, size_t workspace_bytes, void *stream);

/* ----------------------------------------------------------------- stepper */

/* Per-run constants of generate_simulated_tracks (ssrs/movmodel.py:264-318).
 * Fill with ssrs_track_params_init() or by hand. */
typedef struct SsrsTrackParams {
    int32_t rows, cols;
    int32_t burnin;           /* int(min(rows, cols) / 10), movmodel.py:276 */
    int32_t memory_parameter; /* directions[-m:], 0..8 (0 = whole history) */
    int64_t max_moves;        /* ceil(rows / 2 * cols / 2), movmodel.py:277 */
    double scaling_parameter; /* nu; exact parity is claimed for nu == 1 */
    double prior[9];          /* get_directional_probs(move_dirn * pi / 180),
                                 movmodel.py:247-257, computed by the host */
    int32_t steps_per_launch; /* 0 = default (512) */
    int32_t flags;            /* SSRS_TRACKS_* */
} SsrsTrackParams;

#define SSRS_TRACKS_PROFILE 1    /* time every launch with HIP events (stats) */
#define SSRS_TRACKS_NO_SCHEDULE 4 /* keep caller order, release every track at once
                                    (A/B switch for the coherent schedule) */
#define SSRS_TRACKS_NO_BINNING 8  /* histogram by per-step global atomics instead of the
                                    visit buffer + LDS binning kernel (A/B switch) */
#define SSRS_TRACKS_RING_TABLE 16 /* `table` is the f32 ring table of
                                    ssrs_transition_ring_build (one 12-byte gather per step);
                                    needs updraft (+ potential if the table was built with it)
                                    for the exact decision of near-ties, memory_parameter 1,
                                    scaling_parameter 1, traj NULL, even steps_per_launch */
#define SSRS_TRACKS_SCATTERED 32    /* treat the batch as scattered from the first launch: the
                                      stepper counts visits itself, into wave-private copies of the
                                      histogram when the workspace has room for them (tracks that
                                      circle in a pocket of the field otherwise queue up on single
                                      cells), and the ring stepper reads the per-cell zero-mask
                                      byte before gathering.  Default: large batches go from the
                                      per-step window to tile buckets and only then to this
                                      variant; small ones directly.  Results are identical */
#define SSRS_TRACKS_NO_SCATTERED 64 /* never switch to that variant (A/B) */
#define SSRS_TRACKS_THR_TABLE 128   /* `table` is the threshold table of ssrs_transition_thr_build (one 4-byte
                                      gather and two comparisons per step); needs updraft (+ potential
                                      if the table was built with it) for the exact decision of near-ties,
                                      memory_parameter 1, scaling_parameter 1, traj NULL, even steps_per_launch,
                                      and params->prior equal to the prior the table was built with */
#define SSRS_TRACKS_EXACT_ONLY 2 /* disable the guarded division-free decision
                                   (A/B switch; results are identical) */

typedef struct SsrsTrackStats {
    int64_t total_steps; /* moves taken by all tracks of this call */
    int32_t launches;    /* stepper kernel launches */
    float kernel_ms;     /* sum of stepper launch durations (SSRS_TRACKS_PROFILE) */
    float wall_ms;       /* first launch -> last completion, HIP events */
    float hist_ms;       /* sum of histogram-binning launch durations (PROFILE) */
    int32_t window_launches; /* launches whose visits were binned through the per-step row /
                                column window; */
    int32_t tile_launches;   /* ... through raster-tile buckets; the other launches counted
                                in the stepper (atomics on hist or on its private copies) */
    int32_t block_window_launches; /* ... in the stepper, into a histogram window per block in LDS
                                (threshold table; batches whose survivors roam a few basins) */
    int32_t wander_sorts;    /* times the live tracks were sorted into such windows */
    int32_t timed_launches;  /* stepper launches whose durations make up kernel_ms (PROFILE) */
    float first_move_ms;     /* of which: the one-iteration launch of the generic kernel that makes every
                                track's first move before the threshold stepper takes over (PROFILE; else 0) */
    float block_window_ms;   /* of which: the block-window launches (PROFILE; else 0) */
    int32_t block_window_timed;   /* how many of them were timed */
    int64_t block_window_steps;   /* moves taken in batches of block-window launches (from the per-batch
                                     read-backs; a batch is one or two launches of one kind) */
    int32_t roam_launches;        /* block-window launches that stepped through the windows' roam table
                                     (two moves per 64-byte entry, k_step_roam) */
    int32_t reserved0;            /* near-ties those launches settled with the 32-bit fine table */
    int64_t roam_wave_pairs;      /* pairs of moves run by the waves of those launches ... */
    int64_t roam_slow_wave_pairs; /* ... and how many of them sent some lane through the single-move sequence
                                     (near-ties, flag entries, moves out of the window, burn-in) */
    int32_t roam_shuffles;        /* times a SETTLED roaming batch had the tracks of its windows dealt afresh
                                     (every SSRS_TRACKS_ROAM_SHUFFLE batches: default 16, and 2 while 256-lane blocks step
                                     with feeder waves; part of wander_sorts) */
    int32_t roam_wide_launches;   /* of roam_launches: those run with 512-lane blocks (two list blocks of one window per CU: batches
                                     whose survivors outnumber one round of 256-lane blocks; SSRS_TRACKS_ROAM_WIDE) */
    int32_t window_scans;         /* of wander_sorts: those that looked for the windows anew.  A shuffle of a settled batch deals
                                     into the windows of the last scan (SSRS_TRACKS_NO_SHUFFLE_REUSE: every sort scans) */} SsrsTrackStats;

/* Fills rows/cols/burnin/max_moves/memory/nu and zeroes the rest; `prior` must
 * still be supplied by the caller (it needs the host libm/numpy cos). */
int ssrs_track_params_init(SsrsTrackParams *p, int rows, int cols,
                           int memory_parameter, double scaling_parameter);

/* Per-cell move weights of movmodel.py:292-306 for every interior cell:
 *   w_k = hm(max(u_c,1e-6), max(u_k,1e-6)) * f64(f32(phi_c - phi_k) * ninv_k),
 * clipped at 0 (:231), the 8 neighbours k = 0,1,2,3,5,6,7,8 of one cell stored
 * as 8 consecutive f64 (64 B, one aligned fetch per step).  A cell with any NaN
 * weight stores NaN in all 8 (the stepper then takes the :228-230 fallback).
 * potential may be NULL (updraft-only weights).  table: rows*cols*8 f64.
 * This and the two builders below: one launch each, asynchronous on `stream` (`prior` travels as a kernel argument). */
int ssrs_transition_table_build(const double *updraft, const float *potential,
                                double *table, int rows, int cols, void *stream);

/* The same weights for the three-candidate stepper (SSRS_TRACKS_RING_TABLE): after
 * a move only the three cells within +-45 deg are admissible (movmodel.py:185-202),
 * and in clockwise ring order N, NE, E, SE, S, SW, W, NW they are consecutive.  Per
 * cell 10 f32 = the ring-ordered weights rounded to f32, stored as ring 7, 0, 1, ...,
 * 7, 0 (40 B), exact zeros as -0.0f; behind the records one zero-mask byte per cell (bit c:
 * ring weight c is exactly zero).  ring: ssrs_transition_ring_bytes(rows, cols) bytes,
 * 8-byte aligned.  The records and the mask are OVERWRITTEN; the 8 bytes between them and the
 * bytes that round the size up to whole floats are not written (loads may touch them, no value
 * of theirs is used). */
size_t ssrs_transition_ring_bytes(int rows, int cols);
int ssrs_transition_ring_build(const double *updraft, const float *potential, float *ring,
                               int rows, int cols, void *stream);

/* The decision thresholds themselves (SSRS_TRACKS_THR_TABLE): for every cell and every last move
 * rc (ring position 0..7) one dword T1 | T2 << 16 with T1 = round(2^16 a / (a + b + c)), T2 =
 * round(2^16 (a + b) / (a + b + c)) (clamped to 65535), a, b, c the three admissible weights of
 * movmodel.py:292-309 in ascending neighbour index -- the boundaries np.random.choice's inverse-cdf
 * pick compares the uniform with; the stepper decides on the uniform's top 16 bits and hands a
 * uniform within one unit of a boundary (3e-5 per boundary) to the exact sequence.  A row whose
 * weights are all zero carries the masked prior's thresholds (movmodel.py:234-238); boundary cells,
 * poisoned rows and rows where the unmasked prior decides are flag entries (T1 = 0xFFFF > T2 = code).
 * Eight planes (one per last move) of 4-byte entries at a power-of-two stride,
 * ssrs_transition_thr_bytes(rows, cols) bytes in all, 64-byte aligned; the table belongs to one
 * heading (`prior` [host], 9 doubles = SsrsTrackParams.prior).  rows * cols <= 2^26; the
 * table carries a guard band of (cols + 2) dwords at either end, and the first bytes of the leading band
 * name the table (magic, rows, cols, the nine prior values): ssrs_tracks_simulate reads them back and returns
 * SSRS_ERR_INVALID, before any stepper kernel is launched, for a buffer that is not the threshold table of its
 * raster and prior (88 bytes and one stream wait per call).  The header and the eight planes are
 * OVERWRITTEN; the rest of the guard bands and the dwords between a plane's last cell and the next
 * plane are not written (speculative loads may touch them, no value of theirs is used). */
size_t ssrs_transition_thr_bytes(int rows, int cols);
int ssrs_transition_thr_build(const double *updraft, const float *potential, const double *prior,
                              float *thr, int rows, int cols, void *stream);

/* Bytes of device scratch ssrs_tracks_simulate needs for `ntracks` (about 8.3 KB per
 * track: two buffers of 1024 steps x 4 B for the launch's visited cells, in slot and in
 * raster-tile order; a launch takes as many steps as they hold for the live tracks).
 * With the threshold table, a batch whose survivors roam a few basins of the potential
 * field until max_moves (the solved 10 m field: 44 %) is sorted into up to 16 histogram
 * windows of 144 x 256 cells and counted in LDS (SsrsTrackStats.block_window_launches);
 * nothing to size for it.  A stepper workspace (this size or the next) may be handed from call to call as it stands,
 * whatever the raster, table and path of the call before: its contents before a call mean nothing and after it are
 * unspecified. */
size_t ssrs_tracks_workspace_bytes(int64_t ntracks);
/* The same plus (i) the pair table of the roaming regime and the fine table of its near-ties -- 128 + 64
 * bytes per cell (5.76 GB at 5000 x 6000),
 * batches of >= 8192 tracks on rasters below 2^25 cells: with it the block-window launches take two moves
 * per 16-byte gather (SsrsTrackStats.roam_launches), without it they run round 2's one-gather-per-move
 * kernel, 2.1x slower -- and (ii) room for `hist_copies` (2..64) private copies of the histogram.  A
 * workspace of this size lets ssrs_tracks_simulate privatise the histogram once a batch
 * is scattered (many tracks circling in the same pockets of a real potential field make
 * per-step atomics on single cells queue up at the memory side: 3x slower); the copies
 * are added to `hist` before the call returns.  Optional: the smaller workspace works. */
size_t ssrs_tracks_workspace_bytes_ex(int64_t ntracks, int rows, int cols, int hist_copies);

/* generate_simulated_tracks for a batch of tracks (movmodel.py:264-318, driven
 * as Simulator.simulate_tracks does, simulator.py:360-369) + the histogram of
 * compute_presence_counts (movmodel.py:410-419).
 *   updraft    f64 (rows, cols) or NULL;  potential f32 (rows, cols) or NULL
 *              (both NULL = 'drw' mode, simulator.py:370-381)
 *   table      from ssrs_transition_table_build (f64 rows; updraft and potential are
 *              then not read), from ssrs_transition_ring_build with the flag
 *              SSRS_TRACKS_RING_TABLE (updraft / potential are read for the exact
 *              decision of near-ties), or NULL to gather the 3x3 windows of
 *              updraft/potential directly
 *   start_rc   int32 (ntracks, 2) [row, col]
 *   seed       sim_seed + real_id (simulator.py:352); track_id_base = global id
 *              of track 0 of this call (multi-GPU shards pass their offset)
 *   hist       uint32 (rows, cols), ACCUMULATED (+1 per trajectory point), or NULL
 *   end_rc     int16 (ntracks, 2) last point, or NULL
 *   lengths    int32 (ntracks) number of trajectory points, or NULL
 *   traj       int16 pairs, track t at traj[2*traj_offsets[t] ...], or NULL;
 *              traj_offsets int64 (ntracks + 1): exclusive prefix sums of the
 *              lengths of a previous call with the same arguments; points beyond
 *              a track's room [offsets[t], offsets[t+1]) are dropped, never written
 *   workspace  device scratch of ssrs_tracks_workspace_bytes(ntracks); its contents before a call mean nothing
 *              and after it are unspecified
 *   stats      [host] out, may be NULL */
int ssrs_tracks_simulate(const SsrsTrackParams *params, const double *updraft,
                         const float *potential, const double *table,
                         const int32_t *start_rc, int64_t ntracks, uint64_t seed,
                         uint64_t track_id_base, uint32_t *hist, int16_t *end_rc,
                         int32_t *lengths, int16_t *traj,
                         const int64_t *traj_offsets, void *workspace,
                         size_t workspace_bytes, SsrsTrackStats *stats,
                         void *stream);

/* ssrs_tracks_simulate (no trajectories) with the presence counts in 64 bits: compute_presence_counts' int16 raster
 * (movmodel.py:415) wraps at 32 767 visits and this library's uint32 one at 2^32 - 1, which the trap cells of a solved 10 m
 * field reach from ~250 000 tracks of one call on (1.7e4 visits per track).  The kernels count into `hist_scratch`
 * (uint32 (rows, cols), zeroed by the caller: whatever it holds is counted too) and the library empties it into `hist64`
 * (uint64 (rows, cols), ACCUMULATED) every other batch of launches and before it returns, on `stream`, whatever the
 * table, switches and stepper path.  The 32-bit rasters behind the regular workspace (the private copies of a scattered
 * batch, the transposed raster of an east / west front) are added into `hist64` with 64-bit sums before one of their
 * cells could pass 2^32 - 1 (bounded by the tracks times the steps of the launches since) and before it returns. */
int ssrs_tracks_simulate_h64(const SsrsTrackParams *params, const double *updraft,
                             const float *potential, const double *table,
                             const int32_t *start_rc, int64_t ntracks, uint64_t seed,
                             uint64_t track_id_base, uint32_t *hist_scratch, uint64_t *hist64,
                             int16_t *end_rc, int32_t *lengths, void *workspace,
                             size_t workspace_bytes, SsrsTrackStats *stats, void *stream);

/* Trajectory output in ONE simulation pass (the List[int16 (n_i, 2)] that
 * Simulator.simulate_tracks pickles, simulator.py:360-385).  The two-call form above needs
 * the lengths of an earlier identical simulation for `traj_offsets`.  With a recorder the
 * stepper keeps every launch's visited cells in a caller-supplied device pool (4 bytes per
 * step and live slot); when the call returns the lengths are final, the caller forms the
 * offsets (exclusive prefix sums of `lengths`), allocates `traj` and ssrs_tracks_gather
 * appends every track's points in order.  Every stepper path (ring table included) records.
 *   pool        device scratch, 256-byte aligned; when it is exhausted the simulation goes
 *               on unrecorded (results unaffected), ssrs_traj_recorder_complete() returns 0
 *               and the caller falls back to the two-call form or a larger pool
 *   recorder    reusable: each ssrs_tracks_simulate_rec call starts a fresh record */
typedef struct SsrsTrajRecorder SsrsTrajRecorder;
SsrsTrajRecorder *ssrs_traj_recorder_create(void *pool, size_t pool_bytes);
void ssrs_traj_recorder_destroy(SsrsTrajRecorder *recorder);
int ssrs_traj_recorder_complete(const SsrsTrajRecorder *recorder);
size_t ssrs_traj_recorder_used(const SsrsTrajRecorder *recorder);
/* ssrs_tracks_simulate without traj / traj_offsets, recording into `recorder` */
int ssrs_tracks_simulate_rec(const SsrsTrackParams *params, const double *updraft,
                             const float *potential, const double *table,
                             const int32_t *start_rc, int64_t ntracks, uint64_t seed,
                             uint64_t track_id_base, uint32_t *hist, int16_t *end_rc,
                             int32_t *lengths, SsrsTrajRecorder *recorder, void *workspace,
                             size_t workspace_bytes, SsrsTrackStats *stats, void *stream);
/* traj[2 * traj_offsets[t] ...] <- the int16 (row, col) points of track t, start cell first
 * (asynchronous on `stream`; the pool must stay alive until it has run).
 *   start_rc, ntracks   as passed to ssrs_tracks_simulate_rec
 *   traj_offsets        int64 (ntracks + 1), exclusive prefix sums of `lengths`; points
 *                       beyond a track's room are dropped, never written
 *   cursor_ws           device scratch, 4 bytes per track; its contents before a call mean nothing and after it
 *                       are unspecified */
int ssrs_tracks_gather(const SsrsTrajRecorder *recorder, const int32_t *start_rc,
                       int64_t ntracks, const int64_t *traj_offsets, int16_t *traj,
                       void *cursor_ws, size_t cursor_bytes, void *stream);

/* The one exchange step of a track-sharded run (the reference maps the tracks of a
 * case over a process pool, simulator.py:360-369, and adds them up in compute_presence_counts):
 * in-place sum of the ranks' uint32 histograms over xGMI.  `nccl_comm` is an ncclComm_t the caller
 * created with its own RCCL (one process per GPU); root >= 0: ncclReduce to that rank, root < 0:
 * ncclAllReduce.  Asynchronous on `stream`.  RCCL is resolved at run time (the process's own copy
 * first, else librccl.so.1), so the library loads without it.  The sum is 32-bit: a caller whose
 * ranks' largest counts add up to 2^32 or more must widen first (ssrs_amd.distributed does). */
int ssrs_hist_reduce(uint32_t *hist, size_t n, int root, void *nccl_comm, void *stream);

/* --------------------------------------------------------------- presence */

/* compute_presence_counts (ssrs/movmodel.py:410-419) from stored trajectories:
 * hist[row, col] += 1 for each of the npoints int16 (row, col) pairs.  uint32
 * counts (the reference's int16 matrix wraps above 32767 visits).  A point
 * outside the raster is an error (the reference raises IndexError).
 * scratch8: 8 bytes of device scratch; its contents before a call mean nothing and after it are unspecified.
 * The out-of-raster flag is read back, so the call waits for `stream` once, after its launch. */
int ssrs_presence_count(const int16_t *traj, int64_t npoints, uint32_t *hist,
                        int rows, int cols, void *scratch8, void *stream);

size_t ssrs_presence_workspace_bytes(int rows, int cols, int krad);

/* compute_smooth_presence_counts (ssrs/movmodel.py:422-439) on a count matrix:
 * zero-padded 'same' convolution with the disk kernel (x^2+y^2 <= krad^2)/ntaps,
 * f32 out.  Evaluated as 2*krad+1 chords of row prefix sums: exact in integers,
 * then one multiply by 1/ntaps.
 * workspace: ssrs_presence_workspace_bytes(rows, cols, krad) bytes of device scratch, 256-byte aligned; its contents
 * before a call mean nothing and after it are unspecified.
 * The chord half-widths are copied from a host temporary, so the call (and the _u64 form) waits for `stream` once,
 * before its two launches, which go to `stream` in order. */
int ssrs_presence_smooth(const uint32_t *count, int krad, float *out, int rows,
                         int cols, void *workspace, size_t workspace_bytes,
                         void *stream);

/* The same for 64-bit counts: the sum of the ranks' histograms when a 32-bit sum could wrap
 * (tracks that circle in a pocket of the field until max_moves put ~1e9 visits into single
 * cells per 100k tracks).  The chord sums are 64-bit either way. */
int ssrs_presence_smooth_u64(const uint64_t *count, int krad, float *out, int rows,
                             int cols, void *workspace, size_t workspace_bytes,
                             void *stream);

/* The normalisation ladder of Simulator.plot_presence_map (simulator.py:529-546):
 *   acc += src / max(src)     (division in src's precision: f32 for `prprob`,
 *                              f64 for `case_prob`)
 *   out  = f32(src / max(src)) (summary_presence.npy)
 * scratch8: 8 bytes of device scratch; its contents before a call mean nothing and after it are unspecified.
 * A memset and two launches each (the maximum stays on the device), asynchronous on `stream`. */
int ssrs_presence_normalise_add(const void *src, int src_type, double *acc, size_t n,
                                void *scratch8, void *stream);
int ssrs_presence_normalise_f32(const double *src, float *out, size_t n,
                                void *scratch8, void *stream);

/* --------------------------------------------------------------- turbines */

/* Which tracks came within `radius_cells` of which turbine (what the reference's get_turbine_presence,
 * ssrs/simulator.py:594-607, was after), from the trajectories on the device.
 * Geometry: a turbine is (xt, yt) f64 in CELL units relative to the centre of cell (0, 0), x along columns, y along
 * rows; a trajectory point (r, c) encounters it iff dx * dx + dy * dy <= radius_cells * radius_cells with
 * dx = (double)c - xt, dy = (double)r - yt, each product and the sum rounded on their own, `<=`: a point exactly on
 * the circle counts.  NumPy's (c - xt)**2 + (r - yt)**2 <= R * R gives the same answer bit for bit.
 *   traj, traj_offsets  as ssrs_tracks_simulate / ssrs_tracks_gather leave them: int16 (row, col) pairs, track t at
 *                       [traj_offsets[t], traj_offsets[t + 1]) (int64, ntracks + 1; the first need not be 0); equal
 *                       consecutive offsets are an empty track, which has no encounters.  A point outside the raster
 *                       encounters nothing.  traj is 4-byte aligned (16-byte aligned buffers are read 16 bytes a lane)
 *   turbines            (nturb, 2) f64 [xt, yt], 1 <= nturb <= SSRS_TURBINE_MAX
 *   bin_start, bin_items  the CALLER's cull, as the Delaunay triangulation is for the wind calls: a CSR over bins of
 *                       SSRS_TURBINE_BIN x SSRS_TURBINE_BIN cells, bin (r / 32) * nbc + c / 32 with nbr =
 *                       ceil(rows / 32), nbc = ceil(cols / 32); bin_start int32 (nbr * nbc + 1), bin_items int32
 *                       (bin_start[nbr * nbc]) the turbines whose disk can reach the bin.  The lists only cull: the
 *                       test above decides every hit, and a list that OMITS a turbine loses its hits in that bin.
 *                       Items outside [0, nturb) are skipped
 *   hits                uint32 (ntracks, words), words = ceil(nturb / 32): bit t % 32 of word t / 32 of row k is set
 *                       iff track k encountered turbine t.  ACCUMULATED by OR (zero it for a fresh count)
 *   first_step          int32 (ntracks) or NULL: the index within the track of its first point inside any turbine's
 *                       disk, combined by UNSIGNED minimum with what is there: the caller's initial -1 (0xFFFFFFFF)
 *                       means "none"
 * One streaming pass, asynchronous on `stream`; OR and min of integers: the same result from run to run.  The
 * occupied-bin mask lives in LDS for rasters of up to 262 144 bins (16 384 x 16 384 cells); beyond, bin_start is read
 * per point.  NULL pointers (first_step excepted), ntracks outside [0, 2^31), nturb outside [1, SSRS_TURBINE_MAX],
 * rows / cols outside [1, 32767], a negative or NaN radius -> SSRS_ERR_INVALID before any GPU work. */
#define SSRS_TURBINE_BIN 32
#define SSRS_TURBINE_MAX 8192
int ssrs_turbine_encounters(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks,
                            const double *turbines, int nturb, double radius_cells,
                            const int32_t *bin_start, const int32_t *bin_items, int rows, int cols,
                            uint32_t *hits, int32_t *first_step, void *stream);

/* Popcounts of that bitmap: tracks_per_turbine int64 (nturb) = the tracks whose bit t is set, turbines_per_track
 * int32 (ntracks) = the bits of row k (may be NULL).  Both are OVERWRITTEN; bits at and above nturb are ignored.
 * Asynchronous on `stream`. */
int ssrs_turbine_encounter_counts(const uint32_t *hits, int64_t ntracks, int nturb,
                                  int64_t *tracks_per_turbine, int32_t *turbines_per_track, void *stream);

/* K15 -- which tracks passed through which turbine's OWN rotor envelope, and for how many points (the exposure): the
 * encounter test above in three dimensions with per-turbine geometry, from the trajectories and the heights of
 * ssrs_track_altitude on the device.  A turbine t is a vertical cylinder in absolute heights: (xt, yt) f64 in cell units
 * as above, reach_t f64 in cells, and [z_lo_t, z_hi_t] int32 millimetres above the DEM's datum.  Point k = (r, c) of a
 * track is inside turbine t iff
 *     it lies inside the raster,
 *     e = elev[r, c] (cellinfo[(r * cols + c) * 2 + 1]) is not the nodata sentinel INT32_MIN,
 *     dx * dx + dy * dy <= reach_t * reach_t   with dx = (double)c - xt, dy = (double)r - yt, every product and the sum
 *                                               rounded on their own, `<=` (the expression of ssrs_turbine_encounters), and
 *     z_lo_t <= (int64)e + alt[k] <= z_hi_t    both ends included.
 * A turbine whose reach_t is NaN or negative, whose xt or yt is NaN, or whose z_lo_t > z_hi_t is hit by nothing.
 *   traj, traj_offsets, ntracks   exactly what ssrs_turbine_encounters takes (the first offset need not be 0, equal
 *                       consecutive offsets are an empty track, traj 4-byte aligned)
 *   alt                 int32 per point, indexed like traj, 4-byte aligned: the height above the ground of the point's cell
 *                       in mm (ssrs_track_altitude's `alt`).  When traj AND alt are 16-byte aligned both are read 16 bytes a
 *                       lane
 *   cellinfo            the {climb, elev} raster of ssrs_altitude_cellinfo (rows, cols), 8-byte aligned; only elev is read,
 *                       and only for points whose bin holds a turbine
 *   turbines            (nturb, 2) f64 [xt, yt];  reach (nturb) f64;  zband (nturb, 2) int32 [z_lo, z_hi], 8-byte aligned;
 *                       1 <= nturb <= SSRS_TURBINE_MAX
 *   bin_start, bin_items  the caller's cull in the CSR form of ssrs_turbine_encounters, built from the per-turbine reach.
 *                       The lists only cull: the test above decides, a list that omits a turbine loses its hits in that
 *                       bin, and one that names a turbine twice in a bin counts its points there twice
 *   hits                uint32 (ntracks, ceil(nturb / 32)), ORed into: the layout of ssrs_turbine_encounters, so
 *                       ssrs_turbine_encounter_counts serves it unchanged
 *   first_step          int32 (ntracks) or NULL, UNSIGNED minimum with what is there (-1 = none): the index within the
 *                       track of its first point inside any turbine's cylinder
 *   points_per_turbine  uint64 (nturb) or NULL, ADDED to: the track points inside each turbine's cylinder.  64 bits end
 *                       to end towards the caller; inside, a lane keeps one (turbine, count) pair in registers over its
 *                       points, hands it to a uint32 counter per turbine in the block's LDS (4 bytes a turbine) when the
 *                       turbine changes, and the block adds its non-zero counters once, at its end
 * One streaming pass of 8 bytes per point, asynchronous on `stream`; everything is OR, min and sums of integers: the same
 * result from run to run, independent of the launch order.  The occupied-bin mask lives in LDS while it and the exposure
 * counters fit 60 KB together (and the raster has at most 262 144 bins); beyond, bin_start is read per point.
 * NULL pointers (first_step and points_per_turbine excepted), ntracks outside [0, 2^31), nturb outside
 * [1, SSRS_TURBINE_MAX], rows / cols outside [1, 32767], a misaligned traj, alt, cellinfo, zband or points_per_turbine ->
 * SSRS_ERR_INVALID before any GPU work.  ntracks == 0, or no points, returns SSRS_OK and touches nothing. */
int ssrs_rotor_encounters(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks, const int32_t *alt,
                          const int32_t *cellinfo, int rows, int cols, const double *turbines, const double *reach,
                          const int32_t *zband, int nturb, const int32_t *bin_start, const int32_t *bin_items,
                          uint32_t *hits, int32_t *first_step, uint64_t *points_per_turbine, void *stream);

/* K15, timed -- the same walk with the exposure in TIME: ssrs_rotor_encounters' arguments plus
 *   dt                  int32 per point, indexed like traj and alt, 4-byte aligned, required: the microseconds of the move
 *                       that LEAVES the point (ssrs_track_time's `dt`; a track's last point carries 0, so a track that ends
 *                       inside a cylinder adds no time for that point).  Read only for points inside at least one cylinder,
 *                       never outside [traj_offsets[0], traj_offsets[ntracks])
 *   time_per_turbine    uint64 (nturb), 8-byte aligned, required, ADDED to:
 *                           time_per_turbine[t] += (int64)dt[k]   for every point k inside turbine t
 *                       by the four conditions above, unchanged.  The sums are those of the sign-extended dt modulo 2^64:
 *                       ssrs_track_time never writes a negative dt, a caller's negative value is added as it stands.  A cull
 *                       list that names a turbine twice in a bin adds the point's time twice, as it does for the points
 * hits, first_step and points_per_turbine are what ssrs_rotor_encounters gives on the same input, bit for bit; first_step
 * and points_per_turbine stay optional and independent of the time.
 * No atomic per point: a lane's pending pair becomes (turbine, count, time), the time in 64 bits (one dt may be 2^31 - 1),
 * handed over when the turbine changes and at the end of its walk; the block keeps a uint64 time counter per turbine in LDS
 * beside the uint32 point counter (12 bytes a turbine together) and adds the non-zero ones to time_per_turbine once, at its
 * end.  THE LDS RULE: mask, point counters and time counters share the 60 KB.  The mask goes first: it stays in LDS only
 * while all three fit (beyond, bin_start is read per point).  Without the mask the point counters come next and the time
 * counters take what is left, 8 bytes a turbine from turbine 0 upwards: up to SSRS_ROTOR_TIMED_LDS_TURBINES turbines (7680
 * when points_per_turbine is NULL) every counter is in LDS; beyond, the hand-overs of the turbines past the last LDS counter
 * go to time_per_turbine as 64-bit global adds (still one per change of turbine, not one per point).  The result is the
 * same integers on either side.
 * Errors as ssrs_rotor_encounters; a NULL or misaligned dt or time_per_turbine -> SSRS_ERR_INVALID before any GPU work.
 * ntracks == 0, or no points, returns SSRS_OK and touches nothing. */
#define SSRS_ROTOR_TIMED_LDS_TURBINES 5120
int ssrs_rotor_encounters_timed(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks, const int32_t *alt,
                                const int32_t *dt, const int32_t *cellinfo, int rows, int cols, const double *turbines,
                                const double *reach, const int32_t *zband, int nturb, const int32_t *bin_start,
                                const int32_t *bin_items, uint32_t *hits, int32_t *first_step,
                                uint64_t *points_per_turbine, uint64_t *time_per_turbine, void *stream);

/* -------------------------------------------------------------- occupancy */

/* K13 -- how many DISTINCT tracks passed through each cell, from the trajectories on the device: the per-cell analogue
 * of tracks_per_turbine, which the visit histogram cannot give (a track that loiters in a cell is many visits).
 *   traj, traj_offsets  exactly what ssrs_turbine_encounters takes: int16 (row, col) pairs, 4-byte aligned (16-byte
 *                       aligned buffers are read 16 bytes a lane); int64 offsets (ntracks + 1), the first need not be 0,
 *                       equal consecutive offsets are an empty track.  Points outside [0, rows) x [0, cols) are ignored
 *   counts              uint32 (rows, cols), ADDED to: +1 in cell (r, c) for every track with at least one point (r, c),
 *                       so that chunks, sub-batches and calls accumulate in one raster
 *   cells_per_track     uint32 (ntracks) or NULL, ADDED to: the number of distinct in-raster cells of each track.
 *                       Sum(cells_per_track) == Sum(counts) of one call: the caller's checksum
 *   planes              1..SSRS_OCCUPANCY_MAX_PLANES: tracks are taken in rounds of 32 * planes, track k of a round owning
 *                       bit k & 31 of plane k >> 5.  The result does not depend on it
 *   workspace           `planes` uint32 rasters, ssrs_track_occupancy_workspace_bytes = rows * cols * 4 * planes rounded up
 *                       to 256.  It must be ZERO on entry and is left zero on every successful return: calls chain
 *                       without a memset in between (after a failed call, zero it)
 * Per round one "set" kernel over the round's points (test the bit with an L2 load, atomicOr it otherwise; the one lane
 * that is handed the old value without the bit counts the cell) and one clearing step: an "unset" kernel over the same
 * points when they are fewer bytes than the round's planes, else a memset of those.  Exact, and independent of the
 * launch order.  The offsets at the round borders are read back first (each launch is sized from its round's points),
 * so the call waits for `stream` once; its launches go to `stream` in order.
 * NULL traj / traj_offsets / counts / workspace, planes outside [1, SSRS_OCCUPANCY_MAX_PLANES], rows / cols outside
 * [1, 32767], ntracks outside [0, 2^31), a misaligned traj, a workspace that is too small -> SSRS_ERR_INVALID before any
 * GPU work.  ntracks == 0, or no points, returns SSRS_OK and touches nothing. */
#define SSRS_OCCUPANCY_MAX_PLANES 8
size_t ssrs_track_occupancy_workspace_bytes(int rows, int cols, int planes);
int ssrs_track_occupancy(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks,
                         int rows, int cols, int planes,
                         uint32_t *counts, uint32_t *cells_per_track,
                         void *workspace, size_t workspace_bytes, void *stream);

/* --------------------------------------------------------------- altitude */

/* K14 -- flight height above ground along every track, and rotor-zone presence.  THIS BUILD'S OWN MODEL (the reference has
 * no altitude model), defined in integers so that the scan gives the same bits however it is grouped.  All heights are
 * int32 millimetres above ground.
 *   cellinfo  one {int32 climb, int32 elev} pair per cell (8 bytes, 8-byte aligned), built by ssrs_altitude_cellinfo:
 *       climb = (int32) clip(rint((w - sink) * scale), -2^26, 2^26): the millimetres gained on one orthogonal move out of the
 *               cell.  w is the un-thresholded updraft (f32 or f64, widened to f64, NaN read as 0), sink in m/s, scale =
 *               1000 * resolution / airspeed; the subtraction and the product round on their own, as
 *               np.rint((w.astype(f64) - sink) * scale) does
 *       elev  = (int32) clip(rint(1000 * z), -2^30, 2^30) of the DEM z; a NaN (nodata) z gives the sentinel INT32_MIN
 *   a move from point k = (r, c) to point k + 1 = (r', c') of a track is diagonal iff r' != r and c' != c (a burn-in jump
 *       is one move, whatever its length);  step = diagonal ? (int32)(((int64)climb[r, c] * 92682 + 32768) >> 16) : climb[r, c]
 *       (arithmetic shift; 92682 = round(sqrt(2) * 2^16));  a_k = step - (elev[r', c'] - elev[r, c]), the terrain difference
 *       being 0 when either elev is the sentinel;  a_k = 0 when either point lies outside [0, rows) x [0, cols)
 *   h_0 = clamp(start, floor, ceil);  h_{k+1} = clamp(h_k + a_k, floor, ceil), the sum in int64
 *   a point is "in the rotor zone" iff it lies inside the raster and band_lo <= h <= band_hi
 * ssrs_track_altitude:
 *   traj, traj_offsets, ntracks   exactly what ssrs_track_occupancy takes (the first offset need not be 0, equal consecutive
 *                       offsets are an empty track, traj 4-byte aligned)
 *   params              {start, floor, ceil, band_lo, band_hi} in mm
 *   outputs, each may be NULL; the per-point ones are indexed like traj and written for the points
 *   [traj_offsets[0], traj_offsets[ntracks]) only:
 *     alt               int32 per point, OVERWRITTEN: the height
 *     band_hist         uint32 (rows, cols), ADDED to: +1 in the cell of every point in the rotor zone
 *     traj_band         int16 pairs, OVERWRITTEN: traj with every point that is not in the rotor zone replaced by (-1, -1);
 *                       ssrs_turbine_encounters and ssrs_track_occupancy ignore such points, so it feeds them as it stands
 *     in_band, h_min, h_max   int32 (ntracks), OVERWRITTEN: the track's points in the rotor zone, and the least and the
 *                       greatest height over ALL its points; an empty track gets 0, INT32_MAX, INT32_MIN.
 *                       Sum(in_band) == Sum(added to band_hist): the caller's checksum
 *   workspace           24 bytes per tile of SSRS_ALTITUDE_TILE points (its operator and its first and last track), ssrs_track_altitude_workspace_bytes(points of the
 *                       chunk), 16-byte aligned; its contents before a call mean nothing and after it are unspecified
 * Three launches in `stream`'s order: the composed operator x -> min(max(x + A, L), H) of every tile of consecutive points
 * of the chunk; one block that scans those; every tile again behind its carry, writing the outputs.  No block waits for
 * another.  Exact, and independent of the launch order.  traj_offsets[0] and traj_offsets[ntracks] are read back first
 * (the launches are sized from them), so the call waits for `stream` once.  16-byte aligned traj / alt / traj_band are read
 * and written 16 bytes a lane.
 * NULL traj / traj_offsets / cellinfo / params / workspace, rows / cols outside [1, 32767], ntracks outside [0, 2^31), a
 * misaligned traj, traj_band, cellinfo or workspace, floor > ceil, band_lo > band_hi, a workspace smaller than
 * ssrs_track_altitude_workspace_bytes(0) -> SSRS_ERR_INVALID before any GPU work; a workspace too small for the chunk's
 * points -> SSRS_ERR_INVALID once the two offsets are known, before any launch.  ntracks == 0, or no points, returns
 * SSRS_OK and touches nothing.  ssrs_altitude_cellinfo is one raster launch, asynchronous on `stream`. */
#define SSRS_ALTITUDE_TILE 4096
typedef struct SsrsAltitudeParams {
    int32_t start, floor, ceil, band_lo, band_hi;
} SsrsAltitudeParams;
int ssrs_altitude_cellinfo(const void *updraft, int updraft_type, const void *dem, int dem_type, int rows, int cols,
                           double sink, double scale, int32_t *cellinfo, void *stream);
size_t ssrs_track_altitude_workspace_bytes(int64_t npoints);
int ssrs_track_altitude(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks,
                        const int32_t *cellinfo, int rows, int cols, const SsrsAltitudeParams *params,
                        int32_t *alt, uint32_t *band_hist, int16_t *traj_band,
                        int32_t *in_band, int32_t *h_min, int32_t *h_max,
                        void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------ flight time */

/* K16 -- flight time along every track: wind-drift microseconds per cell, per track and over the rotor zone.  THIS BUILD'S
 * OWN MODEL (the reference has none), defined in integers so that any grouping of the work gives the same bits.
 *   scalars   va (airspeed), gmin (least ground speed) in mm/s and res_mm (cell size in mm) of SsrsFlightTimeParams:
 *       1 <= va <= 2^20, 1 <= gmin <= va, 1 <= res_mm <= 10^6.  diag_mm = (res_mm * 92682 + 32768) >> 16;
 *       num_orth = res_mm * 10^6, num_diag = diag_mm * 10^6 (int64);  CAP = 2^31 - 1 microseconds
 *   windinfo  one {int32 wr, int32 wc} pair per cell (8 bytes, 8-byte aligned), built by ssrs_flight_windinfo: the
 *       velocity of the AIR along +row and +col in mm/s.  With (ur, uc) the upwind unit step of the shelter ray below
 *       (SSRS_RAY_ROW_NORTH (cos A, sin A), SSRS_RAY_ROW_EAST (sin A, cos A), A = wdirn * pi / 180 in f64):
 *       wr = (int32) clip(rint((-1000 * wspeed) * ur), -2^20, 2^20), wc likewise with uc; the two products round on their
 *       own; a component that is not a number (NaN speed or direction) is 0, still air.  f32 inputs are widened to f64
 *   a move from point k = (r, c) to point k + 1 = (r', c') of the same track: sr = sign(r' - r), sc = sign(c' - c) (a
 *       burn-in jump is ONE move in the direction of its signs); (wr, wc) is the wind of the cell the move LEAVES.
 *       either point outside [0, rows) x [0, cols): dt = 0
 *       sr == sc == 0:   dt = min((num_orth + va / 2) / va, CAP)
 *       orthogonal:      a = sr * wr or sc * wc (along the move), b = the other component, cross2 = b * b, num = num_orth
 *       diagonal:        a = ((sr * wr + sc * wc) * 46341 + 32768) >> 16 (arithmetic shift), b = sr * wc - sc * wr,
 *                        cross2 = (b * b) >> 1, num = num_diag
 *       s = va * va - cross2 (int64);  g = gmin if s <= 0, else max(a + isqrt(s), gmin), isqrt the exact floor square root
 *       dt = min((num + (g >> 1)) / g, CAP) microseconds, by floor division
 * ssrs_track_time:
 *   traj, traj_offsets, ntracks   exactly what ssrs_track_altitude takes
 *   masked              NULL, or ssrs_track_altitude's traj_band of the same points: point k is "in the zone" iff
 *                       masked[k] has row >= 0
 *   windinfo            the raster above, or NULL: (uniform_wr, uniform_wc), each within +-2^20, in every cell
 *   outputs, each may be NULL; dt is indexed like traj and written for [traj_offsets[0], traj_offsets[ntracks]) only:
 *     time_hist         uint64 (rows, cols) microseconds, ADDED to: the dt of every move, in the cell it leaves
 *     band_time_hist    uint64 (rows, cols), ADDED to: the same for the moves that leave a point in the zone (needs masked)
 *     per_track         int64 (ntracks, 2), OVERWRITTEN (whenever ntracks > 0): [total, in zone] of the track's moves.
 *                       The last point of a track, single-point and empty tracks contribute 0.  Sum(total) == Sum(added
 *                       to time_hist) and Sum(in zone) == Sum(added to band_time_hist) modulo 2^64: the caller's checksums
 *     dt                int32 per point, OVERWRITTEN: the dt of the move that leaves the point, 0 at a track's last point
 * One memset of per_track and one launch in `stream`'s order; a block takes SSRS_FLIGHT_TIME_TILE consecutive points.
 * Exact, and independent of the launch order.  traj_offsets[0] and traj_offsets[ntracks] are read back first (the launch
 * is sized from them), so the call waits for `stream` once.  16-byte aligned traj / masked / dt are read and written 16
 * bytes a lane.
 * NULL traj / traj_offsets / params, rows / cols outside [1, 32767], ntracks outside [0, 2^31), a misaligned buffer, a
 * scalar out of range, band_time_hist without masked -> SSRS_ERR_INVALID before any GPU work.  ntracks == 0 returns SSRS_OK
 * and touches nothing; no points writes per_track only.  ssrs_flight_windinfo is one raster launch, asynchronous on
 * `stream`. */
#define SSRS_FLIGHT_TIME_TILE 4096
typedef struct SsrsFlightTimeParams {
    int32_t va, gmin, res_mm;
} SsrsFlightTimeParams;
int ssrs_flight_windinfo(const void *wspeed, const void *wdirn, int type, int rows, int cols, int ray_axes,
                         int32_t *windinfo, void *stream);
int ssrs_track_time(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks, const int16_t *masked,
                    const int32_t *windinfo, int uniform_wr, int uniform_wc, int rows, int cols,
                    const SsrsFlightTimeParams *params, uint64_t *time_hist, uint64_t *band_time_hist,
                    int64_t *per_track, int32_t *dt, void *stream);

/* ---------------------------------------------------------------- shelter */

/* K9 -- the terrain-shelter angle Sx (Winstral et al. 2002) and the orographic updraft adjusted by it and by a
 * flight-height factor.  Per cell (r0, c0) of the DEM z, with K = floor(dmax / res) >= 1 samples along the upwind ray:
 *   upwind unit step (ur, uc) in (row, col): SSRS_RAY_ROW_NORTH (cos A, sin A), SSRS_RAY_ROW_EAST (sin A, cos A), A the
 *       direction the wind comes from in degrees clockwise from north.  SSRS_RAY_ROW_EAST is the frame of the Horn
 *       aspect that ssrs_slope_aspect / ssrs_updraft_from_dem compute from a DEM alone
 *   for k = 1..K and both axes: o = (double)k * u, io = floor(o), fo = o - io; fo < 1e-9 -> fo = 0;
 *       fo > 1 - 1e-9 -> io += 1, fo = 0.  Sample cell (i, j) = (r0 + io_r, c0 + io_c); valid iff 0 <= i and
 *       (i + 1 <= rows - 1 or (fo_r == 0 and i <= rows - 1)), the same for j.  Invalid samples are skipped
 *   zs = (z[i,j] (1 - fo_c) + z[i,j+1] fo_c) (1 - fo_r) + (z[i+1,j] (1 - fo_c) + z[i+1,j+1] fo_c) fo_r, no
 *       contraction; a neighbour of weight 0 is not read and enters as 0.0
 *   T_k = (zs - z0) * (1.0 / ((double)k * res)); NaN skipped; T = max_k T_k (a T_k replaces T iff T_k > T); T = 0
 *       when no sample is valid, z0 is NaN or the ray direction is NaN.  tan_sx = T, sx_deg = atan(T) 180 / pi.
 * Wind direction: EITHER ray_ur / ray_uc, `batch` HOST doubles each (uniform wind: the caller's cos / sin), OR wdirn,
 * a DEVICE f64 raster (batch, rows, cols) in degrees (the step comes from the device's sine / cosine of degrees).
 * path: SSRS_SHELTER_AUTO stages the DEM tile and its upwind halo of K + 2 cells in LDS when that fits and reads
 * global memory otherwise; _LDS / _GLOBAL force one (A/B; _LDS that does not fit is SSRS_ERR_INVALID).  Both give the
 * same bits.  Outputs f64 (batch, rows, cols); either may be NULL.  Arguments are checked before any GPU work. */
#define SSRS_RAY_ROW_NORTH 0
#define SSRS_RAY_ROW_EAST 1
#define SSRS_SHELTER_AUTO 0
#define SSRS_SHELTER_LDS 1
#define SSRS_SHELTER_GLOBAL 2
int ssrs_shelter_sx(const void *dem, int dem_type, double res, const double *ray_ur, const double *ray_uc,
                    const double *wdirn, double dmax, int ray_axes, int path, double *tan_sx, double *sx_deg,
                    int rows, int cols, int batch, void *stream);

typedef struct SsrsShelterParams {
    double dmax;      /* metres; K = floor(dmax / res) */
    int32_t ray_axes; /* SSRS_RAY_* */
    int32_t path;     /* SSRS_SHELTER_* */
    double height;    /* h, metres above ground */
    double coef[7];   /* a, b, c, d, e, f, g */
} SsrsShelterParams;

/* The adjusted updraft, batched over `batch` wind cases with the terrain read once:
 *   w0   = the orographic updraft before its clamp: with slope / aspect NULL from the Horn stencil of the DEM in the
 *          arithmetic of ssrs_updraft_from_dem (wind direction wdirn0 in degrees), else from the slope / aspect DEVICE
 *          rasters (sa_type SSRS_F32 / _F64, degrees) in the arithmetic of ssrs_orographic_updraft
 *   F_h  = (a h^2 + b h + c) d^(e - cos(slope)) + f, cos(slope) = 8 res / sqrt((8 res)^2 + X^2 + Y^2) from the Horn
 *          sums, or the cosine of the slope raster; d^x = exp(x ln d), d > 0
 *   F_sx = max(0, 1 + g T)
 *   w    = max(min_updraft_val, w0 F_sx / F_h) -> orograph f32; usable f64 = the threshold function of that f32
 *          (threshold > 0 when usable is asked for); sx_deg as above.  Any output may be NULL.
 * Uniform wind: ray_ur, ray_uc, wspeed0, wdirn0, `batch` HOST doubles each, and wspeed = wdirn = NULL.  Per-cell wind:
 * wspeed, wdirn DEVICE f64 (batch, rows, cols), the four host arrays NULL.  Coefficients for which F_h <= 0 can occur
 * (checked at cos(slope) = 0 and 1), d <= 0, height < 0, K < 1: SSRS_ERR_INVALID before any GPU work.  With
 * coef = (0, 0, 1, 1, 0, 0, 0) the outputs equal those of the two calls named above bit for bit. */
int ssrs_updraft_sheltered(const void *dem, int dem_type, double res, const double *ray_ur, const double *ray_uc,
                           const double *wspeed0, const double *wdirn0, const double *wspeed, const double *wdirn,
                           const void *slope, const void *aspect, int sa_type, const SsrsShelterParams *params,
                           double min_updraft_val, double threshold, float *orograph, double *usable,
                           double *sx_deg, int rows, int cols, int batch, void *stream);

/* Sx averaged over an upwind SECTOR of azimuths (Winstral's shelter parameter: typically 30 degrees wide in steps of 5),
 * in one kernel: the tile is staged once for all rays of a cell, the mean stays in registers.  With a half-width
 * W = sector_half_width >= 0 and a step S = sector_step > 0, both in degrees:
 *   H = floor(W / S + 1e-9), M = 2 H + 1 azimuths A_m = A + (double)(m - H) S, m = 0 .. 2 H, A the direction the wind
 *       comes from
 *   T_m = the T of ssrs_shelter_sx for A_m: the same unit step per ray_axes, the same K = floor(dmax / res) samples,
 *       snap, validity rule, unread weight-0 neighbour, NaN skipping and operation order; T_m = 0 without a valid sample,
 *       for a NaN z0 or a NaN direction
 *   sx_deg = Sx-bar = (sum_m atan(T_m) (180 / pi)) / (double)M, summed in ascending m in f64 (starting from 0.0)
 *   tan_sx = T-bar  = tan(Sx-bar (pi / 180)).  For M = 1 (W < S): T-bar = T_0 and Sx-bar = atan(T_0) (180 / pi), no
 *       division and no round trip, so the outputs of the single-ray calls are reproduced bit for bit
 *   the updraft is that of ssrs_updraft_sheltered with T-bar for T: F_sx = max(0, 1 + g T-bar)
 * Uniform wind: ray_ur / ray_uc hold `batch` x M HOST doubles, case-major (entry j M + m = the unit step of A_m of case
 * j, the caller's cos / sin); wdirn0 stays the centre direction A.  Per-cell wind: the device forms A_m from the raster
 * value and takes its sine / cosine of degrees.  Everything else is as in the single-ray calls, `path` included: the
 * LDS halo of a uniform case is K |u| + 2 cells on every side one of its rays points to and 2 on the others, all round
 * for per-cell wind, and a halo that does not fit reads global memory with the same bits.  W not finite or outside
 * [0, 90], S not finite or not > 0, M > 61: SSRS_ERR_INVALID before anything else is looked at and before any GPU
 * work. */
int ssrs_shelter_sx_sector(const void *dem, int dem_type, double res, const double *ray_ur, const double *ray_uc,
                           const double *wdirn, double dmax, int ray_axes, int path, double sector_half_width,
                           double sector_step, double *tan_sx, double *sx_deg, int rows, int cols, int batch,
                           void *stream);
int ssrs_updraft_sheltered_sector(const void *dem, int dem_type, double res, const double *ray_ur, const double *ray_uc,
                                  const double *wspeed0, const double *wdirn0, const double *wspeed,
                                  const double *wdirn, const void *slope, const void *aspect, int sa_type,
                                  const SsrsShelterParams *params, double sector_half_width, double sector_step,
                                  double min_updraft_val, double threshold, float *orograph, double *usable,
                                  double *sx_deg, int rows, int cols, int batch, void *stream);

/* ----------------------------------------------------------------- smooth */

/* K11 -- Gaussian smoothing of the improved orographic updraft: scipy.ndimage.gaussian_filter(x, sigma,
 * mode='reflect') of an f32 raster x (batch, rows, cols), `sigma` in cells, with the clamp and the threshold function
 * of ssrs_updraft_sheltered fused into the second pass.
 *   R = int(4 sigma + 0.5) (truncate = 4).  On the host in f64: e[k] = exp(-0.5 / (sigma sigma) k k), k = -R .. R,
 *       w[k] = e[k] / sum(e) (summed in ascending k): the radius and the weights of ssrs_gaussian_blur.  R = 0
 *       (sigma < 0.125): w = {1}, the blur is the identity.  R > 512: SSRS_ERR_INVALID
 *   load: a non-finite x (NaN, +-inf) enters as 0.0 -- the sheltered kernels give a nodata cell min_updraft_val, which
 *       is -inf when the clamp is lifted, and 0.0 is what the unsmoothed model gives such a cell
 *   boundary: 'reflect' (d c b a | a b c d | d c b a) to any depth.  An index i outside [0, n) reads m = i mod 2 n
 *       taken non-negative, then m < n ? m : 2 n - 1 - m.  R may exceed 2 n; n = 1 is legal
 *   axis 0 (rows) first, then axis 1 (columns), the intermediate in f64.  Per axis and position p:
 *       acc = x[p] * w[0]; for k = R, R - 1, .., 1: acc = acc + (x[p - k] + x[p + k]) * w[k]; every product and sum
 *       rounded (no contraction): the order of scipy's symmetric correlate1d.  The order does not depend on the tile a
 *       cell falls in, on the path or on the case's place in the batch
 *   smooth f64 = the second pass's sum; orograph f32 = (float)(smooth > min_updraft_val ? smooth : min_updraft_val);
 *       usable f64 = the threshold function of that f32 widened again, in the arithmetic ssrs_updraft_sheltered uses
 *       without slope / aspect rasters (that of ssrs_updraft_from_dem).  Any of the three may be NULL, not all;
 *       orograph may be `in` itself (a case's first pass has read it before its second pass writes)
 * path: SSRS_SMOOTH_AUTO stages a tile and its reflected halo of R cells along the pass's axis in LDS when R <= 128
 * (sigma 30, the model's cap of 300 m at 10 m, is R = 120) and reads global memory through the index rule otherwise;
 * _LDS / _GLOBAL force one (A/B; _LDS with R > 128 is SSRS_ERR_INVALID).  All paths give the same bits.
 * workspace: ssrs_smooth_workspace_bytes() DEVICE bytes, 256-byte aligned -- the R + 1 weights and ONE f64 plane, which
 * the cases of a batch use one after the other (the size does not grow with `batch`; 0 for arguments that would be
 * refused); its contents before a call mean nothing and after it are unspecified.
 * Checked before any GPU work: `in` and workspace not NULL, rows, cols, batch >= 1, sigma finite and > 0,
 * R <= 512, min_updraft_val not NaN, a threshold > 0 when usable is asked for, path, the workspace size.
 * Asynchronous on `stream`; no host-device copy and no synchronisation (the weights travel as kernel arguments). */
#define SSRS_SMOOTH_AUTO 0
#define SSRS_SMOOTH_LDS 1
#define SSRS_SMOOTH_GLOBAL 2
size_t ssrs_smooth_workspace_bytes(int rows, int cols, int batch, double sigma);
int ssrs_smooth_reflect(const float *in, double sigma, int path, double min_updraft_val, double threshold,
                        double *smooth, float *orograph, double *usable, int rows, int cols, int batch,
                        void *workspace, size_t workspace_bytes, void *stream);

/* -------------------------------------------------------- allen thermals */

/* K12 -- Allen's (2006) field of discrete thermal updrafts, the model the reference carries commented out at
 * ssrs/layers.py:304-493: one field (rows, cols) per call.  The caller computes, in f64 on the host, from the height z,
 * the boundary-layer height zi and the convective velocity scale wstar:
 *   zzi = z / zi, rbar = 0.102 zzi^(1/3) (1 - 0.25 zzi) zi, wtbar = zzi^(1/3) (1 - 1.1 zzi) wstar, z_below_zi = z < zi,
 *   we = the environment sink (<= 0; 0 = none)
 * Updraft k sits at (xt[k], yt[k]) metres from the centre of cell (0, 0) and has the gains wgain[k], rgain[k].
 * PRECONDITION, checked by the Python wrapper and not here: every coordinate is finite and inside
 * [0, cols res] x [0, rows res], every gain is finite.
 *   table (n_updrafts, SSRS_ALLEN_TABLE_COLS) f64, one thread per updraft, every operation rounded, no contraction:
 *       r2 = max(10, rbar rgain); r1r2 = r2 < 600 ? 0.0011 r2 + 0.14 : 0.8; r1 = r1r2 r2; wbar = wtbar wgain;
 *       wpeak = 3 wbar (r2 r2 r2 - r2 r2 r1) / (r2 r2 r2 - r1 r1 r1), products from the left;
 *       row = the first j in 0..5 with r1r2 < 0.5 (S[j] + S[j+1]), else 6, S = (0.14, 0.25, 0.36, 0.47, 0.58, 0.69, 0.80)
 *       columns: r2, r1r2, r1, wbar, wpeak, row.  Kept in the workspace; also written to `table` when that is not NULL
 *   cell (r, c) at (xc, yc) = (c res, r res) takes the updraft u with the smallest
 *       d2 = (xc - xt)(xc - xt) + (yc - yt)(yc - yt)   (unfused), the lowest index among equal d2
 *       nearest (rows, cols) int32 = u when not NULL
 *   dist = sqrt(d2); rr2 = dist / r2[u]; (k1..k4) = row `row[u]` of Allen's shape table
 *       ws = z_below_zi ? max(1 / (1 + pow(k1 fabs(rr2 + k3), k2)) + k4 rr2, 0) : 0
 *       wl = (dist > r1[u] && rr2 < 2) ? (pi / 6) sin(pi rr2) : 0
 *       wd = (0.5 < zzi && zzi <= 0.9) ? min(2.5 wl (zzi - 0.5), 0) : 0
 *       w  = wpeak[u] ws + wd wbar[u]
 *       if (we != 0 && dist > r1[u])  w = wpeak[u] != 0 ? w (1 - we / wpeak[u]) + we : we
 *       out (rows, cols): SSRS_F64 = w, SSRS_F32 = w rounded once
 * bins: a CSR over nbx x nby square bins of bin_size_m metres (>= res), bin_start int32 (nbx nby + 1), row-major
 * (bin = by nbx + bx), bin_items int32.  An updraft is listed in the bin (min(floor(xt / bin_size_m), nbx - 1),
 * min(floor(yt / bin_size_m), nby - 1)) and in no other; items ascend inside a bin.  Trusted, like the coordinates.
 * path: SSRS_ALLEN_GLOBAL -- every cell scans its own bin, then ring after ring of bins, and stops once its best d2 is
 * strictly below the square of (m - bin_size_m / 2^20), m = its distance to the nearest side of the scanned square that
 * is not the domain's edge, or once no bin is left.  SSRS_ALLEN_AUTO -- a block of 256 cells (16 x 16) first stages the
 * updrafts of the bins that meet its tile, plus one bin around them, in LDS and scans that list; a cell that cannot accept
 * under the same criterion, and every cell of a tile whose list exceeds 512 updrafts, goes on with the ring scan.
 * SSRS_ALLEN_LDS -- as _AUTO, but SSRS_ERR_INVALID ("does not fit") when some tile's list exceeds 512 updrafts; this
 * path alone synchronises `stream` (the longest list comes to the host).  All paths give the same bits.
 * workspace: ssrs_allen_workspace_bytes(n_updrafts) DEVICE bytes, 256-byte aligned (0 for a count that would be
 * refused): 256 bytes of counters, then the table.  After the call its first uint64 holds the number of cells that
 * finished on the ring scan under _AUTO / _LDS (a diagnostic; 0 under _GLOBAL); its contents before a call mean nothing
 * and after it are otherwise unspecified.
 * Checked before any GPU work, each refusal SSRS_ERR_INVALID naming the argument: xt, yt, wgain, rgain, bin_start,
 * bin_items, out, workspace not NULL; 1 <= n_updrafts <= SSRS_ALLEN_MAX_UPDRAFTS; rows, cols >= 1; res finite and > 0;
 * bin_size_m finite and >= res; nbx, nby in [1, 32768]; rbar, wtbar, zzi, we finite, zzi > 0, we <= 0; path; out_type;
 * the workspace size.  Asynchronous on `stream` except as said for _LDS. */
#define SSRS_ALLEN_MAX_UPDRAFTS (1 << 22)
#define SSRS_ALLEN_TABLE_COLS 6
#define SSRS_ALLEN_AUTO 0
#define SSRS_ALLEN_LDS 1
#define SSRS_ALLEN_GLOBAL 2
size_t ssrs_allen_workspace_bytes(int n_updrafts);
int ssrs_allen_thermal_field(const double *xt, const double *yt, const double *wgain, const double *rgain,
                             int n_updrafts, const int32_t *bin_start, const int32_t *bin_items, double bin_size_m,
                             int nbx, int nby, double rbar, double wtbar, double zzi, int z_below_zi, double we,
                             double res, int rows, int cols, int path, void *out, int out_type, int32_t *nearest,
                             double *table, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------- georef */

/* K10 -- Albers Equal Area Conic on an ellipsoid (Snyder, USGS PP 1395, eqs. 14-12 ... 14-21, 3-12, 3-16) and the
 * warp of a longitude / latitude raster onto the projected grid.  With e = sqrt(e2), angles in radians inside:
 *   q(phi) = (1 - e2) (sin phi / (1 - e2 sin^2 phi) - (1 / (2 e)) ln((1 - e sin phi) / (1 + e sin phi)))
 *   m(phi) = cos phi / sqrt(1 - e2 sin^2 phi)
 *   n = (m1^2 - m2^2) / (q2 - q1) (sin lat_1 when lat_1 = lat_2),  C = m1^2 + n q1,  rho0 = a sqrt(C - n q0) / n
 *   forward: rho = a sqrt(C - n q(phi)) / n, theta = n (lambda - lon_0), x = x_0 + rho sin theta,
 *            y = y_0 + rho0 - rho cos theta
 *   inverse: X = x - x_0, Y = rho0 - (y - y_0), rho = sqrt(X^2 + Y^2), theta = atan2(X, Y) (of -X, -Y for n < 0),
 *            qv = (C - (rho n / a)^2) / n, lambda = lon_0 + theta / n, phi from asin(clamp(qv / 2, -1, 1)) by a FIXED
 *            number of iterations of eq. 3-16 (ssrs_amd/csrc/georef.h), no contraction anywhere. */
typedef struct SsrsProjection {
    /* inputs */
    double a;     /* semi-major axis, metres */
    double e2;    /* eccentricity squared, in (0, 1) */
    double lat_1; /* standard parallels, degrees */
    double lat_2;
    double lat_0; /* origin, degrees */
    double lon_0;
    double x_0; /* false easting / northing, metres */
    double y_0;
    /* derived: filled by the init call below */
    double n;
    double C;
    double rho0;
    double e;
} SsrsProjection;

/* [host] fills n, C, rho0, e.  a <= 0, e2 outside (0, 1), |n| < 1e-12 (lat_1 = -lat_2: the cylindrical limit) or a
 * non-finite field -> SSRS_ERR_INVALID.  No GPU work. */
int ssrs_projection_init_albers(SsrsProjection *proj);

/* rasterio's reproject (bilinear) of the reference's get_raster_in_projected_crs (ssrs/raster.py:12-49) for a
 * source on a regular longitude / latitude grid: every destination cell gets the exact inverse projection of its
 * centre and one bilinear gather.
 *   src, src_type   (src_rows, src_cols) SSRS_F32 / _F64; pixel (i, j) has its centre at (lon0 + j dlon, lat0 + i dlat)
 *                   degrees.  dlon, dlat are signed: dlat < 0 is a north-up source (the GeoTIFF order), read in place.
 *                   NULL is allowed when dst is NULL
 *   nodata          source values equal to it count as missing, as NaN pixels always do; NaN = no such value
 *   proj            [host] an initialised SsrsProjection (passed on to the kernel by value)
 *   west, south, res  centre of destination cell (0, 0) and the cell size, metres; destination row 0 = south
 *   dst, dst_type   (rows, cols) SSRS_F32 / _F64 or NULL
 *   lon, lat        (rows, cols) f64 or NULL: the inverse projection of the cell centres itself, degrees
 *   uncovered       uint64, 1 value, or NULL: ACCUMULATED count of the cells of dst that got NaN (zero it first)
 * Cell (r, c): x = west + c res, y = south + r res, (lambda, phi) by the inverse above, fc = (lambda - lon0) / dlon,
 * fr = (phi - lat0) / dlat.  Covered iff 0 <= fr <= src_rows - 1 and 0 <= fc <= src_cols - 1.  i = floor(fr),
 * j = floor(fc), both lowered to src_rows - 2 / src_cols - 2 at the far edge; tr = fr - i, tc = fc - j;
 *   v = (z[i,j] (1 - tc) + z[i,j+1] tc) (1 - tr) + (z[i+1,j] (1 - tc) + z[i+1,j+1] tc) tr
 * in f64 (the order of zs above), then rounded to dst_type; a neighbour whose weight is exactly 0 is not read and
 * enters as 0.0.  A neighbour of non-zero weight that is NaN or equals nodata makes the cell NaN, and so does a cell
 * that is not covered; both count in *uncovered (one atomic per wave).  Nothing is counted when dst is NULL.
 * Asynchronous on `stream`.  dst, lon and lat all NULL, src NULL with dst given, a NULL proj or one that was not
 * initialised, rows / cols outside [1, 32767], src_rows / src_cols < 2, dlon or dlat 0, res <= 0, a type selector
 * that is neither SSRS_F32 nor SSRS_F64, a non-finite lon0 / lat0 / dlon / dlat / west / south / res or an infinite
 * nodata -> SSRS_ERR_INVALID before any GPU work. */
int ssrs_warp_lonlat_raster(const void *src, int src_type, int src_rows, int src_cols, double lon0, double lat0,
                            double dlon, double dlat, double nodata, const SsrsProjection *proj, double west,
                            double south, double res, void *dst, int dst_type, double *lon, double *lat,
                            unsigned long long *uncovered, int rows, int cols, void *stream);

/* -------------------------------------------------------------- potential */

typedef struct SsrsSolveStats {
    int32_t iterations;
    int32_t converged; /* 1 when |r| <= rel_tol |b| was reached */
    double residual;   /* final |r| / |b| */
    float kernel_ms;
    int32_t amg_levels;   /* levels of the aggregation hierarchy (0 = none) */
    int32_t amg_coarsest; /* nodes on its last level */
    float setup_ms;       /* building the hierarchy (not part of kernel_ms) */
    uint64_t workspace_used; /* bytes of `workspace` really touched (the size query is an upper bound) */
} SsrsSolveStats;

#define SSRS_SOLVE_NO_AMG 1  /* plain BiCGStab (A/B switch; stalls on real rasters) */
#define SSRS_SOLVE_K_CYCLE 2 /* K-cycle (two flexible-CG steps per coarse solve) on the
                               first coarse levels instead of the V-cycle; depth in flag
                               bits 12-15 (0 = 3 levels) */
#define SSRS_SOLVE_ONE_SIDED 4 /* aggregation strength relative to the row maximum only
                                 (A/B switch: the previous criterion; pairs dead with live
                                 cells and needs 2-3x the iterations) */
/* flags bits 4-6: extra pairs of Jacobi sweeps; bits 8-11: strict matching rounds of
 * the one-sided criterion (0 = 4) */

/* Device scratch that always suffices (about 1.5 KB per cell).  The hierarchy really takes ~840 B
 * per cell (SsrsSolveStats.workspace_used reports it); a smaller workspace is accepted and the call
 * fails with SSRS_ERR_INVALID ("workspace exhausted") when it does not suffice.  Its contents before a call mean
 * nothing and after it are unspecified. */
size_t ssrs_potential_workspace_bytes(int rows, int cols);

/* MovModel.assemble_sparse_linear_system + solve_sparse_linear_system
 * (ssrs/movmodel.py:59-128) without assembling anything: the row-normalised
 * 8-neighbour conductance operator is applied matrix-free and the Dirichlet
 * problem is solved in f64 by BiCGStab, right-preconditioned with one V-cycle of
 * an aggregation AMG built on the device from the same conductances (the
 * reference factorises with SuperLU).
 *   conductivity  f64 (rows, cols): the usable updraft
 *   fixed_mask    u8  (rows, cols): 1 on Dirichlet cells (get_boundary_nodes,
 *                 movmodel.py:21-57, evaluated by the host)
 *   fixed_values  f64 (rows, cols): boundary energy on those cells
 *   initial_guess f64 (rows, cols) or NULL
 *   potential     f32 (rows, cols) out, as `pot_energy.astype(np.float32)`
 *   max_iterations caps the PCG and BiCGStab iterations together (honoured to the next
 *                 multiple of 5, the interval of PCG's checks); a solve that stops there
 *                 returns SSRS_OK with converged == 0 and its best iterate, projected onto
 *                 the range of the Dirichlet values (the solution obeys the maximum
 *                 principle, an unfinished iterate need not; a converged field is written
 *                 as it is).  Only the fall-back after a BiCGStab breakdown has a budget
 *                 of its own.
 * Synchronous: the call returns after its last kernel, with `potential` and `stats` final.  All its work, the
 * hierarchy's set-up, the scans and the captured graph of the V-cycle included, goes to `stream`.  A NULL `stream`
 * is the one case in this library where work leaves the caller's stream: the null stream cannot be captured, so the
 * solve waits for the null stream once at entry and then runs on a non-blocking stream of its own (one per host
 * thread), which it waits for before it returns. */
int ssrs_potential_solve(const double *conductivity, const uint8_t *fixed_mask,
                         const double *fixed_values, const double *initial_guess,
                         float *potential, int rows, int cols, double rel_tol,
                         int max_iterations, int flags, void *workspace,
                         size_t workspace_bytes,
                         void *stats /* SsrsSolveStats*, [host], may be NULL */,
                         void *stream);

/* n uniforms of the contract above: out[i] = u(seed, track[i], step[i]).
 * Device self-check of the rocRAND-backed draw used by the stepper.  One launch, asynchronous on `stream`. */
int ssrs_uniform_selftest(uint64_t seed, const uint64_t *track,
                          const uint64_t *step, double *out, size_t n,
                          void *stream);

/* The roaming stepper's hand-over word of n (track, block) pairs next to the
 * four words of rocRAND's engine for the same block:
 *   packed[i] = (x & 0xFFFF0000) | (z >> 16) of words[4 i .. 4 i + 3] = x, y, z, w.
 * Device self-check of what a feeder wave writes for its stepping wave.  One launch, asynchronous on `stream`. */
int ssrs_roam_pair_word_selftest(uint64_t seed, const uint64_t *track,
                                 const uint64_t *block, uint32_t *packed,
                                 uint32_t *words, size_t n, void *stream);

/* The roaming regime's tables for a raster, built by the very launches ssrs_tracks_simulate uses when a batch
 * starts to roam.  thr: the table of ssrs_transition_thr_build for the same updraft / potential / prior.
 * pair_out: rows*cols*8 entries of 16 bytes (e0, ea, eb, ec), state = cell*8 + last move;
 * fine_out: rows*cols*8 entries of 8 bytes (t1, t2).
 * prior_words [host], 38 uint32 or NULL: ThrPrior zero_e[8], reversal, thr9[9], rev_ok, rev_rc, rev_e, then
 * FinePrior zero_t1[8], zero_t2[8], reversal.
 * rows, cols >= 3, rows*cols <= 2^25.  Asynchronous on `stream`. */
int ssrs_roam_tables_selftest(const double *updraft, const float *potential, const double *prior, const float *thr,
                              int rows, int cols, void *pair_out, void *fine_out, uint32_t *prior_words, void *stream);

/* Wave-pairs of the roaming stepper in the calling thread's last
 * ssrs_tracks_simulate* call (host values, thread-local; either may be NULL):
 *   fed  pairs whose uniforms a feeder wave handed over
 *   own  pairs whose Philox block the stepping wave computed itself
 * fed + own == SsrsTrackStats.roam_wave_pairs of that call.
 * SSRS_TRACKS_ROAM_FEED=0 runs without feeder waves (fed == 0). */
void ssrs_tracks_roam_feed_counts(int64_t *fed, int64_t *own);

/* Waves of the roaming stepper that left a launch because its stop flag was
 * up (the launch's first wave was through its steps), summed over the calling
 * thread's last ssrs_tracks_simulate* call (host value, thread-local).
 * 0 with SSRS_TRACKS_NO_ROAM_STOP. */
int64_t ssrs_tracks_roam_stopped_waves(void);

#ifdef __cplusplus
}
#endif
#endif /* SSRS_HIP_H_ */
