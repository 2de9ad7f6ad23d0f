// K9 -- terrain-shelter angle Sx (Winstral et al. 2002), of one upwind ray or averaged over the M azimuths of an upwind
// sector, and the orographic updraft adjusted by it and by a flight-height factor, for gfx950 (MI355X).  The model is
// stated in include/ssrs_hip.h and DESIGN.md (K9).
//
// Per cell and ray K = floor(dmax / res) bilinear samples of the DEM: 4 K reads of 8 bytes against 8 bytes of input, so
// the DEM tile and its upwind halo are staged in LDS once per block and every sample of the M rays is an LDS read.  One
// block of 512 threads per CU (8 waves share the one tile; the LDS bounds the residency, and 512 threads leave each lane
// the VGPRs the kernel takes without scratch: 1024 threads spilled):
//   uniform wind   tile 64 x 32 cells, the halo per side from the host (2 cells at least: the Horn stencil and the +1
//                  neighbour of a sample).  One ray at K = 50: 118 x 86 f64 = 81 KB.  (io, fo) of a sample depend on
//                  the ray and k alone, so the block tabulates them, 256 samples at a time, and every lane reads its
//                  entry from LDS as a broadcast
//   per-cell wind  the ray may point anywhere: tile 32 x 32, halo of K + 2 all round.  K = 50: 136 x 136 f64 = 148 KB
// A halo that does not fit is read from global memory instead: the same arithmetic on the same values, hence the same
// bits; the choice is the host's.  Several uniform cases in one launch re-stage the tile only when the halo changes: the
// terrain comes from HBM once.  Built with -ffp-contract=off like the rest (the sample is defined without contraction).
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "raster_math.h"

namespace ssrs {

constexpr int kShelterBlock = 512;
constexpr int kShelterTH = 32;
constexpr int kTileDoubles = 19200;              // 150 KB of the CU's 160 KB
constexpr int kRayChunk = 256;                   // samples tabulated at a time
constexpr int kMaxShelterBatch = 16;
constexpr int kMaxK = 1 << 20;
constexpr int kMaxSectorM = 61;
constexpr int kMaxSectorRays = 128;              // ray steps in the arguments of one launch: min(16, 128 / M) uniform cases

struct ShelterArgs {
    const void *dem;
    const double *wspeed_r, *wdirn_r;            // per-cell wind (batch, rows, cols) or NULL
    const void *slope, *aspect;                  // NULL: Horn stencil of the DEM
    double *tan_sx, *sx_deg, *usable;
    float *orograph;
    int rows, cols, K, batch;
    int row_north, use_lds, sa_f64, want_updraft;
    double res;
    double d, d2, min_val, thr, inv_thr, scale, em1;   // as FusedArgs of K1 (+ e - 1 for the elementwise form)
    double poly, ln_d, ce, cf, cg;                     // a h^2 + b h + c, ln d, e, f, g
    int M, H;                                          // M = 2 H + 1 rays per cell, azimuths A + (m - H) step; one ray: 1, 0
    double step;                                       // S in degrees: per-cell wind forms A_m on the device
    double ur[kMaxSectorRays], uc[kMaxSectorRays];     // uniform wind: case-major, M per case
    int mt[kMaxShelterBatch], ml[kMaxShelterBatch], mb[kMaxShelterBatch], mr[kMaxShelterBatch];   // its halo per side
    double wspeed[kMaxShelterBatch], wdirn[kMaxShelterBatch], cos_w[kMaxShelterBatch], sin_w[kMaxShelterBatch];
};
static_assert(sizeof(ShelterArgs) + 2 * sizeof(int) <= 4096, "the kernel's arguments must fit 4 KB");

// offset of one ray sample along one axis: o = k u -> (io, fo) with the snap that keeps an axis wind on the lattice
__device__ __forceinline__ void ray_offset(double k, double u, int &io, double &fo)
{
    const double o = k * u;
    const double fl = floor(o);
    io = static_cast<int>(fl);
    fo = o - fl;
    if (fo < 1e-9) {
        fo = 0.0;
    } else if (fo > 1.0 - 1e-9) {
        io += 1;
        fo = 0.0;
    }
}

struct DemView {
    double *tile;             // LDS image of rows [tr0, tr0 + lh) x cols [tc0, tc0 + lw), or unused
    int tr0, tc0, lh, lw;
    bool lds;
};

// z[i, j] of a cell inside the raster: from the tile when it holds the cell, else from global memory
template <typename Tin>
__device__ __forceinline__ double dem_at(const Tin *__restrict__ dem, int cols, const DemView &v, int i, int j)
{
    const int li = i - v.tr0, lj = j - v.tc0;
    if (v.lds && li >= 0 && li < v.lh && lj >= 0 && lj < v.lw) return v.tile[li * v.lw + lj];
    return static_cast<double>(dem[static_cast<size_t>(i) * cols + j]);
}

// Stage the tile at (r0, c0) with the halo of case b -- the host's per side under uniform wind, K + 2 all round under
// per-cell wind -- unless that is what the tile holds (block-uniform; an empty view, lh = 0, holds nothing)
template <typename Tin, bool UNIFORM>
__device__ __forceinline__ void stage_tile(const ShelterArgs &a, const Tin *__restrict__ dem, int b, int r0, int c0,
                                           DemView &v)
{
    if (!v.lds) return;
    const int mt = UNIFORM ? a.mt[b] : a.K + 2, ml = UNIFORM ? a.ml[b] : a.K + 2;
    const int mb = UNIFORM ? a.mb[b] : a.K + 2, mr = UNIFORM ? a.mr[b] : a.K + 2;
    const int lh = kShelterTH + mt + mb, lw = (UNIFORM ? 64 : 32) + ml + mr;     // host: lh * lw <= kTileDoubles
    if (r0 - mt == v.tr0 && c0 - ml == v.tc0 && lh == v.lh && lw == v.lw) return;
    __syncthreads();
    v.tr0 = r0 - mt;
    v.tc0 = c0 - ml;
    v.lh = lh;
    v.lw = lw;
    for (int i = threadIdx.x; i < lh * lw; i += kShelterBlock) {
        const int li = i / lw, lj = i - li * lw;
        const int gr = v.tr0 + li, gc = v.tc0 + lj;
        double z = 0.0;                                          // outside the raster: never read (validity rule)
        if (gr >= 0 && gr < a.rows && gc >= 0 && gc < a.cols)
            z = static_cast<double>(dem[static_cast<size_t>(gr) * a.cols + gc]);
        v.tile[i] = z;
    }
    __syncthreads();
}

// One sample: T <- T_k where valid and larger.  (i, j) the sample cell; neighbours of weight 0 are not read.
template <typename Tin>
__device__ __forceinline__ void shelter_sample(const Tin *__restrict__ dem, int rows, int cols, const DemView &v,
                                               int i, int j, double fo_r, double fo_c, double z0, double inv_d,
                                               double &T)
{
    const bool ok_r = i >= 0 && (i + 1 <= rows - 1 || (fo_r == 0.0 && i <= rows - 1));
    const bool ok_c = j >= 0 && (j + 1 <= cols - 1 || (fo_c == 0.0 && j <= cols - 1));
    if (!(ok_r && ok_c)) return;
    const int li = i - v.tr0, lj = j - v.tc0;
    double z00, z01 = 0.0, z10 = 0.0, z11 = 0.0;
    if (v.lds && li >= 0 && li + 1 < v.lh && lj >= 0 && lj + 1 < v.lw) {   // the 2 x 2 footprint lies in the tile
        const double *p = v.tile + li * v.lw + lj;
        z00 = p[0];
        z01 = fo_c != 0.0 ? p[1] : 0.0;
        z10 = fo_r != 0.0 ? p[v.lw] : 0.0;
        z11 = fo_r != 0.0 && fo_c != 0.0 ? p[v.lw + 1] : 0.0;
    } else {
        z00 = dem_at(dem, cols, v, i, j);
        if (fo_c != 0.0) z01 = dem_at(dem, cols, v, i, j + 1);
        if (fo_r != 0.0) {
            z10 = dem_at(dem, cols, v, i + 1, j);
            if (fo_c != 0.0) z11 = dem_at(dem, cols, v, i + 1, j + 1);
        }
    }
    const double zs = (z00 * (1.0 - fo_c) + z01 * fo_c) * (1.0 - fo_r) + (z10 * (1.0 - fo_c) + z11 * fo_c) * fo_r;
    const double tk = (zs - z0) * inv_d;
    if (tk > T) T = tk;                          // false for a NaN: skipped
}

// The sample table of one round: with e0 samples of the case's M K done, entry t is sample (e0 + t) % K + 1 of ray
// (e0 + t) / K
struct RayTable {
    double inv_d[kRayChunk], fo_r[kRayChunk], fo_c[kRayChunk];
    int io_r[kRayChunk], io_c[kRayChunk];
};

// Entries [0, n) of the round that starts at sample e0 of case b, one per thread; per-cell wind tabulates 1 / (k res)
// only.  (The loop over the round's rays is block-uniform: a ray's step is a scalar load.)
template <bool UNIFORM>
__device__ __forceinline__ void fill_ray_table(RayTable &s, const ShelterArgs &a, int b, int e0, int n)
{
    const int K = a.K, tid = threadIdx.x;
    for (int me = e0 / K; me * K < e0 + n; ++me) {
        const int ke = e0 + tid - me * K;                        // entry tid is sample ke + 1 of ray me
        if (tid < n && ke >= 0 && ke < K) {
            const double kd = static_cast<double>(ke + 1);
            s.inv_d[tid] = 1.0 / (kd * a.res);
            if (UNIFORM) {
                int io;
                double fo;
                ray_offset(kd, a.ur[b * a.M + me], io, fo);
                s.io_r[tid] = io;
                s.fo_r[tid] = fo;
                ray_offset(kd, a.uc[b * a.M + me], io, fo);
                s.io_c[tid] = io;
                s.fo_c[tid] = fo;
            }
        }
    }
}

// Sample k of cell (r, c) along its ray, entry kk of the table: the offsets from the table (uniform wind) or from the
// lane's own step (ur, uc)
template <typename Tin, bool UNIFORM>
__device__ __forceinline__ void ray_sample(const RayTable &s, int kk, int k, double ur, double uc,
                                           const Tin *__restrict__ dem, int rows, int cols, const DemView &v, int r, int c,
                                           double z0, double &T)
{
    int io_r, io_c;
    double fo_r, fo_c;
    if (UNIFORM) {
        io_r = s.io_r[kk];
        io_c = s.io_c[kk];
        fo_r = s.fo_r[kk];
        fo_c = s.fo_c[kk];
    } else {
        const double kd = static_cast<double>(k);
        ray_offset(kd, ur, io_r, fo_r);
        ray_offset(kd, uc, io_c, fo_c);
    }
    shelter_sample(dem, rows, cols, v, r + io_r, c + io_c, fo_r, fo_c, z0, s.inv_d[kk], T);
}

__device__ __forceinline__ double load_sa(const void *p, bool f64, size_t i)
{
    return f64 ? static_cast<const double *>(p)[i] : static_cast<double>(static_cast<const float *>(p)[i]);
}

// The adjusted updraft of cell (r, c) = i of case b (output o) from Tq = tan Sx; (sn_w, cs_w) the per-cell wind's
template <typename Tin, bool UNIFORM>
__device__ __forceinline__ void sheltered_updraft(const ShelterArgs &a, const Tin *__restrict__ dem, const DemView &v,
                                                  int b, int r, int c, size_t i, size_t o, double Tq, double sn_w,
                                                  double cs_w)
{
    const int rows = a.rows, cols = a.cols;
    double w0 = 0.0, cos_s = 1.0;
    if (a.slope) {
        // the arithmetic of k_orographic
        const double spd = UNIFORM ? a.wspeed[b] : a.wspeed_r[o];
        const double dir = UNIFORM ? a.wdirn[b] : a.wdirn_r[o];
        double sin_s, ad, unused;
        sincos_deg(load_sa(a.slope, a.sa_f64, i), sin_s, cos_s);
        sincos_deg(load_sa(a.aspect, a.sa_f64, i) - dir, unused, ad);
        ad = ad > 0.0 ? ad : 0.0;
        w0 = spd * (sin_s * ad);
    } else if (r > 0 && c > 0 && r < rows - 1 && c < cols - 1) {
        // the arithmetic of k_updraft_from_dem: un-normalised Horn sums, "x" = row axis
        const double spd = UNIFORM ? a.wspeed[b] : a.wspeed_r[o];
        const double cw = UNIFORM ? a.cos_w[b] : cs_w;
        const double sw = UNIFORM ? a.sin_w[b] : sn_w;
        const double m_l = dem_at(dem, cols, v, r - 1, c - 1), m_c = dem_at(dem, cols, v, r - 1, c),
                     m_r = dem_at(dem, cols, v, r - 1, c + 1);
        const double z_l = dem_at(dem, cols, v, r, c - 1), z_r = dem_at(dem, cols, v, r, c + 1);
        const double p_l = dem_at(dem, cols, v, r + 1, c - 1), p_c = dem_at(dem, cols, v, r + 1, c),
                     p_r = dem_at(dem, cols, v, r + 1, c + 1);
        const double X = (p_r + 2 * p_c + p_l) - (m_r + 2 * m_c + m_l);
        const double Y = (m_r + 2 * z_r + p_r) - (m_l + 2 * z_l + p_l);
        const double rs = rsqrt_pos(a.d2 + (X * X + Y * Y));
        if (X != 0.0) {
            const double P = -(Y * cw + X * sw);
            if (P > 0.0) w0 = spd * (P * rs);
        } else {
            const double dzdy = Y / a.d, dx = 1e-10;
            const double g2 = dzdy * dzdy, gp2 = dx * dx + g2;
            const double proj = -(dzdy * cw + dx * sw);
            if (proj > 0.0 && g2 > 0.0) w0 = spd * (proj * sqrt(g2 / (gp2 * (1.0 + g2))));
        }
        cos_s = a.d * rs;
        cos_s = cos_s == cos_s ? cos_s : 1.0;                    // NaN in the stencil: slope 0, as the layers
    }
    const double f_h = a.poly * exp((a.ce - cos_s) * a.ln_d) + a.cf;
    double f_sx = 1.0 + a.cg * Tq;
    f_sx = f_sx > 0.0 ? f_sx : 0.0;
    double w = w0 * f_sx / f_h;
    w = w > a.min_val ? w : a.min_val;
    const float w32 = static_cast<float>(w);
    if (a.orograph) a.orograph[o] = w32;
    if (a.usable)
        a.usable[o] = a.slope ? usable_updraft(static_cast<double>(w32), a.thr, a.em1)
                              : usable_updraft_fast(static_cast<double>(w32), a.thr, a.inv_thr, a.scale);
}

// The single ray (the host sets M = 1): Sx of every cell of a tile for the batch's cases.
template <typename Tin, bool UNIFORM>
__global__ __launch_bounds__(kShelterBlock) void k_shelter(ShelterArgs a, int tiles_x, int ntiles)
{
    constexpr int TW = UNIFORM ? 64 : 32;
    constexpr int TH = kShelterTH;
    constexpr int CPT = TW * TH / kShelterBlock;                 // cells per thread: 4 or 2
    __shared__ double s_tile[kTileDoubles];
    __shared__ RayTable s_tab;

    const Tin *__restrict__ dem = static_cast<const Tin *>(a.dem);
    const int rows = a.rows, cols = a.cols, K = a.K;
    const int t = xcd_tile(blockIdx.x, ntiles);
    const int r0 = (t / tiles_x) * TH, c0 = (t % tiles_x) * TW;
    const size_t ncell = static_cast<size_t>(rows) * cols;
    const int tid = threadIdx.x;

    DemView v;
    v.tile = s_tile;
    v.lds = a.use_lds != 0;
    v.tr0 = v.tc0 = v.lh = v.lw = 0;

    for (int b = 0; b < a.batch; ++b) {
        stage_tile<Tin, UNIFORM>(a, dem, b, r0, c0, v);

        // ---- this thread's cells, one after the other (every thread takes part in every barrier)
        const double ninf = -__builtin_huge_val();
#pragma unroll 1
        for (int q = 0; q < CPT; ++q) {
            const int cell = tid + q * kShelterBlock;
            const int r = r0 + cell / TW, c = c0 + cell % TW;
            const bool inside = r < rows && c < cols;
            const size_t i = static_cast<size_t>(r) * cols + c;
            const size_t o = b * ncell + i;
            bool live = inside;
            double z0 = 0.0, T = ninf, ur = 0.0, uc = 0.0, sn_w = 0.0, cs_w = 0.0;
            if (inside) {
                z0 = dem_at(dem, cols, v, r, c);
                if (!UNIFORM) {
                    sincos_deg(a.wdirn_r[o], sn_w, cs_w);
                    ur = a.row_north ? cs_w : sn_w;
                    uc = a.row_north ? sn_w : cs_w;
                    live = ur == ur && uc == uc;                 // NaN direction: no sample, T = 0
                }
            }

            // ---- the K samples, tabulated kRayChunk at a time
            for (int k0 = 0; k0 < K; k0 += kRayChunk) {
                const int n = K - k0 < kRayChunk ? K - k0 : kRayChunk;
                __syncthreads();                                 // the previous table is done with
                fill_ray_table<UNIFORM>(s_tab, a, b, k0, n);
                __syncthreads();
                if (!live) continue;
                for (int kk = 0; kk < n; ++kk)
                    ray_sample<Tin, UNIFORM>(s_tab, kk, k0 + kk + 1, ur, uc, dem, rows, cols, v, r, c, z0, T);
            }

            // ---- outputs
            if (!inside) continue;
            const double Tq = (T == ninf || z0 != z0) ? 0.0 : T;
            if (a.tan_sx) a.tan_sx[o] = Tq;
            if (a.sx_deg) a.sx_deg[o] = atan(Tq) * (180.0 / kPi);
            if (a.want_updraft) sheltered_updraft<Tin, UNIFORM>(a, dem, v, b, r, c, i, o, Tq, sn_w, cs_w);
        }
    }
}

// Sx averaged over M = 2 H + 1 azimuths A + (m - H) S (include/ssrs_hip.h): k_shelter's ray M times per cell on ONE
// staging of the tile, the sum of the angles kept in registers, Sx-bar, T-bar and the updraft written once.
template <typename Tin, bool UNIFORM>
__global__ __launch_bounds__(kShelterBlock) void k_shelter_sector(ShelterArgs a, int tiles_x, int ntiles)
{
    constexpr int TW = UNIFORM ? 64 : 32;
    constexpr int TH = kShelterTH;
    constexpr int CPT = TW * TH / kShelterBlock;                 // cells per thread: 4 or 2
    __shared__ double s_tile[kTileDoubles];
    __shared__ RayTable s_tab;

    const Tin *__restrict__ dem = static_cast<const Tin *>(a.dem);
    const int rows = a.rows, cols = a.cols, K = a.K, M = a.M;
    const int MK = M * K;                                        // host: M K < 2^31
    const int t = xcd_tile(blockIdx.x, ntiles);
    const int r0 = (t / tiles_x) * TH, c0 = (t % tiles_x) * TW;
    const size_t ncell = static_cast<size_t>(rows) * cols;
    const int tid = threadIdx.x;

    DemView v;
    v.tile = s_tile;
    v.lds = a.use_lds != 0;
    v.tr0 = v.tc0 = v.lh = v.lw = 0;

    for (int b = 0; b < a.batch; ++b) {
        stage_tile<Tin, UNIFORM>(a, dem, b, r0, c0, v);          // once for the M rays

        const double ninf = -__builtin_huge_val();
#pragma unroll 1
        for (int q = 0; q < CPT; ++q) {
            const int cell = tid + q * kShelterBlock;
            const int r = r0 + cell / TW, c = c0 + cell % TW;
            const bool inside = r < rows && c < cols;
            const size_t i = static_cast<size_t>(r) * cols + c;
            const size_t o = b * ncell + i;
            double z0 = 0.0, A = 0.0, sn_w = 0.0, cs_w = 0.0;
            if (inside) {
                z0 = dem_at(dem, cols, v, r, c);
                if (!UNIFORM) {
                    A = a.wdirn_r[o];
                    sincos_deg(A, sn_w, cs_w);                   // the centre ray's, for the Horn projection below
                }
            }

            // ---- the M K samples, ray after ray, tabulated kRayChunk at a time; (m, k) = the ray and the samples
            //      of it already taken
            double T = ninf, T0 = 0.0, acc = 0.0, ur = 0.0, uc = 0.0;
            bool ray_live = UNIFORM;
            int m = 0, k = 0;
            for (int e0 = 0; e0 < MK; e0 += kRayChunk) {
                const int n = MK - e0 < kRayChunk ? MK - e0 : kRayChunk;
                __syncthreads();                                 // the previous table is done with
                fill_ray_table<UNIFORM>(s_tab, a, b, e0, n);
                __syncthreads();
                if (!inside) continue;
                for (int kk = 0; kk < n; ++kk) {
                    if (!UNIFORM && k == 0) {
                        double sn, cs;
                        sincos_deg(A + static_cast<double>(m - a.H) * a.step, sn, cs);
                        ur = a.row_north ? cs : sn;
                        uc = a.row_north ? sn : cs;
                        ray_live = ur == ur && uc == uc;         // NaN direction: no sample, T_m = 0
                    }
                    if (ray_live) ray_sample<Tin, UNIFORM>(s_tab, kk, k + 1, ur, uc, dem, rows, cols, v, r, c, z0, T);
                    if (++k == K) {                              // ray m is complete: its angle joins the sum
                        const double Tm = (T == ninf || z0 != z0) ? 0.0 : T;
                        acc += atan(Tm) * (180.0 / kPi);
                        if (m == 0) T0 = Tm;
                        T = ninf;
                        k = 0;
                        ++m;
                    }
                }
            }

            // ---- outputs: one ray keeps its own T and angle (no round trip), M > 1 the mean angle and its tangent
            if (!inside) continue;
            double Tq = T0, sx = acc;
            if (M > 1) {
                sx = acc / static_cast<double>(M);
                Tq = tan(sx * (kPi / 180.0));
            }
            if (a.tan_sx) a.tan_sx[o] = Tq;
            if (a.sx_deg) a.sx_deg[o] = sx;
            if (a.want_updraft) sheltered_updraft<Tin, UNIFORM>(a, dem, v, b, r, c, i, o, Tq, sn_w, cs_w);
        }
    }
}

// LDS doubles the tile of a single ray takes, or 0 when it does not fit
static int shelter_tile_doubles(bool uniform, int K)
{
    const long long tw = uniform ? 64 : 32, th = kShelterTH;
    const long long halo = uniform ? static_cast<long long>(K) + 4 : 2 * (static_cast<long long>(K) + 2);
    const long long n = (tw + halo) * (th + halo);
    return n <= kTileDoubles ? static_cast<int>(n) : 0;
}

// The two halo rules of a uniform case: halo (top, left, bottom, right); true when the tile with it fits the LDS.
// A single ray: K + 2 on its two upwind sides, 2 on the others.
static bool single_ray_halo(double ur, double uc, int K, int halo[4])
{
    halo[0] = ur < 0.0 ? K + 2 : 2;
    halo[1] = uc < 0.0 ? K + 2 : 2;
    halo[2] = ur < 0.0 ? 2 : K + 2;
    halo[3] = uc < 0.0 ? 2 : K + 2;
    return shelter_tile_doubles(true, K) > 0;
}

// A sector: what its M rays reach, K |u| + 2 on the side a ray points to, 2 elsewhere
static bool sector_halo(const double *ur, const double *uc, int M, int K, int halo[4])
{
    halo[0] = halo[1] = halo[2] = halo[3] = 2;
    for (int m = 0; m < M; ++m) {
        const int rr = static_cast<int>(ceil(K * fabs(ur[m]))) + 2, rc = static_cast<int>(ceil(K * fabs(uc[m]))) + 2;
        int &side_r = ur[m] < 0.0 ? halo[0] : halo[2], &side_c = uc[m] < 0.0 ? halo[1] : halo[3];
        side_r = rr > side_r ? rr : side_r;
        side_c = rc > side_c ? rc : side_c;
    }
    const long long n = (64ll + halo[1] + halo[3]) * (kShelterTH + halo[0] + halo[2]);
    return n <= kTileDoubles;
}

static int shelter_path(int path)
{
    if (const char *e = std::getenv("SSRS_SHELTER_PATH")) {      // A/B switch: lds | global
        if (!std::strcmp(e, "lds")) path = SSRS_SHELTER_LDS;
        else if (!std::strcmp(e, "global")) path = SSRS_SHELTER_GLOBAL;
    }
    return path;
}

template <typename Tin, bool UNIFORM>
static void shelter_launch(bool sector, const ShelterArgs &a, int tx, int nt, hipStream_t st)
{
    if (sector) hipLaunchKernelGGL((k_shelter_sector<Tin, UNIFORM>), dim3(nt), dim3(kShelterBlock), 0, st, a, tx, nt);
    else hipLaunchKernelGGL((k_shelter<Tin, UNIFORM>), dim3(nt), dim3(kShelterBlock), 0, st, a, tx, nt);
}

// The launches of all four calls.  `a` holds what shelter_common / sheltered_common filled, M, H, step, and the outputs
// and the per-cell wind of case 0; `sector` chooses the halo rule and the kernel.  Uniform cases travel in the kernel's
// arguments, min(16, 128 / M) per launch, with their ray steps, halos and, for the updraft (wspeed0), wind.  `path`
// as shelter_path gives it.
static int shelter_run(const ShelterArgs &a, const char *who, int dem_type, const double *ray_ur, const double *ray_uc,
                       const double *wspeed0, const double *wdirn0, bool sector, int path, int batch, hipStream_t st)
{
    const bool uniform = ray_ur != nullptr, f64 = dem_type == SSRS_F64;
    const int M = a.M;
    const size_t ncell = static_cast<size_t>(a.rows) * a.cols;
    const int tw = uniform ? 64 : 32;
    const int tx = (a.cols + tw - 1) / tw, ty = (a.rows + kShelterTH - 1) / kShelterTH, nt = tx * ty;
    int step = batch;
    if (uniform) step = kMaxSectorRays / M < kMaxShelterBatch ? kMaxSectorRays / M : kMaxShelterBatch;
    for (int b0 = 0; b0 < batch; b0 += step) {
        ShelterArgs l = a;
        l.batch = batch - b0 < step ? batch - b0 : step;
        bool fits = uniform || shelter_tile_doubles(false, a.K) > 0;
        for (int j = 0; uniform && j < l.batch; ++j) {
            int h[4];
            const double *ur = ray_ur + static_cast<size_t>(b0 + j) * M, *uc = ray_uc + static_cast<size_t>(b0 + j) * M;
            // (one case too wide: the launch reads global memory)
            fits = (sector ? sector_halo(ur, uc, M, a.K, h) : single_ray_halo(ur[0], uc[0], a.K, h)) && fits;
            l.mt[j] = h[0];
            l.ml[j] = h[1];
            l.mb[j] = h[2];
            l.mr[j] = h[3];
            for (int m = 0; m < M; ++m) {
                l.ur[j * M + m] = ur[m];
                l.uc[j * M + m] = uc[m];
            }
            if (!wspeed0) continue;
            l.wspeed[j] = wspeed0[b0 + j];
            l.wdirn[j] = wdirn0[b0 + j];
            const double w = wdirn0[b0 + j] * kPi / 180.0;      // as ssrs_updraft_from_dem
            l.cos_w[j] = cos(w);
            l.sin_w[j] = sin(w);
        }
        // (sector_common has refused this already, case by case, for a sector call)
        SSRS_REQUIRE(!(path == SSRS_SHELTER_LDS && !fits), "%s: the halo of K = %d samples does not fit the LDS tile", who, a.K);
        l.use_lds = path != SSRS_SHELTER_GLOBAL && fits;
        if (a.tan_sx) l.tan_sx = a.tan_sx + b0 * ncell;
        if (a.sx_deg) l.sx_deg = a.sx_deg + b0 * ncell;
        if (a.orograph) l.orograph = a.orograph + b0 * ncell;
        if (a.usable) l.usable = a.usable + b0 * ncell;
        if (a.wspeed_r) l.wspeed_r = a.wspeed_r + b0 * ncell;
        if (a.wdirn_r) l.wdirn_r = a.wdirn_r + b0 * ncell;
        if (uniform && f64) shelter_launch<double, true>(sector, l, tx, nt, st);
        else if (uniform) shelter_launch<float, true>(sector, l, tx, nt, st);
        else if (f64) shelter_launch<double, false>(sector, l, tx, nt, st);
        else shelter_launch<float, false>(sector, l, tx, nt, st);
        SSRS_HIP_CHECK(hipGetLastError());
    }
    return SSRS_OK;
}

// The checks the four calls share; fills the geometry of `a`.
static int shelter_common(ShelterArgs &a, const char *who, const void *dem, int dem_type, double res,
                          const double *ray_ur, const double *ray_uc, const double *wdirn, double dmax, int ray_axes,
                          int path, int rows, int cols, int batch, int min_size)
{
    SSRS_REQUIRE(dem != nullptr, "%s: dem is NULL", who);
    SSRS_REQUIRE(dem_type == SSRS_F32 || dem_type == SSRS_F64, "%s: bad element type", who);
    SSRS_REQUIRE(rows >= min_size && cols >= min_size && batch >= 1,
                 "%s: need rows, cols >= %d and batch >= 1 (got %d x %d, batch %d)", who, min_size, rows, cols, batch);
    SSRS_REQUIRE(static_cast<long long>(rows) * cols < (1ll << 31), "%s: more than 2^31 - 1 cells", who);
    SSRS_REQUIRE(res > 0.0 && std::isfinite(res), "%s: res must be > 0", who);
    SSRS_REQUIRE(ray_axes == SSRS_RAY_ROW_NORTH || ray_axes == SSRS_RAY_ROW_EAST, "%s: bad ray_axes %d", who, ray_axes);
    SSRS_REQUIRE(path == SSRS_SHELTER_AUTO || path == SSRS_SHELTER_LDS || path == SSRS_SHELTER_GLOBAL,
                 "%s: bad path %d", who, path);
    SSRS_REQUIRE(dmax > 0.0 && std::isfinite(dmax), "%s: dmax must be > 0", who);
    const double k = floor(dmax / res);
    SSRS_REQUIRE(k >= 1.0, "%s: dmax = %g is less than one cell of %g m (K = floor(dmax / res) < 1)", who, dmax, res);
    SSRS_REQUIRE(k <= kMaxK, "%s: K = floor(dmax / res) exceeds %d", who, kMaxK);
    SSRS_REQUIRE((ray_ur != nullptr) == (ray_uc != nullptr), "%s: give both ray_ur and ray_uc or neither", who);
    SSRS_REQUIRE((ray_ur != nullptr) != (wdirn != nullptr),
                 "%s: give the wind direction either as ray_ur / ray_uc or as a wdirn raster", who);
    for (int j = 0; ray_ur && j < batch; ++j)
        SSRS_REQUIRE(std::isfinite(ray_ur[j]) && std::isfinite(ray_uc[j]) && fabs(ray_ur[j]) <= 1.0 && fabs(ray_uc[j]) <= 1.0,
                     "%s: ray step %d = (%g, %g) is not a unit step", who, j, ray_ur[j], ray_uc[j]);
    a.dem = dem;
    a.rows = rows;
    a.cols = cols;
    a.K = static_cast<int>(k);
    a.res = res;
    a.row_north = ray_axes == SSRS_RAY_ROW_NORTH;
    a.wdirn_r = wdirn;
    return SSRS_OK;
}

// The checks and the fill of `a` that the two updraft calls share (everything but the wind cases of a launch).
static int sheltered_common(ShelterArgs &a, const char *who, const void *dem, int dem_type, double res,
                            const double *ray_ur, const double *ray_uc, const double *wspeed0, const double *wdirn0,
                            const double *wspeed, const double *wdirn, const void *slope, const void *aspect,
                            int sa_type, const SsrsShelterParams *params, double min_updraft_val, double threshold,
                            bool want_usable, int rows, int cols, int batch)
{
    SSRS_REQUIRE(params != nullptr, "%s: params is NULL", who);
    if (int rc = shelter_common(a, who, dem, dem_type, res, ray_ur, ray_uc, wdirn, params->dmax, params->ray_axes,
                                params->path, rows, cols, batch, 3))
        return rc;
    const bool uniform = ray_ur != nullptr;
    SSRS_REQUIRE(uniform ? (wspeed0 && wdirn0 && !wspeed) : (wspeed && !wspeed0 && !wdirn0),
                 "%s: uniform wind takes ray_ur, ray_uc, wspeed0, wdirn0 (host); per-cell wind takes wspeed, wdirn (device)", who);
    SSRS_REQUIRE((slope == nullptr) == (aspect == nullptr), "%s: give both slope and aspect or neither", who);
    SSRS_REQUIRE(!slope || sa_type == SSRS_F32 || sa_type == SSRS_F64, "%s: bad slope / aspect element type", who);
    SSRS_REQUIRE(!(want_usable && !(threshold > 0.0)), "%s: usable requested without a positive threshold", who);
    const double h = params->height;
    const double *cf = params->coef;
    for (int j = 0; j < 7; ++j) SSRS_REQUIRE(std::isfinite(cf[j]), "%s: coefficient %d is not finite", who, j);
    SSRS_REQUIRE(h >= 0.0 && std::isfinite(h), "%s: height must be >= 0 (got %g)", who, h);
    SSRS_REQUIRE(cf[3] > 0.0, "%s: coefficient d must be > 0 (got %g)", who, cf[3]);
    const double poly = cf[0] * h * h + cf[1] * h + cf[2];
    const double fh0 = poly * pow(cf[3], cf[4]) + cf[5], fh1 = poly * pow(cf[3], cf[4] - 1.0) + cf[5];
    SSRS_REQUIRE(fh0 > 0.0 && fh1 > 0.0 && std::isfinite(fh0) && std::isfinite(fh1),
                 "%s: these coefficients allow F_h <= 0 (F_h = %g on flat ground, %g on a vertical face)", who, fh1, fh0);
    a.wspeed_r = wspeed;
    a.slope = slope;
    a.aspect = aspect;
    a.sa_f64 = sa_type == SSRS_F64;
    a.d = 8 * res;
    a.d2 = a.d * a.d;
    a.min_val = min_updraft_val;
    a.thr = threshold;
    a.inv_thr = threshold > 0.0 ? 1.0 / threshold : 0.0;
    a.scale = threshold > 0.0 ? threshold / (exp(1.0) - 1.0) : 0.0;
    a.em1 = exp(1.0) - 1.0;
    a.poly = poly;
    a.ln_d = log(cf[3]);
    a.ce = cf[4];
    a.cf = cf[5];
    a.cg = cf[6];
    return SSRS_OK;
}

// H and M of a sector of half-width W in steps of S degrees; refused before anything else is looked at
static int sector_rays(const char *who, double W, double S, int &H, int &M)
{
    SSRS_REQUIRE(std::isfinite(W) && W >= 0.0 && W <= 90.0,
                 "%s: sector_half_width = %g: expected degrees in [0, 90]", who, W);
    SSRS_REQUIRE(std::isfinite(S) && S > 0.0, "%s: sector_step = %g: expected degrees > 0", who, S);
    const double h = floor(W / S + 1e-9);
    SSRS_REQUIRE(2.0 * h + 1.0 <= kMaxSectorM, "%s: a sector of +-%g degrees in steps of %g takes M = %.0f rays, more than %d",
                 who, W, S, 2.0 * h + 1.0, kMaxSectorM);
    H = static_cast<int>(h);
    M = 2 * H + 1;
    return SSRS_OK;
}

// The checks of a sector call beyond shelter_common's: every one of the batch x M ray steps, and a forced LDS path
// (`path` as shelter_path gives it)
static int sector_common(const ShelterArgs &a, const char *who, const double *ray_ur, const double *ray_uc, int path,
                         int batch)
{
    const int M = a.M;
    SSRS_REQUIRE(static_cast<long long>(M) * a.K < (1ll << 31), "%s: M K = %d x %d samples per cell exceed 2^31 - 1", who, M, a.K);
    int halo[4];
    for (int j = 0; ray_ur && j < batch; ++j) {
        for (int m = 0; m < M; ++m) {
            const double u = ray_ur[j * M + m], w = ray_uc[j * M + m];
            SSRS_REQUIRE(std::isfinite(u) && std::isfinite(w) && fabs(u) <= 1.0 && fabs(w) <= 1.0,
                         "%s: ray step %d of case %d = (%g, %g) is not a unit step", who, m, j, u, w);
        }
        SSRS_REQUIRE(path != SSRS_SHELTER_LDS || sector_halo(ray_ur + j * M, ray_uc + j * M, M, a.K, halo),
                     "%s: the halo of K = %d samples over the sector of case %d does not fit the LDS tile", who, a.K, j);
    }
    SSRS_REQUIRE(ray_ur || path != SSRS_SHELTER_LDS || shelter_tile_doubles(false, a.K) > 0,
                 "%s: the halo of K = %d samples does not fit the LDS tile", who, a.K);
    return SSRS_OK;
}

}  // namespace ssrs

using namespace ssrs;

extern "C" int ssrs_shelter_sx(const void *dem, int dem_type, double res, const double *ray_ur, const double *ray_uc,
                               const double *wdirn, double dmax, int ray_axes, int path, double *tan_sx,
                               double *sx_deg, int rows, int cols, int batch, void *stream)
{
    const char *who = "ssrs_shelter_sx";
    ShelterArgs a = {};
    if (int rc = shelter_common(a, who, dem, dem_type, res, ray_ur, ray_uc, wdirn, dmax, ray_axes, path, rows, cols,
                                batch, 2))
        return rc;
    if (!tan_sx && !sx_deg) return SSRS_OK;
    a.M = 1;
    a.tan_sx = tan_sx;
    a.sx_deg = sx_deg;
    return shelter_run(a, who, dem_type, ray_ur, ray_uc, nullptr, nullptr, false, shelter_path(path), batch,
                       as_stream(stream));
}

extern "C" int ssrs_updraft_sheltered(const void *dem, int dem_type, double res, const double *ray_ur,
                                      const double *ray_uc, const double *wspeed0, const double *wdirn0,
                                      const double *wspeed, const double *wdirn, const void *slope,
                                      const void *aspect, int sa_type, const SsrsShelterParams *params,
                                      double min_updraft_val, double threshold, float *orograph, double *usable,
                                      double *sx_deg, int rows, int cols, int batch, void *stream)
{
    const char *who = "ssrs_updraft_sheltered";
    ShelterArgs a = {};
    if (int rc = sheltered_common(a, who, dem, dem_type, res, ray_ur, ray_uc, wspeed0, wdirn0, wspeed, wdirn, slope,
                                  aspect, sa_type, params, min_updraft_val, threshold, usable != nullptr, rows, cols,
                                  batch))
        return rc;
    if (!orograph && !usable && !sx_deg) return SSRS_OK;
    a.M = 1;
    a.want_updraft = orograph || usable;
    a.orograph = orograph;
    a.usable = usable;
    a.sx_deg = sx_deg;
    return shelter_run(a, who, dem_type, ray_ur, ray_uc, wspeed0, wdirn0, false, shelter_path(params->path),
                       batch, as_stream(stream));
}

extern "C" int ssrs_shelter_sx_sector(const void *dem, int dem_type, double res, const double *ray_ur,
                                      const double *ray_uc, const double *wdirn, double dmax, int ray_axes, int path,
                                      double sector_half_width, double sector_step, double *tan_sx, double *sx_deg,
                                      int rows, int cols, int batch, void *stream)
{
    const char *who = "ssrs_shelter_sx_sector";
    ShelterArgs a = {};
    if (int rc = sector_rays(who, sector_half_width, sector_step, a.H, a.M)) return rc;
    if (int rc = shelter_common(a, who, dem, dem_type, res, ray_ur, ray_uc, wdirn, dmax, ray_axes, path, rows, cols,
                                batch, 2))
        return rc;
    path = shelter_path(path);
    if (int rc = sector_common(a, who, ray_ur, ray_uc, path, batch)) return rc;
    if (!tan_sx && !sx_deg) return SSRS_OK;
    a.step = sector_step;
    a.tan_sx = tan_sx;
    a.sx_deg = sx_deg;
    return shelter_run(a, who, dem_type, ray_ur, ray_uc, nullptr, nullptr, true, path, batch, as_stream(stream));
}

extern "C" int ssrs_updraft_sheltered_sector(const void *dem, int dem_type, double res, const double *ray_ur,
                                             const double *ray_uc, const double *wspeed0, const double *wdirn0,
                                             const double *wspeed, const double *wdirn, const void *slope,
                                             const void *aspect, int sa_type, const SsrsShelterParams *params,
                                             double sector_half_width, double sector_step, double min_updraft_val,
                                             double threshold, float *orograph, double *usable, double *sx_deg,
                                             int rows, int cols, int batch, void *stream)
{
    const char *who = "ssrs_updraft_sheltered_sector";
    ShelterArgs a = {};
    if (int rc = sector_rays(who, sector_half_width, sector_step, a.H, a.M)) return rc;
    if (int rc = sheltered_common(a, who, dem, dem_type, res, ray_ur, ray_uc, wspeed0, wdirn0, wspeed, wdirn, slope,
                                  aspect, sa_type, params, min_updraft_val, threshold, usable != nullptr, rows, cols,
                                  batch))
        return rc;
    const int path = shelter_path(params->path);
    if (int rc = sector_common(a, who, ray_ur, ray_uc, path, batch)) return rc;
    if (!orograph && !usable && !sx_deg) return SSRS_OK;
    a.want_updraft = orograph || usable;
    a.step = sector_step;
    a.orograph = orograph;
    a.usable = usable;
    a.sx_deg = sx_deg;
    return shelter_run(a, who, dem_type, ray_ur, ray_uc, wspeed0, wdirn0, true, path, batch, as_stream(stream));
}
