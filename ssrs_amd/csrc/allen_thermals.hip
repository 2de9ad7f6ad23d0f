// K12 -- Allen's (2006) field of discrete thermal updrafts for gfx950 (MI355X): the model the reference carries
// commented out at ssrs/layers.py:304-493, restated in include/ssrs_hip.h and DESIGN.md (K12).  Every cell takes the
// updraft nearest to it (smallest d2, the lowest index among equals) and evaluates that updraft's rotated-trapezoid
// profile, its downdraft ring and the environment sink, all in f64 with every operation rounded.
//
// k_allen_table, one thread per updraft: the per-updraft table (r2, r1r2, r1, wbar, wpeak, shape row).
// k_allen_field, one cell per thread, a block of 256 = a tile of 16 x 16 cells:
//   LDS path     the block stages (xt, yt, index) of the bins that meet its tile, plus a halo of one bin, once; every lane
//                scans that list (all lanes read the same address: a broadcast, no bank conflict).  A lane accepts its
//                nearest when it is strictly nearer than every side of the staged region that is not the domain's edge;
//                otherwise it goes on with the ring scan below, keeping what it found.  A tile whose list exceeds
//                kAllenLdsCap entries scans no list at all.
//   global path  the cell's own bin, then ring after ring of bins, until the best d2 is strictly below the square of the
//                distance to the nearest side of the scanned square (sides on the domain's edge do not count).
// "Nearer" is decided on (d2, index) lexicographically, so the order in which candidates are met does not matter and
// both paths return the same bits.  The distance to a side is shortened by kAllenMargin bins before it is squared: that
// covers the rounding of the side's coordinate, of the updraft's bin and of d2 itself.
#include <cmath>

#include "common.h"

namespace ssrs {

constexpr int kAllenTile = 16;                                // cells along each side of a block's tile
constexpr int kAllenHalo = 1;                                 // bins staged around the bins of the tile
constexpr int kAllenLdsCap = 512;                             // staged updrafts per tile: 10 KB of LDS
constexpr int kAllenMaxBinRows = 2 * kAllenHalo + kAllenTile + 2;   // bin rows a tile can meet (a bin >= one cell), and one
constexpr int kAllenMaxBins = 1 << 15;                        // bins along one axis
constexpr double kAllenMargin = 1.0 / (1 << 20);              // of a bin's side
constexpr int kAllenTableCols = SSRS_ALLEN_TABLE_COLS;
constexpr size_t kAllenHeadBytes = 256;                       // workspace: counters, then the table
static_assert(kAllenTile * kAllenTile == kBlock, "k_allen_field thread map");

struct AllenArgs {
    const double *xt, *yt;
    const int *bin_start, *bin_items;
    const double *table;
    int n, nbx, nby, rows, cols;
    double bin, res, zzi, we;
    int below;                                                // z < zi
    int use_lds;
    void *out;
    int out_f32;
    int *nearest;
    unsigned long long *left;                                 // cells that finished on the global path
};

// the smaller of two candidates: by d2, then by index
__device__ __forceinline__ void allen_take(double d2, int idx, double &best, int &besti)
{
    if (d2 < best || (d2 == best && idx < besti)) {
        best = d2;
        besti = idx;
    }
}

__device__ __forceinline__ double allen_d2(double xc, double yc, double x, double y)
{
    const double dx = xc - x, dy = yc - y;
    return dx * dx + dy * dy;
}

// bin of a coordinate >= 0 along an axis of nb bins: floor(v / bin), clamped to the last
__device__ __forceinline__ int allen_bin(double v, double bin, int nb)
{
    const double q = floor(v / bin);
    return q < static_cast<double>(nb - 1) ? (q > 0.0 ? static_cast<int>(q) : 0) : nb - 1;
}

// May a cell at (xc, yc) stop once every bin of [bx0, bx1] x [by0, by1] (clipped to the domain) has been scanned?
// Yes when no bin is left, or when `best` is strictly below the square of the shortened distance to the nearest side
// that has bins beyond it.
__device__ __forceinline__ bool allen_settled(const AllenArgs &a, double xc, double yc, int bx0, int bx1, int by0, int by1,
                                              double best)
{
    double m = INFINITY;
    if (bx0 > 0) m = fmin(m, xc - static_cast<double>(bx0) * a.bin);
    if (bx1 < a.nbx - 1) m = fmin(m, static_cast<double>(bx1 + 1) * a.bin - xc);
    if (by0 > 0) m = fmin(m, yc - static_cast<double>(by0) * a.bin);
    if (by1 < a.nby - 1) m = fmin(m, static_cast<double>(by1 + 1) * a.bin - yc);
    if (m == INFINITY) return true;
    const double ms = m - kAllenMargin * a.bin;
    return ms > 0.0 && best < ms * ms;
}

__device__ __forceinline__ void allen_scan_items(const AllenArgs &a, int first, int last, double xc, double yc,
                                                 double &best, int &besti)
{
    for (int j = first; j < last; ++j) {
        const int idx = a.bin_items[j];
        if (static_cast<unsigned>(idx) >= static_cast<unsigned>(a.n)) continue;
        allen_take(allen_d2(xc, yc, a.xt[idx], a.yt[idx]), idx, best, besti);
    }
}

// the ring scan; (best, besti) may already hold the nearest of any set of updrafts
__device__ void allen_scan_global(const AllenArgs &a, double xc, double yc, double &best, int &besti)
{
    const int cbx = allen_bin(xc, a.bin, a.nbx), cby = allen_bin(yc, a.bin, a.nby);
    for (int k = 0;; ++k) {
        const int x0 = cbx - k, x1 = cbx + k, y0 = cby - k, y1 = cby + k;
        const int cx0 = x0 > 0 ? x0 : 0, cx1 = x1 < a.nbx - 1 ? x1 : a.nbx - 1;
        const int cy0 = y0 > 0 ? y0 : 0, cy1 = y1 < a.nby - 1 ? y1 : a.nby - 1;
        for (int y = cy0; y <= cy1; ++y) {
            const size_t row = static_cast<size_t>(y) * a.nbx;
            if (y == y0 || y == y1) {                         // the ring's bottom and top rows: one run of the CSR
                allen_scan_items(a, a.bin_start[row + cx0], a.bin_start[row + cx1 + 1], xc, yc, best, besti);
            } else {                                          // its two columns
                if (x0 >= 0) allen_scan_items(a, a.bin_start[row + x0], a.bin_start[row + x0 + 1], xc, yc, best, besti);
                if (x1 <= a.nbx - 1)
                    allen_scan_items(a, a.bin_start[row + x1], a.bin_start[row + x1 + 1], xc, yc, best, besti);
            }
        }
        if (allen_settled(a, xc, yc, cx0, cx1, cy0, cy1, best)) return;
    }
}

// the seven shapes of the updraft (Allen 2006, table 1; the fifth column of the reference's table is unused)
__device__ __forceinline__ void allen_shape(int row, double &k1, double &k2, double &k3, double &k4)
{
    switch (row) {
    case 0: k1 = 1.5352; k2 = 2.5826; k3 = -0.0113; k4 = -0.1950; break;
    case 1: k1 = 1.5265; k2 = 3.6054; k3 = -0.0176; k4 = -0.1265; break;
    case 2: k1 = 1.4866; k2 = 4.8356; k3 = -0.0320; k4 = -0.0818; break;
    case 3: k1 = 1.2042; k2 = 7.7904; k3 = 0.0848; k4 = -0.0445; break;
    case 4: k1 = 0.8816; k2 = 13.9720; k3 = 0.3404; k4 = -0.0216; break;
    case 5: k1 = 0.7067; k2 = 23.9940; k3 = 0.5689; k4 = -0.0099; break;
    default: k1 = 0.6189; k2 = 42.7965; k3 = 0.7157; k4 = -0.0033; break;
    }
}

// vertical velocity at squared distance d2 from updraft u
__device__ __forceinline__ double allen_velocity(const AllenArgs &a, double d2, int u)
{
    constexpr double pi = 3.141592653589793;
    const double *t = a.table + static_cast<size_t>(u) * kAllenTableCols;
    const double r2 = t[0], r1 = t[2], wbar = t[3], wpeak = t[4];
    double k1, k2, k3, k4;
    allen_shape(static_cast<int>(t[5]), k1, k2, k3, k4);
    const double dist = sqrt(d2), rr2 = dist / r2;
    double ws = 0.0;
    if (a.below) {
        ws = 1.0 / (1.0 + pow(k1 * fabs(rr2 + k3), k2)) + k4 * rr2;
        ws = ws > 0.0 ? ws : 0.0;
    }
    const double wl = (dist > r1 && rr2 < 2.0) ? (pi / 6.0) * sin(pi * rr2) : 0.0;
    double wd = 0.0;
    if (0.5 < a.zzi && a.zzi <= 0.9) {
        wd = 2.5 * wl * (a.zzi - 0.5);
        wd = wd < 0.0 ? wd : 0.0;
    }
    double w = wpeak * ws + wd * wbar;
    if (a.we != 0.0 && dist > r1) w = wpeak != 0.0 ? w * (1.0 - a.we / wpeak) + a.we : a.we;
    return w;
}

__global__ __launch_bounds__(kBlock) void k_allen_table(const double *__restrict__ wgain, const double *__restrict__ rgain,
                                                        int n, double rbar, double wtbar, double *__restrict__ table,
                                                        double *__restrict__ copy, unsigned long long *__restrict__ head)
{
    const size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x;
    if (i == 0) head[0] = 0ull;                               // the count of cells that leave the LDS path
    if (i >= static_cast<size_t>(n)) return;
    const double S[7] = {0.14, 0.25, 0.36, 0.47, 0.58, 0.69, 0.80};
    const double rg = rbar * rgain[i];
    const double r2 = rg > 10.0 ? rg : 10.0;
    const double r1r2 = r2 < 600.0 ? 0.0011 * r2 + 0.14 : 0.8;
    const double r1 = r1r2 * r2;
    const double wbar = wtbar * wgain[i];
    const double wpeak = 3.0 * wbar * (r2 * r2 * r2 - r2 * r2 * r1) / (r2 * r2 * r2 - r1 * r1 * r1);
    int row = 6;
    for (int j = 5; j >= 0; --j)
        if (r1r2 < 0.5 * (S[j] + S[j + 1])) row = j;
    const double v[kAllenTableCols] = {r2, r1r2, r1, wbar, wpeak, static_cast<double>(row)};
    for (int c = 0; c < kAllenTableCols; ++c) {
        table[i * kAllenTableCols + c] = v[c];
        if (copy) copy[i * kAllenTableCols + c] = v[c];
    }
}

// the bins [bxl, bxh] x [byl, byh] a tile stages: those of its cells and the halo
__device__ __forceinline__ void allen_tile_bins(const AllenArgs &a, int tile, int tiles_x, int &bxl, int &bxh, int &byl,
                                                int &byh)
{
    const int r0 = (tile / tiles_x) * kAllenTile, c0 = (tile % tiles_x) * kAllenTile;
    const int r1 = r0 + kAllenTile - 1 < a.rows - 1 ? r0 + kAllenTile - 1 : a.rows - 1;
    const int c1 = c0 + kAllenTile - 1 < a.cols - 1 ? c0 + kAllenTile - 1 : a.cols - 1;
    bxl = allen_bin(static_cast<double>(c0) * a.res, a.bin, a.nbx) - kAllenHalo;
    bxh = allen_bin(static_cast<double>(c1) * a.res, a.bin, a.nbx) + kAllenHalo;
    byl = allen_bin(static_cast<double>(r0) * a.res, a.bin, a.nby) - kAllenHalo;
    byh = allen_bin(static_cast<double>(r1) * a.res, a.bin, a.nby) + kAllenHalo;
    bxl = bxl > 0 ? bxl : 0;
    byl = byl > 0 ? byl : 0;
    bxh = bxh < a.nbx - 1 ? bxh : a.nbx - 1;
    byh = byh < a.nby - 1 ? byh : a.nby - 1;
}

// the longest list any tile would stage (forced _LDS is refused on the host when it exceeds the capacity)
__global__ __launch_bounds__(kBlock) void k_allen_tile_max(AllenArgs a, int tiles_x, int ntiles, int *__restrict__ longest)
{
    const int tile = static_cast<int>(blockIdx.x * kBlock + threadIdx.x);
    if (tile >= ntiles) return;
    int bxl, bxh, byl, byh;
    allen_tile_bins(a, tile, tiles_x, bxl, bxh, byl, byh);
    long long total = 0;
    for (int y = byl; y <= byh; ++y) {
        const size_t row = static_cast<size_t>(y) * a.nbx;
        total += a.bin_start[row + bxh + 1] - a.bin_start[row + bxl];
    }
    atomicMax(longest, total > 0x7fffffff ? 0x7fffffff : static_cast<int>(total));
}

__global__ __launch_bounds__(kBlock) void k_allen_field(AllenArgs a, int tiles_x)
{
    __shared__ double s_x[kAllenLdsCap], s_y[kAllenLdsCap];
    __shared__ int s_i[kAllenLdsCap];
    __shared__ int s_first[kAllenMaxBinRows], s_count[kAllenMaxBinRows], s_off[kAllenMaxBinRows + 1];
    __shared__ unsigned s_left;
    const int tid = static_cast<int>(threadIdx.x);
    const int tile = static_cast<int>(blockIdx.x);
    const int r = (tile / tiles_x) * kAllenTile + tid / kAllenTile, c = (tile % tiles_x) * kAllenTile + tid % kAllenTile;
    const bool live = r < a.rows && c < a.cols;
    const double xc = static_cast<double>(c) * a.res, yc = static_cast<double>(r) * a.res;
    double best = INFINITY;
    int besti = 0x7fffffff;
    bool settled = false;
    if (tid == 0) s_left = 0u;

    if (a.use_lds) {                                          // (uniform over the grid)
        int bxl, bxh, byl, byh;
        allen_tile_bins(a, tile, tiles_x, bxl, bxh, byl, byh);
        const int span = byh - byl + 1;                       // <= kAllenMaxBinRows: a bin is no smaller than a cell
        const int nrow = span <= kAllenMaxBinRows ? span : 0;  // (were it not, the tile would take the global path)
        if (tid < nrow) {
            const size_t row = static_cast<size_t>(byl + tid) * a.nbx;
            const int first = a.bin_start[row + bxl], count = a.bin_start[row + bxh + 1] - first;
            s_first[tid] = first;
            s_count[tid] = count > 0 ? (count < kAllenLdsCap + 1 ? count : kAllenLdsCap + 1) : 0;
        }
        __syncthreads();
        if (tid == 0) {
            int off = 0;
            for (int y = 0; y < nrow; ++y) {
                s_off[y] = off;
                off += s_count[y];                            // (each <= cap + 1, at most 19 of them: no overflow)
            }
            s_off[nrow] = off;
        }
        __syncthreads();
        const int total = s_off[nrow];
        if (nrow > 0 && total <= kAllenLdsCap) {                          // (uniform over the block)
            for (int y = 0; y < nrow; ++y) {
                for (int j = tid; j < s_count[y]; j += kBlock) {
                    int idx = a.bin_items[s_first[y] + j];
                    const bool ok = static_cast<unsigned>(idx) < static_cast<unsigned>(a.n);
                    s_x[s_off[y] + j] = ok ? a.xt[idx] : INFINITY;       // (a stray index is nobody's nearest)
                    s_y[s_off[y] + j] = ok ? a.yt[idx] : INFINITY;
                    s_i[s_off[y] + j] = ok ? idx : 0x7fffffff;
                }
            }
            __syncthreads();
            if (live) {
                for (int j = 0; j < total; ++j) allen_take(allen_d2(xc, yc, s_x[j], s_y[j]), s_i[j], best, besti);
                settled = allen_settled(a, xc, yc, bxl, bxh, byl, byh, best);
            }
        }
    }
    if (live && !settled) {
        allen_scan_global(a, xc, yc, best, besti);
        if (a.use_lds) atomicAdd(&s_left, 1u);
    }
    if (live) {
        const size_t i = static_cast<size_t>(r) * a.cols + c;
        const bool found = besti != 0x7fffffff;               // (false only for lists that name no updraft at all)
        const double w = found ? allen_velocity(a, best, besti) : NAN;
        if (a.out_f32) static_cast<float *>(a.out)[i] = static_cast<float>(w);
        else static_cast<double *>(a.out)[i] = w;
        if (a.nearest) a.nearest[i] = found ? besti : -1;
    }
    __syncthreads();
    if (tid == 0 && s_left) atomicAdd(a.left, static_cast<unsigned long long>(s_left));
}

static size_t allen_table_bytes(int n) { return (static_cast<size_t>(n) * kAllenTableCols * 8 + 255) / 256 * 256; }

}  // namespace ssrs

using namespace ssrs;

extern "C" size_t ssrs_allen_workspace_bytes(int n_updrafts)
{
    if (n_updrafts < 1 || n_updrafts > SSRS_ALLEN_MAX_UPDRAFTS) return 0;
    return kAllenHeadBytes + allen_table_bytes(n_updrafts);
}

extern "C" int ssrs_allen_thermal_field(const double *xt, const double *yt, const double *wgain, const double *rgain,
                                        int n_updrafts, const int32_t *bin_start, const int32_t *bin_items,
                                        double bin_size_m, int nbx, int nby, double rbar, double wtbar, double zzi,
                                        int z_below_zi, double we, double res, int rows, int cols, int path, void *out,
                                        int out_type, int32_t *nearest, double *table, void *workspace,
                                        size_t workspace_bytes, void *stream)
{
    const char *who = "ssrs_allen_thermal_field";
    SSRS_REQUIRE(xt != nullptr, "%s: xt is NULL", who);
    SSRS_REQUIRE(yt != nullptr, "%s: yt is NULL", who);
    SSRS_REQUIRE(wgain != nullptr, "%s: wgain is NULL", who);
    SSRS_REQUIRE(rgain != nullptr, "%s: rgain is NULL", who);
    SSRS_REQUIRE(n_updrafts >= 1, "%s: n_updrafts = %d: expected at least 1", who, n_updrafts);
    SSRS_REQUIRE(n_updrafts <= SSRS_ALLEN_MAX_UPDRAFTS, "%s: n_updrafts = %d: expected at most %d", who, n_updrafts,
                 SSRS_ALLEN_MAX_UPDRAFTS);
    SSRS_REQUIRE(bin_start != nullptr, "%s: bin_start is NULL", who);
    SSRS_REQUIRE(bin_items != nullptr, "%s: bin_items is NULL", who);
    SSRS_REQUIRE(rows >= 1 && cols >= 1, "%s: need rows, cols >= 1 (got %d x %d)", who, rows, cols);
    const int tiles_x = (cols + kAllenTile - 1) / kAllenTile, tiles_y = (rows + kAllenTile - 1) / kAllenTile;
    const long long ntiles = static_cast<long long>(tiles_x) * tiles_y;
    SSRS_REQUIRE(ntiles < (1ll << 31), "%s: rows x cols = %d x %d: raster too large", who, rows, cols);
    SSRS_REQUIRE(std::isfinite(res) && res > 0.0, "%s: res = %g: expected metres > 0", who, res);
    SSRS_REQUIRE(std::isfinite(bin_size_m) && bin_size_m >= res, "%s: bin_size_m = %g: expected at least one cell (res = %g)",
                 who, bin_size_m, res);
    SSRS_REQUIRE(nbx >= 1 && nbx <= kAllenMaxBins, "%s: nbx = %d: expected 1 to %d", who, nbx, kAllenMaxBins);
    SSRS_REQUIRE(nby >= 1 && nby <= kAllenMaxBins, "%s: nby = %d: expected 1 to %d", who, nby, kAllenMaxBins);
    SSRS_REQUIRE(std::isfinite(rbar), "%s: rbar is not finite", who);
    SSRS_REQUIRE(std::isfinite(wtbar), "%s: wtbar is not finite", who);
    SSRS_REQUIRE(std::isfinite(zzi) && zzi > 0.0, "%s: zzi = %g: expected z / zi > 0", who, zzi);
    SSRS_REQUIRE(std::isfinite(we) && we <= 0.0, "%s: we = %g: expected a sink <= 0", who, we);
    SSRS_REQUIRE(path == SSRS_ALLEN_AUTO || path == SSRS_ALLEN_LDS || path == SSRS_ALLEN_GLOBAL, "%s: bad path %d", who, path);
    SSRS_REQUIRE(out != nullptr, "%s: out is NULL", who);
    SSRS_REQUIRE(out_type == SSRS_F32 || out_type == SSRS_F64, "%s: bad out_type %d", who, out_type);
    SSRS_REQUIRE(workspace != nullptr && workspace_bytes >= ssrs_allen_workspace_bytes(n_updrafts),
                 "%s: workspace too small (%zu bytes, need %zu)", who, workspace ? workspace_bytes : static_cast<size_t>(0),
                 ssrs_allen_workspace_bytes(n_updrafts));

    hipStream_t st = as_stream(stream);
    unsigned long long *head = static_cast<unsigned long long *>(workspace);
    double *d_table = reinterpret_cast<double *>(static_cast<char *>(workspace) + kAllenHeadBytes);
    hipLaunchKernelGGL(k_allen_table, dim3(static_cast<unsigned>((n_updrafts + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       wgain, rgain, n_updrafts, rbar, wtbar, d_table, table, head);
    SSRS_HIP_CHECK(hipGetLastError());

    AllenArgs a = {};
    a.xt = xt;
    a.yt = yt;
    a.bin_start = bin_start;
    a.bin_items = bin_items;
    a.table = d_table;
    a.n = n_updrafts;
    a.nbx = nbx;
    a.nby = nby;
    a.rows = rows;
    a.cols = cols;
    a.bin = bin_size_m;
    a.res = res;
    a.zzi = zzi;
    a.we = we;
    a.below = z_below_zi != 0;
    a.use_lds = path != SSRS_ALLEN_GLOBAL;
    a.out = out;
    a.out_f32 = out_type == SSRS_F32;
    a.nearest = nearest;
    a.left = head;
    if (path == SSRS_ALLEN_LDS) {
        // the one synchronising step, on the forced (A/B) path only: the longest list of any tile comes to the host
        int *d_longest = reinterpret_cast<int *>(head + 1), longest = 0;
        SSRS_HIP_CHECK(hipMemsetAsync(d_longest, 0, sizeof(int), st));
        hipLaunchKernelGGL(k_allen_tile_max, dim3(static_cast<unsigned>((ntiles + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                           a, tiles_x, static_cast<int>(ntiles), d_longest);
        SSRS_HIP_CHECK(hipGetLastError());
        SSRS_HIP_CHECK(hipMemcpyAsync(&longest, d_longest, sizeof(int), hipMemcpyDeviceToHost, st));
        SSRS_HIP_CHECK(hipStreamSynchronize(st));
        SSRS_REQUIRE(longest <= kAllenLdsCap, "%s: a tile's list of %d updrafts does not fit the LDS (at most %d)", who, longest,
                     kAllenLdsCap);
    }
    hipLaunchKernelGGL(k_allen_field, dim3(static_cast<unsigned>(ntiles)), dim3(kBlock), 0, st, a, tiles_x);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}
