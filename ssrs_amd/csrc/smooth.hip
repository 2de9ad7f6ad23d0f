// K11 -- Gaussian smoothing of the improved orographic updraft for gfx950 (MI355X): scipy's gaussian_filter with
// mode='reflect' on an f32 raster, f64 inside, the clamp and the threshold function fused into the second pass.  The
// arithmetic is stated in include/ssrs_hip.h and DESIGN.md (K11).
//
// Two passes, axis 0 (f32 -> f64 plane in the workspace) and axis 1 (f64 plane -> outputs).  A pass reads 2 R + 1 values
// per cell, so a block stages its tile and the halo of R cells along the pass's axis in LDS once, REFLECTED as it is
// staged: the inner loop then reads consecutive LDS positions and carries no index arithmetic.  The tile is kSmLines = 32
// lines (the axis the pass does not blur) by kSmSpan = 128 positions along the blur axis; thread (line, group) of the
// 256 owns kSmP = 16 consecutive positions of its line and keeps the two windows x[p - k], x[p + k] of its 16 sums in
// registers: stepping k down by one shifts each window by one position, i.e. two LDS reads per k serve 16 sums
// (1 / 8 read per cell and k against 2 at one output per thread).  The k loop is unrolled by 16 with the windows
// rotating through their registers, so the shift costs no moves; R mod 16 leading steps shift by moves.
//   axis 0  LDS [position][line] f32: the lanes of a half-wave read 32 consecutive floats -- one bank each
//   axis 1  LDS [position][line] f64 with a line stride of 33: the tile is transposed as it is staged (a store of 16 lanes
//           walks 16 positions = a stride of 66 dwords, 16 distinct bank pairs), reads as above; the sums go back through
//           LDS [line][position], stride 129, so that the stores to HBM run along the columns
// Two LDS capacities, picked by R on the host, so that a small radius keeps its occupancy: R <= 32 (sigma 8, the 10 m
// contract case at h = 80 m; 24 KB and 50 KB per block) and R <= 128 (sigma 30, the model's cap; 48 KB and 99 KB).
// A larger R reads global memory through the reflect rule, one cell per thread: the same operations in the same order
// on the same values, hence the same bits.  The order of a cell's sum is k = R .. 1 on every path.
// The weights travel as kernel arguments into the workspace (256 per launch): no copy, no synchronisation.
#include <cmath>
#include <type_traits>

#include "common.h"
#include "gauss.h"
#include "raster_math.h"

namespace ssrs {

constexpr int kSmLines = 32, kSmSpan = 128, kSmP = 16;
constexpr int kSmGroups = kSmSpan / kSmP;                    // 8 groups of 32 lines: 256 threads
constexpr int kSmMaxRadius = 512, kSmLdsRadius = 128, kSmSmallRadius = 32;
constexpr int kSmWeightChunk = 256;
static_assert(kSmLines * kSmGroups == kBlock && kSmLines == 32, "k_smooth_lds thread map");

struct SmoothOut {
    double *smooth, *usable;
    float *orograph;
    double min_val, thr, inv_thr, scale;                     // as FusedArgs of K1
};

struct SmoothWeights { double w[kSmWeightChunk]; };

__global__ __launch_bounds__(kBlock) void k_smooth_weights(SmoothWeights chunk, double *__restrict__ dst, int n)
{
    const int t = static_cast<int>(threadIdx.x);
    if (t < n) dst[t] = chunk.w[t];
}

// index of the 'reflect' extension of [0, n): d c b a | a b c d | d c b a, to any depth
__device__ __forceinline__ int reflect_index(long long i, int n)
{
    if (i < 0 || i >= n) {
        const long long period = 2ll * n;
        long long m = i % period;
        if (m < 0) m += period;
        i = m < n ? m : period - 1 - m;
    }
    return static_cast<int>(i);
}

__device__ __forceinline__ float finite_or_zero(float v) { return __builtin_isfinite(v) ? v : 0.0f; }
__device__ __forceinline__ double finite_or_zero(double v) { return v; }     // (the f64 plane is the first pass's own)

// the second pass's epilogue for cell i
__device__ __forceinline__ void smooth_store(const SmoothOut &o, size_t i, double v)
{
    if (o.smooth) o.smooth[i] = v;
    const float w32 = static_cast<float>(v > o.min_val ? v : o.min_val);
    if (o.orograph) o.orograph[i] = w32;
    if (o.usable) o.usable[i] = usable_updraft_fast(static_cast<double>(w32), o.thr, o.inv_thr, o.scale);
}

// kSmP sums of one line: s[d * stride] is the value at position p0 + d of the line, readable for d in [-R, kSmP - 1 + R];
// w[k] the weight of +-k.  acc[j] = x[p0+j] w[0], then k = R .. 1: acc[j] = acc[j] + (x[p0+j-k] + x[p0+j+k]) w[k].
template <typename TS>
__device__ __forceinline__ void smooth_sums(const TS *s, int stride, int R, const double *__restrict__ w,
                                            double (&acc)[kSmP])
{
    constexpr int P = kSmP;
    double lo[P], hi[P];                                      // x[p0 + j - k], x[p0 + j + k] of the current k
    const double w0 = w[0];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        acc[j] = static_cast<double>(s[j * stride]) * w0;
        lo[j] = static_cast<double>(s[(j - R) * stride]);
        hi[j] = static_cast<double>(s[(j + R) * stride]);
    }
    int k = R;
    for (; k % P != 0; --k) {                                 // R mod P leading steps: the windows shift by moves
        const double wk = w[k];
#pragma unroll
        for (int j = 0; j < P; ++j) acc[j] = acc[j] + (lo[j] + hi[j]) * wk;
#pragma unroll
        for (int j = 0; j < P - 1; ++j) lo[j] = lo[j + 1];
#pragma unroll
        for (int j = P - 1; j > 0; --j) hi[j] = hi[j - 1];
        lo[P - 1] = static_cast<double>(s[(P - k) * stride]);
        hi[0] = static_cast<double>(s[(k - 1) * stride]);
    }
    for (; k >= P; k -= P) {                                  // P steps at a time: the windows rotate in place
#pragma unroll
        for (int q = 0; q < P; ++q) {                         // lo[j] lives in lo[(j + q) % P], hi[j] in hi[(j - q) % P]
            const int kk = k - q;
            const double wk = w[kk];
#pragma unroll
            for (int j = 0; j < P; ++j) acc[j] = acc[j] + (lo[(j + q) % P] + hi[(j - q + P) % P]) * wk;
            lo[q] = static_cast<double>(s[(P - kk) * stride]);
            hi[P - 1 - q] = static_cast<double>(s[(kk - 1) * stride]);
        }
    }
}

// One pass on LDS.  AXIS 0: in f32 (rows, cols), blur along the rows, out -> mid f64.  AXIS 1: in f64, blur along the
// columns, out -> the epilogue.  RMAX: the halo the LDS of this instantiation holds (host: R <= RMAX).
template <int AXIS, int RMAX>
__global__ __launch_bounds__(kBlock) void k_smooth_lds(const void *__restrict__ in_, const double *__restrict__ w,
                                                       int R, int rows, int cols, int tiles_l,
                                                       double *__restrict__ mid, SmoothOut out, size_t out_base)
{
    using TS = typename std::conditional<AXIS == 0, float, double>::type;
    constexpr int LS = AXIS == 0 ? kSmLines : kSmLines + 1;   // stride between positions
    constexpr int OS = kSmSpan + 1;                           // AXIS 1: stride between the lines of the sums
    static_assert(kSmLines * OS <= (kSmSpan + 2 * RMAX) * LS, "the sums reuse the staged tile");
    __shared__ TS s_x[(kSmSpan + 2 * RMAX) * LS];
    const TS *__restrict__ in = static_cast<const TS *>(in_);
    const int tid = static_cast<int>(threadIdx.x);
    const int n_pos = AXIS == 0 ? rows : cols, n_line = AXIS == 0 ? cols : rows;
    const int tile = static_cast<int>(blockIdx.x);
    const int p_tile = (tile / tiles_l) * kSmSpan, l_tile = (tile % tiles_l) * kSmLines;
    const int span = n_pos - p_tile < kSmSpan ? n_pos - p_tile : kSmSpan;        // positions of the tile in the raster
    const int ext = span + 2 * R;                                               // staged positions: p_tile - R ..

    // ---- stage, reflecting the positions; a line beyond the raster holds zeros (its sums are not stored)
    if constexpr (AXIS == 0) {
        for (int i = tid; i < ext * kSmLines; i += kBlock) {
            const int a = i / kSmLines, l = i % kSmLines;
            float v = 0.0f;
            if (l_tile + l < n_line)
                v = finite_or_zero(in[static_cast<size_t>(reflect_index(static_cast<long long>(p_tile) - R + a, n_pos)) * cols + l_tile + l]);
            s_x[a * LS + l] = v;
        }
    } else {
        for (int l = tid / 64; l < kSmLines; l += kBlock / 64) {                 // a wave takes a line at a time
            const bool inside = l_tile + l < n_line;
            const size_t row = static_cast<size_t>(inside ? l_tile + l : 0) * cols;
            for (int a = tid % 64; a < ext; a += 64)
                s_x[a * LS + l] = inside ? in[row + reflect_index(static_cast<long long>(p_tile) - R + a, n_pos)] : 0.0;
        }
    }
    __syncthreads();

    // ---- kSmP sums per thread
    const int l = tid % kSmLines, p0 = (tid / kSmLines) * kSmP;
    const bool live = p0 < span;                                                 // (else nothing of this chunk is stored)
    double acc[kSmP];
    if (live) smooth_sums<TS>(s_x + (R + p0) * LS + l, LS, R, w, acc);

    if constexpr (AXIS == 0) {
        if (live && l_tile + l < n_line) {
#pragma unroll
            for (int j = 0; j < kSmP; ++j)
                if (p0 + j < span) mid[static_cast<size_t>(p_tile + p0 + j) * cols + l_tile + l] = acc[j];
        }
    } else {
        // ---- transpose the sums through LDS: the stores run along the columns
        double *s_o = reinterpret_cast<double *>(s_x);
        __syncthreads();                                                         // the staged tile is done with
        if (live) {
#pragma unroll
            for (int j = 0; j < kSmP; ++j) s_o[l * OS + p0 + j] = acc[j];
        }
        __syncthreads();
        for (int ll = tid / 64; ll < kSmLines; ll += kBlock / 64) {
            if (l_tile + ll >= n_line) break;
            const size_t row = out_base + static_cast<size_t>(l_tile + ll) * cols + p_tile;
            for (int a = tid % 64; a < span; a += 64) smooth_store(out, row + a, s_o[ll * OS + a]);
        }
    }
}

// One pass on global memory, one cell per thread: the same sum through the reflect rule.
template <int AXIS>
__global__ __launch_bounds__(kBlock) void k_smooth_global(const void *__restrict__ in_, const double *__restrict__ w,
                                                          int R, int rows, int cols, double *__restrict__ mid,
                                                          SmoothOut out, size_t out_base)
{
    using TS = typename std::conditional<AXIS == 0, float, double>::type;
    const TS *__restrict__ in = static_cast<const TS *>(in_);
    const size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x;
    if (i >= static_cast<size_t>(rows) * cols) return;
    const int r = static_cast<int>(i / cols), c = static_cast<int>(i - static_cast<size_t>(r) * cols);
    const int n = AXIS == 0 ? rows : cols, p = AXIS == 0 ? r : c;
    auto at = [&](long long q) {
        const int m = reflect_index(q, n);
        const size_t j = AXIS == 0 ? static_cast<size_t>(m) * cols + c : static_cast<size_t>(r) * cols + m;
        return static_cast<double>(finite_or_zero(in[j]));
    };
    double acc = at(p) * w[0];
    for (int k = R; k >= 1; --k) acc = acc + (at(static_cast<long long>(p) - k) + at(static_cast<long long>(p) + k)) * w[k];
    if (AXIS == 0) mid[i] = acc;
    else smooth_store(out, out_base + i, acc);
}

static size_t smooth_weight_bytes(int R) { return (static_cast<size_t>(R + 1) * 8 + 255) / 256 * 256; }

template <int AXIS>
static void smooth_pass(bool lds, int R, const void *in, const double *w, int rows, int cols, double *mid,
                        const SmoothOut &out, size_t out_base, hipStream_t st)
{
    if (!lds) {
        const size_t n = static_cast<size_t>(rows) * cols;
        hipLaunchKernelGGL((k_smooth_global<AXIS>), dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                           in, w, R, rows, cols, mid, out, out_base);
        return;
    }
    const int n_pos = AXIS == 0 ? rows : cols, n_line = AXIS == 0 ? cols : rows;
    const int tiles_l = (n_line + kSmLines - 1) / kSmLines;
    const dim3 grid(static_cast<unsigned>(static_cast<long long>(tiles_l) * ((n_pos + kSmSpan - 1) / kSmSpan)));
    if (R <= kSmSmallRadius)
        hipLaunchKernelGGL((k_smooth_lds<AXIS, kSmSmallRadius>), grid, dim3(kBlock), 0, st, in, w, R, rows, cols, tiles_l, mid,
                           out, out_base);
    else
        hipLaunchKernelGGL((k_smooth_lds<AXIS, kSmLdsRadius>), grid, dim3(kBlock), 0, st, in, w, R, rows, cols, tiles_l, mid,
                           out, out_base);
}

}  // namespace ssrs

using namespace ssrs;

extern "C" size_t ssrs_smooth_workspace_bytes(int rows, int cols, int batch, double sigma)
{
    if (rows < 1 || cols < 1 || batch < 1 || !(sigma > 0.0) || !(4.0 * sigma + 0.5 < kSmMaxRadius + 1.0)) return 0;
    const int R = blur_radius(sigma);
    return smooth_weight_bytes(R) + static_cast<size_t>(rows) * cols * 8;
}

extern "C" int ssrs_smooth_reflect(const float *in, double sigma, int path, double min_updraft_val, double threshold,
                                   double *smooth, float *orograph, double *usable, int rows, int cols, int batch,
                                   void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "ssrs_smooth_reflect";
    SSRS_REQUIRE(rows >= 1 && cols >= 1 && batch >= 1, "%s: need rows, cols, batch >= 1 (got %d x %d, batch %d)", who, rows,
                 cols, batch);
    SSRS_REQUIRE(std::isfinite(sigma) && sigma > 0.0, "%s: sigma = %g: expected cells > 0", who, sigma);
    SSRS_REQUIRE(4.0 * sigma + 0.5 < kSmMaxRadius + 1.0, "%s: sigma = %g cells takes a radius R = int(4 sigma + 0.5) of more than %d",
                 who, sigma, kSmMaxRadius);
    const int R = blur_radius(sigma);
    SSRS_REQUIRE(path == SSRS_SMOOTH_AUTO || path == SSRS_SMOOTH_LDS || path == SSRS_SMOOTH_GLOBAL, "%s: bad path %d", who, path);
    SSRS_REQUIRE(!(path == SSRS_SMOOTH_LDS && R > kSmLdsRadius), "%s: the halo of R = %d cells does not fit the LDS tile (R <= %d)",
                 who, R, kSmLdsRadius);
    SSRS_REQUIRE(smooth || orograph || usable, "%s: smooth, orograph and usable are all NULL", who);
    SSRS_REQUIRE(min_updraft_val == min_updraft_val, "%s: min_updraft_val is NaN", who);
    SSRS_REQUIRE(!(usable && !(threshold > 0.0)), "%s: usable requested without a positive threshold", who);
    SSRS_REQUIRE(in != nullptr, "%s: in is NULL", who);
    SSRS_REQUIRE(static_cast<long long>(rows) * cols < (1ll << 31) * kSmLines, "%s: raster too large", who);
    SSRS_REQUIRE(workspace != nullptr && workspace_bytes >= ssrs_smooth_workspace_bytes(rows, cols, batch, sigma),
                 "%s: workspace too small (%zu bytes, need %zu)", who, workspace ? workspace_bytes : static_cast<size_t>(0),
                 ssrs_smooth_workspace_bytes(rows, cols, batch, sigma));

    hipStream_t st = as_stream(stream);
    const std::vector<double> full = blur_weights(sigma, R);                     // full[R + k] = w[k]
    double *d_w = static_cast<double *>(workspace);
    double *mid = reinterpret_cast<double *>(static_cast<char *>(workspace) + smooth_weight_bytes(R));
    for (int k0 = 0; k0 <= R; k0 += kSmWeightChunk) {
        const int n = R + 1 - k0 < kSmWeightChunk ? R + 1 - k0 : kSmWeightChunk;
        SmoothWeights chunk = {};
        for (int k = 0; k < n; ++k) chunk.w[k] = full[R + k0 + k];
        hipLaunchKernelGGL(k_smooth_weights, dim3(1), dim3(kBlock), 0, st, chunk, d_w + k0, n);
    }
    SSRS_HIP_CHECK(hipGetLastError());

    SmoothOut out = {};
    out.smooth = smooth;
    out.orograph = orograph;
    out.usable = usable;
    out.min_val = min_updraft_val;
    out.thr = threshold;
    out.inv_thr = threshold > 0.0 ? 1.0 / threshold : 0.0;                       // as sheltered_common of K9
    out.scale = threshold > 0.0 ? threshold / (exp(1.0) - 1.0) : 0.0;
    const bool lds = path != SSRS_SMOOTH_GLOBAL && R <= kSmLdsRadius;
    const size_t ncell = static_cast<size_t>(rows) * cols;
    for (int b = 0; b < batch; ++b) {                                            // the cases share the one f64 plane
        smooth_pass<0>(lds, R, in + b * ncell, d_w, rows, cols, mid, out, 0, st);
        smooth_pass<1>(lds, R, mid, d_w, rows, cols, nullptr, out, b * ncell, st);
        SSRS_HIP_CHECK(hipGetLastError());
    }
    return SSRS_OK;
}
