// a5 -- random thermal updraft field for gfx950 (MI355X).
//
// Reference semantics (paths relative to /root/reference):
//   ssrs/layers.py:188-214  compute_thermals: inside a 10 % border, each cell
//       draws num1 = randint(1, int(wt)), wt = 1000 + |aspect-180|/180*2000, and
//       seeds a thermal lognormal(scale + 3, 0.5) when num1 == 5; the seed field
//       is blurred with scipy.ndimage.gaussian_filter(sigma=4, mode='constant').
//   ssrs/simulator.py:217-228 one field per realisation, saved as f32.
//
// The reference consumes the serial global MT19937 in a python double loop
// (1-2 draws per cell in row-major order), which no parallel code can replay;
// only STATISTICAL parity is possible.  Here every
// cell owns a Philox4x32-10 block keyed by (seed, cell index): word 0 decides
// the seeding with the reference's probability 1/(int(wt)-1), words 1-3 feed a
// Box-Muller normal for the lognormal amplitude.  The blur is the same
// separable, zero-padded, 4-sigma-truncated Gaussian as scipy's.
#include <rocrand/rocrand_philox4x32_10.h>

#include <cmath>
#include <vector>

#include "common.h"
#include "gauss.h"          // blur_radius, blur_weights

namespace ssrs {

// the seed of interior cell i = r * cols + c (0 when no thermal starts there)
__device__ __forceinline__ double thermal_seed_value(double aspect_i, double mu, double sigma,
                                                     unsigned long long seed, size_t i)
{
    rocrand_state_philox4x32_10 st;
    rocrand_init(seed, i, 0, &st);
    const uint4 w = rocrand4(&st);
    const double wt = 1000.0 + (fabs(aspect_i - 180.0) / 180.0) * 2000.0;
    const int nvals = static_cast<int>(wt) - 1;         // randint(1, int(wt)): nvals values
    // P(num1 == 5) = 1 / nvals (nvals >= 5 always: wt >= 1000)
    const double u0 = static_cast<double>(w.x) * (1.0 / 4294967296.0);
    double v = 0.0;
    if (u0 * nvals < 1.0) {
        const double u1 = (static_cast<double>(w.y) + 1.0) * (1.0 / 4294967296.0);  // (0,1]
        const double u2 = static_cast<double>(w.z) * (1.0 / 4294967296.0);
        const double z = sqrt(-2.0 * log(u1)) * cos(2.0 * 3.141592653589793 * u2);
        v = exp(mu + sigma * z);
    }
    return v;
}

__global__ __launch_bounds__(kBlock) void k_thermal_seeds(const double *__restrict__ aspect,
                                                         double mu, double sigma,
                                                         unsigned long long seed,
                                                         double *__restrict__ out, int rows,
                                                         int cols)
{
    const size_t n = static_cast<size_t>(rows) * cols;
    const int by = static_cast<int>(0.1 * rows), bx = static_cast<int>(0.1 * cols);
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < n;
         i += static_cast<size_t>(gridDim.x) * kBlock) {
        const int r = static_cast<int>(i / cols), c = static_cast<int>(i % cols);
        double v = 0.0;
        if (r >= by && r < rows - by && c >= bx && c < cols - bx)
            v = thermal_seed_value(aspect[i], mu, sigma, seed, i);
        out[i] = v;
    }
}

// one separable pass: out[r][c] = sum_k w[k] in[.. + k ..] along `axis`, zero padded
__global__ __launch_bounds__(kBlock) void k_blur_pass(const double *__restrict__ in,
                                                     double *__restrict__ out,
                                                     const double *__restrict__ weights, int radius,
                                                     int rows, int cols, int axis)
{
    const size_t n = static_cast<size_t>(rows) * cols;
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < n;
         i += static_cast<size_t>(gridDim.x) * kBlock) {
        const int r = static_cast<int>(i / cols), c = static_cast<int>(i % cols);
        double acc = 0.0;
        for (int k = -radius; k <= radius; ++k) {
            const int rr = axis == 0 ? r + k : r, cc = axis == 0 ? c : c + k;
            if (rr < 0 || rr >= rows || cc < 0 || cc >= cols) continue;
            acc += weights[k + radius] * in[static_cast<size_t>(rr) * cols + cc];
        }
        out[i] = acc;
    }
}

// ---- fused, batched form: seeds -> axis-0 pass -> axis-1 pass in one launch -------------
// A block owns 32 x 64 output cells of one realisation.  It draws the seeds of its tile plus
// a halo of `radius` (<= 16) cells into LDS (the Philox key is the global cell index, so a
// halo cell gets the value its own tile gives it), blurs LDS -> LDS along axis 0 and
// LDS -> registers along axis 1; neither the seed raster nor the axis-0 result reaches HBM.
// About one cell in 2000 is seeded, so both passes walk a bit mask of the tile's non-zero
// COLUMNS (ascending, the chain's order of k) instead of all 2 * radius + 1 taps: a term
// w * (+0.0) leaves an f64 sum of non-negative terms unchanged, and an out-of-raster cell,
// which k_blur_pass skips, is such a zero here.  Each kept term is a rounded multiply and a
// rounded add (-ffp-contract=off), as in k_blur_pass: results are bit-identical to the
// chain k_thermal_seeds -> k_blur_pass(axis 0) -> k_blur_pass(axis 1) at any seed density.
// LDS: seeds 64 x 97 f64 + axis-0 result 32 x 97 f64 + 33 weights + mask = 74 772 B, two
// blocks per CU.  The row stride 97 (odd) keeps the axis-0 pass, whose lanes run down a
// column, off a single bank; axis 1 reads one broadcast address per wave.
constexpr int kThRows = 32, kThCols = 64, kThMaxRadius = 16, kThMaxBatch = 32;
constexpr int kThSeedRows = kThRows + 2 * kThMaxRadius, kThSeedCols = kThCols + 2 * kThMaxRadius;
constexpr int kThStride = kThSeedCols + 1;
constexpr int kThMaskWords = kThSeedCols / 32;
static_assert(kThSeedCols % 32 == 0 && kBlock == 4 * kThCols && kBlock == 8 * kThRows, "k_thermal_fields thread map");

struct ThermalWeights { double w[2 * kThMaxRadius + 1]; };
struct ThermalSeeds { unsigned long long s[kThMaxBatch]; };

template <typename OUT>
__global__ __launch_bounds__(kBlock) void k_thermal_fields(const double *__restrict__ aspect, double mu,
                                                          double sigma, ThermalSeeds seeds,
                                                          ThermalWeights wts, int radius,
                                                          OUT *__restrict__ out, int rows, int cols,
                                                          int tiles_x)
{
    __shared__ double s_seed[kThSeedRows * kThStride];
    __shared__ double s_mid[kThRows * kThStride];
    __shared__ double s_w[2 * kThMaxRadius + 1];
    __shared__ unsigned s_mask[kThMaskWords];
    const int t = static_cast<int>(threadIdx.x);
    const int ty = static_cast<int>(blockIdx.x) / tiles_x, tx = static_cast<int>(blockIdx.x) - ty * tiles_x;
    const int real = static_cast<int>(blockIdx.y);
    const unsigned long long seed = seeds.s[real];
    const int taps = 2 * radius + 1;
    if (t < kThMaskWords) s_mask[t] = 0u;
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < 2 * kThMaxRadius + 1; ++k) s_w[k] = wts.w[k];
    }
    __syncthreads();

    // seeds of the tile and its halo; tile cell (tr, tc) is raster cell (r0 + tr, c0 + tc)
    const int by = static_cast<int>(0.1 * rows), bx = static_cast<int>(0.1 * cols);
    const int th = kThRows + 2 * radius, tw = kThCols + 2 * radius;
    const int r0 = ty * kThRows - radius, c0 = tx * kThCols - radius;
    for (int idx = t; idx < th * tw; idx += kBlock) {
        const int tr = idx / tw, tc = idx - tr * tw;
        const int r = r0 + tr, c = c0 + tc;
        double v = 0.0;
        if (r >= by && r < rows - by && c >= bx && c < cols - bx) {
            const size_t i = static_cast<size_t>(r) * cols + c;
            v = thermal_seed_value(aspect[i], mu, sigma, seed, i);
            if (v != 0.0) atomicOr(&s_mask[tc >> 5], 1u << (tc & 31));
        }
        s_seed[tr * kThStride + tc] = v;
    }
    __syncthreads();

    // axis 0, only in the columns that hold a seed: output row `orow` of the tile sums seed
    // rows orow .. orow + 2 radius; the n-th such column goes to the threads of slot n % 8
    {
        const int orow = t & (kThRows - 1), slot = t / kThRows;
        int n = 0;
        for (int word = 0; word < kThMaskWords; ++word) {
            unsigned m = __builtin_amdgcn_readfirstlane(s_mask[word]);
            for (; m; m &= m - 1, ++n) {
                if ((n & 7) != slot) continue;
                const int j = word * 32 + __ffs(m) - 1;
                double acc = 0.0;
                for (int k = 0; k < taps; ++k) acc += s_w[k] * s_seed[(orow + k) * kThStride + j];
                s_mid[orow * kThStride + j] = acc;
            }
        }
    }
    __syncthreads();

    // axis 1: output column `oc` sums tile columns oc .. oc + 2 radius of the axis-0 result;
    // a wave holds one row at a time (rows q, q + 4, ...), lanes along the columns
    const int oc = t & (kThCols - 1), q = t / kThCols;
    double acc[kThRows / 4];
#pragma unroll
    for (int i = 0; i < kThRows / 4; ++i) acc[i] = 0.0;
    for (int word = 0; word < kThMaskWords; ++word) {
        for (unsigned m = __builtin_amdgcn_readfirstlane(s_mask[word]); m; m &= m - 1) {
            const int j = word * 32 + __ffs(m) - 1;
            const int k = j - oc;
            if (k < 0 || k >= taps) continue;
            const double wk = s_w[k];
#pragma unroll
            for (int i = 0; i < kThRows / 4; ++i) acc[i] += wk * s_mid[(q + 4 * i) * kThStride + j];
        }
    }
    const int c = tx * kThCols + oc;
    if (c >= cols) return;
#pragma unroll
    for (int i = 0; i < kThRows / 4; ++i) {
        const int r = ty * kThRows + q + 4 * i;
        if (r < rows) out[(static_cast<size_t>(real) * rows + r) * cols + c] = static_cast<OUT>(acc[i]);
    }
}

__global__ __launch_bounds__(kBlock) void k_round_to_f32(const double *__restrict__ in, float *__restrict__ out, size_t n)
{
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < n;
         i += static_cast<size_t>(gridDim.x) * kBlock)
        out[i] = static_cast<float>(in[i]);
}

}  // namespace ssrs

using namespace ssrs;

static int blocks_for(size_t n)
{
    size_t b = (n + kBlock - 1) / kBlock;
    return static_cast<int>(b < 1 ? 1 : (b > static_cast<size_t>(kMaxStreamBlocks) ? kMaxStreamBlocks : b));
}

extern "C" size_t ssrs_blur_workspace_bytes(int rows, int cols, double sigma)
{
    if (rows <= 0 || cols <= 0 || !(sigma > 0.0)) return 0;
    const int radius = static_cast<int>(4.0 * sigma + 0.5);
    return static_cast<size_t>(rows) * cols * 8 + (static_cast<size_t>(2 * radius + 1) * 8 + 255) / 256 * 256 + 256;
}

extern "C" int ssrs_gaussian_blur(const double *in, double *out, double sigma, int rows, int cols,
                                  void *workspace, size_t workspace_bytes, void *stream)
{
    SSRS_REQUIRE(in && out && workspace, "ssrs_gaussian_blur: NULL pointer");
    SSRS_REQUIRE(rows > 0 && cols > 0 && sigma > 0.0, "ssrs_gaussian_blur: bad arguments");
    SSRS_REQUIRE(workspace_bytes >= ssrs_blur_workspace_bytes(rows, cols, sigma),
                 "ssrs_gaussian_blur: workspace too small");
    const int radius = blur_radius(sigma);
    const std::vector<double> w = blur_weights(sigma, radius);
    hipStream_t st = as_stream(stream);
    char *base = static_cast<char *>(workspace);
    double *d_w = reinterpret_cast<double *>(base);
    double *tmp = reinterpret_cast<double *>(base + (w.size() * 8 + 255) / 256 * 256);
    SSRS_HIP_CHECK(hipMemcpyAsync(d_w, w.data(), w.size() * 8, hipMemcpyHostToDevice, st));
    SSRS_HIP_CHECK(hipStreamSynchronize(st));
    const size_t n = static_cast<size_t>(rows) * cols;
    // scipy filters axis 0 first, then axis 1
    hipLaunchKernelGGL(k_blur_pass, dim3(blocks_for(n)), dim3(kBlock), 0, st, in, tmp, d_w, radius, rows, cols, 0);
    hipLaunchKernelGGL(k_blur_pass, dim3(blocks_for(n)), dim3(kBlock), 0, st, tmp, out, d_w, radius, rows, cols, 1);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

extern "C" int ssrs_thermal_seeds(const double *aspect, double thermal_intensity_scale,
                                  uint64_t seed, double *seeds, int rows, int cols, void *stream)
{
    SSRS_REQUIRE(aspect && seeds, "ssrs_thermal_seeds: NULL pointer");
    SSRS_REQUIRE(rows > 0 && cols > 0, "ssrs_thermal_seeds: bad sizes");
    const size_t n = static_cast<size_t>(rows) * cols;
    hipLaunchKernelGGL(k_thermal_seeds, dim3(blocks_for(n)), dim3(kBlock), 0, as_stream(stream),
                       aspect, thermal_intensity_scale + 3.0, 0.5,
                       static_cast<unsigned long long>(seed), seeds, rows, cols);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

// radius > kThMaxRadius: the tile of k_thermal_fields does not fit its LDS plan, so every
// realisation takes the three-launch chain through stream-ordered scratch
static int thermal_fields_chain(const double *aspect, double scale, double sigma, int radius,
                                const uint64_t *seeds, int count, void *out, int out_is_f32,
                                int rows, int cols, hipStream_t st)
{
    const std::vector<double> w = blur_weights(sigma, radius);
    const size_t n = static_cast<size_t>(rows) * cols;
    double *scratch = nullptr;
    SSRS_HIP_CHECK(hipMallocAsync(reinterpret_cast<void **>(&scratch), (2 * n + w.size()) * 8, st));
    double *a = scratch, *b = scratch + n, *d_w = scratch + 2 * n;
    hipError_t e = hipMemcpyAsync(d_w, w.data(), w.size() * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);      // `w` is about to leave scope
    for (int i = 0; i < count && e == hipSuccess; ++i) {
        hipLaunchKernelGGL(k_thermal_seeds, dim3(blocks_for(n)), dim3(kBlock), 0, st, aspect, scale + 3.0, 0.5,
                           static_cast<unsigned long long>(seeds[i]), a, rows, cols);
        hipLaunchKernelGGL(k_blur_pass, dim3(blocks_for(n)), dim3(kBlock), 0, st, a, b, d_w, radius, rows, cols, 0);
        double *dst = out_is_f32 ? a : static_cast<double *>(out) + i * n;
        hipLaunchKernelGGL(k_blur_pass, dim3(blocks_for(n)), dim3(kBlock), 0, st, b, dst, d_w, radius, rows, cols, 1);
        if (out_is_f32)
            hipLaunchKernelGGL(k_round_to_f32, dim3(blocks_for(n)), dim3(kBlock), 0, st, a,
                               static_cast<float *>(out) + i * n, n);
        e = hipGetLastError();
    }
    const hipError_t e_free = hipFreeAsync(scratch, st);
    SSRS_HIP_CHECK(e);
    SSRS_HIP_CHECK(e_free);
    return SSRS_OK;
}

extern "C" int ssrs_thermal_fields(const double *aspect, double thermal_intensity_scale, double sigma,
                                   const uint64_t *seeds, int count, void *out, int out_is_f32,
                                   int rows, int cols, void *stream)
{
    SSRS_REQUIRE(aspect && seeds && out, "ssrs_thermal_fields: NULL pointer");
    SSRS_REQUIRE(count > 0, "ssrs_thermal_fields: count must be positive");
    SSRS_REQUIRE(rows > 0 && cols > 0, "ssrs_thermal_fields: bad sizes");
    SSRS_REQUIRE(sigma > 0.0, "ssrs_thermal_fields: sigma must be positive");
    const int radius = blur_radius(sigma);
    hipStream_t st = as_stream(stream);
    if (radius > kThMaxRadius)
        return thermal_fields_chain(aspect, thermal_intensity_scale, sigma, radius, seeds, count, out, out_is_f32,
                                    rows, cols, st);
    const std::vector<double> w = blur_weights(sigma, radius);
    ThermalWeights wts{};
    for (size_t k = 0; k < w.size(); ++k) wts.w[k] = w[k];
    const int tiles_x = (cols + kThCols - 1) / kThCols;
    const long long ntiles = static_cast<long long>(tiles_x) * ((rows + kThRows - 1) / kThRows);
    SSRS_REQUIRE(ntiles <= 0x7fffffffLL, "ssrs_thermal_fields: raster too large");
    const size_t n = static_cast<size_t>(rows) * cols;
    for (int first = 0; first < count; first += kThMaxBatch) {       // seeds travel as a kernel argument
        const int nb = count - first < kThMaxBatch ? count - first : kThMaxBatch;
        ThermalSeeds sd{};
        for (int i = 0; i < nb; ++i) sd.s[i] = static_cast<unsigned long long>(seeds[first + i]);
        const dim3 grid(static_cast<unsigned>(ntiles), static_cast<unsigned>(nb));
        if (out_is_f32)
            hipLaunchKernelGGL(k_thermal_fields<float>, grid, dim3(kBlock), 0, st, aspect, thermal_intensity_scale + 3.0,
                               0.5, sd, wts, radius, static_cast<float *>(out) + first * n, rows, cols, tiles_x);
        else
            hipLaunchKernelGGL(k_thermal_fields<double>, grid, dim3(kBlock), 0, st, aspect, thermal_intensity_scale + 3.0,
                               0.5, sd, wts, radius, static_cast<double *>(out) + first * n, rows, cols, tiles_x);
        SSRS_HIP_CHECK(hipGetLastError());
    }
    return SSRS_OK;
}
