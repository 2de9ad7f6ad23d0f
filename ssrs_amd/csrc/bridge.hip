// K23 -- the gap score for gfx950 (MI355X): n-move transition probabilities between the fixes of sparse telemetry.
//
// For every job (A, s, B, n) the probability that the movement model with memory 1 is at cell B n moves after it was at
// cell A in state s: the forward algorithm over the states (cell, last move).  The definition, rounding by rounding, is in
// include/ssrs_bridge.h.  One workgroup per gap, in a grid-stride loop:
//   - the window is the bounding box of the cells x with cheb(A, x) + cheb(x, B) <= n, clipped to the raster: at most
//     (n + 1)^2 cells.  Its states live in LDS in f64, two buffers of nine planes; the LDS is dynamic, sized by the host from
//     the longest valid job of the call (k_bridge_longest, read back), so that calls of short gaps put several workgroups
//     on a CU;
//   - a value is stored under its SOURCE: plane k at cell y holds alpha(y + delta_k, k), the mass that left y by move k.
//     All nine sums of those targets have y as their only source cell, so the lane that owns y forms them alone, in the
//     defined order (ascending incoming state, from 0.0): no atomic, no dependence on lane or launch order.  The next step
//     reads alpha(x, d) at (x - delta_d, d);
//   - step t visits the rectangle of interior cells within t of A and n - t of B (what is occupied and can still reach B).
//     Both buffers are zeroed once per gap: a cell outside step t's rectangle that step t + 1 reads was in no earlier
//     rectangle (it is further than t from A), so it still holds that zero.  One __syncthreads() per step;
//   - only occupied states evaluate their probabilities (score_model.h, K21's own functions: -ffp-contract=off is
//     required); the window weights of a cell are formed once per step, and only if a state of it is occupied;
//   - lane 0 reads the nine states of B after every step (arrivals) and after the last one (g, P, status, surprisal).
// Block cooperation is dynamic LDS + __syncthreads() only, so tests/hip_host_stub runs this file's own code on the CPU.
#include <climits>
#include <cmath>

#include "common.h"
#include "score_model.h"
#include "../../include/ssrs_bridge.h"

namespace ssrs {

constexpr int kBridgeSmall = 256, kBridgeLarge = 512;      // lanes of a workgroup: windows of up to / more than ...
constexpr int kBridgeSmallCells = 512;                      // ... this many cells
constexpr int kBridgeMaxBlocks = 1 << 16;
constexpr int kBridgeSide = SSRS_BRIDGE_MAX_MOVES + 1;
static_assert(2 * 9 * kBridgeSide * kBridgeSide * 8 == 156816, "the LDS of the longest gap, as ssrs_bridge.h states it");
static_assert(SSRS_BRIDGE_MAX_MOVES <= kBridgeSmall, "k_tracks_bridge zeroes a job's arrivals with one lane each");

struct BridgeArgs {
    const int32_t *jobs;           // (ngaps, SSRS_BRIDGE_JOB)
    long long ngaps;
    int longest;                   // the largest valid `moves` of the call: the launch's LDS holds (longest + 1)^2 cells
    int rows, cols;
    double nu;
    double prior[9];
    const double *updraft;         // may be NULL (drw)
    const float *potential;        // may be NULL
    double *g;                     // (ngaps, 9)
    uint8_t *status;
    u64 *surprisal;
    double *arrivals;              // (ngaps, SSRS_BRIDGE_MAX_MOVES), may be NULL
};

__host__ __device__ __forceinline__ int bridge_abs(int v) { return v < 0 ? -v : v; }
__host__ __device__ __forceinline__ int bridge_min(int a, int b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ int bridge_max(int a, int b) { return a > b ? a : b; }

// the largest `moves` in [1, SSRS_BRIDGE_MAX_MOVES] over the jobs, maxed into *longest (zeroed by the host)
__global__ __launch_bounds__(kBlock) void k_bridge_longest(const int32_t *jobs, long long ngaps, u64 *longest)
{
    __shared__ int s_max[kBlock];
    const int tid = static_cast<int>(threadIdx.x);
    int m = 0;
    for (long long j = static_cast<long long>(blockIdx.x) * kBlock + tid; j < ngaps; j += static_cast<long long>(gridDim.x) * kBlock) {
        const int n = jobs[j * SSRS_BRIDGE_JOB + 5];
        if (n >= 1 && n <= SSRS_BRIDGE_MAX_MOVES && n > m) m = n;
    }
    s_max[tid] = m;
    __syncthreads();
    for (int d = kBlock / 2; d > 0; d >>= 1) {
        if (tid < d && s_max[tid + d] > s_max[tid]) s_max[tid] = s_max[tid + d];
        __syncthreads();
    }
    if (tid == 0 && s_max[0] > 0) atomicMax(longest, static_cast<u64>(s_max[0]));
}

template <int kThreads>
__global__ __launch_bounds__(kThreads) void k_tracks_bridge(const BridgeArgs a)
{
    HIP_DYNAMIC_SHARED(double, s_alpha)                    // [2][9][cells of the job's window]
    const int tid = static_cast<int>(threadIdx.x);

    for (long long j = blockIdx.x; j < a.ngaps; j += gridDim.x) {
        const int32_t *job = a.jobs + j * SSRS_BRIDGE_JOB;
        const int n = job[5];
        uint32_t st;
        int ra = 0, ca = 0, s = 0, rb = 0, cb = 0;
        if (n < 1 || n > a.longest) st = SSRS_BRIDGE_TOO_LONG;     // (longest <= SSRS_BRIDGE_MAX_MOVES is the largest n inside)
        else {
            ra = job[0], ca = job[1], s = job[2], rb = job[3], cb = job[4];
            if (!(ra > 0 && ra < a.rows - 1 && ca > 0 && ca < a.cols - 1) || rb < 0 || rb >= a.rows || cb < 0 || cb >= a.cols ||
                s < 0 || s > 8)
                st = SSRS_BRIDGE_OUT;
            else if (bridge_max(bridge_abs(ra - rb), bridge_abs(ca - cb)) > n) st = SSRS_BRIDGE_ZERO;
            else st = SSRS_BRIDGE_SCORED;                          // to be evaluated
        }
        if (a.arrivals != nullptr && tid < SSRS_BRIDGE_MAX_MOVES && (st != SSRS_BRIDGE_SCORED || tid >= n))
            a.arrivals[j * SSRS_BRIDGE_MAX_MOVES + tid] = 0.0;
        if (st != SSRS_BRIDGE_SCORED) {                            // (the same for every lane: no barrier is skipped by some)
            if (tid < 9) a.g[j * 9 + tid] = 0.0;
            if (tid == 0) a.status[j] = static_cast<uint8_t>(st), a.surprisal[j] = 0;
            continue;
        }

        // the window: rows r0..r1, columns c0..c1 of the raster
        const int er = (n - bridge_abs(ra - rb)) / 2, ec = (n - bridge_abs(ca - cb)) / 2;
        const int r0 = bridge_max(bridge_min(ra, rb) - er, 0), r1 = bridge_min(bridge_max(ra, rb) + er, a.rows - 1);
        const int c0 = bridge_max(bridge_min(ca, cb) - ec, 0), c1 = bridge_min(bridge_max(ca, cb) + ec, a.cols - 1);
        const int wc = c1 - c0 + 1, cells = (r1 - r0 + 1) * wc;   // cells <= (n + 1)^2: inside the launch's LDS
        for (int i = tid; i < 2 * 9 * cells; i += kThreads) s_alpha[i] = 0.0;
        __syncthreads();

        for (int t = 0; t < n; ++t) {
            const double *src = s_alpha + (t & 1) * 9 * cells;
            double *dst = s_alpha + ((t + 1) & 1) * 9 * cells;
            // the sources of step t: interior, within t of A (occupied) and within n - t of B (can still arrive)
            const int lo_r = bridge_max(bridge_max(ra - t, rb - (n - t)), bridge_max(r0, 1));
            const int hi_r = bridge_min(bridge_min(ra + t, rb + (n - t)), bridge_min(r1, a.rows - 2));
            const int lo_c = bridge_max(bridge_max(ca - t, cb - (n - t)), bridge_max(c0, 1));
            const int hi_c = bridge_min(bridge_min(ca + t, cb + (n - t)), bridge_min(c1, a.cols - 2));
            const int aw = hi_c - lo_c + 1;
            const int na = (hi_r >= lo_r && aw > 0) ? (hi_r - lo_r + 1) * aw : 0;
            for (int i = tid; i < na; i += kThreads) {
                const int yr = lo_r + i / aw, yc = lo_c + i % aw;
                double acc[9], w[9], q[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) acc[k] = 0.0;
                bool have_w = false;
#pragma unroll 1
                for (int d = 0; d < 9; ++d) {
                    const int dr = d / 3 - 1, dc = d % 3 - 1;
                    double al;
                    if (t == 0) al = d == s ? 1.0 : 0.0;           // (step 0 visits A alone)
                    else {
                        const int pr = yr - dr, pc = yc - dc;      // alpha_t(y, d) left y - delta_d by move d
                        al = (pr >= r0 && pr <= r1 && pc >= c0 && pc <= c1) ? src[d * cells + (pr - r0) * wc + (pc - c0)] : 0.0;
                    }
                    if (al == 0.0) continue;                       // (a NaN goes on)
                    if (!have_w) {
                        score_window_weights(a, yr, yc, w);
                        have_w = true;
                    }
                    score_probabilities(w, a.prior, a.nu, kScoreAllButCentre & score_restriction(dr, dc), q);
#pragma unroll
                    for (int k = 0; k < 9; ++k) acc[k] = acc[k] + al * q[k];
                }
                const int cell = (yr - r0) * wc + (yc - c0);
#pragma unroll
                for (int k = 0; k < 9; ++k) dst[k * cells + cell] = acc[k];
            }
            __syncthreads();
            if (tid == 0 && (a.arrivals != nullptr || t == n - 1)) {
                double gk[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const int pr = rb - (k / 3 - 1), pc = cb - (k % 3 - 1);
                    gk[k] = (pr >= r0 && pr <= r1 && pc >= c0 && pc <= c1) ? dst[k * cells + (pr - r0) * wc + (pc - c0)] : 0.0;
                }
                const double P = score_sum9(gk);
                if (a.arrivals != nullptr) a.arrivals[j * SSRS_BRIDGE_MAX_MOVES + t] = P;
                if (t == n - 1) {
#pragma unroll
                    for (int k = 0; k < 9; ++k) a.g[j * 9 + k] = gk[k];
                    u64 bits64 = 0;
                    if (P == 0.0) st = SSRS_BRIDGE_ZERO;
                    else if (P > 0.0 && P < __builtin_inf()) {
                        const double bits = -log2(P) * 4294967296.0;       // units of 2^-32 bit
                        bits64 = bits > 0.0 ? static_cast<u64>(rint(bits)) : 0;
                    } else st = SSRS_BRIDGE_UNDEFINED;
                    a.status[j] = static_cast<uint8_t>(st);
                    a.surprisal[j] = bits64;
                }
            }
        }
        __syncthreads();                                           // lane 0 has read the last buffer before it is zeroed
    }
}

// hipDeviceAttributeMaxSharedMemoryPerBlock of the current device, read once
static int bridge_device_lds(int *bytes)
{
    static int cached = -1;
    if (cached < 0) {
        int dev = 0, v = 0;
        SSRS_HIP_CHECK(hipGetDevice(&dev));
        SSRS_HIP_CHECK(hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
        cached = v;
    }
    *bytes = cached;
    return SSRS_OK;
}

template <int kThreads>
static int bridge_launch(const BridgeArgs &a, unsigned lds, hipStream_t st)
{
    if (lds > 64u * 1024u)
        SSRS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_tracks_bridge<kThreads>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    const long long blocks = a.ngaps < kBridgeMaxBlocks ? a.ngaps : kBridgeMaxBlocks;
    hipLaunchKernelGGL((k_tracks_bridge<kThreads>), dim3(static_cast<unsigned>(blocks)), dim3(kThreads), lds, st, a);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

}  // namespace ssrs

using namespace ssrs;

extern "C" int ssrs_tracks_bridge(const SsrsTrackParams *params, const double *updraft, const float *potential,
                                  const int32_t *jobs, int64_t ngaps, double *g, uint8_t *status, uint64_t *surprisal,
                                  double *arrivals, void *stream)
{
    SSRS_REQUIRE(params && jobs && g && status && surprisal,
                 "ssrs_tracks_bridge: NULL pointer (params, jobs, g, status and surprisal are required)");
    SSRS_REQUIRE(updraft || !potential, "ssrs_tracks_bridge: a potential needs an updraft (both NULL = drw)");
    SSRS_REQUIRE(ngaps >= 0 && ngaps <= INT32_MAX, "ssrs_tracks_bridge: ngaps = %lld outside [0, 2^31)",
                 static_cast<long long>(ngaps));
    SSRS_REQUIRE(params->rows >= 3 && params->rows <= 32767 && params->cols >= 3 && params->cols <= 32767,
                 "ssrs_tracks_bridge: a %d x %d raster (3..32767 either way)", params->rows, params->cols);
    SSRS_REQUIRE(params->memory_parameter == 1,
                 "ssrs_tracks_bridge: memory_parameter = %d is not supported: the states of a gap are (cell, last move), "
                 "which is memory_parameter 1", params->memory_parameter);
    SSRS_REQUIRE(params->scaling_parameter >= 0.0, "ssrs_tracks_bridge: scaling_parameter = %g (not negative, not NaN)",
                 params->scaling_parameter);
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(jobs) & 3u) == 0, "ssrs_tracks_bridge: jobs must be 4-byte aligned");
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(g) & 7u) == 0 && (reinterpret_cast<uintptr_t>(surprisal) & 7u) == 0 &&
                 (reinterpret_cast<uintptr_t>(arrivals) & 7u) == 0,
                 "ssrs_tracks_bridge: g, surprisal and arrivals must be 8-byte aligned");
    if (ngaps == 0) return SSRS_OK;
    hipStream_t st = as_stream(stream);

    // the longest valid job, through surprisal[0] (written by the gaps' launch afterwards): the LDS is sized from it
    unsigned long long longest = 0;
    SSRS_HIP_CHECK(hipMemsetAsync(surprisal, 0, sizeof(uint64_t), st));
    const long long scan = (ngaps + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_bridge_longest, dim3(static_cast<unsigned>(scan < kMaxStreamBlocks ? scan : kMaxStreamBlocks)),
                       dim3(kBlock), 0, st, jobs, static_cast<long long>(ngaps), reinterpret_cast<u64 *>(surprisal));
    SSRS_HIP_CHECK(hipGetLastError());
    SSRS_HIP_CHECK(hipMemcpyAsync(&longest, surprisal, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SSRS_HIP_CHECK(hipStreamSynchronize(st));
    SSRS_REQUIRE(longest <= SSRS_BRIDGE_MAX_MOVES, "ssrs_tracks_bridge: the scan of the jobs returned %llu moves", longest);
    const int side = static_cast<int>(longest) + 1;
    const unsigned lds = 2u * 9u * static_cast<unsigned>(side * side) * sizeof(double);
    int offered = 0;
    if (int rc = bridge_device_lds(&offered)) return rc;
    SSRS_REQUIRE(static_cast<long long>(lds) <= offered,
                 "ssrs_tracks_bridge: a gap of %llu moves needs %u bytes of LDS per workgroup, the device offers %d "
                 "(hipDeviceAttributeMaxSharedMemoryPerBlock)", longest, lds, offered);

    BridgeArgs a;
    a.jobs = jobs;
    a.ngaps = ngaps;
    a.longest = static_cast<int>(longest);
    a.rows = params->rows;
    a.cols = params->cols;
    a.nu = params->scaling_parameter;
    for (int k = 0; k < 9; ++k) a.prior[k] = params->prior[k];
    a.updraft = updraft;
    a.potential = potential;
    a.g = g;
    a.status = status;
    a.surprisal = reinterpret_cast<u64 *>(surprisal);
    a.arrivals = arrivals;
    return side * side > kBridgeSmallCells ? bridge_launch<kBridgeLarge>(a, lds, st) : bridge_launch<kBridgeSmall>(a, lds, st);
}
