// K21 -- the track score for gfx950 (MI355X): the stepper's move probabilities read backwards.
//
// For every point of OBSERVED tracks, the probability that the movement model (movmodel.py:264-318, tracks.hip) gives to the
// move that leaves it, its status, and the surprisal of the scored moves summed per track and per cell.  The definition,
// rounding by rounding, is in include/ssrs_score.h.  One launch, one lane per point:
//   - a block takes kBlock consecutive points of the chunk (track borders or not) and stages them, the kScoreBack behind
//     and the kScoreAhead ahead in LDS: 67 lanes load four points each (one 16-byte load where traj is 16-byte aligned and
//     the four lie inside the chunk, point by point otherwise).  A lane's look-back -- the next point and up to
//     memory_parameter + 1 earlier ones -- reads its neighbours' points there;
//   - the tile's first and last track come from two binary searches of the offsets (lanes 0 and 1); every lane then searches
//     between them only (site_risk.hip's way);
//   - the window weights, the restriction masks and the probability sequence are RESTATED in score_model.h (which K22,
//     score_profile.hip, includes too) from tracks.hip (window_weights, restriction, choose_move's exact branch), not
//     shared with it: tests/test_score_emulation.py and
//     tests/test_gpu_score.py pin the restatement to the oracle and to the stepper's own tracks.  -ffp-contract=off is
//     required, every division is a division, sum9 keeps numpy's pairwise order;
//   - the per-track sums are a segmented inclusive scan over the block in LDS (the five counts packed 12 bits each into one
//     uint64 beside the surprisal), after which the last lane of every (block, track) segment adds its totals to `rows`
//     with 64-bit global adds; the maps take one 64-bit and one 32-bit add per SCORED move.
// Block cooperation is __shared__ + __syncthreads() only (no shuffles, ballots or DPP), so tests/hip_host_stub runs this
// file's own code on the CPU.  Integer adds modulo 2^64: the result does not depend on the launch order.
#include <climits>
#include <cmath>

#include "common.h"
#include "score_model.h"
#include "../../include/ssrs_score.h"

namespace ssrs {

struct ScoreArgs {
    const uint32_t *traj;          // one int16 (row, col) pair per dword
    const long long *off;          // ntracks + 1 offsets
    int ntracks;
    int rows, cols, burnin, memory;
    double nu;
    double prior[9];
    long long p0, p1;              // the chunk's points: off[0], off[ntracks]
    const double *updraft;         // may be NULL (drw)
    const float *potential;        // may be NULL
    double *p;                     // may be NULL
    uint8_t *status;               // may be NULL
    u64 *sums;                     // (ntracks, SSRS_SCORE_ROW)
    u64 *surprisal_map;            // may be NULL
    uint32_t *scored_map;          // may be NULL
};

// kVec: traj is 16-byte aligned
template <bool kVec>
__global__ __launch_bounds__(kBlock) void k_tracks_score(const ScoreArgs a)
{
    __shared__ uint32_t s_pts[kScoreStage];
    __shared__ int s_t[2];
    __shared__ int s_track[kBlock];
    __shared__ u64 s_sum[2][kBlock], s_cnt[2][kBlock];
    const int tid = static_cast<int>(threadIdx.x);

    // the stage: points tile0 - kScoreBack .. tile0 + kBlock + kScoreAhead - 1; points outside [p0, p1) are not read
    const long long a0 = a.p0 & ~3LL;                      // tiles are cut at multiples of four points of the BUFFER
    const long long tile0 = a0 + static_cast<long long>(blockIdx.x) * kBlock;
    if (tid < kScoreStage / 4) {
        const long long g = tile0 - kScoreBack + 4 * tid;
        if (kVec && g >= a.p0 && g + 4 <= a.p1) {
            const uint4 v = *reinterpret_cast<const uint4 *>(a.traj + g);
            s_pts[4 * tid + 0] = v.x, s_pts[4 * tid + 1] = v.y, s_pts[4 * tid + 2] = v.z, s_pts[4 * tid + 3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) s_pts[4 * tid + j] = (g + j >= a.p0 && g + j < a.p1) ? a.traj[g + j] : 0u;
        }
    }

    // the track that holds the lane's point: the LAST one that starts at or before it, searched between the tile's first
    // and last track, which lanes 0 and 1 find over all offsets
    const long long first = tile0 > a.p0 ? tile0 : a.p0;
    const long long last = tile0 + kBlock < a.p1 ? tile0 + kBlock - 1 : a.p1 - 1;
    if (tid < 2) {
        const long long key = tid == 0 ? first : last;
        int lo = 0, hi = a.ntracks;
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (a.off[mid] <= key) lo = mid; else hi = mid;
        }
        s_t[tid] = lo;
    }
    __syncthreads();                                       // (covers the stage too)
    const long long i = tile0 + tid;
    const bool valid = i >= a.p0 && i < a.p1;
    int t = s_t[0];
    {
        long long key = i > first ? i : first;
        key = key < last ? key : last;                     // (lanes outside the chunk: any track of the tile will do)
        int hi = s_t[1] + 1;
        while (hi - t > 1) {
            const int mid = t + (hi - t) / 2;
            if (a.off[mid] <= key) t = mid; else hi = mid;
        }
    }
    const long long t_beg = a.off[t], t_end = a.off[t + 1];

    auto point = [&](long long k, int &r, int &c) {        // P_k, for tile0 - kScoreBack <= k < tile0 + kBlock + kScoreAhead
        const uint32_t v = s_pts[kScoreBack + static_cast<int>(k - tile0)];
        r = static_cast<int16_t>(v & 0xFFFF);
        c = static_cast<int16_t>(v >> 16);
    };
    auto base = [&](long long k, int &r, int &c) {         // the cell that move k - t_beg leaves
        point(k, r, c);
        if (k - t_beg <= a.burnin) score_move_away(a.rows, a.cols, r, c);
    };

    uint32_t st = SSRS_SCORE_LAST;
    double pj = 0.0;
    u64 s = 0, cnt = 0;
    if (valid && i + 1 < t_end && i >= t_beg) {
        int br, bc, nr, nc;
        base(i, br, bc);
        point(i + 1, nr, nc);
        const int dr = nr - br, dc = nc - bc;
        if (!(br > 0 && br < a.rows - 1 && bc > 0 && bc < a.cols - 1)) st = SSRS_SCORE_OUT;
        else if (dr < -1 || dr > 1 || dc < -1 || dc > 1) st = SSRS_SCORE_NOT_A_MOVE;
        else {
            uint32_t mask = kScoreAllButCentre;
            for (int k = 1; k <= a.memory; ++k) {
                const long long q = i - k;
                if (q < t_beg) break;                              // the track's start
                int r0, c0, r1, c1;
                base(q, r0, c0);
                point(q + 1, r1, c1);
                const int er = r1 - r0, ec = c1 - c0;
                if (er < -1 || er > 1 || ec < -1 || ec > 1) break; // a gap in the observations: the memory starts here
                mask &= score_restriction(er, ec);
            }
            double w[9], q[9];
            score_window_weights(a, br, bc, w);
            score_probabilities(w, a.prior, a.nu, mask, q);
            const int idx = 3 * (dr + 1) + (dc + 1);
#pragma unroll
            for (int k = 0; k < 9; ++k) pj = k == idx ? q[k] : pj;
            if (pj == 0.0) st = SSRS_SCORE_ZERO;
            else if (pj > 0.0 && pj < __builtin_inf()) {
                st = SSRS_SCORE_SCORED;
                const double bits = -log2(pj) * 4294967296.0;      // units of 2^-32 bit
                s = bits > 0.0 ? static_cast<u64>(rint(bits)) : 0;
                const long long cell = static_cast<long long>(br) * a.cols + bc;
                if (a.surprisal_map != nullptr && s != 0) atomicAdd(a.surprisal_map + cell, s);
                if (a.scored_map != nullptr) atomicAdd(a.scored_map + cell, 1u);
            } else st = SSRS_SCORE_UNDEFINED;
        }
        // rows' columns 1..5 in the order of the header: scored, zero, not_a_move, out, undefined
        const int column = st == SSRS_SCORE_SCORED ? 0 : st == SSRS_SCORE_ZERO ? 1 : st == SSRS_SCORE_NOT_A_MOVE ? 2
                           : st == SSRS_SCORE_OUT ? 3 : 4;
        cnt = static_cast<u64>(1) << (kScoreCountBits * column);
    }
    if (valid) {
        if (a.p != nullptr) a.p[i] = pj;
        if (a.status != nullptr) a.status[i] = static_cast<uint8_t>(st);
    }

    // the segmented inclusive scan: equal track numbers at distance d mean equal numbers in between (tracks are runs)
    const int id = valid ? t : -1;
    s_track[tid] = id;
    s_sum[0][tid] = s;
    s_cnt[0][tid] = cnt;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < kBlock; d <<= 1) {
        if (tid >= d && s_track[tid - d] == id) {
            s += s_sum[cur][tid - d];
            cnt += s_cnt[cur][tid - d];
        }
        cur ^= 1;
        s_sum[cur][tid] = s;
        s_cnt[cur][tid] = cnt;
        __syncthreads();
    }
    if (id >= 0 && (tid == kBlock - 1 || s_track[tid + 1] != id)) {       // the segment's last lane holds its totals
        u64 *row = a.sums + static_cast<long long>(id) * SSRS_SCORE_ROW;
        if (s != 0) atomicAdd(row, s);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const u64 n = (cnt >> (kScoreCountBits * k)) & ((1u << kScoreCountBits) - 1);
            if (n != 0) atomicAdd(row + 1 + k, n);
        }
    }
}

}  // namespace ssrs

using namespace ssrs;

extern "C" int ssrs_tracks_score(const SsrsTrackParams *params, const double *updraft, const float *potential,
                                 const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks, double *p,
                                 uint8_t *status, uint64_t *rows, uint64_t *surprisal_map, uint32_t *scored_map, void *stream)
{
    SSRS_REQUIRE(params && traj && traj_offsets && rows,
                 "ssrs_tracks_score: NULL pointer (params, traj, traj_offsets and rows are required)");
    SSRS_REQUIRE(updraft || !potential, "ssrs_tracks_score: a potential needs an updraft (both NULL = drw)");
    SSRS_REQUIRE(ntracks >= 0 && ntracks <= INT32_MAX, "ssrs_tracks_score: ntracks = %lld outside [0, 2^31)",
                 static_cast<long long>(ntracks));
    SSRS_REQUIRE(params->rows >= 3 && params->rows <= 32767 && params->cols >= 3 && params->cols <= 32767,
                 "ssrs_tracks_score: a %d x %d raster (3..32767 either way)", params->rows, params->cols);
    SSRS_REQUIRE(params->memory_parameter != 0,
                 "ssrs_tracks_score: memory_parameter = 0 (the whole history) is not supported: it needs a running AND "
                 "along the track; give 1..%d", SSRS_SCORE_MAX_MEMORY);
    SSRS_REQUIRE(params->memory_parameter >= 1 && params->memory_parameter <= SSRS_SCORE_MAX_MEMORY,
                 "ssrs_tracks_score: memory_parameter = %d outside [1, %d]", params->memory_parameter, SSRS_SCORE_MAX_MEMORY);
    SSRS_REQUIRE(params->scaling_parameter >= 0.0, "ssrs_tracks_score: scaling_parameter = %g (not negative, not NaN)",
                 params->scaling_parameter);
    SSRS_REQUIRE(params->burnin >= 0, "ssrs_tracks_score: burnin = %d is negative", params->burnin);
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(traj) & 3u) == 0, "ssrs_tracks_score: traj must be 4-byte aligned");
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(p) & 7u) == 0 && (reinterpret_cast<uintptr_t>(rows) & 7u) == 0 &&
                 (reinterpret_cast<uintptr_t>(surprisal_map) & 7u) == 0,
                 "ssrs_tracks_score: p, rows and surprisal_map must be 8-byte aligned");
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(scored_map) & 3u) == 0, "ssrs_tracks_score: scored_map must be 4-byte aligned");
    if (ntracks == 0) return SSRS_OK;
    hipStream_t st = as_stream(stream);

    // the chunk's first and last offset, on the host: the launch is sized from its points
    long long ends[2];
    SSRS_HIP_CHECK(hipMemcpyAsync(&ends[0], traj_offsets, 8, hipMemcpyDeviceToHost, st));
    SSRS_HIP_CHECK(hipMemcpyAsync(&ends[1], traj_offsets + ntracks, 8, hipMemcpyDeviceToHost, st));
    SSRS_HIP_CHECK(hipStreamSynchronize(st));
    SSRS_REQUIRE(ends[0] >= 0, "ssrs_tracks_score: traj_offsets[0] = %lld is negative", ends[0]);
    SSRS_REQUIRE(ends[1] >= ends[0], "ssrs_tracks_score: traj_offsets descends (%lld after %lld)", ends[1], ends[0]);
    if (ends[1] == ends[0]) return SSRS_OK;

    ScoreArgs a;
    a.traj = reinterpret_cast<const uint32_t *>(traj);
    a.off = reinterpret_cast<const long long *>(traj_offsets);
    a.ntracks = static_cast<int>(ntracks);
    a.rows = params->rows;
    a.cols = params->cols;
    a.burnin = params->burnin;
    a.memory = params->memory_parameter;
    a.nu = params->scaling_parameter;
    for (int k = 0; k < 9; ++k) a.prior[k] = params->prior[k];
    a.p0 = ends[0];
    a.p1 = ends[1];
    a.updraft = updraft;
    a.potential = potential;
    a.p = p;
    a.status = status;
    a.sums = reinterpret_cast<u64 *>(rows);
    a.surprisal_map = reinterpret_cast<u64 *>(surprisal_map);
    a.scored_map = scored_map;
    const long long ntiles = (a.p1 - (a.p0 & ~3LL) + kBlock - 1) / kBlock;
    SSRS_REQUIRE(ntiles <= INT32_MAX, "ssrs_tracks_score: %lld points in one call (at most 2^31 tiles of %d)", a.p1 - a.p0,
                 kBlock);
    SSRS_HIP_CHECK(hipMemsetAsync(rows, 0, static_cast<size_t>(ntracks) * SSRS_SCORE_ROW * sizeof(uint64_t), st));
    const bool vec = (reinterpret_cast<uintptr_t>(traj) & 15u) == 0;
    const dim3 grid(static_cast<unsigned>(ntiles)), block(kBlock);
    if (vec) hipLaunchKernelGGL((k_tracks_score<true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_tracks_score<false>), grid, block, 0, st, a);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}
