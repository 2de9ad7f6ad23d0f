// K22 -- the likelihood profile of observed tracks for gfx950 (MI355X): K21's per-track rows for every combination of a
// list of memories and a list of nus, in one pass over the points.
//
// rows[t, a, b, :] is the row ssrs_tracks_score (score.hip) writes for memories[a] and nus[b]; the definition is in
// include/ssrs_score.h, the export's in include/ssrs_score_profile.h.  One launch, one lane per point, built like K21's:
//   - the stage of kBlock points with the kScoreBack behind and the kScoreAhead ahead, the two-level track search, the
//     base, the status tests (LAST, OUT, NOT_A_MOVE) and the raw window weights are computed ONCE per lane;
//   - the mask comes from ONE walk back: the combinations are visited memory by memory, and entering memories[a] the walk
//     goes on from where memories[a - 1] left it, to the track's start or a gap at the latest.  The half of the probability
//     sequence that does not depend on nu (score_probabilities_head) is evaluated when the mask differs from the one it
//     was last evaluated for, so a memory behind a start or a gap reuses the nine values of the memory before;
//   - per nu: score_probability_of (nine pow, none for nu = 1; the second pairwise sum; one division), the status, s_j:
//     the same operations on the same operands as K21's, from the same header (score_model.h), hence the same bits;
//   - the block reduces per (track, combination) with K21's segmented inclusive scan in LDS, kProfileGroup combinations at
//     a time: every lane of the block passes every barrier (the loop bounds are kernel arguments), lanes without an
//     evaluated move contribute their constant counts (not_a_move, out) or zeros.  The last lane of a (block, track)
//     segment adds its non-zero totals to `rows` with 64-bit global adds.
// Block cooperation is __shared__ + __syncthreads() only, so tests/hip_host_stub runs this file's own code on the CPU.
// Integer adds modulo 2^64: the result does not depend on the launch order.
#include <climits>
#include <cmath>

#include "common.h"
#include "score_model.h"
#include "../../include/ssrs_score_profile.h"

namespace ssrs {

constexpr int kProfileGroup = 4;                           // combinations per scan: 9 barriers per group, 32 KiB of LDS
static_assert(SSRS_PROFILE_MAX_MEMORIES <= SSRS_SCORE_MAX_MEMORY, "ascending memories in 1..8 are at most eight");

struct ProfileArgs {
    const uint32_t *traj;          // one int16 (row, col) pair per dword
    const long long *off;          // ntracks + 1 offsets
    int ntracks;
    int rows, cols, burnin;
    int nmem, nnu, ncombo;         // ncombo = nmem * nnu; combination c = a * nnu + b
    int memories[SSRS_PROFILE_MAX_MEMORIES];
    double nus[SSRS_PROFILE_MAX_NUS];
    double prior[9];
    long long p0, p1;              // the chunk's points: off[0], off[ntracks]
    const double *updraft;         // may be NULL (drw)
    const float *potential;        // may be NULL
    u64 *sums;                     // (ntracks, nmem, nnu, SSRS_SCORE_ROW)
};

// kVec: traj is 16-byte aligned
template <bool kVec>
__global__ __launch_bounds__(kBlock) void k_tracks_score_profile(const ProfileArgs a)
{
    __shared__ uint32_t s_pts[kScoreStage];
    __shared__ int s_t[2];
    __shared__ int s_track[kBlock];
    __shared__ u64 s_sum[2][kProfileGroup][kBlock], s_cnt[2][kProfileGroup][kBlock];
    const int tid = static_cast<int>(threadIdx.x);

    // the stage and the track search, as in k_tracks_score
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
    // rows' columns 1..5 in the order of the header: scored, zero, not_a_move, out, undefined
    auto one = [](int column) { return static_cast<u64>(1) << (kScoreCountBits * column); };

    // what does not depend on the combination: the status tests, the move's index and the raw weights
    bool evaluated = false;
    u64 fixed = 0;                                         // the count of a move whose status no combination changes
    int idx = 0;
    double w[9];
    if (valid && i + 1 < t_end && i >= t_beg) {
        int br, bc, nr, nc;
        base(i, br, bc);
        point(i + 1, nr, nc);
        const int dr = nr - br, dc = nc - bc;
        if (!(br > 0 && br < a.rows - 1 && bc > 0 && bc < a.cols - 1)) fixed = one(3);
        else if (dr < -1 || dr > 1 || dc < -1 || dc > 1) fixed = one(2);
        else {
            evaluated = true;
            idx = 3 * (dr + 1) + (dc + 1);
            score_window_weights(a, br, bc, w);
        }
    }
    const int id = valid ? t : -1;
    s_track[tid] = id;                                     // (read after the first barrier below)
    const bool flushes = id >= 0 && (tid == kBlock - 1 || i + 1 == t_end);      // the last lane of a (block, track) segment

    // the walk back and the values of the mask it was last evaluated for
    int depth = 1;                                         // the next delta to look at is delta_{j - depth}
    bool open = true;                                      // neither the start nor a gap was met
    uint32_t mask = kScoreAllButCentre, head_mask = ~0u;   // (no mask equals ~0)
    double q1[9];

    for (int c0 = 0; c0 < a.ncombo; c0 += kProfileGroup) {
        const int n = a.ncombo - c0 < kProfileGroup ? a.ncombo - c0 : kProfileGroup;
#pragma unroll 1
        for (int j = 0; j < n; ++j) {
            const int ai = (c0 + j) / a.nnu, bi = (c0 + j) - ai * a.nnu;
            u64 s = 0, cnt = fixed;
            if (evaluated) {
                if (bi == 0) {                                         // a new memory: the walk goes on to its depth
                    const int memory = a.memories[ai];
                    while (open && depth <= memory) {
                        const long long q = i - depth;
                        if (q < t_beg) { open = false; break; }        // the track's start
                        int fr, fc, tr, tc;
                        base(q, fr, fc);
                        point(q + 1, tr, tc);
                        const int er = tr - fr, ec = tc - fc;
                        if (er < -1 || er > 1 || ec < -1 || ec > 1) { open = false; break; }   // a gap: the memory starts here
                        mask &= score_restriction(er, ec);
                        ++depth;
                    }
                    if (mask != head_mask) {
                        score_probabilities_head(w, a.prior, mask, q1);
                        head_mask = mask;
                    }
                }
                const double pj = score_probability_of(q1, a.nus[bi], idx);
                if (pj == 0.0) cnt = one(1);
                else if (pj > 0.0 && pj < __builtin_inf()) {
                    cnt = one(0);
                    const double bits = -log2(pj) * 4294967296.0;      // units of 2^-32 bit
                    s = bits > 0.0 ? static_cast<u64>(rint(bits)) : 0;
                } else cnt = one(4);
            }
            s_sum[0][j][tid] = s;
            s_cnt[0][j][tid] = cnt;
        }
        __syncthreads();

        // the segmented inclusive scan of the group: equal track numbers at distance d mean equal numbers in between
        int cur = 0;
        for (int d = 1; d < kBlock; d <<= 1) {
            const bool joins = tid >= d && s_track[tid - d] == id;
            for (int j = 0; j < n; ++j) {
                u64 s = s_sum[cur][j][tid], cnt = s_cnt[cur][j][tid];
                if (joins) {
                    s += s_sum[cur][j][tid - d];
                    cnt += s_cnt[cur][j][tid - d];
                }
                s_sum[cur ^ 1][j][tid] = s;
                s_cnt[cur ^ 1][j][tid] = cnt;
            }
            cur ^= 1;
            __syncthreads();
        }
        // (eight steps: cur is 0 again, and a lane's next group overwrites only its own entries of buffer 0)
        if (flushes) {                                                 // the segment's last lane holds its totals
            for (int j = 0; j < n; ++j) {
                u64 *row = a.sums + (static_cast<long long>(id) * a.ncombo + (c0 + j)) * SSRS_SCORE_ROW;
                const u64 s = s_sum[cur][j][tid], cnt = s_cnt[cur][j][tid];
                if (s != 0) atomicAdd(row, s);
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    const u64 m = (cnt >> (kScoreCountBits * k)) & ((1u << kScoreCountBits) - 1);
                    if (m != 0) atomicAdd(row + 1 + k, m);
                }
            }
        }
    }
}

}  // namespace ssrs

using namespace ssrs;

extern "C" int ssrs_tracks_score_profile(const SsrsTrackParams *params, const double *updraft, const float *potential,
                                         const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks,
                                         const int32_t *memories, int32_t nmem, const double *nus, int32_t nnu,
                                         uint64_t *rows, void *stream)
{
    SSRS_REQUIRE(params && traj && traj_offsets && memories && nus && rows,
                 "ssrs_tracks_score_profile: NULL pointer (params, traj, traj_offsets, memories, nus and rows are required)");
    SSRS_REQUIRE(updraft || !potential, "ssrs_tracks_score_profile: a potential needs an updraft (both NULL = drw)");
    SSRS_REQUIRE(ntracks >= 0 && ntracks <= INT32_MAX, "ssrs_tracks_score_profile: ntracks = %lld outside [0, 2^31)",
                 static_cast<long long>(ntracks));
    SSRS_REQUIRE(params->rows >= 3 && params->rows <= 32767 && params->cols >= 3 && params->cols <= 32767,
                 "ssrs_tracks_score_profile: a %d x %d raster (3..32767 either way)", params->rows, params->cols);
    SSRS_REQUIRE(nmem >= 1 && nmem <= SSRS_PROFILE_MAX_MEMORIES, "ssrs_tracks_score_profile: nmem = %d outside [1, %d]", nmem,
                 SSRS_PROFILE_MAX_MEMORIES);
    for (int k = 0; k < nmem; ++k) {
        SSRS_REQUIRE(memories[k] >= 1 && memories[k] <= SSRS_SCORE_MAX_MEMORY,
                     "ssrs_tracks_score_profile: memories[%d] = %d outside [1, %d] (0, the whole history, is not supported)", k,
                     memories[k], SSRS_SCORE_MAX_MEMORY);
        SSRS_REQUIRE(k == 0 || memories[k] > memories[k - 1],
                     "ssrs_tracks_score_profile: memories must ascend strictly (memories[%d] = %d after %d)", k, memories[k],
                     memories[k - 1]);
    }
    SSRS_REQUIRE(nnu >= 1 && nnu <= SSRS_PROFILE_MAX_NUS, "ssrs_tracks_score_profile: nnu = %d outside [1, %d]", nnu,
                 SSRS_PROFILE_MAX_NUS);
    for (int k = 0; k < nnu; ++k)
        SSRS_REQUIRE(nus[k] >= 0.0, "ssrs_tracks_score_profile: nus[%d] = %g (not negative, not NaN)", k, nus[k]);
    SSRS_REQUIRE(params->burnin >= 0, "ssrs_tracks_score_profile: burnin = %d is negative", params->burnin);
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(traj) & 3u) == 0, "ssrs_tracks_score_profile: traj must be 4-byte aligned");
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 7u) == 0, "ssrs_tracks_score_profile: rows must be 8-byte aligned");
    if (ntracks == 0) return SSRS_OK;
    hipStream_t st = as_stream(stream);

    // the chunk's first and last offset, on the host: the launch is sized from its points
    long long ends[2];
    SSRS_HIP_CHECK(hipMemcpyAsync(&ends[0], traj_offsets, 8, hipMemcpyDeviceToHost, st));
    SSRS_HIP_CHECK(hipMemcpyAsync(&ends[1], traj_offsets + ntracks, 8, hipMemcpyDeviceToHost, st));
    SSRS_HIP_CHECK(hipStreamSynchronize(st));
    SSRS_REQUIRE(ends[0] >= 0, "ssrs_tracks_score_profile: traj_offsets[0] = %lld is negative", ends[0]);
    SSRS_REQUIRE(ends[1] >= ends[0], "ssrs_tracks_score_profile: traj_offsets descends (%lld after %lld)", ends[1], ends[0]);
    if (ends[1] == ends[0]) return SSRS_OK;

    ProfileArgs a;
    a.traj = reinterpret_cast<const uint32_t *>(traj);
    a.off = reinterpret_cast<const long long *>(traj_offsets);
    a.ntracks = static_cast<int>(ntracks);
    a.rows = params->rows;
    a.cols = params->cols;
    a.burnin = params->burnin;
    a.nmem = nmem;
    a.nnu = nnu;
    a.ncombo = nmem * nnu;
    for (int k = 0; k < SSRS_PROFILE_MAX_MEMORIES; ++k) a.memories[k] = k < nmem ? memories[k] : 0;
    for (int k = 0; k < SSRS_PROFILE_MAX_NUS; ++k) a.nus[k] = k < nnu ? nus[k] : 0.0;
    for (int k = 0; k < 9; ++k) a.prior[k] = params->prior[k];
    a.p0 = ends[0];
    a.p1 = ends[1];
    a.updraft = updraft;
    a.potential = potential;
    a.sums = reinterpret_cast<u64 *>(rows);
    const long long ntiles = (a.p1 - (a.p0 & ~3LL) + kBlock - 1) / kBlock;
    SSRS_REQUIRE(ntiles <= INT32_MAX, "ssrs_tracks_score_profile: %lld points in one call (at most 2^31 tiles of %d)",
                 a.p1 - a.p0, kBlock);
    SSRS_HIP_CHECK(hipMemsetAsync(rows, 0, static_cast<size_t>(ntracks) * a.ncombo * SSRS_SCORE_ROW * sizeof(uint64_t), st));
    const bool vec = (reinterpret_cast<uintptr_t>(traj) & 15u) == 0;
    const dim3 grid(static_cast<unsigned>(ntiles)), block(kBlock);
    if (vec) hipLaunchKernelGGL((k_tracks_score_profile<true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_tracks_score_profile<false>), grid, block, 0, st, a);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}
