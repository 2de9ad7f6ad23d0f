// K17 -- track passage for gfx950 (MI355X).
//
// How many DISTINCT tracks came within a radius of each cell: with D = {(dr, dc) : dr*dr + dc*dc <= r2},
// counts[r, c] += 1 for every track with at least one in-raster point p such that (r, c) - p is in D.  It is K8's
// tracks_per_turbine evaluated at every cell centre, and K13 (occupancy.hip) with a disk where K13 has a cell; r2 = 0 IS
// K13.  The skeleton is K13's, and so are the words of its comment that are not repeated here:
//   - rounds of 32 * planes consecutive tracks, track k of a round on bit k & 31 of plane k >> 5 of the workspace;
//   - a round's points are one contiguous range of traj; a wave owns a run of 256-point spans, a lane four consecutive
//     points (one 16-byte load when the buffer is 16-byte aligned, the next span's load in flight while this one is
//     worked on); unaligned ends and unaligned buffers go point by point;
//   - the round's offsets (at most 257) in LDS, one binary search a lane, then a walk over empty tracks and track ends.
// What differs is what a point sets: a FIXED set of cells that depends on the point p and on its predecessor q in the
// track only (for a lane's first point one more dword, traj[i - 1], used when that index is still inside the track):
//   - p outside the raster: nothing;
//   - p the first point of its track, q outside the raster, or q in the raster more than one cell away (a burn-in
//     jump): the whole disk p + D;
//   - p == q (a rest): nothing;
//   - a unit move: the crescent (p + D) \ (q + D), O(sqrt(r2)) cells, built row by row from the disk's half-widths
//     w(dy) = isqrt(r2 - dy*dy), which every block derives from r2 into LDS.
// By induction along a track the union over its points is the union of its disks (q's disk is covered when q is in the
// raster, and p + D = crescent + what it shares with q + D), whichever lane does which point and whenever: the sets are
// fixed, the bits are only ever set.  Every cell of a set goes K13's way: the L2 load tests the bit, a clear bit is
// old = atomicOr(word, bit), and the one lane that gets !(old & bit) back adds 1 to counts and to its sum for
// cells_per_track.  No fences; kernel boundaries on the stream are all the ordering there is.
//   - the memo: a lane remembers the last two distinct unit moves (q, p) it worked on within the current track and skips
//     a move that equals either -- a track that ping-pongs in a trap costs a lane two crescents, not one a move.  It
//     skips only work this lane has done for this track in this kernel, so nothing depends on it;
//   - the workspace is scratch: the call clears a round's planes itself BEFORE that round's set kernel, the first
//     round's by a memset, a later round's by whichever moves fewer bytes, a memset of its planes or the "unset" kernel,
//     the previous round's walk storing 0 to every word it tested (pas_unset_bytes is the bound that decides);
//   - stats (optional): every lane of a set kernel adds the mask words it tested and the bits it won, once, at its end.
// No lane talks to another lane (no shuffles, ballots or DPP): tests/hip_host_stub runs the file on the CPU as it stands.
#include <climits>
#include <cmath>
#include <vector>

#include "common.h"
#include "../../include/ssrs_hip_passage.h"

namespace ssrs {

constexpr int kPasWaves = kBlock / 64;
constexpr int kPasSpan = 256;                 // points per wave and iteration: 64 lanes x 4
constexpr long long kPasMinSpans = 4;         // spans per wave at least (K13's figure)
constexpr int kPasBlocks = 256 * 6;           // K13's cap: six blocks per CU
constexpr int kPasRoundMax = 32 * SSRS_PASSAGE_MAX_PLANES;
constexpr int kPasWidths = SSRS_PASSAGE_MAX_RADIUS + 1;

// a load that is served by L2, where the atomics land (K13's occ_load_l2)
__device__ __forceinline__ uint32_t pas_load_l2(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// floor(sqrt(x)) of 0 <= x <= 255 * 255 (exact in f32; the two loops are there for the rounding of sqrtf all the same)
__host__ __device__ inline int pas_isqrt(int x)
{
    int w = static_cast<int>(sqrtf(static_cast<float>(x)));
    while (w * w > x) --w;
    while ((w + 1) * (w + 1) <= x) ++w;
    return w;
}

// Row dy (|dy| <= reach) of the crescent (p + D) \ (q + D) for p = q + (mr, mc), in columns relative to p: the row's
// interval [-w(dy), w(dy)] less q's interval of the same raster row, [-w(dy + mr) - mc, w(dy + mr) - mc] -- at most two
// ranges, [lo0, hi0] and [lo1, hi1], each empty when lo > hi, and disjoint.  `w` holds w(0..reach).
struct PasRow {
    int lo0, hi0, lo1, hi1;
};
__host__ __device__ inline PasRow pas_crescent_row(const uint8_t *w, int reach, int dy, int mr, int mc)
{
    const int wp = w[dy < 0 ? -dy : dy];
    const int e = dy + mr, ae = e < 0 ? -e : e;
    if (ae > reach) return PasRow{-wp, wp, 1, 0};                 // q's disk has no such row
    const int wq = w[ae];
    const int left = -wq - mc - 1, right = wq - mc + 1;
    return PasRow{-wp, left < wp ? left : wp, right > -wp ? right : -wp, wp};
}

struct PasArgs {
    const uint32_t *traj;          // one int16 (row, col) pair per dword
    const long long *off;          // the round's offsets: ntr + 1 of them
    int ntr;                       // tracks of the round, 1..kPasRoundMax
    int rows, cols;
    int r2, reach;                 // reach = isqrt(r2): the disk's rows are -reach..reach
    long long plane_words;         // rows * cols
    uint32_t *mask;                // the workspace: planes x rows x cols
    uint32_t *counts;              // (rows, cols)
    uint32_t *per_track;           // the round's first entry of cells_per_track, or nullptr
    unsigned long long *stats;     // [words tested, bits won], or nullptr
};

// blocks of a launch over the points [p0, p1): occ_grid's rule
inline unsigned pas_grid(long long p0, long long p1)
{
    const long long nspans = (p1 - (p0 & ~3LL) + kPasSpan - 1) / kPasSpan;
    const long long per_block = kPasWaves * kPasMinSpans;
    const long long blocks = (nspans + per_block - 1) / per_block;
    return static_cast<unsigned>(blocks < 1 ? 1 : blocks > kPasBlocks ? kPasBlocks : blocks);
}

// |D| and the largest of the eight crescents, from the half-widths
inline void pas_disk_sizes(int r2, long long *disk, long long *crescent)
{
    const int reach = pas_isqrt(r2);
    uint8_t w[kPasWidths];
    for (int i = 0; i <= reach; ++i) w[i] = static_cast<uint8_t>(pas_isqrt(r2 - i * i));
    *disk = 0;
    for (int dy = -reach; dy <= reach; ++dy) *disk += 2 * w[dy < 0 ? -dy : dy] + 1;
    *crescent = 0;
    for (int mr = -1; mr <= 1; ++mr)
        for (int mc = -1; mc <= 1; ++mc) {
            if (mr == 0 && mc == 0) continue;
            long long n = 0;
            for (int dy = -reach; dy <= reach; ++dy) {
                const PasRow x = pas_crescent_row(w, reach, dy, mr, mc);
                n += (x.hi0 >= x.lo0 ? x.hi0 - x.lo0 + 1 : 0) + (x.hi1 >= x.lo1 ? x.hi1 - x.lo1 + 1 : 0);
            }
            *crescent = n > *crescent ? n : *crescent;
        }
}

// The most bytes the unset kernel of a round of `points` points in `ntr` tracks can move: it reads every point, and
// stores 4 bytes to a whole disk for a track's first point at worst and to a crescent for every other point.  (Jumps
// and points after an out-of-raster one set whole disks as well; the stepper makes one jump a track, and the bound is
// a rule for choosing between two correct ways to clear, not a promise.)
inline unsigned long long pas_unset_bytes(long long points, int ntr, long long disk, long long crescent)
{
    return static_cast<unsigned long long>(points) * 4ull * static_cast<unsigned long long>(1 + crescent) +
           static_cast<unsigned long long>(ntr) * 4ull * static_cast<unsigned long long>(disk);
}

// kVec: 16-byte loads (traj is 16-byte aligned).  kSet: set the bits and count; otherwise store 0 to the same words.
template <bool kVec, bool kSet>
__global__ __launch_bounds__(kBlock) void k_track_passage(const PasArgs a)
{
    __shared__ long long s_off[kPasRoundMax + 1];
    __shared__ uint8_t s_w[kPasWidths];
    for (int i = threadIdx.x; i <= a.ntr; i += kBlock) s_off[i] = a.off[i];
    for (int i = threadIdx.x; i <= a.reach; i += kBlock) s_w[i] = static_cast<uint8_t>(pas_isqrt(a.r2 - i * i));
    __syncthreads();                             // (the only barrier: the returns below are behind it)

    const long long p0 = s_off[0], p1 = s_off[a.ntr];
    if (p0 < 0 || p1 <= p0) return;
    // spans are cut at multiples of four points of the BUFFER, so that a lane's four points are one aligned load
    const long long a0 = p0 & ~3LL;
    const long long nspans = (p1 - a0 + kPasSpan - 1) / kPasSpan;
    const long long nwaves = static_cast<long long>(gridDim.x) * kPasWaves;
    long long per_wave = (nspans + nwaves - 1) / nwaves;
    per_wave = per_wave < kPasMinSpans ? kPasMinSpans : per_wave;
    const int lane = threadIdx.x & 63, wave = static_cast<int>(threadIdx.x) >> 6;
    const long long u0 = (static_cast<long long>(blockIdx.x) * kPasWaves + wave) * per_wave;
    const long long u1 = u0 + per_wave < nspans ? u0 + per_wave : nspans;
    if (u0 >= u1) return;

    // the track that holds this lane's first point: the LAST one that starts at or before it (K13's search)
    int t = 0;
    {
        const long long first = a0 + u0 * kPasSpan + 4 * lane;
        const long long key = first > p0 ? first : p0;
        int lo = 0, hi = a.ntr;
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (s_off[mid] <= key) lo = mid; else hi = mid;
        }
        t = lo;
    }
    long long t_begin = s_off[t], t_end = s_off[t + 1];
    uint32_t mine = 0;                           // cells that this lane was the first to set for track t
    unsigned long long tested = 0, won = 0;      // this lane's share of stats
    // the memo: the last two distinct unit moves of track t this lane worked on.  A move has q != p, so (0, 0) is none.
    uint32_t memo_q0 = 0, memo_p0 = 0, memo_q1 = 0, memo_p1 = 0;

    struct Fetched {
        uint4 v;
        uint32_t before;                         // traj[i0 - 1], or 0 where that is not a point of the round
    };
    auto fetch = [&](long long u) {
        const long long i0 = a0 + u * kPasSpan + 4 * lane;
        Fetched f;
        f.before = i0 - 1 >= p0 ? a.traj[i0 - 1] : 0u;
        f.v = *reinterpret_cast<const uint4 *>(a.traj + i0);
        return f;
    };
    auto fetch_edge = [&](long long u) {
        const long long i0 = a0 + u * kPasSpan + 4 * lane;
        Fetched f;
        f.before = (i0 - 1 >= p0 && i0 - 1 < p1) ? a.traj[i0 - 1] : 0u;
        f.v = make_uint4(0, 0, 0, 0);
        if (i0 + 0 >= p0 && i0 + 0 < p1) f.v.x = a.traj[i0 + 0];
        if (i0 + 1 >= p0 && i0 + 1 < p1) f.v.y = a.traj[i0 + 1];
        if (i0 + 2 >= p0 && i0 + 2 < p1) f.v.z = a.traj[i0 + 2];
        if (i0 + 3 >= p0 && i0 + 3 < p1) f.v.w = a.traj[i0 + 3];
        return f;
    };

    // the cells [c_lo, c_hi] of raster row rr, clipped to the raster, on track t's bit
    auto touch_row = [&](const int rr, int c_lo, int c_hi) {
        c_lo = c_lo < 0 ? 0 : c_lo;
        c_hi = c_hi >= a.cols ? a.cols - 1 : c_hi;
        if (c_lo > c_hi) return;
        const int cell0 = rr * a.cols;
        uint32_t *plane = a.mask + (t >> 5) * a.plane_words;
        const uint32_t bit = 1u << (t & 31);
        for (int cell = cell0 + c_lo; cell <= cell0 + c_hi; ++cell) {
            if (kSet) {
                ++tested;
                if (pas_load_l2(plane + cell) & bit) continue;
                const uint32_t old = atomicOr(plane + cell, bit);
                if (!(old & bit)) {
                    atomicAdd(a.counts + cell, 1u);
                    ++mine;
                    ++won;
                }
            } else {
                plane[cell] = 0u;
            }
        }
    };

    auto span = [&](const long long u, const Fetched cur) {
        const long long i0 = a0 + u * kPasSpan + 4 * lane;
        const uint32_t pts[5] = {cur.before, cur.v.x, cur.v.y, cur.v.z, cur.v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long i = i0 + j;
            if (i < p0 || i >= p1) continue;
            // (i < p1 = s_off[ntr]: the walk stops at a track below ntr)
            while (t_end <= i) {
                if (kSet && mine != 0 && a.per_track != nullptr) atomicAdd(a.per_track + t, mine);
                mine = 0;
                memo_q0 = memo_p0 = memo_q1 = memo_p1 = 0;
                ++t;
                t_begin = t_end;
                t_end = s_off[t + 1];
            }
            const uint32_t pw = pts[j + 1];
            const int r = static_cast<int16_t>(pw & 0xFFFF), c = static_cast<int16_t>(pw >> 16);
            if (r < 0 || c < 0 || r >= a.rows || c >= a.cols) continue;
            // the predecessor, when the track has one: pts[j] is traj[i - 1] (i - 1 >= t_begin >= p0, so it was loaded)
            bool whole = true;
            int mr = 0, mc = 0;
            if (i - 1 >= t_begin) {
                const uint32_t qw = pts[j];
                const int qr = static_cast<int16_t>(qw & 0xFFFF), qc = static_cast<int16_t>(qw >> 16);
                if (qr >= 0 && qc >= 0 && qr < a.rows && qc < a.cols) {
                    mr = r - qr;
                    mc = c - qc;
                    if (mr == 0 && mc == 0) continue;                                   // a rest
                    if (mr >= -1 && mr <= 1 && mc >= -1 && mc <= 1) {
                        if ((qw == memo_q0 && pw == memo_p0) || (qw == memo_q1 && pw == memo_p1)) continue;
                        memo_q1 = memo_q0;
                        memo_p1 = memo_p0;
                        memo_q0 = qw;
                        memo_p0 = pw;
                        whole = false;
                    }
                }
            }
            const int dy_lo = -a.reach < -r ? -r : -a.reach;
            const int dy_hi = a.reach > a.rows - 1 - r ? a.rows - 1 - r : a.reach;
            if (whole) {
                for (int dy = dy_lo; dy <= dy_hi; ++dy) {
                    const int w = s_w[dy < 0 ? -dy : dy];
                    touch_row(r + dy, c - w, c + w);
                }
            } else {
                for (int dy = dy_lo; dy <= dy_hi; ++dy) {
                    const PasRow x = pas_crescent_row(s_w, a.reach, dy, mr, mc);
                    touch_row(r + dy, c + x.lo0, c + x.hi0);
                    touch_row(r + dy, c + x.lo1, c + x.hi1);
                }
            }
        }
    };

    // Spans that end at or before p1 stream through 16-byte loads, one span ahead; the last span of the data, and
    // every span of an unaligned buffer, go point by point (K13's loop).
    long long u = u0;
    if (kVec) {
        const long long whole = (p1 - a0) / kPasSpan;
        const long long u_vec = u1 < whole ? u1 : whole;
        if (u < u_vec) {
            Fetched next = fetch(u);
            for (; u < u_vec; ++u) {
                const Fetched cur = next;
                next = fetch(u + 1 < u_vec ? u + 1 : u);
                span(u, cur);
            }
        }
    }
    for (; u < u1; ++u) span(u, fetch_edge(u));
    if (kSet && mine != 0 && a.per_track != nullptr) atomicAdd(a.per_track + t, mine);
    if (kSet && a.stats != nullptr) {
        if (tested != 0) atomicAdd(a.stats + 0, tested);
        if (won != 0) atomicAdd(a.stats + 1, won);
    }
}

template <bool kSet>
static void pas_launch(const PasArgs &a, bool vec, unsigned blocks, hipStream_t st)
{
    const dim3 grid(blocks), block(kBlock);
    if (vec) hipLaunchKernelGGL((k_track_passage<true, kSet>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_track_passage<false, kSet>), grid, block, 0, st, a);
}

}  // namespace ssrs

using namespace ssrs;

extern "C" size_t ssrs_track_passage_workspace_bytes(int rows, int cols, int planes)
{
    if (rows < 1 || cols < 1 || planes < 1) return 0;
    const size_t bytes = static_cast<size_t>(rows) * static_cast<size_t>(cols) * 4 * static_cast<size_t>(planes);
    return (bytes + 255) / 256 * 256;
}

extern "C" int ssrs_track_passage(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks, int rows, int cols,
                                  int64_t r2, int planes, uint32_t *counts, uint32_t *cells_per_track, uint64_t *stats,
                                  void *workspace, size_t workspace_bytes, void *stream)
{
    SSRS_REQUIRE(traj && traj_offsets && counts && workspace, "ssrs_track_passage: NULL pointer");
    SSRS_REQUIRE(planes >= 1 && planes <= SSRS_PASSAGE_MAX_PLANES, "ssrs_track_passage: planes = %d outside [1, %d]",
                 planes, SSRS_PASSAGE_MAX_PLANES);
    SSRS_REQUIRE(rows >= 1 && rows <= 32767 && cols >= 1 && cols <= 32767,
                 "ssrs_track_passage: a %d x %d raster (int16 points: 1..32767 either way)", rows, cols);
    SSRS_REQUIRE(r2 >= 0 && r2 <= static_cast<int64_t>(SSRS_PASSAGE_MAX_RADIUS) * SSRS_PASSAGE_MAX_RADIUS,
                 "ssrs_track_passage: r2 = %lld outside [0, %d * %d]", static_cast<long long>(r2), SSRS_PASSAGE_MAX_RADIUS,
                 SSRS_PASSAGE_MAX_RADIUS);
    // (as ssrs_track_occupancy: the kernel keeps track numbers as int)
    SSRS_REQUIRE(ntracks >= 0 && ntracks <= INT32_MAX, "ssrs_track_passage: ntracks = %lld outside [0, 2^31)",
                 static_cast<long long>(ntracks));
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(traj) & 3u) == 0, "ssrs_track_passage: traj must be 4-byte aligned");
    SSRS_REQUIRE(workspace_bytes >= ssrs_track_passage_workspace_bytes(rows, cols, planes),
                 "ssrs_track_passage: workspace of %zu bytes, %zu needed for %d planes of %d x %d", workspace_bytes,
                 ssrs_track_passage_workspace_bytes(rows, cols, planes), planes, rows, cols);
    if (ntracks == 0) return SSRS_OK;
    hipStream_t st = as_stream(stream);

    // the offsets at the round borders, on the host: every launch is sized from its round's points
    const long long round_tracks = 32LL * planes;
    const long long nrounds = (ntracks + round_tracks - 1) / round_tracks;
    std::vector<long long> border(static_cast<size_t>(nrounds) + 1);
    SSRS_HIP_CHECK(hipMemcpy2DAsync(border.data(), 8, traj_offsets, static_cast<size_t>(round_tracks) * 8, 8,
                                    static_cast<size_t>(nrounds), hipMemcpyDeviceToHost, st));
    SSRS_HIP_CHECK(hipMemcpyAsync(&border[nrounds], traj_offsets + ntracks, 8, hipMemcpyDeviceToHost, st));
    SSRS_HIP_CHECK(hipStreamSynchronize(st));
    SSRS_REQUIRE(border[0] >= 0, "ssrs_track_passage: traj_offsets[0] = %lld is negative", border[0]);
    for (long long k = 0; k < nrounds; ++k)
        SSRS_REQUIRE(border[k + 1] >= border[k], "ssrs_track_passage: traj_offsets descends (%lld after %lld)",
                     border[k + 1], border[k]);

    long long disk = 0, crescent = 0;
    pas_disk_sizes(static_cast<int>(r2), &disk, &crescent);
    PasArgs a;
    a.traj = reinterpret_cast<const uint32_t *>(traj);
    a.rows = rows;
    a.cols = cols;
    a.r2 = static_cast<int>(r2);
    a.reach = pas_isqrt(a.r2);
    a.plane_words = static_cast<long long>(rows) * cols;
    a.mask = static_cast<uint32_t *>(workspace);
    a.counts = counts;
    a.stats = reinterpret_cast<unsigned long long *>(stats);
    const bool vec = (reinterpret_cast<uintptr_t>(traj) & 15u) == 0;
    bool have_prev = false;
    PasArgs prev = a;                                                 // the last round that ran a set kernel
    unsigned prev_blocks = 0;
    long long prev_points = 0;
    for (long long k = 0; k < nrounds; ++k) {
        const long long p0 = border[k], p1 = border[k + 1];
        if (p1 <= p0) continue;                                       // (a round of empty tracks)
        const long long t0 = k * round_tracks;
        a.off = reinterpret_cast<const long long *>(traj_offsets) + t0;
        a.ntr = static_cast<int>(ntracks - t0 < round_tracks ? ntracks - t0 : round_tracks);
        a.per_track = cells_per_track ? cells_per_track + t0 : nullptr;
        // clearing, before the set kernel: this round's planes by a memset, or every word the round before tested by
        // its unset walk (that round had as many planes at least, and the first memset covered them all)
        const size_t used_bytes = static_cast<size_t>((a.ntr + 31) / 32) * static_cast<size_t>(a.plane_words) * 4;
        if (have_prev && pas_unset_bytes(prev_points, prev.ntr, disk, crescent) < used_bytes)
            pas_launch<false>(prev, vec, prev_blocks, st);
        else
            SSRS_HIP_CHECK(hipMemsetAsync(workspace, 0, used_bytes, st));
        const unsigned blocks = pas_grid(p0, p1);
        pas_launch<true>(a, vec, blocks, st);
        have_prev = true;
        prev = a;
        prev_blocks = blocks;
        prev_points = p1 - p0;
    }
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}
