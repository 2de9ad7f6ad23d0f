// K18 -- rotor transits, and K19 -- collision risk, for gfx950 (MI355X).
//
// How many simulated flights went THROUGH each turbine's rotor disk, and which way: the disk is a circle of radius reach_t
// around the hub in the plane whose normal is the turbine's axis (the upwind unit step the host hands over), and a transit
// is a unit move of a track whose straight segment, heights interpolated linearly, meets it.  The definition, rounding by
// rounding, is in include/ssrs_hip_transits.h; K8's, K14's and K15's buffers are the inputs.  One streaming pass of 8 B a
// point (traj and alt), K15's skeleton without its cross-lane steps:
//   - a wave owns a contiguous run of 256-point spans; a lane takes four consecutive points and their heights (two 16-byte
//     loads when both buffers are 16-byte aligned, the next span's in flight while this one is worked on; point by point at
//     the chunk's ends and for unaligned buffers);
//   - the common point has no turbine near it: one lookup in the bit-per-bin mask in LDS and nothing else.  Only a point
//     of an occupied bin is looked at as the FIRST point of a move: the lane finds its track (it keeps the last one it
//     found and gallops along the offsets from there, so a long track costs one search), takes the successor -- the next
//     of its own four, or one more load of traj[i + 1] and alt[i + 1] across the lane and span cut, a line L1 / L2 hold
//     anyway and an index the move's own definition keeps inside the track --, drops ends outside the raster, jumps and
//     rests, gathers the two elevations and walks the bin's list;
//   - per turbine the plane test comes first: the division and the second half run only for moves that cross its plane;
//   - no global atomic per transit.  A lane keeps ONE pending (2 * turbine + direction, count) in registers over its
//     points and spans and hands it to the block's uint32 counters in LDS when the key changes and at its end; the block
//     adds its non-zero counters to the uint64 totals once.  Turbines past the LDS rule's limit (the header) hand over
//     with a 64-bit global add instead, still one per change of key;
//   - the bitmap is K8's: a lane remembers the last word it knows, tests an unknown one with a load from L2 and ORs only
//     news (bits are only ever set: a stale read costs a redundant atomic, never a wrong result).
// No lane talks to another lane (no shuffles, ballots or DPP); the block's lanes meet at two __syncthreads() around the
// walk.  tests/hip_host_stub runs the file on the CPU as it stands.  Integer adds and ORs: the result does not depend on
// the launch order.
//
// K19 (ssrs_rotor_collision_risk, include/ssrs_hip_collision.h) is the same walk with one more compile-time switch, kRisk:
// the test keeps the ratio lhs / rhs it compares and turns it into one of 256 equal-area rings; the transit reads its
// probability q32 from the host's table in global memory (once per transit, and transits are rare); the lane's pending
// pair carries the q32 sum beside the count and hands it to a uint64 sum beside the uint32 counter in LDS; and one more
// pending (track, q32 sum) goes to `track_risk` with one 64-bit global add when the lane's track changes and at its end.
// The instantiations without kRisk are K18's as they were.
#include <climits>
#include <cmath>

#include "common.h"
#include "rotor_disk.h"
#include "../../include/ssrs_hip_collision.h"

namespace ssrs {

constexpr int kTrnWaves = kBlock / 64;
constexpr int kTrnSpan = 256;                 // points per wave and iteration: 64 lanes x 4
constexpr long long kTrnMinSpans = 4;         // spans per wave at least (K8's figure)
constexpr int kTrnBlocks = 256 * 6;           // K8's cap: six blocks per CU
constexpr int kTrnMaskWords = 8192;           // 32 KB of LDS: rasters of up to 262 144 bins keep the mask there
constexpr int kTrnLdsWords = 15 * 1024;       // mask and counters (two uint32 a turbine) together, 60 KB
static_assert(kTrnLdsWords / 2 == SSRS_ROTOR_TRANSIT_LDS_TURBINES, "the header's LDS rule");
static_assert(kTrnLdsWords / 6 == SSRS_ROTOR_COLLISION_LDS_TURBINES, "K19's LDS rule: two uint32 and two uint64 a turbine");
static_assert(SSRS_TURBINE_BIN == 32, "a point's bin is (r >> 5, c >> 5)");

// a load that is served by L2, where the atomics land (K8's load_l2)
__device__ __forceinline__ uint32_t trn_load_l2(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct TrnArgs {
    const uint32_t *traj;          // one int16 (row, col) pair per dword
    const int32_t *alt;            // mm above ground, indexed like traj
    const long long *off;
    long long ntracks;
    long long p0, p1;              // the chunk's points: off[0], off[ntracks]
    const int32_t *cellinfo;       // {climb, elev} per cell
    int rows, cols, nbc, nbins, words;
    const double *turb, *reach, *axis;
    const int32_t *hub;
    double mm_per_cell;
    int nturb;
    const int *bin_start, *bin_items;
    uint32_t *hits;
    unsigned long long *transits;  // (nturb, 2)
    int cnt_off;                   // the block's counters: s_lds[cnt_off + 2 * turbine + direction]
    int cnt_lds;                   // turbines [0, cnt_lds) have them; the others' hand-overs go to `transits`
    // ---- K19 only
    const int32_t *cls;            // (nturb): the turbine's row of `table`; outside [0, nclass): no risk
    const uint32_t *table;         // (nclass, 2, SSRS_COLLISION_RINGS) probabilities in units of 2^-32
    int nclass;
    unsigned long long *risk;      // (nturb, 2)
    unsigned long long *track_risk;  // (ntracks) or NULL
    int sum_off;                   // the block's uint64 sums start at word s_lds[sum_off] (even), indexed like the counters
};

// The header's test of one testable move (r0, c0, z0) -> (r1, c1, z1) against turbine tb: -1 for no transit, else the
// direction.  The arithmetic is rotor_disk.h's, which K20 shares; the plane test comes first, and the turbine's reach and
// hub are read only behind it.  kRing (K19): `ring` gets the equal-area ring of the crossing point.
template <bool kRing>
__device__ __forceinline__ int trn_test(const TrnArgs &a, int tb, int r0, int c0, long long z0, int r1, int c1, long long z1,
                                        int &ring)
{
    const double xt = a.turb[2 * tb], yt = a.turb[2 * tb + 1];
    const double ax = a.axis[2 * tb], ay = a.axis[2 * tb + 1];
    RotorPlane plane;
    if (!rotor_plane_test(xt, yt, ax, ay, r0, c0, r1, c1, plane)) return -1;
    return rotor_disk_test<kRing>(plane, ax, ay, a.reach[tb], a.hub[tb], z0, z1, a.mm_per_cell, ring);
}

// The walk of one lane over its wave's spans (no barrier inside: a wave without spans returns at once).
// kVec: 16-byte loads (traj and alt are 16-byte aligned).  kMask: the occupied-bin mask is in LDS.  kRisk: K19, with the
// block's uint64 sums in s_sum.
template <bool kVec, bool kMask, bool kRisk>
__device__ __forceinline__ void trn_walk(const TrnArgs &a, const uint32_t *s_mask, uint32_t *s_cnt,
                                         unsigned long long *s_sum, const long long a0, const long long nspans,
                                         const long long per_wave)
{
    const int lane = threadIdx.x & 63, wave = static_cast<int>(threadIdx.x) >> 6;
    const long long p0 = a.p0, p1 = a.p1;
    const long long u0 = (static_cast<long long>(blockIdx.x) * kTrnWaves + wave) * per_wave;
    const long long u1 = u0 + per_wave < nspans ? u0 + per_wave : nspans;
    if (u0 >= u1) return;

    // A lane's four points of span u and their heights.  fetch: 16-byte loads without a branch around them, for spans that
    // end at or before p1 (points in front of p0 belong to the buffers: a0 >= 0; they are masked later).
    struct Fetched {
        uint4 pt;
        int4 alt;
    };
    auto fetch = [&](long long u) {
        const long long i0 = a0 + u * kTrnSpan + 4 * lane;
        Fetched f;
        f.pt = *reinterpret_cast<const uint4 *>(a.traj + i0);
        f.alt = *reinterpret_cast<const int4 *>(a.alt + i0);
        return f;
    };
    auto fetch_edge = [&](long long u) {
        const long long i0 = a0 + u * kTrnSpan + 4 * lane;
        Fetched f;
        f.pt = make_uint4(0, 0, 0, 0);
        f.alt = make_int4(0, 0, 0, 0);
        if (i0 + 0 >= p0 && i0 + 0 < p1) f.pt.x = a.traj[i0 + 0], f.alt.x = a.alt[i0 + 0];
        if (i0 + 1 >= p0 && i0 + 1 < p1) f.pt.y = a.traj[i0 + 1], f.alt.y = a.alt[i0 + 1];
        if (i0 + 2 >= p0 && i0 + 2 < p1) f.pt.z = a.traj[i0 + 2], f.alt.z = a.alt[i0 + 2];
        if (i0 + 3 >= p0 && i0 + 3 < p1) f.pt.w = a.traj[i0 + 3], f.alt.w = a.alt[i0 + 3];
        return f;
    };

    // the track the lane found last: off[t] <= the point it was found for < t_end = off[t + 1].  t_end = p0 before the
    // first search: every point of the chunk is at or past it
    long long t = 0, t_end = p0;
    // the LAST track that starts at or before point i (p0 <= i < p1, and i is at or past every point sought before):
    // doubling steps from t, then a binary search between the last two
    auto seek = [&](const long long i) {
        long long lo = t, step = 1;
        while (lo + step < a.ntracks && a.off[lo + step] <= i) {
            lo += step;
            step <<= 1;
        }
        long long hi = lo + step < a.ntracks ? lo + step : a.ntracks;      // off[hi] > i (off[ntracks] = p1)
        while (hi - lo > 1) {
            const long long mid = lo + (hi - lo) / 2;
            if (a.off[mid] <= i) lo = mid; else hi = mid;
        }
        t = lo;
        t_end = a.off[lo + 1];
    };

    // what this lane knows to be settled: the bits of one bitmap word
    long long known_word = -1;
    uint32_t known_bits = 0;
    // the transits this lane has not handed on yet: pend_cnt of key pend_key = 2 * turbine + direction
    int pend_key = 0;
    uint32_t pend_cnt = 0;
    // kRisk: their q32 sum (below 2^32 a transit, and a lane walks fewer than 2^32 moves), and the q32 sum of track
    // pend_trk that has not gone to track_risk yet
    unsigned long long pend_sum = 0, pend_trk_sum = 0;
    long long pend_trk = 0;
    auto hand_over = [&]() {
        if ((pend_key >> 1) < a.cnt_lds) {
            atomicAdd(&s_cnt[pend_key], pend_cnt);
            if constexpr (kRisk) if (pend_sum != 0) atomicAdd(&s_sum[pend_key], pend_sum);
        } else {
            atomicAdd(a.transits + pend_key, static_cast<unsigned long long>(pend_cnt));
            if constexpr (kRisk) if (pend_sum != 0) atomicAdd(a.risk + pend_key, pend_sum);
        }
        pend_cnt = 0;
        pend_sum = 0;
    };

    auto span = [&](const long long u, const Fetched cur) {
        const long long i0 = a0 + u * kTrnSpan + 4 * lane;
        const uint32_t pts[4] = {cur.pt.x, cur.pt.y, cur.pt.z, cur.pt.w};
        const int alts[4] = {cur.alt.x, cur.alt.y, cur.alt.z, cur.alt.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long i = i0 + j;
            const int r = static_cast<int16_t>(pts[j] & 0xFFFF), c = static_cast<int16_t>(pts[j] >> 16);
            if (i < p0 || i >= p1 || r < 0 || c < 0 || r >= a.rows || c >= a.cols) continue;
            const int bin = (r >> 5) * a.nbc + (c >> 5);
            if (kMask && !(s_mask[bin >> 5] >> (bin & 31) & 1u)) continue;
            const int k0 = a.bin_start[bin], k1 = a.bin_start[bin + 1];
            if (k0 >= k1) continue;
            // ---- the move that leaves point i: its track, its other end
            if (t_end <= i) seek(i);
            if (i + 1 >= t_end) continue;                                   // the track's last point
            uint32_t nw;
            int nalt;
            if (j < 3) {
                nw = pts[j + 1];
                nalt = alts[j + 1];
            } else {
                nw = a.traj[i + 1];                                         // (i + 1 < t_end <= p1)
                nalt = a.alt[i + 1];
            }
            const int r1 = static_cast<int16_t>(nw & 0xFFFF), c1 = static_cast<int16_t>(nw >> 16);
            if (r1 < 0 || c1 < 0 || r1 >= a.rows || c1 >= a.cols) continue;
            const int dr = r1 - r, dc = c1 - c;
            if (dr < -1 || dr > 1 || dc < -1 || dc > 1) continue;           // a burn-in jump
            if (dr == 0 && dc == 0) continue;                               // a rest: s_0 == s_1, never a crossing
            const int e0 = a.cellinfo[2 * (static_cast<long long>(r) * a.cols + c) + 1];
            const int e1 = a.cellinfo[2 * (static_cast<long long>(r1) * a.cols + c1) + 1];
            if (e0 == INT_MIN || e1 == INT_MIN) continue;                   // nodata under an end
            const long long z0 = static_cast<long long>(e0) + alts[j], z1 = static_cast<long long>(e1) + nalt;
            for (int k = k0; k < k1; ++k) {
                const int tb = a.bin_items[k];
                if (static_cast<unsigned>(tb) >= static_cast<unsigned>(a.nturb)) continue;
                int ring = 0;
                const int dir = trn_test<kRisk>(a, tb, r, c, z0, r1, c1, z1, ring);
                if (dir < 0) continue;
                // ---- one more transit of tb in direction dir
                const int key = 2 * tb + dir;
                if (key != pend_key && pend_cnt != 0) hand_over();
                pend_key = key;
                ++pend_cnt;
                if constexpr (kRisk) {
                    // ---- its probability, from the class's row of the table
                    const int cl = a.cls[tb];
                    if (static_cast<unsigned>(cl) < static_cast<unsigned>(a.nclass)) {
                        const unsigned long long q32 = a.table[(cl * 2 + dir) * SSRS_COLLISION_RINGS + ring];
                        pend_sum += q32;
                        if (a.track_risk) {
                            if (t != pend_trk && pend_trk_sum != 0) {
                                atomicAdd(a.track_risk + pend_trk, pend_trk_sum);
                                pend_trk_sum = 0;
                            }
                            pend_trk = t;
                            pend_trk_sum += q32;
                        }
                    }
                }
                // ---- hits: bit tb of the track's row
                const long long word = t * a.words + (tb >> 5);
                const uint32_t bit = 1u << (tb & 31);
                if (word == known_word && (known_bits & bit)) continue;
                const uint32_t seen = trn_load_l2(a.hits + word);
                known_word = word;
                known_bits = seen | bit;
                if (!(seen & bit)) atomicOr(a.hits + word, bit);
            }
        }
    };

    // Spans that end at or before p1 stream through 16-byte loads, one span ahead; the last span of the data, and every
    // span of an unaligned buffer, go point by point (K8's loop).
    long long u = u0;
    if (kVec) {
        const long long whole = (p1 - a0) / kTrnSpan;
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
    if (pend_cnt != 0) hand_over();
    if constexpr (kRisk) if (pend_trk_sum != 0) atomicAdd(a.track_risk + pend_trk, pend_trk_sum);
}

template <bool kVec, bool kMask, bool kRisk>
__global__ __launch_bounds__(kBlock) void k_rotor_transits(const TrnArgs a)
{
    // the mask (kMask), then two counters a turbine below cnt_lds, then (kRisk) two uint64 sums a turbine
    extern __shared__ uint32_t s_trn_lds[];

    // spans are cut at multiples of four points of the BUFFER, so that a lane's four points are one aligned load
    const long long a0 = a.p0 & ~3LL;
    const long long nspans = (a.p1 - a0 + kTrnSpan - 1) / kTrnSpan;
    const long long nwaves = static_cast<long long>(gridDim.x) * kTrnWaves;
    long long per_wave = (nspans + nwaves - 1) / nwaves;
    per_wave = per_wave < kTrnMinSpans ? kTrnMinSpans : per_wave;
    if (static_cast<long long>(blockIdx.x) * kTrnWaves * per_wave >= nspans) return;      // (the whole block)

    if (kMask) {
        for (int w = threadIdx.x; w < (a.nbins + 31) / 32; w += kBlock) {
            uint32_t bits = 0;
            const int b0 = w * 32, b1 = b0 + 32 < a.nbins ? b0 + 32 : a.nbins;
            int lo = a.bin_start[b0];
            for (int b = b0; b < b1; ++b) {
                const int hi = a.bin_start[b + 1];
                bits |= hi > lo ? 1u << (b - b0) : 0u;
                lo = hi;
            }
            s_trn_lds[w] = bits;
        }
    }
    // the block's counters, uint32: a block walks far fewer than 2^32 moves
    uint32_t *const s_cnt = s_trn_lds + a.cnt_off;
    for (int k = threadIdx.x; k < 2 * a.cnt_lds; k += kBlock) s_cnt[k] = 0;
    unsigned long long *const s_sum = kRisk ? reinterpret_cast<unsigned long long *>(s_trn_lds + a.sum_off) : nullptr;
    if constexpr (kRisk)
        for (int k = threadIdx.x; k < 2 * a.cnt_lds; k += kBlock) s_sum[k] = 0;
    __syncthreads();

    trn_walk<kVec, kMask, kRisk>(a, s_trn_lds, s_cnt, s_sum, a0, nspans, per_wave);

    // every wave of the block arrives here: one 64-bit add per (turbine, direction) the block met
    __syncthreads();
    for (int k = threadIdx.x; k < 2 * a.cnt_lds; k += kBlock)
        if (s_cnt[k] != 0) atomicAdd(a.transits + k, static_cast<unsigned long long>(s_cnt[k]));
    if constexpr (kRisk)
        for (int k = threadIdx.x; k < 2 * a.cnt_lds; k += kBlock)
            if (s_sum[k] != 0) atomicAdd(a.risk + k, s_sum[k]);
}

// blocks of a launch over the points [p0, p1): enough for kTrnMinSpans spans a wave, K8's cap at most
inline unsigned trn_grid(long long p0, long long p1)
{
    const long long nspans = (p1 - (p0 & ~3LL) + kTrnSpan - 1) / kTrnSpan;
    const long long per_block = kTrnWaves * kTrnMinSpans;
    const long long blocks = (nspans + per_block - 1) / per_block;
    return static_cast<unsigned>(blocks < 1 ? 1 : blocks > kTrnBlocks ? kTrnBlocks : blocks);
}

}  // namespace ssrs

using namespace ssrs;

// Both exports: the checks, the chunk's ends, the LDS rule and the launch.  kRisk: K19, with its five arguments.
template <bool kRisk>
static int trn_call(const char *who, const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks, const int32_t *alt,
                    const int32_t *cellinfo, int rows, int cols, const double *turbines, const double *reach,
                    const int32_t *hub, const double *axis, double mm_per_cell, int nturb, const int32_t *bin_start,
                    const int32_t *bin_items, uint32_t *hits, uint64_t *transits, const int32_t *cls, const uint32_t *table,
                    int nclass, uint64_t *risk, uint64_t *track_risk, void *stream)
{
    SSRS_REQUIRE(traj && traj_offsets && alt && cellinfo && turbines && reach && bin_start && bin_items && hits,
                 "%s: NULL pointer", who);
    SSRS_REQUIRE(hub && axis && transits, "%s: NULL pointer (hub, axis and transits are required)", who);
    SSRS_REQUIRE(ntracks >= 0 && ntracks <= INT32_MAX, "%s: ntracks = %lld outside [0, 2^31)", who,
                 static_cast<long long>(ntracks));
    SSRS_REQUIRE(nturb >= 1 && nturb <= SSRS_TURBINE_MAX, "%s: nturb = %d outside [1, %d]", who, nturb, SSRS_TURBINE_MAX);
    SSRS_REQUIRE(rows >= 1 && rows <= 32767 && cols >= 1 && cols <= 32767,
                 "%s: a %d x %d raster (int16 points: 1..32767 either way)", who, rows, cols);
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(traj) & 3u) == 0 && (reinterpret_cast<uintptr_t>(alt) & 3u) == 0,
                 "%s: traj and alt must be 4-byte aligned", who);
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(cellinfo) & 7u) == 0, "%s: cellinfo must be 8-byte aligned", who);
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(transits) & 7u) == 0 && (reinterpret_cast<uintptr_t>(axis) & 7u) == 0,
                 "%s: transits and axis must be 8-byte aligned", who);
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(hub) & 3u) == 0, "%s: hub must be 4-byte aligned", who);
    SSRS_REQUIRE(std::isfinite(mm_per_cell) && mm_per_cell > 0.0, "%s: mm_per_cell = %g (finite and > 0)", who, mm_per_cell);
    if (kRisk) {
        SSRS_REQUIRE(cls && table && risk, "%s: NULL pointer (cls, table and risk are required)", who);
        SSRS_REQUIRE(nclass >= 1, "%s: nclass = %d (at least one class)", who, nclass);
        SSRS_REQUIRE((reinterpret_cast<uintptr_t>(cls) & 3u) == 0 && (reinterpret_cast<uintptr_t>(table) & 3u) == 0,
                     "%s: cls and table must be 4-byte aligned", who);
        SSRS_REQUIRE((reinterpret_cast<uintptr_t>(risk) & 7u) == 0 && (reinterpret_cast<uintptr_t>(track_risk) & 7u) == 0,
                     "%s: risk and track_risk must be 8-byte aligned", who);
    }
    if (ntracks == 0) return SSRS_OK;
    hipStream_t st = as_stream(stream);

    // the chunk's first and last offset, on the host: the launch is sized from its points
    long long ends[2];
    SSRS_HIP_CHECK(hipMemcpyAsync(&ends[0], traj_offsets, 8, hipMemcpyDeviceToHost, st));
    SSRS_HIP_CHECK(hipMemcpyAsync(&ends[1], traj_offsets + ntracks, 8, hipMemcpyDeviceToHost, st));
    SSRS_HIP_CHECK(hipStreamSynchronize(st));
    SSRS_REQUIRE(ends[0] >= 0, "%s: traj_offsets[0] = %lld is negative", who, ends[0]);
    SSRS_REQUIRE(ends[1] >= ends[0], "%s: traj_offsets descends (%lld after %lld)", who, ends[1], ends[0]);
    if (ends[1] == ends[0]) return SSRS_OK;

    TrnArgs a = {};
    a.traj = reinterpret_cast<const uint32_t *>(traj);
    a.alt = alt;
    a.off = reinterpret_cast<const long long *>(traj_offsets);
    a.ntracks = ntracks;
    a.p0 = ends[0];
    a.p1 = ends[1];
    a.cellinfo = cellinfo;
    a.rows = rows;
    a.cols = cols;
    a.nbc = (cols + SSRS_TURBINE_BIN - 1) / SSRS_TURBINE_BIN;
    a.nbins = (rows + SSRS_TURBINE_BIN - 1) / SSRS_TURBINE_BIN * a.nbc;
    a.words = (nturb + 31) / 32;
    a.turb = turbines;
    a.reach = reach;
    a.axis = axis;
    a.hub = hub;
    a.mm_per_cell = mm_per_cell;
    a.nturb = nturb;
    a.bin_start = bin_start;
    a.bin_items = bin_items;
    a.hits = hits;
    a.transits = reinterpret_cast<unsigned long long *>(transits);
    a.cls = cls;
    a.table = table;
    a.nclass = nclass;
    a.risk = reinterpret_cast<unsigned long long *>(risk);
    a.track_risk = reinterpret_cast<unsigned long long *>(track_risk);
    // the headers' LDS rule: the mask stays while it and every turbine's counters fit the 60 KB; without it the counters of
    // the first SSRS_ROTOR_TRANSIT_LDS_TURBINES (K19: SSRS_ROTOR_COLLISION_LDS_TURBINES) turbines do.  A turbine has two
    // uint32 counters and, in K19, two uint64 sums behind all counters; K19 pads the mask to an even number of words
    constexpr int per_turbine = kRisk ? 6 : 2;
    constexpr int lds_turbines = kRisk ? SSRS_ROTOR_COLLISION_LDS_TURBINES : SSRS_ROTOR_TRANSIT_LDS_TURBINES;
    const int mask_words = (a.nbins + 31) / 32;
    const int mask_room = kRisk ? (mask_words + 1) & ~1 : mask_words;
    const bool mask = mask_words <= kTrnMaskWords && mask_room + per_turbine * nturb <= kTrnLdsWords;
    a.cnt_off = mask ? mask_room : 0;
    a.cnt_lds = mask || nturb < lds_turbines ? nturb : lds_turbines;
    a.sum_off = a.cnt_off + 2 * a.cnt_lds;
    const size_t lds = static_cast<size_t>(a.cnt_off + per_turbine * a.cnt_lds) * 4;
    const bool vec = ((reinterpret_cast<uintptr_t>(traj) | reinterpret_cast<uintptr_t>(alt)) & 15u) == 0;
    const dim3 grid(trn_grid(a.p0, a.p1)), block(kBlock);
    if (vec && mask) hipLaunchKernelGGL((k_rotor_transits<true, true, kRisk>), grid, block, lds, st, a);
    else if (vec) hipLaunchKernelGGL((k_rotor_transits<true, false, kRisk>), grid, block, lds, st, a);
    else if (mask) hipLaunchKernelGGL((k_rotor_transits<false, true, kRisk>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((k_rotor_transits<false, false, kRisk>), grid, block, lds, st, a);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

extern "C" int ssrs_rotor_transits(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks, const int32_t *alt,
                                   const int32_t *cellinfo, int rows, int cols, const double *turbines, const double *reach,
                                   const int32_t *hub, const double *axis, double mm_per_cell, int nturb,
                                   const int32_t *bin_start, const int32_t *bin_items, uint32_t *hits, uint64_t *transits,
                                   void *stream)
{
    return trn_call<false>("ssrs_rotor_transits", traj, traj_offsets, ntracks, alt, cellinfo, rows, cols, turbines, reach, hub,
                           axis, mm_per_cell, nturb, bin_start, bin_items, hits, transits, nullptr, nullptr, 0, nullptr,
                           nullptr, stream);
}

extern "C" int ssrs_rotor_collision_risk(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks,
                                         const int32_t *alt, const int32_t *cellinfo, int rows, int cols,
                                         const double *turbines, const double *reach, const int32_t *hub, const double *axis,
                                         double mm_per_cell, int nturb, const int32_t *bin_start, const int32_t *bin_items,
                                         uint32_t *hits, uint64_t *transits, const int32_t *cls, const uint32_t *table,
                                         int nclass, uint64_t *risk, uint64_t *track_risk, void *stream)
{
    return trn_call<true>("ssrs_rotor_collision_risk", traj, traj_offsets, ntracks, alt, cellinfo, rows, cols, turbines, reach,
                          hub, axis, mm_per_cell, nturb, bin_start, bin_items, hits, transits, cls, table, nclass, risk,
                          track_risk, stream);
}
