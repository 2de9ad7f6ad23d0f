// K13 -- track occupancy for gfx950 (MI355X).
//
// How many DISTINCT tracks passed through each cell: counts[r, c] += 1 for every track with at least one point (r, c),
// from the trajectories the stepper leaves on the device.  The visit histogram cannot give it (a track that loiters in
// a trap cell for 1.7e4 moves is 1.7e4 visits and one track).
//   - tracks are taken in rounds of 32 * planes consecutive tracks; track k of a round owns bit k & 31 of plane k >> 5
//     of the workspace, `planes` uint32 rasters that are zero between rounds;
//   - a round's points are one contiguous range of traj.  The "set" kernel streams it as K8 does: a wave owns a
//     contiguous run of 256-point spans, a lane takes four consecutive points (one 16-byte load when the buffer is
//     16-byte aligned, the next span's load issued before this one is worked on);
//   - the round's offsets (at most 257) sit in LDS.  A lane finds the track of its first point by one binary search
//     and then advances along them, over empty tracks and over track ends inside its four points;
//   - an in-raster point tests its bit with an L2 load first: a set bit costs nothing more (bits are only ever set
//     inside the kernel, so a stale read costs a redundant atomic, never a wrong count) -- a track that ping-pongs in a
//     trap for millions of moves is one load a point.  Otherwise old = atomicOr(word, bit), and the ONE lane that gets
//     !(old & bit) back is the track's first visit to the cell: it alone adds 1 to counts and to its own sum for
//     cells_per_track.  Any number of lanes of any waves may race for a bit; the returned old value picks one;
//   - a lane adds its sum to cells_per_track once per track it worked on (and only when it is not 0);
//   - the round's bits are cleared by whichever moves fewer bytes: the "unset" kernel, the same walk storing 0 to
//     every touched word, or a memset of the round's planes.
// No lane talks to another lane (no shuffles, ballots or DPP): the walk is per-lane code, which tests/hip_host_stub runs
// on the CPU as it stands.  The mask words are touched by atomics, L2 loads and whole-kernel zeroing only, so kernel
// boundaries are all the ordering there is; integer ORs and adds: the result does not depend on the launch order.
#include <climits>
#include <vector>

#include "common.h"

namespace ssrs {

constexpr int kOccWaves = kBlock / 64;
constexpr int kOccSpan = 256;                 // points per wave and iteration: 64 lanes x 4
constexpr long long kOccMinSpans = 4;         // spans per wave at least (K8's figure)
constexpr int kOccBlocks = 256 * 6;           // K8's cap: six blocks per CU
constexpr int kOccRoundMax = 32 * SSRS_OCCUPANCY_MAX_PLANES;

// a load that is served by L2, where the atomics land (K8's load_l2)
__device__ __forceinline__ uint32_t occ_load_l2(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct OccArgs {
    const uint32_t *traj;          // one int16 (row, col) pair per dword
    const long long *off;          // the round's offsets: ntr + 1 of them
    int ntr;                       // tracks of the round, 1..kOccRoundMax
    int rows, cols;
    long long plane_words;         // rows * cols
    uint32_t *mask;                // the workspace: planes x rows x cols
    uint32_t *counts;              // (rows, cols)
    uint32_t *per_track;           // the round's first entry of cells_per_track, or nullptr
};

// blocks of a launch over the points [p0, p1): every wave gets kOccMinSpans spans at least, K8's cap at most
inline unsigned occ_grid(long long p0, long long p1)
{
    const long long nspans = (p1 - (p0 & ~3LL) + kOccSpan - 1) / kOccSpan;
    const long long per_block = kOccWaves * kOccMinSpans;
    const long long blocks = (nspans + per_block - 1) / per_block;
    return static_cast<unsigned>(blocks < 1 ? 1 : blocks > kOccBlocks ? kOccBlocks : blocks);
}

// kVec: 16-byte loads (traj is 16-byte aligned).  kSet: set the bits and count; otherwise store 0 to the touched words.
template <bool kVec, bool kSet>
__global__ __launch_bounds__(kBlock) void k_track_occupancy(const OccArgs a)
{
    __shared__ long long s_off[kOccRoundMax + 1];
    for (int i = threadIdx.x; i <= a.ntr; i += kBlock) s_off[i] = a.off[i];
    __syncthreads();                             // (the only barrier: the returns below are behind it)

    const long long p0 = s_off[0], p1 = s_off[a.ntr];
    if (p0 < 0 || p1 <= p0) return;
    // spans are cut at multiples of four points of the BUFFER, so that a lane's four points are one aligned load
    const long long a0 = p0 & ~3LL;
    const long long nspans = (p1 - a0 + kOccSpan - 1) / kOccSpan;
    const long long nwaves = static_cast<long long>(gridDim.x) * kOccWaves;
    long long per_wave = (nspans + nwaves - 1) / nwaves;
    per_wave = per_wave < kOccMinSpans ? kOccMinSpans : per_wave;
    const int lane = threadIdx.x & 63, wave = static_cast<int>(threadIdx.x) >> 6;
    const long long u0 = (static_cast<long long>(blockIdx.x) * kOccWaves + wave) * per_wave;
    const long long u1 = u0 + per_wave < nspans ? u0 + per_wave : nspans;
    if (u0 >= u1) return;

    // the track that holds this lane's first point: the LAST one that starts at or before it (the ones before it that
    // start there too are empty).  Lanes whose first point lies past the end find nothing to do in any span.
    int t = 0;
    {
        const long long first = a0 + u0 * kOccSpan + 4 * lane;
        const long long key = first > p0 ? first : p0;
        int lo = 0, hi = a.ntr;
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (s_off[mid] <= key) lo = mid; else hi = mid;
        }
        t = lo;
    }
    long long t_end = s_off[t + 1];
    uint32_t mine = 0;                           // cells whose first visit by track t this lane made

    auto fetch = [&](long long u) {
        return *reinterpret_cast<const uint4 *>(a.traj + (a0 + u * kOccSpan + 4 * lane));
    };
    auto fetch_edge = [&](long long u) {
        const long long i0 = a0 + u * kOccSpan + 4 * lane;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (i0 + 0 >= p0 && i0 + 0 < p1) v.x = a.traj[i0 + 0];
        if (i0 + 1 >= p0 && i0 + 1 < p1) v.y = a.traj[i0 + 1];
        if (i0 + 2 >= p0 && i0 + 2 < p1) v.z = a.traj[i0 + 2];
        if (i0 + 3 >= p0 && i0 + 3 < p1) v.w = a.traj[i0 + 3];
        return v;
    };

    auto span = [&](const long long u, const uint4 cur) {
        const long long i0 = a0 + u * kOccSpan + 4 * lane;
        const uint32_t pts[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long i = i0 + j;
            if (i < p0 || i >= p1) continue;
            // (i < p1 = s_off[ntr]: the walk stops at a track below ntr)
            while (t_end <= i) {
                if (kSet && mine != 0 && a.per_track != nullptr) atomicAdd(a.per_track + t, mine);
                mine = 0;
                ++t;
                t_end = s_off[t + 1];
            }
            const int r = static_cast<int16_t>(pts[j] & 0xFFFF), c = static_cast<int16_t>(pts[j] >> 16);
            if (r < 0 || c < 0 || r >= a.rows || c >= a.cols) continue;
            const int cell = r * a.cols + c;
            uint32_t *word = a.mask + ((t >> 5) * a.plane_words + cell);
            if (kSet) {
                const uint32_t bit = 1u << (t & 31);
                if (occ_load_l2(word) & bit) continue;
                const uint32_t old = atomicOr(word, bit);
                if (!(old & bit)) {
                    atomicAdd(a.counts + cell, 1u);
                    ++mine;
                }
            } else {
                *word = 0u;
            }
        }
    };

    // Spans that end at or before p1 stream through 16-byte loads, one span ahead; the last span of the data, and
    // every span of an unaligned buffer, go point by point (K8's loop).
    long long u = u0;
    if (kVec) {
        const long long whole = (p1 - a0) / kOccSpan;
        const long long u_vec = u1 < whole ? u1 : whole;
        if (u < u_vec) {
            uint4 next = fetch(u);
            for (; u < u_vec; ++u) {
                const uint4 cur = next;
                next = fetch(u + 1 < u_vec ? u + 1 : u);
                span(u, cur);
            }
        }
    }
    for (; u < u1; ++u) span(u, fetch_edge(u));
    if (kSet && mine != 0 && a.per_track != nullptr) atomicAdd(a.per_track + t, mine);
}

template <bool kSet>
static void occ_launch(const OccArgs &a, bool vec, unsigned blocks, hipStream_t st)
{
    const dim3 grid(blocks), block(kBlock);
    if (vec) hipLaunchKernelGGL((k_track_occupancy<true, kSet>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_track_occupancy<false, kSet>), grid, block, 0, st, a);
}

}  // namespace ssrs

using namespace ssrs;

extern "C" size_t ssrs_track_occupancy_workspace_bytes(int rows, int cols, int planes)
{
    if (rows < 1 || cols < 1 || planes < 1) return 0;
    const size_t bytes = static_cast<size_t>(rows) * static_cast<size_t>(cols) * 4 * static_cast<size_t>(planes);
    return (bytes + 255) / 256 * 256;
}

extern "C" int ssrs_track_occupancy(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks, int rows, int cols,
                                    int planes, uint32_t *counts, uint32_t *cells_per_track, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    SSRS_REQUIRE(traj && traj_offsets && counts && workspace, "ssrs_track_occupancy: NULL pointer");
    SSRS_REQUIRE(planes >= 1 && planes <= SSRS_OCCUPANCY_MAX_PLANES, "ssrs_track_occupancy: planes = %d outside [1, %d]",
                 planes, SSRS_OCCUPANCY_MAX_PLANES);
    SSRS_REQUIRE(rows >= 1 && rows <= 32767 && cols >= 1 && cols <= 32767,
                 "ssrs_track_occupancy: a %d x %d raster (int16 points: 1..32767 either way)", rows, cols);
    // (as ssrs_turbine_encounters: the kernel keeps track numbers as int)
    SSRS_REQUIRE(ntracks >= 0 && ntracks <= INT32_MAX, "ssrs_track_occupancy: ntracks = %lld outside [0, 2^31)",
                 static_cast<long long>(ntracks));
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(traj) & 3u) == 0, "ssrs_track_occupancy: traj must be 4-byte aligned");
    SSRS_REQUIRE(workspace_bytes >= ssrs_track_occupancy_workspace_bytes(rows, cols, planes),
                 "ssrs_track_occupancy: workspace of %zu bytes, %zu needed for %d planes of %d x %d", workspace_bytes,
                 ssrs_track_occupancy_workspace_bytes(rows, cols, planes), planes, rows, cols);
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
    SSRS_REQUIRE(border[0] >= 0, "ssrs_track_occupancy: traj_offsets[0] = %lld is negative", border[0]);
    for (long long k = 0; k < nrounds; ++k)
        SSRS_REQUIRE(border[k + 1] >= border[k], "ssrs_track_occupancy: traj_offsets descends (%lld after %lld)",
                     border[k + 1], border[k]);

    OccArgs a;
    a.traj = reinterpret_cast<const uint32_t *>(traj);
    a.rows = rows;
    a.cols = cols;
    a.plane_words = static_cast<long long>(rows) * cols;
    a.mask = static_cast<uint32_t *>(workspace);
    a.counts = counts;
    const bool vec = (reinterpret_cast<uintptr_t>(traj) & 15u) == 0;
    for (long long k = 0; k < nrounds; ++k) {
        const long long p0 = border[k], p1 = border[k + 1];
        if (p1 <= p0) continue;                                       // (a round of empty tracks)
        const long long t0 = k * round_tracks;
        a.off = reinterpret_cast<const long long *>(traj_offsets) + t0;
        a.ntr = static_cast<int>(ntracks - t0 < round_tracks ? ntracks - t0 : round_tracks);
        a.per_track = cells_per_track ? cells_per_track + t0 : nullptr;
        const unsigned blocks = occ_grid(p0, p1);
        occ_launch<true>(a, vec, blocks, st);
        // clearing: one 4-byte store per point against the round's planes
        const size_t used_bytes = static_cast<size_t>((a.ntr + 31) / 32) * static_cast<size_t>(a.plane_words) * 4;
        if (static_cast<unsigned long long>(p1 - p0) * 4 < used_bytes) occ_launch<false>(a, vec, blocks, st);
        else SSRS_HIP_CHECK(hipMemsetAsync(workspace, 0, used_bytes, st));
    }
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}
