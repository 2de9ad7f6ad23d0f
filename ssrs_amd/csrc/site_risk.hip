// K20 -- the site collision-risk map for gfx950 (MI355X): K19 turned inside out.
//
// For EVERY cell of the raster, the transits through the rotor disk of one candidate turbine class standing on that cell,
// and the exact sum of their Band probabilities.  The definition, rounding by rounding, is K18's and K19's (include/
// ssrs_hip_transits.h, ssrs_hip_collision.h) with the site's numbers from include/ssrs_hip_sites.h; the arithmetic is
// rotor_disk.h's, the one statement K18 and K19 call too.  K8's, K14's and K15's buffers are the inputs.  One launch:
//   - a block takes a tile of kSiteTile consecutive points of the chunk (track borders or not), a lane kSiteRun consecutive
//     points, their heights and the one behind them (four 16-byte loads when both buffers are 16-byte aligned, point by
//     point at the chunk's ends and for unaligned buffers);
//   - every point is looked at as the FIRST point of a move -- every cell is a site, so there is no occupied-bin mask to
//     skip the common point.  The tile's first and last track come from two binary searches of the offsets (lanes 0 and
//     1); every lane then searches between them only and walks the offsets from there, over empty tracks and track ends
//     inside its run (K16's way);
//   - a testable move is tested against the sites of the window |r - r0| <= W, |c - c0| <= W, W = floor(reach + 1.5),
//     clipped to the raster (the header proves that no other site can be transited).  Per site the plane test comes first:
//     the site's elevation is gathered, and the divisions and the second half run, only for moves that cross its plane.
//     In uniform mode the axis is two scalars; per cell it is one 16-byte gather a site;
//   - a transit goes to `transits` and `risk` as two 64-bit global adds.  A table of sites in LDS in front of them (K16's
//     kTimeHash turned to this use: 2048 entries of two uint32 counts and two uint64 sums, flushed once a block) was built
//     and measured on tracks parked on four cells, where 2e7 transits fall on a few dozen sites: it changed the pass by 1 %,
//     inside the run-to-run spread, because the plane tests set the pace and not the adds, and its 56 KB held the kernel
//     at two blocks a CU (profiles/site_collision_risk.md).  It is not kept;
//   - the class's table, 2 KB, is staged in LDS.
// Block cooperation is __shared__ + __syncthreads() only (no shuffles, ballots or DPP), so tests/hip_host_stub runs this
// file's own code on the CPU.  Integer adds modulo 2^64: the result does not depend on the launch order.
#include <climits>
#include <cmath>

#include "common.h"
#include "rotor_disk.h"
#include "../../include/ssrs_hip_sites.h"

namespace ssrs {

constexpr int kSiteRun = 8;                                // consecutive points a lane takes
constexpr int kSiteTile = kBlock * kSiteRun;               // points a block takes
constexpr int kSiteTable = 2 * SSRS_COLLISION_RINGS;       // the class's table, uint32
typedef unsigned long long u64;
static_assert(kSiteRun % 4 == 0, "a lane's run is whole 16-byte loads");
constexpr size_t kSitePerCellLds = 60 * 1024;              // dynamic LDS of a per-cell launch: two blocks a CU (see the launch)

struct SiteArgs {
    const uint32_t *traj;          // one int16 (row, col) pair per dword
    const int32_t *alt;            // mm above ground, indexed like traj
    const long long *off;          // ntracks + 1 offsets
    int ntracks;
    int rows, cols;
    long long p0, p1;              // the chunk's points: off[0], off[ntracks]
    const int32_t *cellinfo;       // {climb, elev} per cell
    double reach;
    int window;                    // W = floor(reach + 1.5)
    int hub_mm;
    const double *axis;            // (rows, cols, 2), or the one pair
    double mm_per_cell;
    const uint32_t *table;         // (2, SSRS_COLLISION_RINGS)
    u64 *transits, *risk;          // (rows, cols, 2); transits may be NULL
};

__device__ __forceinline__ bool site_inside(uint32_t pt, int rows, int cols, int &r, int &c)
{
    r = static_cast<int16_t>(pt & 0xFFFF);
    c = static_cast<int16_t>(pt >> 16);
    return r >= 0 && c >= 0 && r < rows && c < cols;
}

// kVec: traj and alt are 16-byte aligned.  kPerCell: every site has an axis of its own.
template <bool kVec, bool kPerCell>
__global__ __launch_bounds__(kBlock) void k_site_risk(const SiteArgs a)
{
    __shared__ int s_t[2];
    __shared__ uint32_t s_table[kSiteTable];
    for (int k = threadIdx.x; k < kSiteTable; k += kBlock) s_table[k] = a.table[k];

    // the lane's run and the point behind it; points outside [p0, p1) are not read
    const long long a0 = a.p0 & ~3LL;                      // tiles are cut at multiples of four points of the BUFFER
    const long long tile0 = a0 + static_cast<long long>(blockIdx.x) * kSiteTile;
    const long long i0 = tile0 + static_cast<long long>(threadIdx.x) * kSiteRun;
    const bool whole = kVec && tile0 >= a.p0 && tile0 + kSiteTile <= a.p1;
    uint32_t pts[kSiteRun + 1];
    int alts[kSiteRun + 1];
    if (whole) {
#pragma unroll
        for (int q = 0; q < kSiteRun / 4; ++q) {
            const uint4 v = *reinterpret_cast<const uint4 *>(a.traj + (i0 + 4 * q));
            const int4 h = *reinterpret_cast<const int4 *>(a.alt + (i0 + 4 * q));
            pts[4 * q + 0] = v.x, pts[4 * q + 1] = v.y, pts[4 * q + 2] = v.z, pts[4 * q + 3] = v.w;
            alts[4 * q + 0] = h.x, alts[4 * q + 1] = h.y, alts[4 * q + 2] = h.z, alts[4 * q + 3] = h.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < kSiteRun; ++j) {
            const long long i = i0 + j;
            const bool valid = i >= a.p0 && i < a.p1;
            pts[j] = valid ? a.traj[i] : 0u;
            alts[j] = valid ? a.alt[i] : 0;
        }
    }
    {
        const bool valid = i0 + kSiteRun >= a.p0 && i0 + kSiteRun < a.p1;
        pts[kSiteRun] = valid ? a.traj[i0 + kSiteRun] : 0u;
        alts[kSiteRun] = valid ? a.alt[i0 + kSiteRun] : 0;
    }

    // the track that holds the lane's first valid point: the LAST one that starts at or before it, searched between the
    // tile's first and last track, which lanes 0 and 1 find over all offsets
    const long long first = tile0 > a.p0 ? tile0 : a.p0;
    const long long last = tile0 + kSiteTile < a.p1 ? tile0 + kSiteTile - 1 : a.p1 - 1;
    if (threadIdx.x < 2) {
        const long long key = threadIdx.x == 0 ? first : last;
        int lo = 0, hi = a.ntracks;
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (a.off[mid] <= key) lo = mid; else hi = mid;
        }
        s_t[threadIdx.x] = lo;
    }
    __syncthreads();                                       // (covers the staged table too)
    int t = s_t[0];
    {
        long long key = i0 > first ? i0 : first;
        key = key < last ? key : last;                     // (lanes past the end: any track of the tile will do)
        int hi = s_t[1] + 1;
        while (hi - t > 1) {
            const int mid = t + (hi - t) / 2;
            if (a.off[mid] <= key) t = mid; else hi = mid;
        }
    }
    long long t_end = a.off[t + 1];

    // one more transit of `site` in direction dir, with the probability q32
    auto hand_over = [&](long long site, int dir, uint32_t q32) {
        const long long k = 2 * site + dir;
        if (a.transits != nullptr) atomicAdd(a.transits + k, static_cast<u64>(1));
        if (q32 != 0) atomicAdd(a.risk + k, static_cast<u64>(q32));
    };

    const double uax = kPerCell ? 0.0 : a.axis[0], uay = kPerCell ? 0.0 : a.axis[1];
    const int W = a.window;
#pragma unroll
    for (int j = 0; j < kSiteRun; ++j) {
        const long long i = i0 + j;
        if (i < a.p0 || i >= a.p1) continue;
        while (t_end <= i) {                               // (i < p1 = off[ntracks]: the walk stops below ntracks)
            ++t;
            t_end = a.off[t + 1];
        }
        if (i + 1 >= t_end) continue;                      // the track's last point
        int r0, c0, r1, c1;
        if (!site_inside(pts[j], a.rows, a.cols, r0, c0) || !site_inside(pts[j + 1], a.rows, a.cols, r1, c1)) continue;
        const int dr = r1 - r0, dc = c1 - c0;
        if (dr < -1 || dr > 1 || dc < -1 || dc > 1) continue;              // a burn-in jump
        if (dr == 0 && dc == 0) continue;                                  // a rest: s_0 == s_1, never a crossing
        const int e0 = a.cellinfo[2 * (static_cast<long long>(r0) * a.cols + c0) + 1];
        const int e1 = a.cellinfo[2 * (static_cast<long long>(r1) * a.cols + c1) + 1];
        if (e0 == INT_MIN || e1 == INT_MIN) continue;                      // nodata under an end
        const long long z0 = static_cast<long long>(e0) + alts[j], z1 = static_cast<long long>(e1) + alts[j + 1];
        // ---- the window of the move's first point, clipped to the raster
        const int rlo = r0 - W > 0 ? r0 - W : 0, rhi = r0 + W < a.rows - 1 ? r0 + W : a.rows - 1;
        const int clo = c0 - W > 0 ? c0 - W : 0, chi = c0 + W < a.cols - 1 ? c0 + W : a.cols - 1;
        for (int rr = rlo; rr <= rhi; ++rr) {
            const long long row = static_cast<long long>(rr) * a.cols;
            for (int cc = clo; cc <= chi; ++cc) {
                double ax = uax, ay = uay;
                if (kPerCell) ax = a.axis[2 * (row + cc)], ay = a.axis[2 * (row + cc) + 1];
                RotorPlane plane;
                if (!rotor_plane_test(static_cast<double>(cc), static_cast<double>(rr), ax, ay, r0, c0, r1, c1, plane)) continue;
                const int elev = a.cellinfo[2 * (row + cc) + 1];
                if (elev == INT_MIN) continue;                             // a site on nodata
                long long hub = static_cast<long long>(elev) + a.hub_mm;
                hub = hub > INT_MAX ? INT_MAX : hub < INT_MIN ? INT_MIN : hub;
                int ring = 0;
                const int dir = rotor_disk_test<true>(plane, ax, ay, a.reach, hub, z0, z1, a.mm_per_cell, ring);
                if (dir < 0) continue;
                hand_over(row + cc, dir, s_table[dir * SSRS_COLLISION_RINGS + ring]);
            }
        }
    }
}

}  // namespace ssrs

using namespace ssrs;

extern "C" int ssrs_site_collision_risk(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks, const int32_t *alt,
                                        const int32_t *cellinfo, int rows, int cols, double reach, int hub_mm,
                                        const double *axis, int axis_per_cell, double mm_per_cell, const uint32_t *table,
                                        uint64_t *transits, uint64_t *risk, void *stream)
{
    SSRS_REQUIRE(traj && traj_offsets && alt && cellinfo && axis && table && risk,
                 "ssrs_site_collision_risk: NULL pointer (only transits may be NULL)");
    SSRS_REQUIRE(ntracks >= 0 && ntracks <= INT32_MAX, "ssrs_site_collision_risk: ntracks = %lld outside [0, 2^31)",
                 static_cast<long long>(ntracks));
    SSRS_REQUIRE(rows >= 1 && rows <= 32767 && cols >= 1 && cols <= 32767,
                 "ssrs_site_collision_risk: a %d x %d raster (int16 points: 1..32767 either way)", rows, cols);
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(traj) & 3u) == 0 && (reinterpret_cast<uintptr_t>(alt) & 3u) == 0,
                 "ssrs_site_collision_risk: traj and alt must be 4-byte aligned");
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(cellinfo) & 7u) == 0 && (reinterpret_cast<uintptr_t>(axis) & 7u) == 0,
                 "ssrs_site_collision_risk: cellinfo and axis must be 8-byte aligned");
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(table) & 3u) == 0, "ssrs_site_collision_risk: table must be 4-byte aligned");
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(transits) & 7u) == 0 && (reinterpret_cast<uintptr_t>(risk) & 7u) == 0,
                 "ssrs_site_collision_risk: transits and risk must be 8-byte aligned");
    SSRS_REQUIRE(std::isfinite(mm_per_cell) && mm_per_cell > 0.0, "ssrs_site_collision_risk: mm_per_cell = %g (finite and > 0)",
                 mm_per_cell);
    SSRS_REQUIRE(!(reach > SSRS_SITE_MAX_REACH), "ssrs_site_collision_risk: reach = %g cells (at most %g)", reach,
                 SSRS_SITE_MAX_REACH);
    if (!(reach >= 0.0)) return SSRS_OK;                   // nothing transits a NaN or negative reach
    if (ntracks == 0) return SSRS_OK;
    hipStream_t st = as_stream(stream);

    // the chunk's first and last offset, on the host: the launch is sized from its points
    long long ends[2];
    SSRS_HIP_CHECK(hipMemcpyAsync(&ends[0], traj_offsets, 8, hipMemcpyDeviceToHost, st));
    SSRS_HIP_CHECK(hipMemcpyAsync(&ends[1], traj_offsets + ntracks, 8, hipMemcpyDeviceToHost, st));
    SSRS_HIP_CHECK(hipStreamSynchronize(st));
    SSRS_REQUIRE(ends[0] >= 0, "ssrs_site_collision_risk: traj_offsets[0] = %lld is negative", ends[0]);
    SSRS_REQUIRE(ends[1] >= ends[0], "ssrs_site_collision_risk: traj_offsets descends (%lld after %lld)", ends[1], ends[0]);
    if (ends[1] == ends[0]) return SSRS_OK;

    SiteArgs a;
    a.traj = reinterpret_cast<const uint32_t *>(traj);
    a.alt = alt;
    a.off = reinterpret_cast<const long long *>(traj_offsets);
    a.ntracks = static_cast<int>(ntracks);
    a.rows = rows;
    a.cols = cols;
    a.p0 = ends[0];
    a.p1 = ends[1];
    a.cellinfo = cellinfo;
    a.reach = reach;
    a.window = static_cast<int>(std::floor(reach + 1.5));
    a.hub_mm = hub_mm;
    a.axis = axis;
    a.mm_per_cell = mm_per_cell;
    a.table = table;
    a.transits = reinterpret_cast<u64 *>(transits);
    a.risk = reinterpret_cast<u64 *>(risk);
    const long long ntiles = (a.p1 - (a.p0 & ~3LL) + kSiteTile - 1) / kSiteTile;
    SSRS_REQUIRE(ntiles <= INT32_MAX, "ssrs_site_collision_risk: %lld points in one call (at most 2^31 tiles of %d)",
                 a.p1 - a.p0, kSiteTile);
    const bool vec = ((reinterpret_cast<uintptr_t>(traj) | reinterpret_cast<uintptr_t>(alt)) & 15u) == 0;
    const dim3 grid(static_cast<unsigned>(ntiles)), block(kBlock);
    // With an axis per cell every site costs a 16-byte gather, and neighbouring lanes' windows overlap: the pass lives on
    // L1 hits, and two blocks a CU keep them where five evict each other's lines (profiles/site_collision_risk.md).  The
    // kernel has no other way to ask for fewer blocks a CU than to ask for LDS: kSitePerCellLds bytes it never touches.
    if (vec && axis_per_cell) hipLaunchKernelGGL((k_site_risk<true, true>), grid, block, kSitePerCellLds, st, a);
    else if (vec) hipLaunchKernelGGL((k_site_risk<true, false>), grid, block, 0, st, a);
    else if (axis_per_cell) hipLaunchKernelGGL((k_site_risk<false, true>), grid, block, kSitePerCellLds, st, a);
    else hipLaunchKernelGGL((k_site_risk<false, false>), grid, block, 0, st, a);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}
