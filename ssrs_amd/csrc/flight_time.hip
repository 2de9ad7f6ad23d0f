// K16 -- flight time along every track for gfx950 (MI355X): wind-drift microseconds per cell, track and rotor zone.
//
// This build's own model (the reference has none; DESIGN.md K16, include/ssrs_hip.h "flight time"), in integers so that
// every grouping of the work gives the same bits.  Per cell `windinfo` holds {wr, wc}: the velocity of the AIR along +row
// and +col in mm/s.  The move from point k to point k + 1 of a track takes dt microseconds: the length of the move over the
// ground speed the bird keeps along it at airspeed va in the wind of the cell it LEAVES (never less than gmin), and dt is
// credited to that cell, to the track, and -- where the caller's `masked` copy of the points says the point is in the
// rotor zone -- to a second raster and the track's second sum.  dt depends on a point and its successor only: no scan.
//   - one launch.  A block takes a tile of SSRS_FLIGHT_TIME_TILE consecutive points of the chunk (track borders or not), a
//     lane kTimeRun consecutive points and the one behind them (four 16-byte loads when the buffers are 16-byte aligned,
//     point by point at the chunk's ends and for unaligned buffers), and one 8-byte windinfo load a point, all of a run
//     issued before anything waits for one;
//   - the tile's first and last track come from two binary searches of the offsets (lanes 0 and 1); every lane then
//     searches between them only -- nothing at all inside a long track -- and walks the offsets from there, over empty
//     tracks and track ends inside its run, as K13's and K14's lanes do;
//   - the exact floor square root and the exact quotient are an f64 estimate corrected by integer multiplies: the result is
//     the integer whatever the hardware's sqrt and division round to;
//   - the rasters: a lane keeps three (cell, sum, zone sum) triples in registers over its run and hands one on when it is
//     pushed out and at the end.  A triple that took more than one move (the lane came back to the cell: a track in a
//     trap of two or three cells) goes to a table of kTimeHash cells in LDS, one 64-bit LDS atomic a sum, and the block
//     sends every cell of the table to global memory once at its end; a triple of one move, or one whose slot holds
//     another cell, goes to global memory as it is.  The lanes of a trapped track all add to the same few cells: 64-bit
//     global atomics on one address are served one after another, so without the table they set the pace of the pass
//     (profiles/flight_time.md);
//   - per-track sums: a lane combines in registers, the block in LDS slots (track - the tile's first track, 256 of them),
//     and one lane per touched slot goes to global memory with one 64-bit atomic a sum.  Tracks past the slots (more than
//     256 tracks in a tile: they are short) go to global memory by lane.
// Block cooperation is __shared__ + __syncthreads() only (no shuffles, ballots or DPP), so tests/hip_host_stub runs this
// file's own code on the CPU.  Integer adds modulo 2^64: the result does not depend on the launch order.
#include <climits>
#include <cmath>

#include "common.h"

namespace ssrs {

constexpr int kTimeRun = 16;                               // consecutive points a lane takes
constexpr int kTimeTile = SSRS_FLIGHT_TIME_TILE;           // points a block takes
static_assert(kTimeTile == kBlock * kTimeRun, "a tile is one run per lane of a block");
constexpr int kTimeSlots = 256;                            // LDS slots for the per-track sums of a tile
constexpr int kTimeHash = 1024;                            // LDS table of the cells a block's lanes came back to
constexpr long long kTimeSqrt2 = 92682;                    // round(sqrt(2) * 2^16)
constexpr long long kTimeHalfSqrt2 = 46341;                // round(sqrt(1/2) * 2^16)
constexpr int kTimeWindClip = 1 << 20;                     // |wr|, |wc| and va in mm/s
typedef unsigned long long u64;

struct TimeArgs {
    const uint32_t *traj;          // one int16 (row, col) pair per dword
    const long long *off;          // ntracks + 1 offsets
    int ntracks;
    int rows, cols;
    const uint32_t *masked;        // traj with (-1, -1) where the point is not in the rotor zone, or NULL
    const int2 *windinfo;          // {wr, wc} per cell, or NULL: (uwr, uwc) everywhere
    int uwr, uwc;
    long long p0, p1;              // the chunk's points: off[0], off[ntracks]
    long long va2, num_orth, num_diag;
    int gmin, dt_stay;
    u64 *time_hist, *band_time_hist, *per_track;
    int *dt;
};

// floor(sqrt(s)), 0 < s <= 2^40: the f64 estimate is within one of it whatever sqrt rounds to; the loops make it exact
__host__ __device__ __forceinline__ long long time_isqrt(long long s)
{
    long long r = static_cast<long long>(sqrt(static_cast<double>(s)));
    while (r * r > s) --r;
    while ((r + 1) * (r + 1) <= s) ++r;
    return r;
}

// floor(n / g), 0 <= n < 2^42, 1 <= g < 2^23: both exact in f64, the quotient's estimate within one
__host__ __device__ __forceinline__ long long time_div(long long n, long long g)
{
    long long q = static_cast<long long>(static_cast<double>(n) / static_cast<double>(g));
    long long rem = n - q * g;
    while (rem < 0) --q, rem += g;
    while (rem >= g) ++q, rem -= g;
    return q;
}

__device__ __forceinline__ bool time_inside(uint32_t pt, int rows, int cols, int &r, int &c)
{
    r = static_cast<int16_t>(pt & 0xFFFF);
    c = static_cast<int16_t>(pt >> 16);
    return r >= 0 && c >= 0 && r < rows && c < cols;
}

// dt of the move from -> to between two cells inside the raster, in the wind w of `from`
__host__ __device__ __forceinline__ int time_move(const TimeArgs &a, uint32_t from, uint32_t to, int2 w)
{
    const int dr = static_cast<int16_t>(to & 0xFFFF) - static_cast<int16_t>(from & 0xFFFF);
    const int dc = static_cast<int16_t>(to >> 16) - static_cast<int16_t>(from >> 16);
    const int sr = (dr > 0) - (dr < 0), sc = (dc > 0) - (dc < 0);
    if (sr == 0 && sc == 0) return a.dt_stay;
    long long along = sr * w.x + sc * w.y, cross2, num;
    if (sr != 0 && sc != 0) {
        along = (along * kTimeHalfSqrt2 + 32768) >> 16;
        const long long b = sr * w.y - sc * w.x;
        cross2 = (b * b) >> 1;
        num = a.num_diag;
    } else {
        const long long b = sr != 0 ? w.y : w.x;
        cross2 = b * b;
        num = a.num_orth;
    }
    const long long s = a.va2 - cross2;
    long long g = a.gmin;                                  // (s <= 0: the bird cannot hold the heading)
    if (s > 0) {
        const long long v = along + time_isqrt(s);
        g = v > g ? v : g;
    }
    const long long q = time_div(num + (g >> 1), g);
    return q > INT_MAX ? INT_MAX : static_cast<int>(q);
}

// Sums of one cell go to the rasters
__device__ __forceinline__ void time_to_rasters(const TimeArgs &a, int cell, u64 sum, u64 zone)
{
    if (a.time_hist != nullptr && sum != 0) atomicAdd(a.time_hist + cell, sum);
    if (a.band_time_hist != nullptr && zone != 0) atomicAdd(a.band_time_hist + cell, zone);
}

// kVec: traj (and masked, dt) are 16-byte aligned.
template <bool kVec>
__global__ __launch_bounds__(kBlock) void k_track_time(const TimeArgs a)
{
    __shared__ int s_t[2];
    __shared__ u64 s_tot[kTimeSlots], s_zone[kTimeSlots];
    __shared__ int s_cell[kTimeHash];
    __shared__ u64 s_cell_sum[kTimeHash], s_cell_zone[kTimeHash];
    for (int k = threadIdx.x; k < kTimeSlots; k += kBlock) s_tot[k] = 0, s_zone[k] = 0;
    for (int k = threadIdx.x; k < kTimeHash; k += kBlock) s_cell[k] = -1, s_cell_sum[k] = 0, s_cell_zone[k] = 0;

    // the lane's run and the point behind it; points outside [p0, p1) are not read
    const long long a0 = a.p0 & ~3LL;                      // tiles are cut at multiples of four points of the BUFFER
    const long long tile0 = a0 + static_cast<long long>(blockIdx.x) * kTimeTile;
    const long long i0 = tile0 + static_cast<long long>(threadIdx.x) * kTimeRun;
    const bool whole = kVec && tile0 >= a.p0 && tile0 + kTimeTile <= a.p1;
    uint32_t pts[kTimeRun + 1], msk[kTimeRun];
    if (whole) {
#pragma unroll
        for (int q = 0; q < kTimeRun / 4; ++q) {
            const uint4 v = *reinterpret_cast<const uint4 *>(a.traj + (i0 + 4 * q));
            pts[4 * q + 0] = v.x, pts[4 * q + 1] = v.y, pts[4 * q + 2] = v.z, pts[4 * q + 3] = v.w;
            uint4 m = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
            if (a.masked != nullptr) m = *reinterpret_cast<const uint4 *>(a.masked + (i0 + 4 * q));
            msk[4 * q + 0] = m.x, msk[4 * q + 1] = m.y, msk[4 * q + 2] = m.z, msk[4 * q + 3] = m.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < kTimeRun; ++j) {
            const long long i = i0 + j;
            const bool valid = i >= a.p0 && i < a.p1;
            pts[j] = valid ? a.traj[i] : 0u;
            msk[j] = valid && a.masked != nullptr ? a.masked[i] : 0xFFFFFFFFu;
        }
    }
    pts[kTimeRun] = i0 + kTimeRun >= a.p0 && i0 + kTimeRun < a.p1 ? a.traj[i0 + kTimeRun] : 0u;

    // the wind of the lane's points: one 8-byte load each, all of them independent of one another and of the track walk
    uint32_t inside = 0;                                   // bit j: point j is a point of the chunk inside the raster
    int2 wind[kTimeRun];
#pragma unroll
    for (int j = 0; j <= kTimeRun; ++j) {
        const long long i = i0 + j;
        int r, c;
        if (j < kTimeRun) wind[j] = make_int2(a.uwr, a.uwc);
        if (i >= a.p0 && i < a.p1 && time_inside(pts[j], a.rows, a.cols, r, c)) {
            inside |= 1u << j;
            if (j < kTimeRun && a.windinfo != nullptr) wind[j] = a.windinfo[static_cast<long long>(r) * a.cols + c];
        }
    }

    // the track that holds the lane's first valid point: the LAST one that starts at or before it, searched between the
    // tile's first and last track, which lanes 0 and 1 find over all offsets
    const long long first = tile0 > a.p0 ? tile0 : a.p0;
    const long long last = tile0 + kTimeTile < a.p1 ? tile0 + kTimeTile - 1 : a.p1 - 1;
    if (threadIdx.x < 2) {
        const long long key = threadIdx.x == 0 ? first : last;
        int lo = 0, hi = a.ntracks;
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (a.off[mid] <= key) lo = mid; else hi = mid;
        }
        s_t[threadIdx.x] = lo;
    }
    __syncthreads();                                       // (covers the slots' initial values too)
    const int t_first = s_t[0];
    int t = t_first;
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

    u64 tot = 0, zone = 0;                                 // of track t, by this lane
    auto flush = [&]() {
        if (a.per_track != nullptr && (tot | zone) != 0) {
            const int slot = t - t_first;
            if (slot < kTimeSlots) {
                if (tot != 0) atomicAdd(&s_tot[slot], tot);
                if (zone != 0) atomicAdd(&s_zone[slot], zone);
            } else {
                u64 *const sums = a.per_track + 2 * static_cast<long long>(t);
                if (tot != 0) atomicAdd(sums, tot);
                if (zone != 0) atomicAdd(sums + 1, zone);
            }
        }
        tot = 0, zone = 0;
    };
    // the register cache: entry 0 is the newest; a miss pushes entry 2 out.  again: the entry took more than one move
    int cell0 = -1, cell1 = -1, cell2 = -1;
    u64 sum0 = 0, sum1 = 0, sum2 = 0, zon0 = 0, zon1 = 0, zon2 = 0;
    bool again0 = false, again1 = false, again2 = false;
    auto evict = [&](int cell, u64 sum, u64 zone, bool again) {
        if (cell < 0) return;
        if (again) {
            const int slot = static_cast<int>(static_cast<uint32_t>(cell) * 2654435761u >> 22);        // 10 bits: kTimeHash
            const int held = atomicCAS(&s_cell[slot], -1, cell);
            if (held == -1 || held == cell) {
                if (sum != 0) atomicAdd(&s_cell_sum[slot], sum);
                if (zone != 0) atomicAdd(&s_cell_zone[slot], zone);
                return;
            }
        }
        time_to_rasters(a, cell, sum, zone);
    };
    int dts[kTimeRun];
#pragma unroll
    for (int j = 0; j < kTimeRun; ++j) {
        const long long i = i0 + j;
        dts[j] = 0;
        if (i < a.p0 || i >= a.p1) continue;
        while (t_end <= i) {                               // (i < p1 = off[ntracks]: the walk stops below ntracks)
            flush();
            ++t;
            t_end = a.off[t + 1];
        }
        if (i + 1 >= t_end || (inside >> j & 3u) != 3u) continue;          // the track's last point, or an end outside
        const int dt = time_move(a, pts[j], pts[j + 1], wind[j]);
        dts[j] = dt;
        const u64 zdt = static_cast<int16_t>(msk[j] & 0xFFFF) >= 0 ? dt : 0;
        tot += static_cast<u64>(dt);
        zone += zdt;
        const int cell = static_cast<int16_t>(pts[j] & 0xFFFF) * a.cols + static_cast<int16_t>(pts[j] >> 16);   // (< 2^30)
        if (cell == cell0) {
            sum0 += dt, zon0 += zdt, again0 = true;
        } else if (cell == cell1) {
            sum1 += dt, zon1 += zdt, again1 = true;
        } else if (cell == cell2) {
            sum2 += dt, zon2 += zdt, again2 = true;
        } else {
            evict(cell2, sum2, zon2, again2);
            cell2 = cell1, sum2 = sum1, zon2 = zon1, again2 = again1;
            cell1 = cell0, sum1 = sum0, zon1 = zon0, again1 = again0;
            cell0 = cell, sum0 = dt, zon0 = zdt, again0 = false;
        }
    }
    flush();
    evict(cell0, sum0, zon0, again0);
    evict(cell1, sum1, zon1, again1);
    evict(cell2, sum2, zon2, again2);

    if (a.dt != nullptr) {
        if (whole) {
#pragma unroll
            for (int q = 0; q < kTimeRun / 4; ++q)
                *reinterpret_cast<int4 *>(a.dt + (i0 + 4 * q)) = make_int4(dts[4 * q], dts[4 * q + 1], dts[4 * q + 2], dts[4 * q + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < kTimeRun; ++j) {
                const long long i = i0 + j;
                if (i >= a.p0 && i < a.p1) a.dt[i] = dts[j];
            }
        }
    }

    __syncthreads();
    for (int k = threadIdx.x; k < kTimeHash; k += kBlock)
        if (s_cell[k] >= 0) time_to_rasters(a, s_cell[k], s_cell_sum[k], s_cell_zone[k]);
    if (a.per_track == nullptr) return;
    for (int k = threadIdx.x; k < kTimeSlots; k += kBlock) {
        u64 *const sums = a.per_track + 2 * static_cast<long long>(t_first + k);
        if (s_tot[k] != 0) atomicAdd(sums, s_tot[k]);      // (a slot past the tile's last track holds nothing)
        if (s_zone[k] != 0) atomicAdd(sums + 1, s_zone[k]);
    }
}

template <class T>
__device__ __forceinline__ double time_read(const void *p, size_t i)
{
    return static_cast<double>(static_cast<const T *>(p)[i]);
}

// one component of windinfo: clip(rint((-1000 * wspeed) * u)), 0 where that is not a number.  Every product rounds on its own.
__host__ __device__ __forceinline__ int time_wind_component(double wspeed, double u)
{
    const double scaled = -1000.0 * wspeed;
    double v = rint(scaled * u);
    if (v != v) return 0;
    v = v < -kTimeWindClip ? -kTimeWindClip : v > kTimeWindClip ? kTimeWindClip : v;
    return static_cast<int>(v);
}

// windinfo = {wr, wc} (include/ssrs_hip.h): the upwind unit step of K9 (ssrs_shelter_sx), times -wspeed
__global__ __launch_bounds__(kBlock) void k_flight_windinfo(const void *wspeed, const void *wdirn, int type, size_t n, int ray_axes,
                                                            int2 *out)
{
    for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * kBlock) {
        const double ws = type == SSRS_F64 ? time_read<double>(wspeed, i) : time_read<float>(wspeed, i);
        const double wd = type == SSRS_F64 ? time_read<double>(wdirn, i) : time_read<float>(wdirn, i);
        const double rad = wd * 3.141592653589793 / 180.0;
        const double sn = sin(rad), cs = cos(rad);
        const double ur = ray_axes == SSRS_RAY_ROW_NORTH ? cs : sn, uc = ray_axes == SSRS_RAY_ROW_NORTH ? sn : cs;
        out[i] = make_int2(time_wind_component(ws, ur), time_wind_component(ws, uc));
    }
}

}  // namespace ssrs

using namespace ssrs;

extern "C" int ssrs_flight_windinfo(const void *wspeed, const void *wdirn, int type, int rows, int cols, int ray_axes,
                                    int32_t *windinfo, void *stream)
{
    SSRS_REQUIRE(wspeed && wdirn && windinfo, "ssrs_flight_windinfo: NULL pointer");
    SSRS_REQUIRE(type == SSRS_F32 || type == SSRS_F64, "ssrs_flight_windinfo: type = %d (SSRS_F32 or SSRS_F64)", type);
    SSRS_REQUIRE(rows >= 1 && rows <= 32767 && cols >= 1 && cols <= 32767,
                 "ssrs_flight_windinfo: a %d x %d raster (int16 points: 1..32767 either way)", rows, cols);
    SSRS_REQUIRE(ray_axes == SSRS_RAY_ROW_NORTH || ray_axes == SSRS_RAY_ROW_EAST,
                 "ssrs_flight_windinfo: ray_axes = %d (SSRS_RAY_ROW_NORTH or SSRS_RAY_ROW_EAST)", ray_axes);
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(windinfo) & 7u) == 0, "ssrs_flight_windinfo: windinfo must be 8-byte aligned");
    const size_t n = static_cast<size_t>(rows) * static_cast<size_t>(cols);
    const size_t blocks = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_flight_windinfo, dim3(static_cast<unsigned>(blocks < kMaxStreamBlocks ? blocks : kMaxStreamBlocks)),
                       dim3(kBlock), 0, as_stream(stream), wspeed, wdirn, type, n, ray_axes, reinterpret_cast<int2 *>(windinfo));
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

extern "C" int ssrs_track_time(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks, const int16_t *masked,
                               const int32_t *windinfo, int uniform_wr, int uniform_wc, int rows, int cols,
                               const SsrsFlightTimeParams *params, uint64_t *time_hist, uint64_t *band_time_hist,
                               int64_t *per_track, int32_t *dt, void *stream)
{
    SSRS_REQUIRE(traj && traj_offsets && params, "ssrs_track_time: NULL pointer");
    SSRS_REQUIRE(rows >= 1 && rows <= 32767 && cols >= 1 && cols <= 32767,
                 "ssrs_track_time: a %d x %d raster (int16 points: 1..32767 either way)", rows, cols);
    SSRS_REQUIRE(ntracks >= 0 && ntracks <= INT32_MAX, "ssrs_track_time: ntracks = %lld outside [0, 2^31)",
                 static_cast<long long>(ntracks));
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(traj) & 3u) == 0, "ssrs_track_time: traj must be 4-byte aligned");
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(masked) & 3u) == 0, "ssrs_track_time: masked must be 4-byte aligned");
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(windinfo) & 7u) == 0, "ssrs_track_time: windinfo must be 8-byte aligned");
    SSRS_REQUIRE(((reinterpret_cast<uintptr_t>(time_hist) | reinterpret_cast<uintptr_t>(band_time_hist) |
                   reinterpret_cast<uintptr_t>(per_track)) & 7u) == 0,
                 "ssrs_track_time: time_hist, band_time_hist and per_track must be 8-byte aligned");
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(dt) & 3u) == 0, "ssrs_track_time: dt must be 4-byte aligned");
    SSRS_REQUIRE(params->va >= 1 && params->va <= kTimeWindClip, "ssrs_track_time: va = %d mm/s outside [1, 2^20]", params->va);
    SSRS_REQUIRE(params->gmin >= 1 && params->gmin <= params->va, "ssrs_track_time: gmin = %d mm/s outside [1, va = %d]",
                 params->gmin, params->va);
    SSRS_REQUIRE(params->res_mm >= 1 && params->res_mm <= 1000000, "ssrs_track_time: res_mm = %d outside [1, 10^6]",
                 params->res_mm);
    SSRS_REQUIRE(windinfo != nullptr || (uniform_wr >= -kTimeWindClip && uniform_wr <= kTimeWindClip &&
                                         uniform_wc >= -kTimeWindClip && uniform_wc <= kTimeWindClip),
                 "ssrs_track_time: uniform wind (%d, %d) mm/s outside +-2^20", uniform_wr, uniform_wc);
    SSRS_REQUIRE(band_time_hist == nullptr || masked != nullptr, "ssrs_track_time: band_time_hist needs masked");
    if (ntracks == 0) return SSRS_OK;
    hipStream_t st = as_stream(stream);
    if (per_track != nullptr) SSRS_HIP_CHECK(hipMemsetAsync(per_track, 0, static_cast<size_t>(ntracks) * 16, st));

    // the chunk's first and last offset, on the host: the launch is sized from its points
    long long ends[2];
    SSRS_HIP_CHECK(hipMemcpyAsync(&ends[0], traj_offsets, 8, hipMemcpyDeviceToHost, st));
    SSRS_HIP_CHECK(hipMemcpyAsync(&ends[1], traj_offsets + ntracks, 8, hipMemcpyDeviceToHost, st));
    SSRS_HIP_CHECK(hipStreamSynchronize(st));
    SSRS_REQUIRE(ends[0] >= 0, "ssrs_track_time: traj_offsets[0] = %lld is negative", ends[0]);
    SSRS_REQUIRE(ends[1] >= ends[0], "ssrs_track_time: traj_offsets descends (%lld after %lld)", ends[1], ends[0]);
    if (ends[1] == ends[0]) return SSRS_OK;

    TimeArgs a;
    a.traj = reinterpret_cast<const uint32_t *>(traj);
    a.off = reinterpret_cast<const long long *>(traj_offsets);
    a.ntracks = static_cast<int>(ntracks);
    a.rows = rows;
    a.cols = cols;
    a.masked = reinterpret_cast<const uint32_t *>(masked);
    a.windinfo = reinterpret_cast<const int2 *>(windinfo);
    a.uwr = uniform_wr;
    a.uwc = uniform_wc;
    a.p0 = ends[0];
    a.p1 = ends[1];
    const long long va = params->va, res_mm = params->res_mm;
    a.va2 = va * va;
    a.num_orth = res_mm * 1000000;
    a.num_diag = ((res_mm * kTimeSqrt2 + 32768) >> 16) * 1000000;
    a.gmin = params->gmin;
    const long long stay = (a.num_orth + va / 2) / va;
    a.dt_stay = stay > INT_MAX ? INT_MAX : static_cast<int>(stay);
    a.time_hist = reinterpret_cast<u64 *>(time_hist);
    a.band_time_hist = reinterpret_cast<u64 *>(band_time_hist);
    a.per_track = reinterpret_cast<u64 *>(per_track);
    a.dt = dt;
    const long long ntiles = (a.p1 - (a.p0 & ~3LL) + kTimeTile - 1) / kTimeTile;
    const bool vec = ((reinterpret_cast<uintptr_t>(traj) | reinterpret_cast<uintptr_t>(masked) | reinterpret_cast<uintptr_t>(dt)) & 15u) == 0;
    const dim3 grid(static_cast<unsigned>(ntiles)), block(kBlock);
    if (vec) hipLaunchKernelGGL(k_track_time<true>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_track_time<false>, grid, block, 0, st, a);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}
