// K14 -- flight height along every track and rotor-zone presence for gfx950 (MI355X).
//
// This build's own model (the reference has none), in integers so that every grouping of the scan gives
// the same bits.  Heights are int32 millimetres above ground.  Per cell `cellinfo` holds {climb, elev}: the millimetres
// gained on one orthogonal move out of the cell, and the terrain height.  The move from point k to point k + 1 of a track
// adds a_k = step - (elev' - elev), step = climb (times sqrt(2) in 16.16 fixed point on a diagonal), and the height is
// clamped to [floor, ceil] after every move: h_{k+1} = clamp(h_k + a_k).
//   - x -> min(max(x + A, L), H) is closed under composition and the composition is exactly associative, so the heights
//     of a whole chunk are ONE scan of (A, L, H) triples.  A track's first point is the constant (0, h0, h0): it absorbs
//     everything to its left, so the scan needs no segment flags, and every inclusive prefix has L == H, the height;
//   - three launches.  "ops": a block composes the operators of its tile of SSRS_ALTITUDE_TILE consecutive points of
//     the chunk (track borders or not) into one, 16 bytes a tile.  "carry": ONE block scans those in place, leaving each
//     tile the composition of all tiles before it.  "emit": every tile is scanned again behind its carry and writes the
//     outputs.  No block waits for another: kernel boundaries are all the ordering there is;
//   - a lane takes kAltRun consecutive points serially (four 16-byte loads when the buffers are 16-byte aligned) and one
//     8-byte cellinfo load a point, all 17 of a run issued before anything waits for one (a move's other cell is the
//     lane's previous point); the 256 lane operators of a block are scanned in LDS (Hillis-Steele, two buffers);
//   - the tile's first and last track come from two binary searches of the offsets (lanes 0 and 1 of "ops", which leaves
//     them in the workspace, 8 bytes a tile, for "emit"); every lane then searches between them only -- nothing at all
//     inside a long track -- and walks the offsets from there, over empty tracks and track ends inside its run, as
//     K13's lanes do;
//   - per-track in_band / h_min / h_max: a lane combines in registers, the block in LDS slots (track - the tile's first
//     track, 256 of them), and one lane per touched slot goes to global memory: a track costs three atomics a tile it
//     lies in.  Tracks past the slots (more than 256 tracks in a tile: they are short) go to global memory by lane;
//   - band_hist takes one atomic per run of consecutive in-band points of a lane in one cell.
// Block cooperation is __shared__ + __syncthreads() only (no shuffles, ballots or DPP), so tests/hip_host_stub runs this
// file's own code on the CPU.  Integer adds, mins and maxes: the result does not depend on the launch order.
#include <climits>

#include "common.h"

namespace ssrs {

constexpr int kAltRun = 16;                                // consecutive points a lane takes
constexpr int kAltTile = SSRS_ALTITUDE_TILE;               // points a block takes
static_assert(kAltTile == kBlock * kAltRun, "a tile is one run per lane of a block");
constexpr int kAltSlots = 256;                             // LDS slots for the per-track outputs of a tile
constexpr long long kAltSqrt2 = 92682;                     // round(sqrt(2) * 2^16)

// x -> min(max(x + A, L), H).  16 bytes: the workspace holds one per tile.
struct AltOp {
    long long A;
    int L, H;
};

__host__ __device__ __forceinline__ int alt_clamp(long long x, int lo, int hi)
{
    return static_cast<int>(x < lo ? lo : x > hi ? hi : x);
}

// f, then g.  A constant (L == H) keeps A = 0: the value is the same function, and A stays the sum of ONE track's moves
__host__ __device__ __forceinline__ AltOp alt_then(const AltOp &f, const AltOp &g)
{
    AltOp o;
    o.L = alt_clamp(f.L + g.A, g.L, g.H);
    o.H = alt_clamp(f.H + g.A, g.L, g.H);
    o.A = o.L == o.H ? 0 : f.A + g.A;
    return o;
}

// Inclusive scan, in lane order, of one operator per thread of the block; returns this thread's EXCLUSIVE prefix behind
// `carry` (thread 0: `carry` itself) and leaves the block's total in *total when it is asked for.
__device__ __forceinline__ AltOp alt_block_scan(const AltOp mine, const AltOp carry, AltOp *total)
{
    __shared__ AltOp s_op[2][kBlock];
    const int i = threadIdx.x;
    int cur = 0;
    s_op[0][i] = mine;
    __syncthreads();
    for (int d = 1; d < kBlock; d *= 2) {
        const AltOp v = i >= d ? alt_then(s_op[cur][i - d], s_op[cur][i]) : s_op[cur][i];
        s_op[cur ^ 1][i] = v;
        cur ^= 1;
        __syncthreads();                         // (the buffer read in this round is written in the next one only)
    }
    if (total != nullptr) *total = s_op[cur][kBlock - 1];
    const AltOp before = i > 0 ? alt_then(carry, s_op[cur][i - 1]) : carry;
    __syncthreads();                             // (the next call of a block writes s_op[0])
    return before;
}

struct AltArgs {
    const uint32_t *traj;          // one int16 (row, col) pair per dword
    const long long *off;          // ntracks + 1 offsets
    int ntracks;
    int rows, cols;
    const int2 *cellinfo;          // {climb, elev} per cell
    long long p0, p1;              // the chunk's points: off[0], off[ntracks]
    int h0, floor, ceil, band_lo, band_hi;
    AltOp *tile_ops;               // the workspace: an operator per tile,
    int2 *tile_tracks;             // then the first and the last track of every tile ("ops" finds them, "emit" reuses them)
    int *alt;
    uint32_t *band_hist;
    uint32_t *traj_band;
    int *in_band, *h_min, *h_max;
};

__device__ __forceinline__ bool alt_inside(uint32_t pt, int rows, int cols, int &r, int &c)
{
    r = static_cast<int16_t>(pt & 0xFFFF);
    c = static_cast<int16_t>(pt >> 16);
    return r >= 0 && c >= 0 && r < rows && c < cols;
}

// a_k of the move prev -> cur between two cells inside the raster (0 otherwise), from their cellinfo
__device__ __forceinline__ long long alt_move(uint32_t prev, uint32_t cur, bool both_in, int2 ci_prev, int2 ci_cur)
{
    const bool diagonal = (prev & 0xFFFFu) != (cur & 0xFFFFu) && (prev >> 16) != (cur >> 16);
    const int step = diagonal ? static_cast<int>((static_cast<long long>(ci_prev.x) * kAltSqrt2 + 32768) >> 16) : ci_prev.x;
    const long long dz = ci_prev.y == INT_MIN || ci_cur.y == INT_MIN ? 0 : static_cast<long long>(ci_cur.y) - ci_prev.y;
    return both_in ? step - dz : 0;
}

// The walk of one lane over its run of a tile: the points, their tracks and their moves.  Used by both kernels.
struct AltLane {
    long long i0;                  // index of the run's first point
    uint32_t pts[kAltRun];
    uint32_t before;               // the point in front of the run
    uint32_t inside;               // bit j: point j is a point of the chunk inside the raster; bit kAltRun: `before` is
    int2 cells[kAltRun + 1];       // cellinfo of `before` and of the points, where `inside` says so
    int t;                         // track of the run's first valid point
    long long t_begin, t_end;      // its offsets
};

// kVec: traj (and alt, traj_band) are 16-byte aligned.  Loads the lane's run; points outside [p0, p1) are not read.
template <bool kVec>
__device__ __forceinline__ void alt_load(const AltArgs &a, long long tile, AltLane &w)
{
    const long long a0 = a.p0 & ~3LL;                      // tiles are cut at multiples of four points of the BUFFER
    const long long t0 = a0 + tile * kAltTile;
    w.i0 = t0 + static_cast<long long>(threadIdx.x) * kAltRun;
    if (kVec && t0 >= a.p0 && t0 + kAltTile <= a.p1) {
#pragma unroll
        for (int q = 0; q < kAltRun / 4; ++q) {
            const uint4 v = *reinterpret_cast<const uint4 *>(a.traj + (w.i0 + 4 * q));
            w.pts[4 * q + 0] = v.x, w.pts[4 * q + 1] = v.y, w.pts[4 * q + 2] = v.z, w.pts[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < kAltRun; ++j) {
            const long long i = w.i0 + j;
            w.pts[j] = i >= a.p0 && i < a.p1 ? a.traj[i] : 0u;
        }
    }
    w.before = w.i0 > a.p0 && w.i0 <= a.p1 ? a.traj[w.i0 - 1] : 0u;
}

// The cellinfo of the lane's points: one 8-byte load each, all of them independent of one another and of the track walk
// (a move's other cell is the lane's previous point, so `before` is the only extra load).
__device__ __forceinline__ void alt_gather(const AltArgs &a, AltLane &w)
{
    w.inside = 0;
    int r, c;
    w.cells[0] = make_int2(0, INT_MIN);
    if (w.i0 > a.p0 && w.i0 <= a.p1 && alt_inside(w.before, a.rows, a.cols, r, c)) {
        w.cells[0] = a.cellinfo[static_cast<long long>(r) * a.cols + c];
        w.inside |= 1u << kAltRun;
    }
#pragma unroll
    for (int j = 0; j < kAltRun; ++j) {
        const long long i = w.i0 + j;
        w.cells[j + 1] = make_int2(0, INT_MIN);
        if (i >= a.p0 && i < a.p1 && alt_inside(w.pts[j], a.rows, a.cols, r, c)) {
            w.cells[j + 1] = a.cellinfo[static_cast<long long>(r) * a.cols + c];
            w.inside |= 1u << j;
        }
    }
}

// The track that holds the lane's first valid point: the LAST one that starts at or before it, searched between the
// tile's first and last track (s_t).  kSearch ("ops"): lanes 0 and 1 find those two over all offsets and leave them in
// tile_tracks; otherwise ("emit") they are read from there.  One barrier; every thread of the block must call it.
template <bool kSearch>
__device__ __forceinline__ void alt_find_track(const AltArgs &a, long long tile, AltLane &w, int *s_t)
{
    const long long a0 = a.p0 & ~3LL;
    const long long first = a0 + tile * kAltTile > a.p0 ? a0 + tile * kAltTile : a.p0;
    const long long last = a0 + (tile + 1) * kAltTile < a.p1 ? a0 + (tile + 1) * kAltTile - 1 : a.p1 - 1;
    if (threadIdx.x < 2) {
        int lo = 0;
        if (kSearch) {
            const long long key = threadIdx.x == 0 ? first : last;
            int hi = a.ntracks;
            while (hi - lo > 1) {
                const int mid = lo + (hi - lo) / 2;
                if (a.off[mid] <= key) lo = mid; else hi = mid;
            }
            reinterpret_cast<int *>(a.tile_tracks + tile)[threadIdx.x] = lo;
        } else {
            lo = reinterpret_cast<const int *>(a.tile_tracks + tile)[threadIdx.x];
        }
        s_t[threadIdx.x] = lo;
    }
    __syncthreads();
    long long key = w.i0 > first ? w.i0 : first;
    key = key < last ? key : last;                         // (lanes past the end: any track of the tile will do)
    int lo = s_t[0], hi = s_t[1] + 1;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (a.off[mid] <= key) lo = mid; else hi = mid;
    }
    w.t = lo;
    w.t_begin = a.off[lo];
    w.t_end = a.off[lo + 1];
}

// The lane's operator: its valid points composed in order (a run without one gives a placeholder that nothing reads:
// such runs lie in front of the chunk's first point, a constant, or behind its last).  moves[j] is a_{i-1} of point
// i = i0 + j, whatever it is at a track's first point; starts bit j: point j is its track's first.
__device__ __forceinline__ AltOp alt_lane_op(const AltArgs &a, const AltLane &w, long long *moves, uint32_t &starts)
{
    AltOp op{0, 0, 0};
    bool have = false;                                     // op holds a point
    long long t_begin = w.t_begin, t_end = w.t_end;
    int t = w.t;
    starts = 0;
#pragma unroll
    for (int j = 0; j < kAltRun; ++j) {
        const bool prev_in = w.inside >> (j == 0 ? kAltRun : j - 1) & 1u;
        moves[j] = alt_move(j == 0 ? w.before : w.pts[j - 1], w.pts[j], prev_in && (w.inside >> j & 1u), w.cells[j],
                            w.cells[j + 1]);
    }
#pragma unroll
    for (int j = 0; j < kAltRun; ++j) {
        const long long i = w.i0 + j;
        if (i >= a.p0 && i < a.p1) {
            while (t_end <= i) {                           // (i < p1 = off[ntracks]: the walk stops below ntracks)
                ++t;
                t_begin = t_end;
                t_end = a.off[t + 1];
            }
            if (i == t_begin) {
                starts |= 1u << j;
                op = AltOp{0, a.h0, a.h0};                 // (a constant absorbs what stands in front of it)
            } else {
                const AltOp move{a.floor == a.ceil ? 0 : moves[j], a.floor, a.ceil};
                op = have ? alt_then(op, move) : move;
            }
            have = true;
        }
    }
    return op;
}

// Launch 1: the tile's operator.  Also the initial values of the per-track outputs (this launch is ahead of "emit").
template <bool kVec>
__global__ __launch_bounds__(kBlock) void k_altitude_ops(const AltArgs a)
{
    __shared__ int s_t[2];
    for (long long k = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; k < a.ntracks;
         k += static_cast<long long>(gridDim.x) * kBlock) {
        if (a.in_band != nullptr) a.in_band[k] = 0;
        if (a.h_min != nullptr) a.h_min[k] = INT_MAX;
        if (a.h_max != nullptr) a.h_max[k] = INT_MIN;
    }
    AltLane w;
    alt_load<kVec>(a, blockIdx.x, w);
    alt_gather(a, w);                                      // (in flight during the searches)
    alt_find_track<true>(a, blockIdx.x, w, s_t);
    long long moves[kAltRun];
    uint32_t starts;
    const AltOp mine = alt_lane_op(a, w, moves, starts);
    AltOp total;
    alt_block_scan(mine, AltOp{0, 0, 0}, &total);
    if (threadIdx.x == 0) a.tile_ops[blockIdx.x] = total;
}

// Launch 2: ONE block turns the tiles' operators into their exclusive prefixes, in place.  Tile 0 gets a placeholder:
// its first point is a track's first.
__global__ __launch_bounds__(kBlock) void k_altitude_carry(AltOp *ops, long long ntiles)
{
    const long long per = (ntiles + kBlock - 1) / kBlock;
    const long long b = static_cast<long long>(threadIdx.x) * per;
    const long long e = b + per < ntiles ? b + per : ntiles;
    AltOp mine{0, 0, 0};
    for (long long k = b; k < e; ++k) mine = k == b ? ops[k] : alt_then(mine, ops[k]);
    AltOp carry = alt_block_scan(mine, AltOp{0, 0, 0}, nullptr);
    for (long long k = b; k < e; ++k) {
        const AltOp op = ops[k];
        ops[k] = carry;
        carry = alt_then(carry, op);
    }
}

// Launch 3: the heights of the tile's points behind its carry, and the outputs.
template <bool kVec>
__global__ __launch_bounds__(kBlock) void k_altitude_emit(const AltArgs a)
{
    __shared__ int s_t[2];
    __shared__ int s_cnt[kAltSlots], s_min[kAltSlots], s_max[kAltSlots];
    const bool per_track = a.in_band != nullptr || a.h_min != nullptr || a.h_max != nullptr;
    for (int k = threadIdx.x; k < kAltSlots; k += kBlock) s_cnt[k] = 0, s_min[k] = INT_MAX, s_max[k] = INT_MIN;
    AltLane w;
    alt_load<kVec>(a, blockIdx.x, w);
    alt_gather(a, w);                                      // (in flight during the searches)
    alt_find_track<false>(a, blockIdx.x, w, s_t);          // (its barrier covers the slots' initial values too)
    long long moves[kAltRun];
    uint32_t starts;
    const AltOp mine = alt_lane_op(a, w, moves, starts);
    const uint32_t inside = w.inside;
    const AltOp before = alt_block_scan(mine, a.tile_ops[blockIdx.x], nullptr);
    const int t_first = s_t[0];

    int h = before.L;                                      // (L == H behind any track's first point)
    int t = w.t;
    long long t_end = w.t_end;
    int cnt = 0, lo = INT_MAX, hi = INT_MIN;               // of track t, by this lane
    auto flush = [&]() {
        if (per_track && lo <= hi) {
            const int slot = t - t_first;
            if (slot < kAltSlots) {
                if (cnt != 0) atomicAdd(&s_cnt[slot], cnt);
                atomicMin(&s_min[slot], lo);
                atomicMax(&s_max[slot], hi);
            } else {
                if (a.in_band != nullptr && cnt != 0) atomicAdd(a.in_band + t, cnt);
                if (a.h_min != nullptr) atomicMin(a.h_min + t, lo);
                if (a.h_max != nullptr) atomicMax(a.h_max + t, hi);
            }
        }
        cnt = 0, lo = INT_MAX, hi = INT_MIN;
    };
    long long run_cell = -1;                               // consecutive in-band points in one cell: one atomic
    uint32_t run_n = 0;
    int heights[kAltRun];
    uint32_t masked[kAltRun];
#pragma unroll
    for (int j = 0; j < kAltRun; ++j) {
        const long long i = w.i0 + j;
        heights[j] = 0;
        masked[j] = 0xFFFFFFFFu;                           // (-1, -1)
        if (i < a.p0 || i >= a.p1) continue;
        while (t_end <= i) {
            flush();
            ++t;
            t_end = a.off[t + 1];
        }
        h = starts >> j & 1u ? a.h0 : alt_clamp(h + moves[j], a.floor, a.ceil);
        heights[j] = h;
        lo = h < lo ? h : lo;
        hi = h > hi ? h : hi;
        if ((inside >> j & 1u) && h >= a.band_lo && h <= a.band_hi) {
            masked[j] = w.pts[j];
            ++cnt;
            if (a.band_hist != nullptr) {
                const long long cell = static_cast<long long>(static_cast<int16_t>(w.pts[j] & 0xFFFF)) * a.cols +
                                       static_cast<int16_t>(w.pts[j] >> 16);
                if (cell != run_cell) {
                    if (run_n != 0) atomicAdd(a.band_hist + run_cell, run_n);
                    run_cell = cell, run_n = 0;
                }
                ++run_n;
            }
        }
    }
    flush();
    if (run_n != 0) atomicAdd(a.band_hist + run_cell, run_n);

    const long long a0 = a.p0 & ~3LL;
    const long long tile0 = a0 + static_cast<long long>(blockIdx.x) * kAltTile;
    if (kVec && tile0 >= a.p0 && tile0 + kAltTile <= a.p1) {
#pragma unroll
        for (int q = 0; q < kAltRun / 4; ++q) {
            if (a.alt != nullptr)
                *reinterpret_cast<int4 *>(a.alt + (w.i0 + 4 * q)) =
                    make_int4(heights[4 * q], heights[4 * q + 1], heights[4 * q + 2], heights[4 * q + 3]);
            if (a.traj_band != nullptr)
                *reinterpret_cast<uint4 *>(a.traj_band + (w.i0 + 4 * q)) =
                    make_uint4(masked[4 * q], masked[4 * q + 1], masked[4 * q + 2], masked[4 * q + 3]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < kAltRun; ++j) {
            const long long i = w.i0 + j;
            if (i < a.p0 || i >= a.p1) continue;
            if (a.alt != nullptr) a.alt[i] = heights[j];
            if (a.traj_band != nullptr) a.traj_band[i] = masked[j];
        }
    }

    if (!per_track) return;                                // (uniform over the block)
    __syncthreads();
    for (int k = threadIdx.x; k < kAltSlots; k += kBlock) {
        if (s_min[k] > s_max[k]) continue;                 // (no point of that track in this tile)
        const int tr = t_first + k;
        if (a.in_band != nullptr && s_cnt[k] != 0) atomicAdd(a.in_band + tr, s_cnt[k]);
        if (a.h_min != nullptr) atomicMin(a.h_min + tr, s_min[k]);
        if (a.h_max != nullptr) atomicMax(a.h_max + tr, s_max[k]);
    }
}

template <class T>
__device__ __forceinline__ double alt_read(const void *p, size_t i)
{
    return static_cast<double>(static_cast<const T *>(p)[i]);
}

// cellinfo = {climb, elev} (include/ssrs_hip.h).  The product and the subtraction round on their own.
__global__ __launch_bounds__(kBlock) void k_altitude_cellinfo(const void *updraft, int updraft_type, const void *dem,
                                                              int dem_type, size_t n, double sink, double scale, int2 *out)
{
    for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * kBlock) {
        double w = updraft_type == SSRS_F64 ? alt_read<double>(updraft, i) : alt_read<float>(updraft, i);
        const double z = dem_type == SSRS_F64 ? alt_read<double>(dem, i) : alt_read<float>(dem, i);
        if (w != w) w = 0.0;
        const double lift = w - sink;
        double climb = rint(lift * scale);
        climb = climb < -67108864.0 ? -67108864.0 : climb > 67108864.0 ? 67108864.0 : climb;          // 2^26
        int elev = INT_MIN;
        if (z == z) {
            double e = rint(1000.0 * z);
            e = e < -1073741824.0 ? -1073741824.0 : e > 1073741824.0 ? 1073741824.0 : e;              // 2^30
            elev = static_cast<int>(e);
        }
        out[i] = make_int2(static_cast<int>(climb), elev);
    }
}

inline long long alt_tiles(long long p0, long long p1)
{
    return (p1 - (p0 & ~3LL) + kAltTile - 1) / kAltTile;
}

}  // namespace ssrs

using namespace ssrs;

extern "C" int ssrs_altitude_cellinfo(const void *updraft, int updraft_type, const void *dem, int dem_type, int rows, int cols,
                                      double sink, double scale, int32_t *cellinfo, void *stream)
{
    SSRS_REQUIRE(updraft && dem && cellinfo, "ssrs_altitude_cellinfo: NULL pointer");
    SSRS_REQUIRE((updraft_type == SSRS_F32 || updraft_type == SSRS_F64) && (dem_type == SSRS_F32 || dem_type == SSRS_F64),
                 "ssrs_altitude_cellinfo: updraft_type = %d, dem_type = %d (SSRS_F32 or SSRS_F64)", updraft_type, dem_type);
    SSRS_REQUIRE(rows >= 1 && rows <= 32767 && cols >= 1 && cols <= 32767,
                 "ssrs_altitude_cellinfo: a %d x %d raster (int16 points: 1..32767 either way)", rows, cols);
    SSRS_REQUIRE(sink == sink && scale == scale, "ssrs_altitude_cellinfo: sink = %g, scale = %g (NaN)", sink, scale);
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(cellinfo) & 7u) == 0, "ssrs_altitude_cellinfo: cellinfo must be 8-byte aligned");
    const size_t n = static_cast<size_t>(rows) * static_cast<size_t>(cols);
    const size_t blocks = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_altitude_cellinfo, dim3(static_cast<unsigned>(blocks < kMaxStreamBlocks ? blocks : kMaxStreamBlocks)),
                       dim3(kBlock), 0, as_stream(stream), updraft, updraft_type, dem, dem_type, n, sink, scale,
                       reinterpret_cast<int2 *>(cellinfo));
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

extern "C" size_t ssrs_track_altitude_workspace_bytes(int64_t npoints)
{
    if (npoints < 0) return 0;
    // (a chunk whose first point is not a multiple of four points into the buffer may take one tile more)
    const size_t tiles = static_cast<size_t>(npoints) / kAltTile + 2;
    return (tiles * (sizeof(AltOp) + sizeof(int2)) + 255) / 256 * 256;
}

extern "C" int ssrs_track_altitude(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks, const int32_t *cellinfo,
                                   int rows, int cols, const SsrsAltitudeParams *params, int32_t *alt, uint32_t *band_hist,
                                   int16_t *traj_band, int32_t *in_band, int32_t *h_min, int32_t *h_max, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    static_assert(sizeof(AltOp) == 16, "one operator is 16 bytes");
    SSRS_REQUIRE(traj && traj_offsets && cellinfo && params && workspace, "ssrs_track_altitude: NULL pointer");
    SSRS_REQUIRE(rows >= 1 && rows <= 32767 && cols >= 1 && cols <= 32767,
                 "ssrs_track_altitude: a %d x %d raster (int16 points: 1..32767 either way)", rows, cols);
    SSRS_REQUIRE(ntracks >= 0 && ntracks <= INT32_MAX, "ssrs_track_altitude: ntracks = %lld outside [0, 2^31)",
                 static_cast<long long>(ntracks));
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(traj) & 3u) == 0, "ssrs_track_altitude: traj must be 4-byte aligned");
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(traj_band) & 3u) == 0, "ssrs_track_altitude: traj_band must be 4-byte aligned");
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(cellinfo) & 7u) == 0, "ssrs_track_altitude: cellinfo must be 8-byte aligned");
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15u) == 0, "ssrs_track_altitude: workspace must be 16-byte aligned");
    SSRS_REQUIRE(params->floor <= params->ceil, "ssrs_track_altitude: floor = %d above ceil = %d", params->floor, params->ceil);
    SSRS_REQUIRE(params->band_lo <= params->band_hi, "ssrs_track_altitude: band_lo = %d above band_hi = %d", params->band_lo,
                 params->band_hi);
    SSRS_REQUIRE(workspace_bytes >= ssrs_track_altitude_workspace_bytes(0),
                 "ssrs_track_altitude: workspace of %zu bytes, %zu needed at least", workspace_bytes,
                 ssrs_track_altitude_workspace_bytes(0));
    if (ntracks == 0) return SSRS_OK;
    hipStream_t st = as_stream(stream);

    // the chunk's first and last offset, on the host: the launches are sized from its points
    long long ends[2];
    SSRS_HIP_CHECK(hipMemcpyAsync(&ends[0], traj_offsets, 8, hipMemcpyDeviceToHost, st));
    SSRS_HIP_CHECK(hipMemcpyAsync(&ends[1], traj_offsets + ntracks, 8, hipMemcpyDeviceToHost, st));
    SSRS_HIP_CHECK(hipStreamSynchronize(st));
    SSRS_REQUIRE(ends[0] >= 0, "ssrs_track_altitude: traj_offsets[0] = %lld is negative", ends[0]);
    SSRS_REQUIRE(ends[1] >= ends[0], "ssrs_track_altitude: traj_offsets descends (%lld after %lld)", ends[1], ends[0]);
    if (ends[1] == ends[0]) return SSRS_OK;
    SSRS_REQUIRE(workspace_bytes >= ssrs_track_altitude_workspace_bytes(ends[1] - ends[0]),
                 "ssrs_track_altitude: workspace of %zu bytes, %zu needed for %lld points", workspace_bytes,
                 ssrs_track_altitude_workspace_bytes(ends[1] - ends[0]), ends[1] - ends[0]);

    AltArgs a;
    a.traj = reinterpret_cast<const uint32_t *>(traj);
    a.off = reinterpret_cast<const long long *>(traj_offsets);
    a.ntracks = static_cast<int>(ntracks);
    a.rows = rows;
    a.cols = cols;
    a.cellinfo = reinterpret_cast<const int2 *>(cellinfo);
    a.p0 = ends[0];
    a.p1 = ends[1];
    a.floor = params->floor;
    a.ceil = params->ceil;
    a.h0 = alt_clamp(params->start, params->floor, params->ceil);
    a.band_lo = params->band_lo;
    a.band_hi = params->band_hi;
    a.tile_ops = static_cast<AltOp *>(workspace);
    a.alt = alt;
    a.band_hist = band_hist;
    a.traj_band = reinterpret_cast<uint32_t *>(traj_band);
    a.in_band = in_band;
    a.h_min = h_min;
    a.h_max = h_max;
    const long long ntiles = alt_tiles(a.p0, a.p1);
    a.tile_tracks = reinterpret_cast<int2 *>(a.tile_ops + ntiles);
    const bool vec = ((reinterpret_cast<uintptr_t>(traj) | reinterpret_cast<uintptr_t>(alt) |
                       reinterpret_cast<uintptr_t>(traj_band)) & 15u) == 0;
    const dim3 grid(static_cast<unsigned>(ntiles)), block(kBlock);
    if (vec) hipLaunchKernelGGL(k_altitude_ops<true>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_altitude_ops<false>, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_altitude_carry, dim3(1), block, 0, st, a.tile_ops, ntiles);
    if (vec) hipLaunchKernelGGL(k_altitude_emit<true>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_altitude_emit<false>, grid, block, 0, st, a);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}
