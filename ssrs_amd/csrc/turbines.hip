// K8 -- turbine encounters for gfx950 (MI355X).
//
// Which simulated tracks came within R of which turbine, and after how many moves: the per-turbine number the
// reference's half-written get_turbine_presence (ssrs/simulator.py:594-607) was after, from the trajectories
// the stepper leaves on the device.  One streaming pass over the int16 (row, col) points, 4 B each:
//   - a wave owns a contiguous run of 256-point spans; a lane takes four consecutive points (one 16-byte load
//     when the buffer is 16-byte aligned), and the next span's load is issued before this one is worked on;
//   - the common point has no turbine near it: one lookup in a bit-per-bin mask in LDS (bins of 32 x 32 cells,
//     3.7 KB at 5000 x 6000) and nothing else.  Only points of occupied bins walk the bin's turbine list;
//   - a wave finds the track of its first point by ONE binary search, then advances along traj_offsets: a span
//     inside one track is one scalar load; a span that crosses track ends marks the starts of the tracks that
//     begin in it in LDS and takes a running maximum (any number of tracks per span, empty ones included);
//   - hits are ORed and first steps min-ed, both order-independent integers.  A track that sits in a disk for
//     millions of moves costs neither: every lane remembers the last bitmap word / first step it knows to be
//     settled, an unknown one is tested with a load (bits are only ever set and steps only ever fall, so a stale
//     read costs a redundant atomic, never a wrong result), and the lanes of a wave that still have news for
//     the same word combine it before ONE atomic.
//
// K15 -- rotor encounters: the same walk (kRotor) with a cylinder per turbine instead of one disk for all.  The height
// above ground of every point streams in next to it (4 B more), the elevation of its cell is gathered only in occupied
// bins, and the test is reach_t in the plane and z_lo_t <= elev + alt <= z_hi_t in 64-bit millimetres.  The exposure
// (points inside each cylinder) is counted without an atomic per point: a lane keeps ONE (turbine, count) pair in
// registers across its points and spans and adds it to the block's uint32 counter in LDS only when the turbine changes
// or the wave ends; the block adds its non-zero counters to the uint64 totals once, at its end.
//
// K15, timed (kTimed) -- the exposure in microseconds: dt[i] of every point inside a cylinder is added to that turbine's
// total.  dt is loaded only for a point that hit (the common point still costs one mask lookup; 4 B more per point INSIDE a
// cylinder, and a parked track's hits are consecutive points, so those loads coalesce).  The lane's pair becomes (turbine,
// count, time) with the time in 64 bits, the block keeps a uint64 counter per turbine in LDS behind the uint32 ones, and
// adds the non-zero ones once.  The LDS rule is in the header: the mask goes first, then the time counters of the highest
// turbines, whose hand-overs become global 64-bit adds.
#include <climits>

#include "common.h"

namespace ssrs {

constexpr int kTurbWaves = kBlock / 64;
constexpr int kTurbSpan = 256;                // points per wave and iteration: 64 lanes x 4
constexpr long long kTurbMinSpans = 4;        // spans per wave at least: small inputs advance the track cursor too
// Six blocks per CU.  With the mask of a 5000 x 6000 raster (8 KB of LDS a block, 70 VGPRs: 7 waves per SIMD) all of them
// are resident at once; a mask near the 32 KB limit leaves room for four per CU and the rest run as a second round.
// Nothing but speed depends on it: the blocks do not talk to each other.
constexpr int kTurbBlocks = 256 * 6;
constexpr int kTurbMaskWords = 8192;          // 32 KB of LDS: rasters of up to 262 144 bins keep the mask there
constexpr int kRotorLdsWords = 15 * 1024;     // K15: mask and exposure counters (4 B a turbine) together, 60 KB
// (timed: 4 + 8 B a turbine; without the mask that many turbines keep every counter in LDS)
static_assert(kRotorLdsWords / 3 == SSRS_ROTOR_TIMED_LDS_TURBINES, "the header's LDS rule");

__device__ __forceinline__ int wave_or(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ unsigned wave_min(unsigned v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = static_cast<unsigned>(__shfl_xor(static_cast<int>(v), off));
        v = o < v ? o : v;
    }
    return v;
}

// a load that is served by L2, where the atomics land (the vector L1 would keep handing out the stale line)
__device__ __forceinline__ uint32_t load_l2(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct TurbArgs {
    const uint32_t *traj;          // one int16 (row, col) pair per dword
    const long long *off;
    long long ntracks;
    const double *turb;
    int nturb;
    double r2;
    const int *bin_start, *bin_items;
    int rows, cols, nbc, nbins, words;
    uint32_t *hits, *first_step;
    // kRotor only
    const int32_t *alt;            // mm above ground, indexed like traj
    const int32_t *cellinfo;       // {climb, elev} per cell
    const double *reach;           // cells, per turbine
    const int2 *zband;             // {z_lo, z_hi} mm above the datum, per turbine
    unsigned long long *points;    // per turbine, or NULL
    int cnt_off;                   // the block's counters: s_mask[cnt_off + turbine]
    // kTimed only
    const int32_t *dt;             // microseconds of the move that leaves the point, indexed like traj
    unsigned long long *time;      // per turbine
    int time_off;                  // the block's time counters: 8-byte words from s_mask + time_off (even)
    int time_lds;                  // turbines [0, time_lds) have one; the others' hand-overs go to `time`
};

// The walk of one wave over its spans (no barrier inside: a wave without spans returns at once).
// kVec: 16-byte loads (traj, and alt with it, are 16-byte aligned).  kMask: the occupied-bin mask fits LDS.
// kRotor: K15's cylinders; s_cnt = the block's exposure counters, or NULL when they are not asked for.
// kTimed (with kRotor): the time inside the cylinders too; s_time = the block's time counters.
template <bool kVec, bool kMask, bool kRotor, bool kTimed>
__device__ __forceinline__ void turbine_walk(const TurbArgs &a, const uint32_t *s_mask, uint32_t *s_cnt,
                                             unsigned long long *s_time, int (*s_mark)[kTurbSpan], const long long p0,
                                             const long long p1, const long long a0, const long long nspans,
                                             const long long per_wave)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    int *mark = s_mark[wave];
    const long long u0 = (static_cast<long long>(blockIdx.x) * kTurbWaves + wave) * per_wave;
    const long long u1 = u0 + per_wave < nspans ? u0 + per_wave : nspans;
    if (u0 >= u1) return;                        // (no barrier below this line)

    // the last track that starts at or before the wave's first point: the one that holds it
    long long t;
    {
        const long long first = a0 + u0 * kTurbSpan;
        const long long key = first > p0 ? first : p0;
        long long lo = 0, hi = a.ntracks;
        while (hi - lo > 1) {
            const long long mid = lo + (hi - lo) / 2;
            if (a.off[mid] <= key) lo = mid; else hi = mid;
        }
        t = lo;
    }

    // A lane's four points of span u.  fetch: one 16-byte load without a branch around it, for spans that end at or
    // before p1 (points in front of p0 belong to the buffer: a0 >= 0; they are masked later).  fetch_edge: point by point.
    auto fetch = [&](long long u) {
        return *reinterpret_cast<const uint4 *>(a.traj + (a0 + u * kTurbSpan + 4 * lane));
    };
    auto fetch_edge = [&](long long u) {
        const long long i0 = a0 + u * kTurbSpan + 4 * lane;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (i0 + 0 >= p0 && i0 + 0 < p1) v.x = a.traj[i0 + 0];
        if (i0 + 1 >= p0 && i0 + 1 < p1) v.y = a.traj[i0 + 1];
        if (i0 + 2 >= p0 && i0 + 2 < p1) v.z = a.traj[i0 + 2];
        if (i0 + 3 >= p0 && i0 + 3 < p1) v.w = a.traj[i0 + 3];
        return v;
    };
    // (kRotor) the heights of the same four points, fetched the same way; without kRotor nothing is read
    auto fetch_alt = [&](long long u) {
        if constexpr (!kRotor) return make_int4(0, 0, 0, 0);
        else return *reinterpret_cast<const int4 *>(a.alt + (a0 + u * kTurbSpan + 4 * lane));
    };
    auto fetch_alt_edge = [&](long long u) {
        int4 v = make_int4(0, 0, 0, 0);
        if constexpr (kRotor) {
            const long long i0 = a0 + u * kTurbSpan + 4 * lane;
            if (i0 + 0 >= p0 && i0 + 0 < p1) v.x = a.alt[i0 + 0];
            if (i0 + 1 >= p0 && i0 + 1 < p1) v.y = a.alt[i0 + 1];
            if (i0 + 2 >= p0 && i0 + 2 < p1) v.z = a.alt[i0 + 2];
            if (i0 + 3 >= p0 && i0 + 3 < p1) v.w = a.alt[i0 + 3];
        }
        return v;
    };

    // what this lane knows to be settled: the bits of one bitmap word, the first step of one track
    long long known_word = -1, known_track = -1, known_start = 0;
    uint32_t known_bits = 0, known_step = 0xFFFFFFFFu;
    // (kRotor) the exposure this lane has not handed to the block yet: pend_cnt points inside turbine pend_tb
    int pend_tb = 0;
    uint32_t pend_cnt = 0;
    // (kTimed) and their time, modulo 2^64: the pair is kept whether or not the points are asked for
    unsigned long long pend_time = 0;
    auto hand_over = [&]() {
        if (s_cnt != nullptr) atomicAdd(&s_cnt[pend_tb], pend_cnt);
        if (pend_time != 0) {
            if (pend_tb < a.time_lds) atomicAdd(&s_time[pend_tb], pend_time);
            else atomicAdd(a.time + pend_tb, pend_time);
        }
        pend_cnt = 0;
        pend_time = 0;
    };

    // one span: `cur` its points (`cur_alt` their heights), `t_end` = off[t + 1]
    auto span = [&](const long long u, const uint4 cur, const int4 cur_alt, const long long t_end) {
        const long long s = a0 + u * kTurbSpan, s_end = s + kTurbSpan;
        const long long i0 = s + 4 * lane;
        const uint32_t pts[4] = {cur.x, cur.y, cur.z, cur.w};
        const int alts[4] = {cur_alt.x, cur_alt.y, cur_alt.z, cur_alt.w};

        // ---- the track of every point: off[t] <= max(s, p0), and every later track starts at or after s
        int rel[4] = {0, 0, 0, 0};
        int span_rel = 0;
        if (t_end < s_end) {
            *reinterpret_cast<int4 *>(mark + 4 * lane) = make_int4(0, 0, 0, 0);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // a track that is not empty and starts inside the span marks its first point (starts are distinct)
            for (long long tb = t + 1;; tb += 64) {
                const long long tt = tb + lane;
                long long o = LLONG_MAX;
                if (tt < a.ntracks) {
                    o = a.off[tt];
                    if (o >= s && o < s_end && a.off[tt + 1] > o) mark[o - s] = static_cast<int>(tt - t);
                }
                const long long last = __shfl(o, 63);
                if (last >= s_end) break;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const int4 m = *reinterpret_cast<const int4 *>(mark + 4 * lane);
            rel[0] = m.x;
            rel[1] = m.y > rel[0] ? m.y : rel[0];
            rel[2] = m.z > rel[1] ? m.z : rel[1];
            rel[3] = m.w > rel[2] ? m.w : rel[2];
            int incl = rel[3];                    // inclusive running maximum over the lanes
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(incl, d);
                if (lane >= d) incl = o > incl ? o : incl;
            }
            int excl = __shfl_up(incl, 1);
            excl = lane == 0 ? 0 : excl;
#pragma unroll
            for (int j = 0; j < 4; ++j) rel[j] = rel[j] > excl ? rel[j] : excl;
            span_rel = __shfl(incl, 63);
            __builtin_amdgcn_wave_barrier();      // (the next span's zeroing comes after every lane's read)
        }

#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long i = i0 + j;
            const int r = static_cast<int16_t>(pts[j] & 0xFFFF), c = static_cast<int16_t>(pts[j] >> 16);
            const bool inside_raster = i >= p0 && i < p1 && r >= 0 && c >= 0 && r < a.rows && c < a.cols;
            const int bin = inside_raster ? (r >> 5) * a.nbc + (c >> 5) : 0;
            // (no global load on this side of the branch: what waits for one would wait for the span in flight too)
            bool occupied = inside_raster;
            if (kMask) occupied = occupied && (s_mask[bin >> 5] >> (bin & 31) & 1u);
            if (__ballot(occupied) == 0) continue;
            int k0 = 0, k1 = 0;
            if (occupied) {
                k0 = a.bin_start[bin];
                k1 = a.bin_start[bin + 1];
            }
            long long z = 0;                      // (kRotor) the point's height above the datum, mm
            if constexpr (kRotor) {
                if (k0 < k1) {
                    const int elev = a.cellinfo[2 * (static_cast<long long>(r) * a.cols + c) + 1];
                    z = static_cast<long long>(elev) + alts[j];
                    if (elev == INT_MIN) k1 = k0;  // nodata under the point: inside no cylinder
                }
            }
            const long long track = t + rel[j];
            bool in_any = false;
            unsigned long long dt_us = 0;         // (kTimed) dt[i], sign-extended, loaded at the point's first hit
            bool have_dt = false;
            while (__ballot(k0 < k1) != 0) {
                bool hit = false;
                int tb = 0;
                if (k0 < k1) {
                    tb = a.bin_items[k0++];
                    if (static_cast<unsigned>(tb) < static_cast<unsigned>(a.nturb)) {
                        const double dx = static_cast<double>(c) - a.turb[2 * tb];
                        const double dy = static_cast<double>(r) - a.turb[2 * tb + 1];
                        const double d2 = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
                        if constexpr (kRotor) {
                            const double reach = a.reach[tb];
                            hit = reach >= 0.0 && d2 <= __dmul_rn(reach, reach);
                            if (hit) {
                                const int2 zb = a.zband[tb];
                                hit = z >= zb.x && z <= zb.y;
                            }
                        } else {
                            hit = d2 <= a.r2;
                        }
                    }
                }
                in_any |= hit;
                if constexpr (kTimed) {
                    // ---- exposure in points and time (a hit lies inside [p0, p1): so does the load)
                    if (hit) {
                        if (!have_dt) {
                            dt_us = static_cast<unsigned long long>(static_cast<long long>(a.dt[i]));
                            have_dt = true;
                        }
                        if (tb != pend_tb && pend_cnt != 0) hand_over();
                        pend_tb = tb;
                        ++pend_cnt;
                        pend_time += dt_us;
                    }
                } else if constexpr (kRotor) {
                    // ---- exposure: one more point inside tb; the block hears of it when the lane moves to another turbine
                    if (hit && s_cnt != nullptr) {
                        if (tb != pend_tb && pend_cnt != 0) {
                            atomicAdd(&s_cnt[pend_tb], pend_cnt);
                            pend_cnt = 0;
                        }
                        pend_tb = tb;
                        ++pend_cnt;
                    }
                }
                // ---- hits: bit tb of the track's row
                const long long word = track * a.words + (tb >> 5);
                const uint32_t bit = 1u << (tb & 31);
                bool news = hit && !(word == known_word && (known_bits & bit));
                if (__ballot(news) == 0) continue;
                if (news) {
                    const uint32_t seen = load_l2(a.hits + word);
                    known_word = word;
                    known_bits = seen;
                    news = !(seen & bit);
                }
                unsigned long long todo;
                while ((todo = __ballot(news)) != 0) {
                    const int leader = __ffsll(static_cast<long long>(todo)) - 1;
                    const bool mine = news && word == __shfl(word, leader);
                    const uint32_t bits = static_cast<uint32_t>(wave_or(mine ? static_cast<int>(bit) : 0));
                    if (lane == leader) atomicOr(a.hits + word, bits);
                    if (mine) {
                        known_bits |= bits;
                        news = false;
                    }
                }
            }
            // ---- first_step: the earliest point of the track inside any disk
            if (a.first_step == nullptr || __ballot(in_any) == 0) continue;
            uint32_t step = 0;
            bool news = false;
            if (in_any) {
                if (track != known_track) {
                    known_track = track;
                    known_start = a.off[track];
                    known_step = 0xFFFFFFFFu;
                }
                step = static_cast<uint32_t>(i - known_start);
                news = step < known_step;
            }
            if (__ballot(news) == 0) continue;
            if (news) {
                const uint32_t seen = load_l2(a.first_step + track);
                known_step = seen;
                news = step < seen;
            }
            unsigned long long todo;
            while ((todo = __ballot(news)) != 0) {
                const int leader = __ffsll(static_cast<long long>(todo)) - 1;
                const bool mine = news && track == __shfl(track, leader);
                const uint32_t first = wave_min(mine ? step : 0xFFFFFFFFu);
                if (lane == leader) atomicMin(a.first_step + track, first);
                if (mine) {
                    known_step = first;
                    news = false;
                }
            }
        }
        t += span_rel;
    };

    // Spans that end at or before p1 stream through 16-byte loads, one span ahead and nothing but straight-line code
    // between a load and its use; off[t + 1] is asked for BEFORE the next span (loads return in order: waiting for it
    // leaves the span in flight).  The last span of the data, and every span of an unaligned buffer, go point by point.
    long long u = u0;
    if (kVec) {
        const long long whole = (p1 - a0) / kTurbSpan;
        const long long u_vec = u1 < whole ? u1 : whole;
        if (u < u_vec) {
            uint4 next = fetch(u);
            int4 next_alt = fetch_alt(u);
            for (; u < u_vec; ++u) {
                const uint4 cur = next;
                const int4 cur_alt = next_alt;
                const long long t_end = a.off[t + 1];
                next = fetch(u + 1 < u_vec ? u + 1 : u);
                next_alt = fetch_alt(u + 1 < u_vec ? u + 1 : u);
                span(u, cur, cur_alt, t_end);
            }
        }
    }
    for (; u < u1; ++u) span(u, fetch_edge(u), fetch_alt_edge(u), a.off[t + 1]);
    if constexpr (kTimed) {
        if (pend_cnt != 0) hand_over();
    } else if constexpr (kRotor) {
        if (pend_cnt != 0) atomicAdd(&s_cnt[pend_tb], pend_cnt);
    }
}

template <bool kVec, bool kMask, bool kRotor, bool kTimed>
__global__ __launch_bounds__(kBlock) void k_turbine_encounters(const TurbArgs a)
{
    static_assert(kRotor || !kTimed, "the timed walk is the rotor walk");
    extern __shared__ uint32_t s_mask[];
    __shared__ alignas(16) int s_mark[kTurbWaves][kTurbSpan];       // (read and zeroed 16 bytes a lane)

    const long long p0 = a.off[0], p1 = a.off[a.ntracks];
    if (p0 < 0 || p1 <= p0) return;
    // spans are cut at multiples of four points of the BUFFER, so that a lane's four points are one aligned load
    const long long a0 = p0 & ~3LL;
    const long long nspans = (p1 - a0 + kTurbSpan - 1) / kTurbSpan;
    const long long nwaves = static_cast<long long>(gridDim.x) * kTurbWaves;
    long long per_wave = (nspans + nwaves - 1) / nwaves;
    per_wave = per_wave < kTurbMinSpans ? kTurbMinSpans : per_wave;
    if (static_cast<long long>(blockIdx.x) * kTurbWaves * per_wave >= nspans) return;      // (the whole block)

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
            s_mask[w] = bits;
        }
    }
    // (kRotor) the block's exposure counters, uint32: a block walks far fewer than 2^32 points
    uint32_t *s_cnt = kRotor && a.points != nullptr ? s_mask + a.cnt_off : nullptr;
    if (s_cnt != nullptr)
        for (int tb = threadIdx.x; tb < a.nturb; tb += kBlock) s_cnt[tb] = 0;
    // (kTimed) the block's time counters, uint64: the same dynamic LDS under an 8-byte aligned name
    unsigned long long *s_time = nullptr;
    if constexpr (kTimed) {
        extern __shared__ unsigned long long s_dyn64[];
        s_time = s_dyn64 + (a.time_off >> 1);
        for (int tb = threadIdx.x; tb < a.time_lds; tb += kBlock) s_time[tb] = 0;
    }
    if (kMask || kRotor) __syncthreads();

    turbine_walk<kVec, kMask, kRotor, kTimed>(a, s_mask, s_cnt, s_time, s_mark, p0, p1, a0, nspans, per_wave);

    if constexpr (kTimed) {
        // every wave of the block arrives here: one 64-bit add per turbine the block met, for the points and for the time
        __syncthreads();
        if (s_cnt != nullptr)
            for (int tb = threadIdx.x; tb < a.nturb; tb += kBlock)
                if (s_cnt[tb] != 0) atomicAdd(a.points + tb, static_cast<unsigned long long>(s_cnt[tb]));
        for (int tb = threadIdx.x; tb < a.time_lds; tb += kBlock)
            if (s_time[tb] != 0) atomicAdd(a.time + tb, s_time[tb]);
    } else if constexpr (kRotor) {
        // every wave of the block arrives here: one 64-bit add per turbine the block met
        if (s_cnt != nullptr) {
            __syncthreads();
            for (int tb = threadIdx.x; tb < a.nturb; tb += kBlock)
                if (s_cnt[tb] != 0) atomicAdd(a.points + tb, static_cast<unsigned long long>(s_cnt[tb]));
        }
    }
}

// turbines_per_track[k] = popcount of row k (bits at and above nturb are not counted)
__global__ __launch_bounds__(kBlock) void k_turbines_per_track(const uint32_t *__restrict__ hits, long long ntracks,
                                                              int nturb, int words, int32_t *__restrict__ out)
{
    const uint32_t tail = nturb & 31 ? (1u << (nturb & 31)) - 1u : 0xFFFFFFFFu;
    for (long long k = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; k < ntracks;
         k += static_cast<long long>(gridDim.x) * kBlock) {
        int n = 0;
        for (int w = 0; w < words; ++w) n += __popc(hits[k * words + w] & (w == words - 1 ? tail : 0xFFFFFFFFu));
        out[k] = n;
    }
}

// tracks_per_turbine[t] += the set bits of column t: counted per block in LDS, then one 64-bit add per turbine
__global__ __launch_bounds__(kBlock) void k_tracks_per_turbine(const uint32_t *__restrict__ hits, long long ntracks,
                                                              int nturb, int words,
                                                              unsigned long long *__restrict__ out)
{
    extern __shared__ uint32_t s_count[];
    for (int t = threadIdx.x; t < words * 32; t += kBlock) s_count[t] = 0;
    __syncthreads();
    const long long n = ntracks * words;
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        uint32_t bits = hits[i];
        const int w = static_cast<int>(i % words);
        while (bits) {
            const int b = __ffs(static_cast<int>(bits)) - 1;
            bits &= bits - 1;
            atomicAdd(&s_count[w * 32 + b], 1u);
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nturb; t += kBlock)
        if (s_count[t]) atomicAdd(&out[t], static_cast<unsigned long long>(s_count[t]));
}

// what both walks take: the trajectories, the turbines, the cull lists and the per-track outputs
static TurbArgs walk_args(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks, const double *turbines,
                          int nturb, const int32_t *bin_start, const int32_t *bin_items, int rows, int cols,
                          uint32_t *hits, int32_t *first_step)
{
    TurbArgs a = {};
    a.traj = reinterpret_cast<const uint32_t *>(traj);
    a.off = reinterpret_cast<const long long *>(traj_offsets);
    a.ntracks = ntracks;
    a.turb = turbines;
    a.nturb = nturb;
    a.bin_start = bin_start;
    a.bin_items = bin_items;
    a.rows = rows;
    a.cols = cols;
    a.nbc = (cols + SSRS_TURBINE_BIN - 1) / SSRS_TURBINE_BIN;
    a.nbins = (rows + SSRS_TURBINE_BIN - 1) / SSRS_TURBINE_BIN * a.nbc;
    a.words = (nturb + 31) / 32;
    a.hits = hits;
    a.first_step = reinterpret_cast<uint32_t *>(first_step);
    return a;
}

template <bool kRotor, bool kTimed = false>
static void launch_encounters(const TurbArgs &a, bool vec, bool mask, size_t lds, hipStream_t st)
{
    const dim3 grid(kTurbBlocks), block(kBlock);
    if (vec && mask) hipLaunchKernelGGL((k_turbine_encounters<true, true, kRotor, kTimed>), grid, block, lds, st, a);
    else if (vec) hipLaunchKernelGGL((k_turbine_encounters<true, false, kRotor, kTimed>), grid, block, lds, st, a);
    else if (mask) hipLaunchKernelGGL((k_turbine_encounters<false, true, kRotor, kTimed>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((k_turbine_encounters<false, false, kRotor, kTimed>), grid, block, lds, st, a);
}

}  // namespace ssrs

using namespace ssrs;

extern "C" int ssrs_turbine_encounters(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks,
                                       const double *turbines, int nturb, double radius_cells,
                                       const int32_t *bin_start, const int32_t *bin_items, int rows, int cols,
                                       uint32_t *hits, int32_t *first_step, void *stream)
{
    SSRS_REQUIRE(traj && traj_offsets && turbines && bin_start && bin_items && hits,
                 "ssrs_turbine_encounters: NULL pointer");
    // (beyond the issue's `ntracks < 0`: the kernel keeps track numbers relative to a wave's cursor as int, in LDS and in
    // registers, and a bitmap of 2^31 rows would be 8 GB a word column)
    SSRS_REQUIRE(ntracks >= 0 && ntracks <= INT32_MAX, "ssrs_turbine_encounters: ntracks = %lld outside [0, 2^31)",
                 static_cast<long long>(ntracks));
    SSRS_REQUIRE(nturb >= 1 && nturb <= SSRS_TURBINE_MAX, "ssrs_turbine_encounters: nturb = %d outside [1, %d]", nturb,
                 SSRS_TURBINE_MAX);
    SSRS_REQUIRE(rows >= 1 && rows <= 32767 && cols >= 1 && cols <= 32767,
                 "ssrs_turbine_encounters: a %d x %d raster (int16 points: 1..32767 either way)", rows, cols);
    SSRS_REQUIRE(radius_cells >= 0.0, "ssrs_turbine_encounters: radius_cells is negative or NaN");
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(traj) & 3u) == 0, "ssrs_turbine_encounters: traj must be 4-byte aligned");
    if (ntracks == 0) return SSRS_OK;
    TurbArgs a = walk_args(traj, traj_offsets, ntracks, turbines, nturb, bin_start, bin_items, rows, cols, hits, first_step);
    a.r2 = radius_cells * radius_cells;
    const bool vec = (reinterpret_cast<uintptr_t>(traj) & 15u) == 0;
    const int mask_words = (a.nbins + 31) / 32;
    const bool mask = mask_words <= kTurbMaskWords;
    launch_encounters<false>(a, vec, mask, mask ? static_cast<size_t>(mask_words) * 4 : 0, as_stream(stream));
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

// ssrs_rotor_encounters and its timed form (`timed`: dt and time_per_turbine are required): one set of checks, one launch
static int rotor_call(const char *who, bool timed, const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks,
                      const int32_t *alt, const int32_t *dt, const int32_t *cellinfo, int rows, int cols,
                      const double *turbines, const double *reach, const int32_t *zband, int nturb, const int32_t *bin_start,
                      const int32_t *bin_items, uint32_t *hits, int32_t *first_step, uint64_t *points_per_turbine,
                      uint64_t *time_per_turbine, void *stream)
{
    SSRS_REQUIRE(traj && traj_offsets && alt && cellinfo && turbines && reach && zband && bin_start && bin_items && hits,
                 "%s: NULL pointer", who);
    SSRS_REQUIRE(!timed || (dt && time_per_turbine), "%s: NULL pointer (dt and time_per_turbine are required)", who);
    SSRS_REQUIRE(ntracks >= 0 && ntracks <= INT32_MAX, "%s: ntracks = %lld outside [0, 2^31)", who,
                 static_cast<long long>(ntracks));
    SSRS_REQUIRE(nturb >= 1 && nturb <= SSRS_TURBINE_MAX, "%s: nturb = %d outside [1, %d]", who, nturb, SSRS_TURBINE_MAX);
    SSRS_REQUIRE(rows >= 1 && rows <= 32767 && cols >= 1 && cols <= 32767,
                 "%s: a %d x %d raster (int16 points: 1..32767 either way)", who, rows, cols);
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(traj) & 3u) == 0 && (reinterpret_cast<uintptr_t>(alt) & 3u) == 0,
                 "%s: traj and alt must be 4-byte aligned", who);
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(cellinfo) & 7u) == 0 && (reinterpret_cast<uintptr_t>(zband) & 7u) == 0 &&
                     (reinterpret_cast<uintptr_t>(points_per_turbine) & 7u) == 0,
                 "%s: cellinfo, zband and points_per_turbine must be 8-byte aligned", who);
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(dt) & 3u) == 0, "%s: dt must be 4-byte aligned", who);
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(time_per_turbine) & 7u) == 0, "%s: time_per_turbine must be 8-byte aligned", who);
    if (ntracks == 0) return SSRS_OK;
    TurbArgs a = walk_args(traj, traj_offsets, ntracks, turbines, nturb, bin_start, bin_items, rows, cols, hits, first_step);
    a.alt = alt;
    a.cellinfo = cellinfo;
    a.reach = reach;
    a.zband = reinterpret_cast<const int2 *>(zband);
    a.points = reinterpret_cast<unsigned long long *>(points_per_turbine);
    const bool vec = ((reinterpret_cast<uintptr_t>(traj) | reinterpret_cast<uintptr_t>(alt)) & 15u) == 0;
    // mask and counters share the dynamic LDS; together with the 4 KB of marks a block stays within 64 KB
    const int mask_words = (a.nbins + 31) / 32;
    const int cnt_words = a.points ? nturb : 0;
    if (!timed) {
        const bool mask = mask_words <= kTurbMaskWords && mask_words + cnt_words <= kRotorLdsWords;
        a.cnt_off = mask ? mask_words : 0;
        launch_encounters<true>(a, vec, mask, static_cast<size_t>(a.cnt_off + cnt_words) * 4, as_stream(stream));
    } else {
        // the header's LDS rule: the mask stays only while the time counters of every turbine fit behind it and the point
        // counters (at an even word: they are 8 bytes each); without it the time counters take what the point counters leave
        a.dt = dt;
        a.time = reinterpret_cast<unsigned long long *>(time_per_turbine);
        const bool mask = mask_words <= kTurbMaskWords && ((mask_words + cnt_words + 1) & ~1) + 2 * nturb <= kRotorLdsWords;
        a.cnt_off = mask ? mask_words : 0;
        a.time_off = (a.cnt_off + cnt_words + 1) & ~1;
        const int room = (kRotorLdsWords - a.time_off) / 2;
        a.time_lds = nturb < room ? nturb : room;
        launch_encounters<true, true>(a, vec, mask, static_cast<size_t>(a.time_off + 2 * a.time_lds) * 4, as_stream(stream));
    }
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

extern "C" int ssrs_rotor_encounters(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks, const int32_t *alt,
                                     const int32_t *cellinfo, int rows, int cols, const double *turbines,
                                     const double *reach, const int32_t *zband, int nturb, const int32_t *bin_start,
                                     const int32_t *bin_items, uint32_t *hits, int32_t *first_step,
                                     uint64_t *points_per_turbine, void *stream)
{
    return rotor_call("ssrs_rotor_encounters", false, traj, traj_offsets, ntracks, alt, nullptr, cellinfo, rows, cols, turbines,
                      reach, zband, nturb, bin_start, bin_items, hits, first_step, points_per_turbine, nullptr, stream);
}

extern "C" int ssrs_rotor_encounters_timed(const int16_t *traj, const int64_t *traj_offsets, int64_t ntracks,
                                           const int32_t *alt, const int32_t *dt, const int32_t *cellinfo, int rows, int cols,
                                           const double *turbines, const double *reach, const int32_t *zband, int nturb,
                                           const int32_t *bin_start, const int32_t *bin_items, uint32_t *hits,
                                           int32_t *first_step, uint64_t *points_per_turbine, uint64_t *time_per_turbine,
                                           void *stream)
{
    return rotor_call("ssrs_rotor_encounters_timed", true, traj, traj_offsets, ntracks, alt, dt, cellinfo, rows, cols, turbines,
                      reach, zband, nturb, bin_start, bin_items, hits, first_step, points_per_turbine, time_per_turbine, stream);
}

extern "C" int ssrs_turbine_encounter_counts(const uint32_t *hits, int64_t ntracks, int nturb,
                                             int64_t *tracks_per_turbine, int32_t *turbines_per_track, void *stream)
{
    SSRS_REQUIRE(hits && tracks_per_turbine, "ssrs_turbine_encounter_counts: NULL pointer");
    // (the same limit as ssrs_turbine_encounters, whose bitmap this is)
    SSRS_REQUIRE(ntracks >= 0 && ntracks <= INT32_MAX, "ssrs_turbine_encounter_counts: ntracks = %lld outside [0, 2^31)",
                 static_cast<long long>(ntracks));
    SSRS_REQUIRE(nturb >= 1 && nturb <= SSRS_TURBINE_MAX, "ssrs_turbine_encounter_counts: nturb = %d outside [1, %d]",
                 nturb, SSRS_TURBINE_MAX);
    hipStream_t st = as_stream(stream);
    const int words = (nturb + 31) / 32;
    SSRS_HIP_CHECK(hipMemsetAsync(tracks_per_turbine, 0, static_cast<size_t>(nturb) * 8, st));
    if (ntracks == 0) return SSRS_OK;
    size_t blocks = (static_cast<size_t>(ntracks) * words + kBlock - 1) / kBlock;
    blocks = blocks > 1024 ? 1024 : blocks;
    hipLaunchKernelGGL(k_tracks_per_turbine, dim3(static_cast<unsigned>(blocks)), dim3(kBlock),
                       static_cast<size_t>(words) * 32 * 4, st, hits, static_cast<long long>(ntracks), nturb, words,
                       reinterpret_cast<unsigned long long *>(tracks_per_turbine));
    if (turbines_per_track) {
        size_t b2 = (static_cast<size_t>(ntracks) + kBlock - 1) / kBlock;
        b2 = b2 > static_cast<size_t>(kMaxStreamBlocks) ? kMaxStreamBlocks : b2;
        hipLaunchKernelGGL(k_turbines_per_track, dim3(static_cast<unsigned>(b2)), dim3(kBlock), 0, st, hits,
                           static_cast<long long>(ntracks), nturb, words, turbines_per_track);
    }
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}
