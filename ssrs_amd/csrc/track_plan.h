// The list arithmetic of the stepper that the host and the device must agree on: the slots per XCD list
// (workspace_layout), the deal of a wander sort (k_deal_sorted) and the host's bound on the longest list
// after it.  No HIP runtime here: tests/track_plan_driver.cpp checks the three against each other on a CPU.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define SSRS_HD __host__ __device__
#else
#define SSRS_HD
#endif

namespace ssrs {

// Live tracks are kept in kXcd separate lists, one per XCD: blocks are dealt to
// the XCDs round-robin (block b runs on XCD b % 8), so block b serves list b % 8
// and a track stays on the XCD it was dealt to.  With the coherent schedule the
// lists are contiguous bands of the across-track coordinate: the table rows a
// band walks over are fetched into ONE XCD's L2 instead of all eight.
constexpr int kXcd = 8;
constexpr uint32_t kPlanBlock = 256;         // lanes of a narrow stepper block (kBlock, common.h)

// block histogram windows of wandering batches (k_step_thr<6>, k_wander_windows)
// 144 rows: 144 KB of LDS, one block per CU (rounds 2-3); 72 rows: 72 KB, two blocks per CU (-DSSRS_WIN_ROWS=72, A/B)
#ifndef SSRS_WIN_ROWS
#define SSRS_WIN_ROWS 144
#endif
constexpr int kWinRows = SSRS_WIN_ROWS, kWinCols = 256;
static_assert(kWinRows == 144 || kWinRows == 72, "a window is 4 or 2 rows of coarse bins");
constexpr int kWanderWindows = 16;
constexpr uint32_t kDealBlocks = kWinRows == 144 ? 232 : 464;   // blocks the contiguous deal spreads the live tracks over (+ one per
                                                   // window in use and the padding: under the 256 CUs x blocks per CU)
constexpr int64_t kWanderMinTracks = 8192;   // smaller batches are never sorted into windows

// Slots per XCD list for n tracks.  cap is a whole number of the widest blocks (k_step_roam<REV, 1024>: the wide
// deal rounds every list up to whole groups of blocks, and its dense fall-back must still fit)
inline size_t list_cap(int64_t n)
{
    const size_t unit = 4 * kPlanBlock;
    return ((static_cast<size_t>(n) + kXcd - 1) / kXcd + unit - 1) / unit * unit;
}

// The deal of a wander sort.  lo[k] (k = 0 .. kWanderWindows + 2) is the first position of key k in the sorted
// order of the cap * kXcd slots (key kWanderWindows: outside every window, kWanderWindows + 1: dead, not dealt),
// so lo[kWanderWindows + 1] is the live count.  Fills off[0 .. kWanderWindows + 2]: key k's run starts at position
// off[k] of the dealt order, off[kWanderWindows + 1] is the total dealt (a multiple of kXcd blocks of `width`), and
// off[kWanderWindows + 2] != 0 marks the dense fall-back (blocks may mix windows).  Returns the tracks a block of
// kPlanBlock slots keeps (`fill`, the rest are tombstones).
// width 2 / 4 (k_step_roam<REV, 512 / 1024>): a window's run is whole groups of `width` blocks and every list holds whole groups
SSRS_HD inline uint32_t deal_plan(const uint32_t *lo, uint32_t cap, bool contiguous, uint32_t width, uint32_t *off)
{
    const uint32_t slots = cap * kXcd;
    const uint32_t uw = width;
    const uint32_t kRun = kXcd * kPlanBlock * uw;
    // contiguous deal: a block keeps `fill` of its kBlock slots (the rest are tombstones), chosen so that the
    // live tracks make about one block per CU.  A block-window kernel holds 144 KB of LDS, one block per
    // CU, and a divergent gather costs its CU ~4 clocks per lane: 44k survivors in 180 full blocks leave 76
    // CUs idle while the others take 1030 clocks per step.
    const uint32_t live = lo[kWanderWindows + 1];
    uint32_t fill = kPlanBlock;
    if (contiguous) {
        // the blocks must stay under the 256 CUs x blocks per CU (a block beyond the first round of a launch finds the
        // stop flag up and waits for the others to finish the pass): kDealBlocks + one partial block per window IN USE
        // (round 4: the allowance of the unused ones goes to the deal, 246 instead of 232 blocks with two basins =
        // 63 000 instead of 59 392 live tracks in one round) + the padding to whole blocks of every list.
        // Wide: 216 groups + one per window + the padding
        uint32_t in_use = 0;
        for (int k = 0; k <= kWanderWindows; ++k) in_use += lo[k + 1] > lo[k] ? 1u : 0u;
        const uint32_t deal_blocks = uw > 1u ? uw * 216u : kDealBlocks + (kWanderWindows + 1u - in_use);
        fill = (live + deal_blocks - 1) / deal_blocks;
        fill = fill < 64u ? 64u : (fill > kPlanBlock ? kPlanBlock : fill);
    }
    uint32_t run = 0;
    for (int pass = 0; pass < 2; ++pass) {
        run = 0;
        for (int k = 0; k <= kWanderWindows; ++k) {              // (key kWanderWindows + 1 = dead: not dealt)
            off[k] = run;
            uint32_t blocks = (lo[k + 1] - lo[k] + fill - 1) / fill;
            blocks = (blocks + uw - 1u) / uw * uw;
            // round-robin deal: a window's run is whole blocks of EVERY list
            run += contiguous ? blocks * kPlanBlock : (blocks * kPlanBlock + kRun - 1) / kRun * kRun;
        }
        run = (run + kRun - 1) / kRun * kRun;
        if (run <= slots || fill == kPlanBlock) break;
        fill = kPlanBlock;                                       // no room for the thinned blocks
    }
    off[kWanderWindows + 1] = run;
    if (run > slots) {
        // no room for the padding (nearly every slot is live): dense deal, blocks may mix windows
        run = 0;
        for (int k = 0; k <= kWanderWindows + 1; ++k) { off[k] = run; if (k <= kWanderWindows) run += lo[k + 1] - lo[k]; }
        off[kWanderWindows + 1] = (run + kRun - 1) / kRun * kRun;   // (<= slots: cap is a multiple of 4 blocks, list_cap)
        off[kWanderWindows + 2] = 1;                             // dense
    } else {
        off[kWanderWindows + 2] = 0;
    }
    return fill;
}

// The host's bound on the longest XCD list after a deal of `width`, from its bound `upper` before it.  The padded
// deal makes the lists LONGER (each window's run is rounded up to whole blocks of every list).
// (thinned blocks: at most kDealBlocks + one per window + the padding, 264 blocks = 33 per list)
inline uint32_t deal_upper(uint32_t upper, uint32_t cap, bool contiguous, uint32_t width)
{
    const unsigned long long wf = width;                         // (wide: runs are whole groups of blocks)
    unsigned long long padded = static_cast<unsigned long long>(upper) + (kWanderWindows + 1ull) * kPlanBlock * wf;
    const unsigned long long kDealPerList = (wf * kDealBlocks + wf * (kWanderWindows + 1)) / kXcd + 3;      // 34 blocks per list (144 rows)
    if (contiguous && padded < kDealPerList * kPlanBlock) padded = kDealPerList * kPlanBlock;
    return padded > cap ? cap : static_cast<uint32_t>(padded);
}

}  // namespace ssrs
