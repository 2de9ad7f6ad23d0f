// The per-batch policy of the track stepper (tracks.hip: tracks_simulate_impl).  No HIP runtime here: the policy
// sees nothing of the device but the read-back slots of the batches.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "track_plan.h"

namespace ssrs {

// Launches are queued kBatch deep; a batch's read-back goes to one of kRing slots of kSlotWords pinned words: the head
// of the control block (TrackCtl) in one copy, [4][kXcd] list counts, error, par_min, steps (2 words at kSlotSteps),
// strays (2 words)
constexpr int kBatch = 2, kRing = 8;
constexpr int kSlotWords = 40;           // 160 bytes of TrackCtl: counts .. strays
constexpr int kSlotSteps = 4 * kXcd + 2;
static_assert(kSlotSteps + 4 <= kSlotWords, "read-back slot");

// The per-batch policy.  It owns the path of the launches to come (row window, tile buckets, block windows,
// per-step atomics), the wish for a wander sort or a re-deal of the lists and the bound on the longest list, and
// changes them from nothing but the read-back slots of the batches, in order.
struct TrackPolicy {
    // fixed for the call
    bool thr = false, tiles_ok = false, cache_ok = false, never_scattered = false;
    bool front = false;                      // a north / south front (prefetch wave)
    bool may_rebalance = true, debug = false;
    int roam_shuffle = 16;
    bool reuse_windows = true;               // a periodic shuffle deals into the windows of the last scan
    long long ntracks = 0, crossing = 0;     // crossing: rows + cols
    // the path
    bool binning_on = false, tiles_on = false, cached = false, scattered = false;
    bool want_wander_sort = false, want_rebalance = false, sort_is_periodic = false;
    bool shuffle_rescans = false;            // ... a periodic one whose batch strayed like one that asks for a real sort
    int wander_cooldown = 0;
    int rebalance_cooldown = 0;              // batches to look past after a re-deal (their counts are older than it)
    int stable_batches = 0, stable_roam = 0, since_shuffle = 0;
    int judge_from = 0;
    uint32_t upper = 0;                      // bound on the longest XCD list
    int upper_from = 0;
    uint32_t undealt = 0;                    // the last bound that was seen on lists, not derived from a deal's padding
    bool upper_is_padded = false;
    uint32_t prev_total = 0;
    unsigned long long seen_steps = 0, seen_strays = 0;
    // the batches examined so far
    int checked = 0;
    bool finished = false;
    int wander_sorts = 0, roam_shuffles = 0;
    int window_scans = 0;                    // sorts that looked for the windows anew (k_wander_windows)
    int dealt_width = 0;                     // block width of the last deal (0: none yet)
    long long block_window_steps = 0;

    // Does the sort that is wanted now look for the windows anew?  A periodic shuffle of a settled batch does not: the
    // basins stay where they are, and the windows of the last scan are still on the device.  It does when its batch
    // strayed like one that asks for a real sort (those are capped), and when the deal's width hangs on the live count
    // that the scan takes (`width_by_live`: the lists are long enough for wide blocks) and the last deal was wide -- a
    // narrow deal stays narrow, the live count only shrinks.
    bool scan_windows(bool width_by_live) const
    {
        if (!sort_is_periodic || !reuse_windows || window_scans == 0 || shuffle_rescans) return true;
        return width_by_live && dealt_width > 1;
    }

    // a wander sort's deal of `width` was queued as batch `batches` was being filled; `scanned`: it looked for its windows
    void dealt(int batches, uint32_t cap, bool contiguous, int width, bool scanned = true)
    {
        ++wander_sorts;
        if (scanned) ++window_scans;
        dealt_width = width;
        shuffle_rescans = false;
        want_wander_sort = false;
        want_rebalance = false;
        // (the batches queued before a real sort report the strays of the old windows: they are looked past.  A shuffle
        // into the same windows changes nothing about the strays, and with no scan to pay for the next may follow at once)
        wander_cooldown = (sort_is_periodic && !scanned) ? 0 : 3;
        stable_roam = sort_is_periodic ? 2 : 0;      // (a shuffle of a settled batch: the launches stay long)
        if (sort_is_periodic) ++roam_shuffles;
        sort_is_periodic = false;
        // the padded deal makes the lists LONGER: raise the bound now, and let no batch queued before this point lower it.
        // A deal places the live tracks afresh, whatever the lists' lengths: deal_upper of ANY bound on an eighth of the
        // live tracks holds behind it, and the live count only shrinks.  So when deals follow each other faster than their
        // batches are read back, each pads the last bound that was seen on lists (`undealt`), not the padded bound of
        // the deal before it -- that would grow to the lists' capacity, and every launch would start that many blocks
        if (!upper_is_padded) undealt = upper;
        upper = deal_upper(undealt, cap, contiguous, static_cast<uint32_t>(width));
        upper_is_padded = true;
        upper_from = batches;
    }

    void rebalanced()
    {
        want_rebalance = false;
        rebalance_cooldown = 3;
    }

    // The read-back slot of the next batch in order: its survivors went to row `row` of the counts; the batch ran in
    // block windows (`block_window`); `batches` have been queued, the threshold stepper is `it_done` iterations in,
    // the other steppers `steps_done` steps
    void examine(const uint32_t *slot, int row, bool block_window, int batches, long long it_done, long long steps_done,
                 bool roam_ready)
    {
        uint32_t c = 0;                         // longest list
        const uint32_t *cnt = slot + kXcd * row;
        for (int x = 0; x < kXcd; ++x) c = cnt[x] > c ? cnt[x] : c;
        unsigned long long tot[2];                 // steps, strays
        memcpy(tot, slot + kSlotSteps, sizeof(tot));
        ++checked;
        if (block_window) block_window_steps += static_cast<long long>(tot[0] - seen_steps);
        if (c == 0) { finished = true; return; }
        // the live count only shrinks, a stale bound is safe -- except across a wander sort
        if (checked - 1 >= upper_from) { upper = c; upper_is_padded = false; }      // (lists as the last deal left them, or shorter)
        else if (c > upper) upper = c;
        uint32_t total = 0;
        for (int x = 0; x < kXcd; ++x) total += cnt[x];
        if (tiles_on && cache_ok && front) {
            // a front that outgrew the row window goes through tile buckets while part of the batch
            // still travels; once nobody finishes any more (the survivors roam their basins until
            // max_moves) the block windows take over
            // (nobody finishing YET is not stable: some must have finished, or the batch is older
            // than two raster crossings)
            const bool started = static_cast<long long>(total) * 50 < ntracks * 49 || it_done > 2ll * crossing;
            if (started && prev_total != 0 && total >= prev_total - prev_total / 32 && ++stable_batches >= 2) {
                tiles_on = false;
                cached = true;
                want_wander_sort = true;
            }
            if (prev_total == 0 || total < prev_total - prev_total / 32) stable_batches = 0;
        }
        prev_total = total;
        if (thr && may_rebalance) {
            if (rebalance_cooldown > 0) --rebalance_cooldown;
            else if (c >= 1024 && 5ull * c >= static_cast<unsigned long long>(total) + 64ull) want_rebalance = true;   // longest list >= 1.6 x the mean
        }
        // binning pays only while the batch moves as a front: once more than a
        // quarter of a batch's visits miss the LDS window, later launches go back
        // to in-stepper atomics
        if (binning_on || tiles_on) {
            // row window: strays = visits outside it (stop above a quarter); tiles:
            // strays = cells flushed (stop below two visits per cell)
            // (batches queued before a switch still report the old path's strays)
            const unsigned long long dsteps = tot[0] - seen_steps, dstray = tot[1] - seen_strays;
            if (checked - 1 >= judge_from && dsteps > 0 && dstray * (tiles_on ? 2 : 4) > dsteps) {
                judge_from = batches;
                if (binning_on && cache_ok && !tiles_ok) {
                    // the front has outgrown the row window and there are no tile buckets
                    binning_on = false;
                    cached = true;
                    want_wander_sort = true;
                } else if (binning_on && tiles_ok) {
                    // the front has outgrown the row window; its visits may still cluster
                    binning_on = false;
                    tiles_on = true;
                } else {
                    binning_on = tiles_on = false;
                    scattered = !never_scattered;      // no front any more: zero-mask variant
                    cached = cache_ok && scattered;
                    want_wander_sort = cached;
                }
            }
        }
        if (cached && !(binning_on || tiles_on)) {
            // block windows: strays = visits outside them.  Tracks still on their way into a basin
            // (or out of their block's box) show up here: sort again, a few times at most
            const unsigned long long dsteps = tot[0] - seen_steps, dstray = tot[1] - seen_strays;
            if (debug && checked < 60)
                fprintf(stderr, "[tracks] batch %d block windows: %llu steps, %llu strays (%.3f), live %u\n", checked, dsteps, dstray,
                        dsteps ? static_cast<double>(dstray) / static_cast<double>(dsteps) : 0.0, total);
            if (wander_cooldown > 0) --wander_cooldown;
            else if (dsteps > 0 && dstray * 64 > dsteps && wander_sorts < 12) want_wander_sort = true;
            else if (roam_shuffle > 0 && ++since_shuffle >= roam_shuffle && stable_roam >= 2 && roam_ready) {
                want_wander_sort = true;            // settled: every roam_shuffle batches the windows' tracks are dealt afresh
                sort_is_periodic = true;
                shuffle_rescans = dsteps > 0 && dstray * 64 > dsteps;      // (the real sorts have run out)
                since_shuffle = 0;
            } else ++stable_roam;                   // settled in its windows: the launches may grow
        }
        // batches that never binned (small, unsorted, very wide rasters) give no stray
        // signal: tracks still alive after four raster crossings are wandering
        if (!binning_on && !tiles_on && !scattered && !never_scattered && (thr ? it_done : steps_done) > 4ll * crossing) {
            scattered = true;
            if (cache_ok && !cached) { cached = true; want_wander_sort = true; }
        }
        seen_steps = tot[0];
        seen_strays = tot[1];
    }
};

}  // namespace ssrs
