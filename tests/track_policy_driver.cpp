// Host-only check of the stepper's per-batch policy (ssrs_amd/csrc/track_policy.h) on a settled roaming batch: read-back
// slots go to TrackPolicy::examine in order, as tracks_simulate_impl feeds them, and the sorts it asks for are "dealt" the
// way TrackRun::wander_sort does.  Checked: a periodic shuffle asks for no window scan (unless its batch strayed, the last
// deal was wide and the width hangs on the live count, or the reuse is switched off), real sorts always scan, stable_roam
// and since_shuffle keep the launches long and the shuffles evenly spaced, and the bound on the longest list holds across
// every deal.  tests/test_track_policy.py builds and runs this; it prints one line per failure (the first 20) and a
// summary, and exits 1 on any failure.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../ssrs_amd/csrc/track_policy.h"

using namespace ssrs;

namespace {

long long checks = 0, failures = 0;

void check(bool ok, const char *what, int scenario, int batch)
{
    ++checks;
    if (ok) return;
    if (failures++ < 20) std::printf("FAIL %s: scenario %d, batch %d\n", what, scenario, batch);
}

// The host loop around the policy: one read-back slot per batch; a batch is examined when the one behind it is queued
struct Loop {
    TrackPolicy pol;
    int scenario = 0;
    uint32_t cap = 0, live = 0;
    uint32_t lists = 0;                       // length of every list (the contiguous deal makes them equal)
    uint32_t first_bound = 0;                 // the policy's bound before the first deal
    int batches = 0, width = 1;
    bool roam_ready = true, width_by_live = false;
    unsigned long long steps = 0, strays = 0;
    std::vector<uint32_t> slots;              // the slots of the batches queued so far
    // what the sorts did
    int sorts = 0, scans = 0, periodic = 0, periodic_scans = 0;
    std::vector<int> shuffle_at;              // batches queued when a periodic shuffle was dealt

    Loop(int scenario_, long long ntracks, int roam_shuffle, bool reuse) : scenario(scenario_)
    {
        cap = static_cast<uint32_t>(list_cap(ntracks));
        live = static_cast<uint32_t>(ntracks);
        lists = (live + kXcd - 1) / kXcd;
        pol.thr = true; pol.cache_ok = true; pol.cached = true; pol.scattered = true;
        pol.roam_shuffle = roam_shuffle;
        pol.reuse_windows = reuse;
        pol.ntracks = ntracks; pol.crossing = 11000;
        pol.want_wander_sort = true;
        pol.upper = lists < cap ? lists : cap;
        first_bound = pol.upper;
    }

    // as TrackRun::wander_sort: scan or not, the deal (two basins and a few tracks outside them), the policy's bound
    void sort()
    {
        const bool was_periodic = pol.sort_is_periodic;
        const bool scan = pol.scan_windows(width_by_live);
        ++sorts;
        scans += scan ? 1 : 0;
        if (was_periodic) { ++periodic; periodic_scans += scan ? 1 : 0; shuffle_at.push_back(batches); }
        check(was_periodic || scan, "a real sort without a window scan", scenario, batches);
        check(scan || pol.window_scans > 0, "windows reused before any scan", scenario, batches);
        check(scan || width == 1 || !width_by_live, "a wide deal whose width hangs on the live count was not counted", scenario, batches);
        uint32_t lo[kWanderWindows + 3], off[kWanderWindows + 3];
        const uint32_t outside = live / 400, first = (live - outside) * 2 / 3;
        lo[0] = 0; lo[1] = first; lo[2] = live - outside;
        for (int k = 3; k <= kWanderWindows; ++k) lo[k] = lo[2];
        lo[kWanderWindows + 1] = live;
        lo[kWanderWindows + 2] = cap * kXcd;
        (void)deal_plan(lo, cap, true, static_cast<uint32_t>(width), off);
        lists = off[kWanderWindows + 1] / kXcd;
        const int before_scans = pol.window_scans, before_shuffles = pol.roam_shuffles;
        pol.dealt(batches, cap, true, width, scan);
        check(pol.window_scans == before_scans + (scan ? 1 : 0), "window_scans", scenario, batches);
        check(pol.roam_shuffles == before_shuffles + (was_periodic ? 1 : 0), "roam_shuffles", scenario, batches);
        check(pol.stable_roam == (was_periodic ? 2 : 0), "stable_roam after a deal (a shuffle keeps the launches long)", scenario, batches);
        // (a shuffle without a scan: the next may follow at once; behind every other sort three batches are looked past)
        check(!pol.want_wander_sort && !pol.sort_is_periodic && pol.wander_cooldown == (was_periodic && !scan ? 0 : 3),
              "state after a deal", scenario, batches);
        check(lists <= pol.upper && pol.upper <= cap, "deal_upper does not bound the dealt lists", scenario, batches);
        // (deals that follow each other faster than their batches are read back do not pad each other's padding)
        check(pol.upper <= deal_upper(first_bound, cap, true, static_cast<uint32_t>(width)), "the bound creeps from deal to deal", scenario, batches);
    }

    // one batch: `stray_share` of its steps fall outside the block windows, `dying` of 1024 live tracks end
    void batch(double stray_share, uint32_t dying)
    {
        if (pol.want_wander_sort) sort();
        check(lists <= pol.upper, "a list longer than the policy's bound at a launch", scenario, batches);
        live -= static_cast<uint32_t>(static_cast<unsigned long long>(live) * dying / 1024);
        const unsigned long long dsteps = 2ull * 65536ull * live;
        steps += dsteps;
        strays += static_cast<unsigned long long>(static_cast<double>(dsteps) * stray_share);
        std::vector<uint32_t> slot(kSlotWords, 0u);
        for (int x = 0; x < kXcd; ++x) slot[kXcd * (batches & 3) + x] = lists;     // (blocks keep their slots: the lists keep their length)
        const unsigned long long tot[2] = {steps, strays};
        memcpy(&slot[kSlotSteps], tot, sizeof(tot));
        slots.insert(slots.end(), slot.begin(), slot.end());
        ++batches;
        while (pol.checked < batches - 1 && !pol.finished) {
            const int b = pol.checked;
            pol.examine(&slots[static_cast<size_t>(kSlotWords) * b], b & 3, true, batches, 0, 0, roam_ready);
        }
    }
};

// a settled batch: shuffles every cooldown + roam_shuffle batches, none of them scans, the first sort does
void settled(int scenario, int roam_shuffle, bool reuse)
{
    Loop l(scenario, 100000, roam_shuffle, reuse);
    for (int b = 0; b < 90; ++b) l.batch(0.001, 2);
    check(l.sorts == l.periodic + 1 && l.pol.wander_sorts == l.sorts, "one real sort, then shuffles", scenario, -1);
    check(l.pol.window_scans == l.scans, "window_scans against the scans made", scenario, -1);
    if (roam_shuffle == 0) {
        check(l.periodic == 0, "shuffles with the interval 0", scenario, -1);
        return;
    }
    check(l.periodic >= 3, "a settled batch is shuffled", scenario, -1);
    check(l.periodic_scans == (reuse ? 0 : l.periodic), "window scans of periodic shuffles", scenario, -1);
    check(reuse ? l.scans < l.sorts : l.scans == l.sorts, "fewer scans than sorts", scenario, -1);
    // evenly spaced: every roam_shuffle batches -- and the three batches that are looked past behind a deal that scanned.
    // The first one waits for stable_roam to reach 2 as well
    for (size_t i = 1; i < l.shuffle_at.size(); ++i)
        check(l.shuffle_at[i] - l.shuffle_at[i - 1] == (reuse ? 0 : 3) + roam_shuffle, "interval of the shuffles", scenario, l.shuffle_at[i]);
    check(l.shuffle_at[0] >= 1 + 3 + (roam_shuffle > 2 ? roam_shuffle : 2), "first shuffle before the batch had settled", scenario, l.shuffle_at[0]);
}

// not ready to roam (no pair table yet): no shuffle at all
void not_ready(int scenario)
{
    Loop l(scenario, 100000, 4, true);
    l.roam_ready = false;
    for (int b = 0; b < 40; ++b) l.batch(0.001, 2);
    check(l.periodic == 0 && l.sorts == 1, "a shuffle before the batch roams", scenario, -1);
    check(l.pol.stable_roam >= 2, "stable_roam grows while the batch waits", scenario, -1);
}

// a batch that strays asks for REAL sorts (they scan), at most 12 sorts in all; a shuffle of a straying batch then scans too
void straying(int scenario)
{
    Loop l(scenario, 100000, 4, true);
    for (int b = 0; b < 20; ++b) l.batch(0.001, 2);
    for (int b = 0; b < 2; ++b) l.batch(0.05, 8);                   // (a batch is examined when the one behind it is queued)
    const int shuffles = l.periodic;
    check(shuffles > 0 && l.periodic_scans == 0, "settled start", scenario, -1);
    for (int b = 0; b < 16; ++b) l.batch(0.05, 8);                  // 1 / 20 > 1 / 64
    check(l.periodic == shuffles && l.sorts > shuffles + 1, "straying batches get real sorts", scenario, -1);
    check(l.pol.stable_roam < 2 + 4, "stable_roam starts again behind a real sort", scenario, -1);
    const int real = l.sorts - l.periodic;
    check(l.scans == real, "every real sort scans", scenario, -1);
    for (int b = 0; b < 120; ++b) l.batch(0.05, 8);
    check(l.sorts - l.periodic <= 12, "more than 12 real sorts", scenario, -1);
    check(l.periodic > shuffles, "shuffles go on when the real sorts have run out", scenario, -1);
    check(l.periodic_scans == l.periodic - shuffles, "a shuffle of a straying batch looks for the windows anew", scenario, -1);
    const int scans = l.scans, sorts = l.sorts;
    for (int b = 0; b < 40; ++b) l.batch(0.0005, 1);                // settled again: no scans any more
    check(l.sorts > sorts && l.scans <= scans + 1, "settled again, still scanning", scenario, -1);
}

// a wide deal whose width hangs on the live count keeps its scan (the scan takes the count); a narrow one does not
void wide(int scenario, int width, bool by_live)
{
    Loop l(scenario, 250000, 16, true);
    l.width = width;
    l.width_by_live = by_live;
    for (int b = 0; b < 70; ++b) l.batch(0.001, 1);
    check(l.periodic >= 2, "a settled wide batch is shuffled", scenario, -1);
    check(l.periodic_scans == (width > 1 && by_live ? l.periodic : 0), "scans of a wide batch's shuffles", scenario, -1);
}

// the batch dies out: the policy finishes, the bound never fell under a list
void to_the_end(int scenario)
{
    Loop l(scenario, 20000, 1, true);
    int b = 0;
    for (; b < 400 && !l.pol.finished; ++b) {
        l.batch(0.002, 200);
        if (l.live < 16) { l.live = 0; l.lists = 0; }
    }
    check(l.pol.finished, "the policy never saw the batch end", scenario, b);
}

}  // namespace

int main()
{
    int scenario = 0;
    for (int interval : {0, 1, 2, 4, 16})
        for (bool reuse : {true, false}) settled(scenario++, interval, reuse);
    not_ready(scenario++);
    straying(scenario++);
    for (int width : {1, 2, 4})
        for (bool by_live : {false, true}) wide(scenario++, width, by_live);
    to_the_end(scenario++);
    std::printf("%d scenarios, %lld checks, %lld failures\n", scenario, checks, failures);
    return failures == 0 ? 0 : 1;
}
