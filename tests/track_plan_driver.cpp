// Host-only check of the deal plan (ssrs_amd/csrc/track_plan.h): the slots per list, the deal of a wander sort and
// the host's bound on the longest list after it must agree.  tests/test_track_plan.py builds and runs this;
// it prints one line per failure (the first 20) and a summary, and exits 1 on any failure.
#include <cstdio>
#include <vector>

#include "../ssrs_amd/csrc/track_plan.h"

using namespace ssrs;

namespace {

long long cases = 0, failures = 0;

struct Case {
    long long ntracks;
    int windows, shape, width;
    bool contiguous;
};

void check(bool ok, const char *what, const Case &c)
{
    if (ok) return;
    if (failures++ < 20)
        std::printf("FAIL %s: ntracks %lld, windows %d, shape %d, width %d, %s deal\n", what, c.ntracks, c.windows, c.shape,
                    c.width, c.contiguous ? "contiguous" : "round-robin");
}

// count[k]: the live tracks of key k (k < kWanderWindows: a window, kWanderWindows: outside every window)
void one(const Case &c, const std::vector<uint32_t> &count)
{
    ++cases;
    const uint32_t cap = static_cast<uint32_t>(list_cap(c.ntracks));
    const uint32_t slots = cap * kXcd;
    const uint32_t w = static_cast<uint32_t>(c.width);
    const uint32_t unit = kXcd * kPlanBlock * w;             // the deal's run unit: one group of blocks per list
    uint32_t lo[kWanderWindows + 3];
    lo[0] = 0;
    for (int k = 0; k <= kWanderWindows; ++k) lo[k + 1] = lo[k] + count[k];
    lo[kWanderWindows + 2] = slots;                          // the dead: the rest of the slots
    const uint32_t live = lo[kWanderWindows + 1];
    check(live <= c.ntracks && c.ntracks <= slots, "case set-up", c);
    uint32_t off[kWanderWindows + 3];
    const uint32_t fill = deal_plan(lo, cap, c.contiguous, w, off);
    const uint32_t total = off[kWanderWindows + 1];
    const bool dense = off[kWanderWindows + 2] != 0;

    check(total <= slots, "dealt total beyond cap * kXcd", c);
    check(total % unit == 0, "dealt total not a multiple of the run unit", c);
    check(fill >= 64 && fill <= kPlanBlock && (c.contiguous || fill == kPlanBlock), "fill", c);
    // every window's run holds all its tracks (k_deal_sorted: key k runs from off[k] to the next key's start)
    if (dense) {
        check(total >= live, "dense deal shorter than the live tracks", c);
        for (int k = 0; k <= kWanderWindows; ++k) check(off[k] == lo[k], "dense deal out of sorted order", c);
    } else {
        for (int k = 0; k <= kWanderWindows; ++k) {
            const uint32_t end = k < kWanderWindows ? off[k + 1] : total;
            check(off[k] <= end && off[k] % (kPlanBlock * w) == 0 && end % (kPlanBlock * w) == 0,
                  "a run not of whole groups of blocks", c);
            const unsigned long long held = static_cast<unsigned long long>((end - off[k]) / kPlanBlock) * fill;
            check(held >= count[k], "a window's run too short for its tracks", c);
        }
    }
    // the longest list is at most the host's bound, which is at most cap (before the deal the host's bound is at
    // least the longest list, which holds at least an eighth of the live tracks)
    const uint32_t before = (live + kXcd - 1) / kXcd;
    const uint32_t bound = deal_upper(before < cap ? before : cap, cap, c.contiguous, w);
    check(total / kXcd <= bound, "longest list beyond the host's bound", c);
    check(bound <= cap, "host's bound beyond cap", c);
    // the dense fall-back is taken only when the padded deal of full blocks does not fit
    unsigned long long padded = 0;
    for (int k = 0; k <= kWanderWindows; ++k) {
        const unsigned long long blocks = (count[k] + kPlanBlock - 1) / kPlanBlock;
        const unsigned long long groups = (blocks + w - 1) / w * w * kPlanBlock;
        padded += c.contiguous ? groups : (groups + unit - 1) / unit * unit;
    }
    padded = (padded + unit - 1) / unit * unit;
    check(dense == (padded > slots), "dense fall-back taken when the padded deal fits, or not taken when it does not", c);
}

// `live` tracks over the keys in use, spread by `shape`: 0 even, 1 one large window and many tiny ones
void spread(Case c, uint32_t live)
{
    std::vector<int> keys;
    for (int i = 0; i < c.windows; ++i) keys.push_back(i * (kWanderWindows + 1) / c.windows);
    if (static_cast<uint32_t>(c.windows) > live) return;
    std::vector<uint32_t> count(kWanderWindows + 1, 0u);
    if (c.shape == 0) {
        for (int i = 0; i < c.windows; ++i) count[keys[i]] = live / c.windows + (static_cast<uint32_t>(i) < live % c.windows ? 1u : 0u);
    } else {
        for (int i = 0; i + 1 < c.windows; ++i) count[keys[i]] = 1 + static_cast<uint32_t>(i % 3);
        uint32_t rest = live;
        for (int i = 0; i + 1 < c.windows; ++i) rest -= count[keys[i]];
        count[keys[c.windows - 1]] = rest;
    }
    one(c, count);
}

}  // namespace

int main()
{
    std::vector<long long> ntracks;
    const long long step = 4ll * kPlanBlock * kXcd;          // a whole number of the widest groups in every list
    for (long long m = step; m <= 250000; m += step)
        for (long long d = -1; d <= 1; ++d) ntracks.push_back(m + d);
    for (long long d = 0; d <= 64; d += 8) ntracks.push_back(kWanderMinTracks + d);
    ntracks.push_back(250000);
    for (long long n : ntracks)
        for (int windows = 1; windows <= kWanderWindows + 1; ++windows)
            for (int shape = 0; shape < 2; ++shape)
                for (int width : {1, 2, 4})
                    for (bool contiguous : {true, false}) {
                        const Case c = {n, windows, shape, width, contiguous};
                        // every track live (nearly every slot, next to a multiple of the list unit), most, half, few
                        for (long long live : {n, n - n / 16, n / 2, n / 7, 3000ll})
                            if (live > 0 && live <= n) spread(c, static_cast<uint32_t>(live));
                    }
    std::printf("%lld cases, %lld failures\n", cases, failures);
    return failures == 0 ? 0 : 1;
}
