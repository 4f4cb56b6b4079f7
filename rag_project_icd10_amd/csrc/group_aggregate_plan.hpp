// group_aggregate_plan.hpp - the host-made plan of the group scorers SUM / AVG: how the positions of a
// grouping's (group, row) order are cut into work for group_aggregate_kernel.hpp. A top-s with an ORDERED sum cannot be combined
// across a cut the way group_best_kernel's maximum is, so the cuts are group boundaries:
//
//   pack       consecutive WHOLE groups, each of at most GA_PACK positions, whose runs together fit GA_PACK positions: one
//              wave, one lane per position. Greedy, left to right: a pack ends in front of the first group that no longer fits.
//   long item  a group of more than GA_PACK positions, alone: one wave walks its run.
//
// Every position lies in exactly one of the two. No HIP header and no handle: included by group_aggregate_kernel.hpp and by
// tests/group_aggregate_plan_check.cpp, which runs ga_plan under the host sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace icd {

constexpr int GA_PACK = 64;      // positions of one pack: the lanes of a wave
constexpr int GA_QW = 4;         // queries a pack's wave reduces at once (group_best_kernel's QW)
constexpr int GA_WAVES = 4;      // waves of one work-group, in both kernels

// the scorers of icd_index_search_grouped_scored (include/icd_search.h ICD_GROUP_SCORER_*)
constexpr int GA_MAX = 0, GA_SUM = 1, GA_AVG = 2;

struct GaPack {
    int p0;    // first position
    int len;   // positions, 1 .. GA_PACK; it starts and ends on group boundaries
};

struct GaPlan {
    std::vector<GaPack> packs;
    std::vector<int> long_groups;   // dense numbers of the groups of more than GA_PACK positions, ascending
    size_t bytes() const { return packs.size() * sizeof(GaPack) + long_groups.size() * sizeof(int); }
};

// seg: [G + 1] first position of every group, seg[G] = n (icd_grouping_create's table); every group holds at least one row
inline GaPlan ga_plan(const int *seg, int G) {
    GaPlan plan;
    GaPack open{0, 0};
    auto close = [&]() {
        if (open.len > 0) plan.packs.push_back(open);
        open.len = 0;
    };
    for (int g = 0; g < G; ++g) {
        const int b = seg[g], run = seg[g + 1] - seg[g];
        if (run > GA_PACK) {
            close();
            plan.long_groups.push_back(g);
            continue;
        }
        if (open.len > 0 && open.len + run > GA_PACK) close();
        if (open.len == 0) open.p0 = b;
        open.len += run;
    }
    close();
    return plan;
}

// work-groups of the pack kernel for nb queries, and of the long kernel (one wave per (query, long group))
inline long long ga_pack_blocks(long long npacks, long long nb) { return (npacks * ((nb + GA_QW - 1) / GA_QW) + GA_WAVES - 1) / GA_WAVES; }
inline long long ga_long_blocks(long long nlong, long long nb) { return (nlong * nb + GA_WAVES - 1) / GA_WAVES; }

}  // namespace icd
