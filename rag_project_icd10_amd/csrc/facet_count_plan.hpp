// facet_count_plan.hpp - the arithmetic of the facet counts over row masks: which segment of the select's grid
// a row falls into, which of the two accumulation forms a grouping of G groups takes, how many queries' counts fit a result block
// and how many passes a batch then needs. No HIP header and no handle: included by facet_count_kernel.hpp (the kernel calls these
// very functions), by icd_facet.hpp (the launch geometry, the passes) and by tests/facet_count_plan_check.cpp, which runs them under
// the host sanitizers. The segments themselves are mask_select_plan.hpp's: one grid shape for everything that walks a mask.
#pragma once
#include "mask_select_plan.hpp"

#ifndef ICD_FC_LDS_GROUPS
#define ICD_FC_LDS_GROUPS 8192   // (a build may set another bound to measure it: scripts/probe/facet_counts.py)
#endif

namespace icd {

// Groups up to which a work-group counts into a histogram of its own in LDS (4 bytes a bin: 32 KB); above it the lanes add into
// the query's global row directly. _native.FACET_LDS_GROUPS repeats the value for the tests.
constexpr int FC_LDS_GROUPS = ICD_FC_LDS_GROUPS;
static_assert(FC_LDS_GROUPS >= 1 && FC_LDS_GROUPS <= 16384, "the histogram is static LDS: at most 64 KB");

constexpr long long FC_MAX_GRID = 0x7FFFFFFFll;   // work-groups of one launch (a flat grid x)

// the segment of the grid that counts row `row` (rows >= 0), and the lane of its work-group that holds the row's bit
MS_HD inline long long fc_segment_of(long long row) { return row / MS_SEG_ROWS; }
MS_HD inline int fc_lane_of(long long row) { return (int)((row % MS_SEG_ROWS) / MS_LANE_ROWS); }

// the accumulation form of a grouping of G groups: true = the LDS histogram, false = global adds
MS_HD inline bool fc_lds_form(long long G) { return G >= 1 && G <= FC_LDS_GROUPS; }

// queries whose [G] int32 counts fit a block of `block_bytes` bytes (0: the block cannot hold one query)
MS_HD inline long long fc_block_queries(long long block_bytes, long long G) {
    if (block_bytes <= 0 || G <= 0) return 0;
    return block_bytes / (G * 4);
}

// queries of ONE launch: what the block holds (`per_block` < 0: no block, the caller's device buffer takes every query) and what a
// flat grid of `segments` work-groups per query addresses
MS_HD inline long long fc_pass_queries(long long nq, long long per_block, long long segments) {
    if (nq <= 0 || segments <= 0) return 0;
    long long per = nq;
    if (per_block >= 0 && per_block < per) per = per_block;
    const long long by_grid = FC_MAX_GRID / segments;
    return per < by_grid ? per : by_grid;
}

// launches of a batch of nq queries at `per` queries each (0 for an empty batch; -1 when `per` is 0: nothing fits)
MS_HD inline long long fc_passes(long long nq, long long per) {
    if (nq <= 0) return 0;
    if (per <= 0) return -1;
    return (nq - 1) / per + 1;
}

}  // namespace icd
