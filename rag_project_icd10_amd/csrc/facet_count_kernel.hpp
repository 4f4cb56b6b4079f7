// facet_count_kernel.hpp - facet counts over a batch of row masks: for every query q of a batch and every
// group g of a grouping, counts[q][g] = the rows r < n whose bit is set in mask q and whose dense group number dense_of[r] is g. The
// terms aggregation of a search front end, Milvus's group-by count; the reference has no such call (services/milvus_service.py:280-285
// is its only read of the collection).
//
// ONE launch over mask_select_kernel.hpp's grid: one work-group of MS_THREADS lanes per (query, segment of MS_SEG_ROWS rows), the
// segment the fast index of a flat grid. The caller zeroes counts on the stream in front of the launch.
//   rows      lane l takes its 64 rows through ms_lane_bits (bits at or behind n and words at or behind mask_words read 0). A lane
//             whose 64 bits are all set - a NULL mask, a dense one - reads its 64 dense_of entries as sixteen 16-byte loads; any other
//             lane walks its set bits and reads dense_of for those rows only.
//   runs      consecutive set rows of one group are ONE add of the run's length (rows of a group are often neighbours: a corpus
//             sorted by code keeps a category's and a parent's rows together), so a lane of a single group issues one add.
//   G <= FC_LDS_GROUPS   the adds go to a histogram in LDS (integer ds_add, no return value); behind a barrier lane l adds the
//                        non-zero bins l, l + MS_THREADS, ... to counts[q] with one global integer add each.
//   G above it           the adds go to counts[q] directly (global integer add, no return value).
// Integer addition commutes and associates: whatever order the adds arrive in, the counts are the same bytes on every run. No float
// is added anywhere.
//
// VGPRs: 26 in both forms. LDS: FC_LDS_GROUPS x 4 bytes = 32 KB in the LDS form (five work-groups a CU), none in the global form. No
// scratch.
#pragma once
#include "facet_count_plan.hpp"
#include "mask_select_kernel.hpp"   // ms_lane_bits

namespace icd {

struct FacetCountArgs {
    const uint32_t *const *masks;   // [nq] -> bitset in icd_rowmask_pack's layout (an entry may be NULL: every row of the index)
    const int *dense_of;            // [n] the row's group, 0 .. G - 1 (16-byte aligned: a device allocation of its own)
    int *counts;                    // [nq][G], zero when the kernel starts
    long long n;                    // rows of the index
    long long mask_words;           // rowmask_tile_words(n)
    int segments;                   // ms_segments(n)
    int G;
};

// a run of `c` consecutive set rows of group `g` ends: one add
template <bool LDS>
__device__ __forceinline__ void fc_add(int *__restrict__ bins, int g, int c) {
    if (LDS) __hip_atomic_fetch_add(bins + g, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_fetch_add(bins + g, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the next set row's group: extends the run or ends it
template <bool LDS>
__device__ __forceinline__ void fc_row(int *__restrict__ bins, int g, int &run_g, int &run_c) {
    if (g == run_g) { ++run_c; return; }
    if (run_c) fc_add<LDS>(bins, run_g, run_c);
    run_g = g; run_c = 1;
}

template <bool LDS>
__global__ __launch_bounds__(MS_THREADS) void facet_count_kernel(const FacetCountArgs a) {
    __shared__ int hist[LDS ? FC_LDS_GROUPS : 1];
    const int tid = threadIdx.x;
    const long long q = blockIdx.x / (unsigned)a.segments, seg = blockIdx.x - (unsigned)q * (unsigned)a.segments;
    int *__restrict__ out = a.counts + q * a.G;
    int *__restrict__ bins = LDS ? hist : out;
    if (LDS) {
        for (int g = tid; g < a.G; g += MS_THREADS) hist[g] = 0;
        __syncthreads();
    }

    const unsigned long long bits = ms_lane_bits(a.masks[q], a.n, a.mask_words, seg, tid);
    const long long row0 = seg * MS_SEG_ROWS + (long long)tid * MS_LANE_ROWS;
    int run_g = -1, run_c = 0;
    if (bits == ~0ull) {   // all 64 rows lie in front of n (ms_lane_bits cleared the others) and count
        const int4 *__restrict__ src = reinterpret_cast<const int4 *>(a.dense_of + row0);
#pragma unroll
        for (int c = 0; c < 4; ++c) {   // four loads in flight, sixteen in all
            const int4 v0 = src[4 * c], v1 = src[4 * c + 1], v2 = src[4 * c + 2], v3 = src[4 * c + 3];
            fc_row<LDS>(bins, v0.x, run_g, run_c); fc_row<LDS>(bins, v0.y, run_g, run_c); fc_row<LDS>(bins, v0.z, run_g, run_c); fc_row<LDS>(bins, v0.w, run_g, run_c);
            fc_row<LDS>(bins, v1.x, run_g, run_c); fc_row<LDS>(bins, v1.y, run_g, run_c); fc_row<LDS>(bins, v1.z, run_g, run_c); fc_row<LDS>(bins, v1.w, run_g, run_c);
            fc_row<LDS>(bins, v2.x, run_g, run_c); fc_row<LDS>(bins, v2.y, run_g, run_c); fc_row<LDS>(bins, v2.z, run_g, run_c); fc_row<LDS>(bins, v2.w, run_g, run_c);
            fc_row<LDS>(bins, v3.x, run_g, run_c); fc_row<LDS>(bins, v3.y, run_g, run_c); fc_row<LDS>(bins, v3.z, run_g, run_c); fc_row<LDS>(bins, v3.w, run_g, run_c);
        }
    } else {
        unsigned long long rest = bits;
        while (rest) {
            const int b = __ffsll((long long)rest) - 1;
            rest &= rest - 1ull;
            fc_row<LDS>(bins, a.dense_of[row0 + b], run_g, run_c);
        }
    }
    if (run_c) fc_add<LDS>(bins, run_g, run_c);

    if (LDS) {
        __syncthreads();
        for (int g = tid; g < a.G; g += MS_THREADS) {
            const int c = hist[g];
            if (c) __hip_atomic_fetch_add(out + g, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace icd
