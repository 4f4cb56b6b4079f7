// maxsim_kernel.hpp - the embedding-list search (Milvus 2.6 embedding lists, metric MAX_SIM): a query is a
// LIST of vectors and a group of rows scores the sum, over the list's vectors, of its best row's inner product. Runs behind
// group_scores_kernel and group_best_kernel (group_topk.hpp), which stay as they are, on their output for one pass of whole
// lists (maxsim_plan.hpp):
//
//   in    best[vector][group] = make_key(score, row) of the group's best row under that vector, 0 for no hit
//   1. maxsim_reduce_kernel   agg[list][group] = make_key(aggregate, row of the first hitting vector's best row), 0 for no hit.
//                             A lane owns ONE group of ONE list and walks the list's rows of `best` in list order: the chain of
//                             IEEE fp32 adds never leaves the lane (rounding does not commute: the order is the contract), and
//                             the lanes of a wave read 64 neighbouring groups of the same row. Every cell is written exactly once
//                             with a plain store - no atomics, no zeroing in front.
//   2. maxsim_finish_kernel   one wave per list: the k best cells (wave_select, group_topk.hpp), the groups' scores and ids, and
//                             for every vector of the list the gather of best[vector][winning group] into the match outputs.
//
// The reference searches its segments one by one (services/multi_diagnosis_service.py) and has no counterpart.
#pragma once
#include "group_aggregate_kernel.hpp"   // ga_add, ga_div: ONE IEEE fp32 operation each
#include "group_topk.hpp"
#include "maxsim_plan.hpp"

namespace icd {

struct MaxsimReduceArgs {
    const u64 *best;     // [vectors of the pass][G]
    u64 *agg;            // [lists of the pass][G]; every cell of the launch's lists is written
    int G, mean;         // mean = 1: divide the sum by the number of hitting vectors
    MaxsimLists lists;
};

// block (x, y) = 256 consecutive groups of list y of the launch
__global__ __launch_bounds__(256) void maxsim_reduce_kernel(MaxsimReduceArgs a) {
    const int g = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y;
    if (g >= a.G || l >= a.lists.n) return;
    const int t0 = a.lists.off[l], t1 = a.lists.off[l + 1];
    const u64 *col = a.best + (size_t)t0 * a.G + g;
    float acc = 0.0f;
    uint32_t row = 0u;
    int hits = 0;
    for (int t = t0; t < t1; ++t, col += a.G) {
        const u64 key = *col;
        if (key == 0ull) continue;
        if (hits == 0) { acc = key_score(key); row = key_row(key); }
        else acc = ga_add(acc, key_score(key));
        ++hits;
    }
    u64 cell = 0ull;
    if (hits > 0) {
        const float v = a.mean ? ga_div(acc, (float)hits) : acc;
        if (v == v) cell = make_key(v, row);   // (+inf + -inf: a NaN aggregate is no hit)
    }
    a.agg[(size_t)(a.lists.first + l) * a.G + g] = cell;
}

struct MaxsimFinishArgs {
    const u64 *agg;            // [lists of the pass][G]
    const u64 *best;           // [vectors of the pass][G]
    const int *dense_of;       // [n] dense group of every row
    const int *groups;         // [n] the caller's group id of every row
    const int *levels;         // [n] or null
    const long long *row_map;  // a view's global ids, or null
    long long id_base;
    int G, k;
    long long v_base, l_base;  // first vector and first list of the pass: the outputs are indexed by the call's numbering
    MaxsimLists lists;
    float *out_group_scores;   // [list][k]; -inf in padding
    int *out_group_ids;        // [list][k]; -1 in padding
    float *out_match_scores;   // [vector][k]; -inf in padding   } any of the three may be null
    long long *out_match_ids;  // [vector][k]; -1 in padding
    int *out_match_levels;     // [vector][k]; 0 in padding
};

constexpr int MAXSIM_FIN_WAVE_LDS = 256 * 8 + 128 * 4;   // select buffer | dense numbers of the winning groups

template <int KP, int E>
__global__ __launch_bounds__(256) void maxsim_finish_kernel(MaxsimFinishArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[4 * MAXSIM_FIN_WAVE_LDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l = blockIdx.x * 4 + wave;
    if (l >= a.lists.n) return;
    u64 *buf = reinterpret_cast<u64 *>(smem + (size_t)wave * MAXSIM_FIN_WAVE_LDS);
    int *gsel = reinterpret_cast<int *>(buf + 256);

    const u64 *cells = a.agg + (size_t)(a.lists.first + l) * a.G;
    const int ng = min(a.k, wave_select<KP, E>([&](int i) { return cells[i]; }, a.G, buf, lane));
    const size_t o = (size_t)(a.l_base + a.lists.first + l) * a.k;
    for (int j = lane; j < a.k; j += 64) {
        const int row = j < ng ? (int)key_row(buf[j]) : 0;
        if (a.out_group_scores) a.out_group_scores[o + j] = j < ng ? key_score(buf[j]) : -INFINITY;
        if (a.out_group_ids) a.out_group_ids[o + j] = j < ng ? a.groups[row] : -1;
        if (j < ng) gsel[j] = a.dense_of[row];
    }
    if (!a.out_match_scores && !a.out_match_ids && !a.out_match_levels) return;
    const int t0 = a.lists.off[l], T = a.lists.off[l + 1] - t0;
    for (int i = lane; i < T * a.k; i += 64) {
        const int t = i / a.k, j = i - t * a.k;
        const u64 key = j < ng ? a.best[(size_t)(t0 + t) * a.G + gsel[j]] : 0ull;
        const size_t w = (size_t)(a.v_base + t0 + t) * a.k + j;
        const int row = (int)key_row(key);
        if (a.out_match_scores) a.out_match_scores[w] = key ? key_score(key) : -INFINITY;
        if (a.out_match_ids) a.out_match_ids[w] = key ? (a.row_map ? a.row_map[row] : a.id_base + row) : -1ll;
        if (a.out_match_levels) a.out_match_levels[w] = key ? (a.levels ? a.levels[row] : 1) : 0;
    }
}

}  // namespace icd
