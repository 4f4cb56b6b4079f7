// group_aggregate_kernel.hpp - the group scorers SUM / AVG of the grouping search: a group ranks by the
// sum, or the mean, of the scores of its min(group_size, hits) best members instead of by its best row. Takes group_best_kernel's
// place between group_scores_kernel and group_finish_kernel (group_topk.hpp), which stay as they are:
//
//   in    S[query][position], the canonical scores in (group, row) order
//   out   best[query][group] = make_key(aggregate, row of the group's best member), 0 for no hit
//
// The aggregate is ONE chain of IEEE fp32 adds, best member first (rounding does not commute: the order is the contract), and for
// AVG one IEEE fp32 divide by the member count behind it. Such a chain cannot be combined across a cut, so the work is cut at
// group boundaries by the host (group_aggregate_plan.hpp): packs of whole groups for one wave, one wave per long group. Every
// (query, group) cell is written exactly once with a plain store - no atomics, no zeroing in front, no scratch.
//
// The reference has no counterpart (services/milvus_service.py:280-285 passes no grouping at all); Milvus names the scorers
// max / sum / avg in its grouping search.
#pragma once
#include "group_aggregate_plan.hpp"
#include "group_topk.hpp"

namespace icd {

struct GroupAggArgs {
    const float *S;
    long long ldS;
    const int *order;         // [n] row at every position
    const int *gpos;          // [n] dense group at every position
    const int *seg;           // [G + 1] first position of every group
    const GaPack *packs;      // [npacks]
    const int *long_groups;   // [nlong]
    int nq, G, s, avg;        // queries of this pass, groups, group_size, 1 = divide by the member count
    int npacks, nlong;
    u64 *best;                // [nq][G]; every cell is written
};

// ONE IEEE fp32 add / divide, rounded once: nothing contracted, nothing reassociated (boost_mul's rule)
__device__ __forceinline__ float ga_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float ga_div(float a, float b) {
#pragma clang fp contract(off)
    return a / b;
}

// make_key(aggregate, best member's row); a NaN aggregate (+inf + -inf) is no hit
__device__ __forceinline__ u64 ga_key(float sum, int m, int avg, u64 best_member) {
    const float agg = avg ? ga_div(sum, (float)m) : sum;
    return agg == agg ? make_key(agg, key_row(best_member)) : 0ull;
}

// One wave = one pack x GA_QW queries, lane l = position p0 + l (the groups' boundaries are the same for every query).
//   1. rank-by-count inside the group: 64 wave-uniform lane reads, independent of group_size (the alternative, group_size
//      extract-the-maximum rounds of the segmented scan, costs 6 shuffle steps per round and query: section 24.3)
//   2. one forward permute puts the key of rank r into lane (group's first lane + r): the run is sorted in place
//   3. the group's first lane adds the scores of lanes +1, +2, ... in that order, one backward permute per step
__global__ __launch_bounds__(256) void group_aggregate_pack_kernel(GroupAggArgs a) {
    constexpr int QW = GA_QW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long w = (long long)blockIdx.x * GA_WAVES + wave;
    const int q0 = (int)(w / a.npacks) * QW;
    if (q0 >= a.nq) return;
    const GaPack pk = a.packs[(int)(w % a.npacks)];
    const bool in = lane < pk.len;
    const int p = pk.p0 + (in ? lane : 0);   // (an idle lane reads the pack's first position and holds no key)
    const int g = in ? a.gpos[p] : -2;
    const uint32_t row = (uint32_t)a.order[p];
    const int first = in ? a.seg[g] - pk.p0 : lane;        // the lane of the group's first position
    const int run = in ? a.seg[g + 1] - a.seg[g] : 0;
    const bool leader = in && lane == first;

    u64 key[QW];
    int rank[QW], hits[QW];
#pragma unroll
    for (int i = 0; i < QW; ++i) {
        key[i] = 0ull; rank[i] = 0; hits[i] = 0;
        if (in && q0 + i < a.nq) {
            const float sc = a.S[(size_t)(q0 + i) * a.ldS + p];
            if (sc == sc) key[i] = make_key(sc, row);   // (a NaN score is no hit)
        }
    }
    for (int j = 0; j < pk.len; ++j) {
        const bool same = readlane<int>(g, j) == g;
#pragma unroll
        for (int i = 0; i < QW; ++i) {
            const u64 kj = readlane_u64(key[i], j);
            rank[i] += (same && kj > key[i]) ? 1 : 0;
            hits[i] += (same && kj != 0ull) ? 1 : 0;
        }
    }
    // A hit's rank is below its group's hit count; every non-hit of a group has rank == that count, which is below `run` when
    // there is one: all targets lie inside the group's own lanes, and lanes that collide all carry key 0.
    u64 sorted[QW];
    float x[QW], acc[QW];
#pragma unroll
    for (int i = 0; i < QW; ++i) {
        const int dst = (first + rank[i]) << 2;
        const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_permute(dst, (int)(uint32_t)key[i]);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_permute(dst, (int)(uint32_t)(key[i] >> 32));
        sorted[i] = ((u64)hi << 32) | lo;
        x[i] = key_score(sorted[i]);
        acc[i] = x[i];
    }
    const int steps = min(a.s, run);   // members the group's first lane adds up, at most
    for (int t = 1; __ballot(leader && t < steps) != 0ull; ++t) {
        const int src = min(first + t, 63);
#pragma unroll
        for (int i = 0; i < QW; ++i) {
            const float v = __shfl(x[i], src);
            if (leader && t < min(a.s, hits[i])) acc[i] = ga_add(acc[i], v);
        }
    }
    if (leader) {
#pragma unroll
        for (int i = 0; i < QW; ++i)
            if (q0 + i < a.nq)
                a.best[(size_t)(q0 + i) * a.G + g] = hits[i] > 0 ? ga_key(acc[i], min(a.s, hits[i]), a.avg, sorted[i]) : 0ull;
    }
}

// One wave = one (query, long group): the group_size best of the run by wave_select (KP >= group_size; its buffer compacts every
// 64 (E - 1) appended keys), sorted best first, then the chain over them - every lane the same adds from the same LDS words.
template <int KP, int E>
__global__ __launch_bounds__(256) void group_aggregate_long_kernel(GroupAggArgs a) {
    __shared__ u64 smem[GA_WAVES * 64 * E];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long item = (long long)blockIdx.x * GA_WAVES + wave;
    if (item >= (long long)a.nlong * a.nq) return;
    const int q = (int)(item / a.nlong), g = a.long_groups[(int)(item % a.nlong)];
    const int b = a.seg[g], e = a.seg[g + 1];
    u64 *buf = smem + (size_t)wave * 64 * E;
    const float *sq = a.S + (size_t)q * a.ldS;
    const int m = min(a.s, wave_select<KP, E>([&](int i) {
        const float sc = sq[b + i];
        return sc == sc ? make_key(sc, (uint32_t)a.order[b + i]) : 0ull;
    }, e - b, buf, lane));
    u64 out = 0ull;
    if (m > 0) {
        const u64 top = buf[0];
        float acc = key_score(top);
        for (int i = 1; i < m; ++i) acc = ga_add(acc, key_score(buf[i]));
        out = ga_key(acc, m, a.avg, top);
    }
    if (lane == 0) a.best[(size_t)q * a.G + g] = out;
}

}  // namespace icd
