// recommend_kernel.hpp - recommend search: rank every row by a request's positive and negative examples,
// exact over the whole index. Replaces what a caller does today: every example's scores pulled to the host, folded and sorted
// there - best_score and sum_scores are functions of every example's score on every row, so no list of an existing search holds
// the answer.
//
// recommend_examples_kernel   one work-group per vector of the block's E[vector][dim]. best_score / sum_scores: example e of the
//                             block, a copy of the stored fp32 row or of the caller's vector. average_vector: request r's ONE target,
//                             per component mp = the positives summed in list order from +0.0f, one correctly rounded divide by
//                             (float)P, mn the same over the negatives, t = mp + (mp - mn) (N > 0) or mp. No multiply stands next
//                             to an add: nothing to contract.
// (wide_scores_kernel         over E, unmasked and unbanded, into SE[vector][n padded]: order_f32(score), 0 for a NaN score or a
//                             row past n. Untouched; the examples of many requests share its 128-query tiles.)
// recommend_combine_kernel    grid (row segments, requests), every lane four consecutive rows: per example of the request ONE
//                             16-byte load of the rows' ordered words, decoded and folded in list order (best_score: the largest
//                             positive and the largest negative score by plain compares, c = bp if bp > bn else -(bn * bn);
//                             sum_scores: acc + s over the positives, then acc - s over the negatives, from +0.0f; average_vector:
//                             the target's own score). Then the request's mask bits, the example-row exclusion (at most 16
//                             compares against the lane's first row), the band, and ONE 16-byte store of order_f32(c) - 0 for a row
//                             that does not rank - into S[request][n padded]. A word of 0 in any example makes the row's word 0.
//                             (P + N + 1) x 4 bytes per row, nothing else: memory-bound. No LDS, no scratch, no atomics.
// (wide_threshold_kernel, wide_collect_kernel, wide_sort_emit_kernel<TIER> over S, untouched.)
// Vector stores only, no printf or assert: the same bytes on every run.
#pragma once
#include "group_aggregate_kernel.hpp"   // ga_add, ga_div: ONE IEEE fp32 operation each
#include "recommend_plan.hpp"
#include "topk_select.hpp"
#include "wide_select_kernel.hpp"

namespace icd {

__device__ __forceinline__ float rc_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ float rc_neg_square(float a) {   // one fp32 multiply, then the sign flip
#pragma clang fp contract(off)
    const float sq = a * a;
    return -sq;
}

// the request table of a call (rc_table_*): device pointers into ONE block
struct RecommendTable {
    const int *off;     // [nr + 1]
    const int *npos;    // [nr]
    const int *rows;    // [ne]
};

struct RecommendExampleArgs {
    const float *corpus;    // [n][dim]
    const float *vectors;   // nullable (no example of the call is a vector): [ne][dim] in the call's example order
    RecommendTable t;
    float *E;               // [vectors of the block][dim]
    int r0, e0;             // the block's first request and first example
    int dim, average;       // average: one target per request; else one vector per example
};

__global__ __launch_bounds__(RC_EXAMPLE_THREADS) void recommend_examples_kernel(const RecommendExampleArgs a) {
    const int dim4 = a.dim / 4;   // (dim is a multiple of 32)
    float4 *dst = reinterpret_cast<float4 *>(a.E + (size_t)blockIdx.x * a.dim);
    auto source = [&](int e) {
        const int row = a.t.rows[e];
        return reinterpret_cast<const float4 *>(row >= 0 ? a.corpus + (size_t)row * a.dim : a.vectors + (size_t)e * a.dim);
    };
    if (!a.average) {
        const float4 *src = source(a.e0 + (int)blockIdx.x);
        for (int d = threadIdx.x; d < dim4; d += RC_EXAMPLE_THREADS) dst[d] = src[d];
        return;
    }
    const int r = a.r0 + (int)blockIdx.x;
    const int b = a.t.off[r], cnt = a.t.off[r + 1] - b, P = a.t.npos[r], N = cnt - P;
    auto mean = [&](int first, int m, int d) {
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int j = 0; j < m; ++j) {
            const float4 v = source(first + j)[d];
            acc.x = ga_add(acc.x, v.x); acc.y = ga_add(acc.y, v.y); acc.z = ga_add(acc.z, v.z); acc.w = ga_add(acc.w, v.w);
        }
        const float fm = (float)m;
        return make_float4(__fdiv_rn(acc.x, fm), __fdiv_rn(acc.y, fm), __fdiv_rn(acc.z, fm), __fdiv_rn(acc.w, fm));
    };
    for (int d = threadIdx.x; d < dim4; d += RC_EXAMPLE_THREADS) {
        float4 t = mean(b, P, d);
        if (N > 0) {
            const float4 mn = mean(b + P, N, d);
            t.x = ga_add(t.x, rc_sub(t.x, mn.x)); t.y = ga_add(t.y, rc_sub(t.y, mn.y));
            t.z = ga_add(t.z, rc_sub(t.z, mn.z)); t.w = ga_add(t.w, rc_sub(t.w, mn.w));
        }
        dst[d] = t;
    }
}

struct RecommendCombineArgs {
    const uint32_t *SE;     // [vectors of the block][n_pad]
    uint32_t *S;            // [requests of the block][n_pad]
    long long n_pad;
    RecommendTable t;
    RowMasks mask;          // nullable: no request of the call is masked; else the block's entries
    const float *lo, *hi;   // nullable each: radius / range_filter of the block's requests
    int r0, e0;             // the block's first request and first example
    int average;            // SE holds ONE run per request: the target's scores
};

template <bool SUM>
__global__ __launch_bounds__(RC_COMBINE_THREADS) void recommend_combine_kernel(const RecommendCombineArgs a) {
    const int rb = blockIdx.y, r = a.r0 + rb;
    const long long row0 = ((long long)blockIdx.x * RC_COMBINE_THREADS + threadIdx.x) * RC_LANE_ROWS;
    if (row0 >= a.n_pad) return;   // (n_pad is a multiple of 128: a lane's four rows are inside it or past it)
    const int b = a.t.off[r], cnt = a.t.off[r + 1] - b;
    // the runs folded: the request's examples, positives first - or the one run of its target, a single positive
    const int slot0 = a.average ? rb : b - a.e0, runs = a.average ? 1 : cnt, np = a.average ? 1 : a.t.npos[r];
    const uint32_t *run = a.SE + ws_s_offset(slot0, a.n_pad) + row0;

    float x[4], y[4];   // SUM: x = acc. else x = bp, y = bn
#pragma unroll
    for (int j = 0; j < 4; ++j) { x[j] = SUM ? 0.0f : -INFINITY; y[j] = -INFINITY; }
    uint32_t dead = 0u;   // bit j: an example's word of row j is 0 (a NaN score, a row past n)
#pragma unroll 4
    for (int e = 0; e < runs; ++e) {
        const uint4 v = *reinterpret_cast<const uint4 *>(run + (size_t)e * (size_t)a.n_pad);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const bool positive = e < np;   // (uniform)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            dead |= (w[j] == 0u ? 1u : 0u) << j;
            const float s = unorder_f32(w[j]);
            if (SUM) {
                x[j] = positive ? ga_add(x[j], s) : rc_sub(x[j], s);
            } else if (positive) {
                x[j] = s > x[j] ? s : x[j];
            } else {
                y[j] = s > y[j] ? s : y[j];
            }
        }
    }

    // what ranks: the mask's four bits (row0 is a multiple of 4: one word), not an example row of the request, the band
    uint32_t live = 0xFu;
    if (a.mask) live = (a.mask[rb][row0 >> 5] >> (uint32_t)(row0 & 31)) & 0xFu;
    for (int e = 0; e < cnt; ++e) {
        const uint32_t d = (uint32_t)(a.t.rows[b + e] - (int)row0);   // (a vector example is -1: never inside)
        if (d < 4u) live &= ~(1u << d);
    }
    live &= ~dead;
    const bool open_lo = a.lo == nullptr;   // (no radius: a combined score of -inf ranks, as in the wide search)
    const float lo = a.lo ? a.lo[rb] : -INFINITY, hi = a.hi ? a.hi[rb] : INFINITY;
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float c = SUM ? x[j] : (x[j] > y[j] ? x[j] : rc_neg_square(y[j]));
        const bool in = (((live >> j) & 1u) != 0u) & (c == c) & (open_lo | (lo < c)) & (c <= hi);
        o[j] = in ? order_f32(c) : 0u;
    }
    *reinterpret_cast<uint4 *>(a.S + ws_s_offset(rb, a.n_pad) + row0) = make_uint4(o[0], o[1], o[2], o[3]);
}

}  // namespace icd
