// mmr_select_kernel.hpp - MMR search, step 2: out of a query's exact candidate list, the k hits that are
// not copies of each other. Replaces, on the device, what a caller of LangChain's Milvus max_marginal_relevance_search does on
// the host with fetch_k vectors of 3 KB each and a fetch_k x fetch_k similarity in numpy.
//
// One work-group of 256 lanes (64 quads) per query. LDS holds the candidates' rel / row / level / pen / value / picked arrays and
// the row of the newest pick. Pick 0 is candidate 0; every further step
//   1. stages the newest pick's fp32 row into LDS with coalesced 16-byte loads;
//   2. runs ONE canonical chain per unpicked candidate against it - the strict d-ascending fmaf chain from +0.0f, the bits of
//      oracle/icd_oracle.c chain_score - four lanes to a row as in finalize.hpp's rescoring walk: lane qi of a quad loads piece
//      4 b + qi of every 64-byte block b, all four run their four fmaf from the same running value and the quad adopts lane 0's,
//      1's, 2's, 3's result in turn (one DPP quad broadcast per step). The pick's row is read from LDS: four addresses per wave,
//      a broadcast;
//   3. updates the candidate's pen and value (mmr_plan.hpp: the arithmetic the host check runs);
//   4. takes the argmax over (value, -index): every wave folds the 128 entries with mmr_fold in a butterfly, so every lane
//      holds the winner and no broadcast round trip is needed.
// The ORDER of the chain is the contract (a different order gives other bits, and a value that ties under one order does not
// under another); everything else here is free. No atomics, nothing data-dependent in an output position: the same call twice
// gives the same bytes. Rows are 64-bit: id_base is subtracted on the way in and added on the way out.
//
// LDS: the lists, 6 272 bytes static (128 x rel, row, level, pen, value, picked, pick, pick value, adjusted score), and the row,
// dim floats dynamic (16 KB at dim 4096). 64 VGPRs, no scratch.
#pragma once
#include "finalize.hpp"
#include "mmr_plan.hpp"

namespace icd {

constexpr int MMR_THREADS = 256;
constexpr int MMR_QUADS = MMR_THREADS / 4;
static_assert(MMR_MAX_FETCH == FIN_MAX_K, "a candidate list is a search's output");
static_assert(MMR_MAX_FETCH == 2 * MMR_QUADS, "a quad owns candidates quad and quad + 64");

struct MmrArgs {
    const float *st_raw;          // [nq][fetch_k] the candidate lists, raw order (staging of the handle)
    const long long *st_ids;      // global ids, -1 = padding (behind the hits)
    const int *st_levels;         // the hits' levels
    const float *corpus;          // [n][dim] the fp32 rows the canonical scores are computed from
    long long n, id_base;
    int dim, k, fetch_k, reweighted;
    double lambda, one_minus;     // one_minus = 1 - lambda, computed once on the host
    double *out_adj;              // [nq][k], reweighted only
    float *out_raw;
    long long *out_ids;
    int *out_levels;              // nullable
    double *out_mmr;              // nullable
};

// The canonical chain of corpus row `row` against the row staged at `prow` (LDS), four lanes per row; every lane of the quad
// returns the chain value. dim is a multiple of 32: FIN_WALK blocks of 64 bytes per trip while they last, then pairs.
__device__ __forceinline__ float mmr_quad_chain(const float *corpus, long long row, int dim, const float *prow, int qi) {
    const int nblk = dim >> 4;
    const f32x4 *c4 = reinterpret_cast<const f32x4 *>(corpus + (size_t)row * dim) + qi;
    const f32x4 *p4 = reinterpret_cast<const f32x4 *>(prow) + qi;
    float acc = 0.0f;
#define ICD_MMR_STEP(ctrl)                                                                              \
    {                                                                                                   \
        float t = acc;                                                                                  \
        t = __builtin_fmaf(pv.x, cv.x, t);                                                              \
        t = __builtin_fmaf(pv.y, cv.y, t);                                                              \
        t = __builtin_fmaf(pv.z, cv.z, t);                                                              \
        t = __builtin_fmaf(pv.w, cv.w, t);                                                              \
        acc = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(t), ctrl, 0xf, 0xf, false)); \
    }
#define ICD_MMR_TRIP(WALK)                                                         \
    {                                                                              \
        f32x4 cvv[WALK];                                                           \
        _Pragma("unroll") for (int u = 0; u < WALK; ++u) cvv[u] = c4[4 * (b0 + u)]; \
        _Pragma("unroll") for (int u = 0; u < WALK; ++u) {                         \
            const f32x4 cv = cvv[u];                                               \
            const f32x4 pv = p4[4 * (b0 + u)];                                     \
            ICD_MMR_STEP(0x00)                                                     \
            ICD_MMR_STEP(0x55)                                                     \
            ICD_MMR_STEP(0xAA)                                                     \
            ICD_MMR_STEP(0xFF)                                                     \
        }                                                                          \
    }
    int b0 = 0;
    for (; b0 + FIN_WALK <= nblk; b0 += FIN_WALK) ICD_MMR_TRIP(FIN_WALK)
    for (; b0 < nblk; b0 += 2) ICD_MMR_TRIP(2)
#undef ICD_MMR_TRIP
#undef ICD_MMR_STEP
    return acc;
}

// the winner of the 128 slots, in every lane of the calling wave
__device__ __forceinline__ MmrEntry mmr_wave_winner(const double *val, const unsigned char *picked, int C, int lane) {
    const int i0 = lane, i1 = lane + 64;
    MmrEntry e = mmr_entry(i0 < C ? val[i0] : 0.0, i0, i0 >= C || picked[i0] != 0);
    e = mmr_fold(e, mmr_entry(i1 < C ? val[i1] : 0.0, i1, i1 >= C || picked[i1] != 0));
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        MmrEntry o;
        o.value = __shfl_xor(e.value, m, 64);
        o.idx = __shfl_xor(e.idx, m, 64);
        e = mmr_fold(e, o);
    }
    return e;
}

#pragma clang fp contract(off)
__global__ __launch_bounds__(MMR_THREADS) void mmr_select_kernel(const MmrArgs a) {
    extern __shared__ __attribute__((aligned(16))) float prow[];   // [dim] the newest pick's row
    __shared__ float rel[MMR_MAX_FETCH];
    __shared__ long long rows[MMR_MAX_FETCH];
    __shared__ int lvl[MMR_MAX_FETCH];
    __shared__ float pen[MMR_MAX_FETCH];
    __shared__ double val[MMR_MAX_FETCH];
    __shared__ unsigned char picked[MMR_MAX_FETCH];
    __shared__ int pick_of[MMR_MAX_FETCH];       // pick t = candidate pick_of[t]
    __shared__ double pick_val[MMR_MAX_FETCH];   // ... won with this value
    __shared__ double adjbuf[MMR_MAX_FETCH];
    const int tid = threadIdx.x, lane = tid & 63;
    const int quad = tid >> 2, qi = tid & 3;
    const int q = blockIdx.x;
    const int k = a.k, F = a.fetch_k;
    const size_t sbase = (size_t)q * F;

    // candidates: the hits of the staged list (padding sits behind them; a slot whose id is no row of the index ends the list too)
    bool hit = false;
    if (tid < MMR_MAX_FETCH) {
        long long r = -1;
        if (tid < F) {
            const long long id = a.st_ids[sbase + tid];
            r = id < 0 ? -1 : id - a.id_base;
            hit = r >= 0 && r < a.n;
            rel[tid] = a.st_raw[sbase + tid];
            lvl[tid] = a.st_levels[sbase + tid];
        }
        rows[tid] = hit ? r : -1;
        picked[tid] = 0;
    }
    __syncthreads();
    int C = 0;   // the hits in front of the first slot without one (a broadcast read per step, once per query)
    while (C < F && rows[C] >= 0) ++C;
    const int npick = min(k, C);

    MmrEntry win;
    win.idx = 0;
    win.value = C > 0 ? mmr_first_value(a.lambda, rel[0]) : 0.0;
    for (int t = 0; t < npick; ++t) {
        const int w = win.idx;
        if (tid == 0) { pick_of[t] = w; pick_val[t] = win.value; }   // (read behind the loop only)
        if (t == npick - 1) break;
        // 1. the pick's row -> LDS
        {
            const f32x4 *src = reinterpret_cast<const f32x4 *>(a.corpus + (size_t)rows[w] * a.dim);
            f32x4 *dst = reinterpret_cast<f32x4 *>(prow);
            for (int i = tid; i < (a.dim >> 2); i += MMR_THREADS) dst[i] = src[i];
        }
        __syncthreads();
        // 2. + 3. one chain per unpicked candidate, its pen and value
#pragma unroll 1
        for (int c = quad; c < C; c += MMR_QUADS) {
            // (both quad-uniform: the DPP moves below run with whole quads. picked[c] is written and, inside this phase, read by
            //  the quad that owns c alone; the winner's fold reads it behind the barrier)
            if (c == w) { if (qi == 0) picked[c] = 1; continue; }
            if (picked[c]) continue;
            const float s = mmr_quad_chain(a.corpus, rows[c], a.dim, prow, qi);
            if (qi == 0) {
                const float p = t == 0 ? s : mmr_pen_update(pen[c], s);
                pen[c] = p;
                val[c] = mmr_value(a.lambda, a.one_minus, rel[c], p);
            }
        }
        __syncthreads();
        // 4. the winner, in every lane of every wave
        win = mmr_wave_winner(val, picked, C, lane);
    }
    __syncthreads();

    // outputs: pick order, or the level weight in double and ONE stable descending re-sort (emit_outputs' step)
    const size_t o = (size_t)q * k;
    float raw = -INFINITY;
    double adj = -INFINITY, mv = -INFINITY;
    long long row = -1;
    int lv = 0;
    if (tid < npick) {
        const int c = pick_of[tid];
        raw = rel[c]; row = rows[c]; lv = lvl[c]; mv = pick_val[tid];
        adj = (double)raw * level_weight(lv);
        adjbuf[tid] = adj;
    }
    __syncthreads();
    if (tid >= k) return;
    int pos = tid;
    if (a.reweighted && tid < npick) {
        pos = 0;
        for (int i = 0; i < npick; ++i) {
            const double ai = adjbuf[i];
            pos += (ai > adj || (ai == adj && i < tid)) ? 1 : 0;
        }
    }
    const size_t wpos = o + pos;
    if (a.reweighted) a.out_adj[wpos] = adj;
    a.out_raw[wpos] = raw;
    a.out_ids[wpos] = row >= 0 ? a.id_base + row : -1ll;
    if (a.out_levels) a.out_levels[wpos] = lv;
    if (a.out_mmr) a.out_mmr[wpos] = mv;
}
#pragma clang fp contract(fast)

}  // namespace icd
