// hybrid_fuse.hpp — hybrid search, step 2: fuse the R exact sub-lists of a query into ONE hit list.
//
// Replaces, on the device, what a caller of Milvus's hybrid_search gets from the server's reranker (RRFRanker / WeightedRanker;
// the reference sends one search per phrasing and has no code of its own for the merge, services/milvus_service.py:280-285).
//
// One work-group of 256 lanes per query. The query's up to R * 128 = 1024 entries are read from the fusion's staging (list r cut
// at L_r), keyed by (local row, r, j) and sorted in LDS by a bitonic network; every run of equal rows is then summed by its
// first entry, in ascending r, in double, one rounding per operation; the run heads are sorted a second time
// by (fused desc, row asc) - a 64-bit double plus a 31-bit row, two words per slot - and the first min(k, heads) of them go
// through the double-score form of emit_outputs (finalize.hpp): level weight, one stable descending re-sort, row_map.
//
// The double arithmetic of rules 2, 3 and 6 sits between `#pragma clang fp contract(off)` and `contract(fast)`, as in
// hier_kernel.hpp and stats_kernel.hpp: the .hip is built with the compiler's default contraction, and hipcc's __dadd_rn /
// __dmul_rn are plain `+` / `*` (they would fuse into v_fmac_f64 like any other), so the pragma is what keeps product and sum apart.
//
// LDS: two u64 arrays of 1024 slots + 128 doubles = 17 KB per work-group; no scratch.
#pragma once
#include "finalize.hpp"

namespace icd {

constexpr int HY_MAX_R = 8;
constexpr int HY_MAX_L = 128;
constexpr int HY_SLOTS = HY_MAX_R * HY_MAX_L;   // 1024
constexpr int HY_THREADS = 256;
enum { HY_RANK_RRF = 0, HY_RANK_WEIGHTED = 1 };
enum { HY_NORM_NONE = 0, HY_NORM_COSINE = 1, HY_NORM_ATAN = 2 };

struct HybridArgs {
    const float *st_scores;       // [nq * R][lmax] the sub-lists, raw order (staging of the fusion)
    const long long *st_ids;      // global ids, -1 = padding
    int R, lmax, k, slots;        // slots: the power of two >= R * lmax the sort runs over (>= 2)
    int limits[HY_MAX_R];
    double weights[HY_MAX_R];
    double rrf_c;
    int ranker, norm, reweighted;
    long long n, id_base;
    const long long *row_map;     // nullable (a view): strictly increasing global id of every local row
    const int *levels;            // nullable
    double *out_adj;              // [nq][k], reweighted only
    double *out_fused;
    long long *out_ids;
    int *out_levels;              // nullable
    uint32_t *out_reqbits;        // nullable
};

// order-preserving image of a double: larger value = larger word
__device__ __forceinline__ u64 order_f64(double v) {
    const u64 u = (u64)__double_as_longlong(v);
    return u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull);
}
__device__ __forceinline__ double unorder_f64(u64 o) {
    const u64 u = o ^ ((o >> 63) ? 0x8000000000000000ull : ~0ull);
    return __longlong_as_double((long long)u);
}

// local row of a global id (-1: none). A view's ids are found in its strictly increasing row map.
__device__ __forceinline__ int hybrid_local_row(const HybridArgs &a, long long id) {
    if (id < 0) return -1;
    if (!a.row_map) {
        const long long r = id - a.id_base;
        return (r >= 0 && r < a.n) ? (int)r : -1;
    }
    long long lo = 0, hi = a.n;   // first local row with row_map[row] >= id
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (a.row_map[mid] < id) lo = mid + 1; else hi = mid; }
    return (lo < a.n && a.row_map[lo] == id) ? (int)lo : -1;
}

// ---- contraction off from here to the end of the kernel: every `*` and `+` below rounds once -------------------------------
#pragma clang fp contract(off)
// one term of a fused score (rules 2 and 3)
__device__ __forceinline__ double hybrid_term(const HybridArgs &a, int r, int j, float score) {
    if (a.ranker == HY_RANK_RRF) return 1.0 / ((a.rrf_c + (double)j) + 1.0);
    double s = (double)score;
    if (a.norm == HY_NORM_COSINE) s = (1.0 + s) * 0.5;
    else if (a.norm == HY_NORM_ATAN) s = 0.5 + atan(s) / 3.141592653589793;
    return a.weights[r] * s;
}

// ascending bitonic sort of `slots` (a power of two, <= HY_SLOTS) entries; PAIR: (ka, kb) lexicographic, else ka alone
template <bool PAIR>
__device__ __forceinline__ void hybrid_bitonic(u64 *ka, u64 *kb, int slots, int tid) {
    for (int size = 2; size <= slots; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = tid; t < (slots >> 1); t += HY_THREADS) {
                const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));   // the lower slot of pair t
                const int p = i | stride;
                const bool up = (i & size) == 0;
                const u64 ai = ka[i], ap = ka[p];
                bool gt;
                u64 bi = 0, bp = 0;
                if (PAIR) { bi = kb[i]; bp = kb[p]; gt = ai > ap || (ai == ap && bi > bp); }
                else gt = ai > ap;
                if (gt == up) {
                    ka[i] = ap; ka[p] = ai;
                    if (PAIR) { kb[i] = bp; kb[p] = bi; }
                }
            }
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(HY_THREADS) void hybrid_fuse_kernel(const HybridArgs a) {
    __shared__ u64 ka[HY_SLOTS];
    __shared__ u64 kb[HY_SLOTS];
    __shared__ double adjbuf[FIN_MAX_K];
    __shared__ int nheads;
    const int tid = threadIdx.x;
    const int q = blockIdx.x;
    const int slots = a.slots;
    const size_t base = (size_t)q * a.R * a.lmax;
    if (tid == 0) nheads = 0;

    // 1. gather: slot i = (r, j) of the staging; key = row << 10 | r << 7 | j, ~0 where there is no hit
    for (int i = tid; i < slots; i += HY_THREADS) {
        const int r = i / a.lmax, j = i - r * a.lmax;
        u64 key = ~0ull;
        if (r < a.R && j < a.limits[r]) {
            const int row = hybrid_local_row(a, a.st_ids[base + (size_t)r * a.lmax + j]);
            if (row >= 0) key = ((u64)(uint32_t)row << 10) | ((u64)r << 7) | (u64)j;
        }
        ka[i] = key;
    }
    // 2. order by (row, r)
    hybrid_bitonic<false>(ka, kb, slots, tid);

    // 3. the first entry of every run of equal rows sums the run (ascending r: the sort's order), left to right from 0.0
    constexpr int PER = HY_SLOTS / HY_THREADS;
    u64 fa[PER], fb[PER];
    int mine = 0;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const int p = tid + e * HY_THREADS;
        fa[e] = ~0ull; fb[e] = ~0ull;
        if (p >= slots) continue;
        const u64 key = ka[p];
        if (key == ~0ull) continue;
        const uint32_t row = (uint32_t)(key >> 10);
        if (p > 0 && (uint32_t)(ka[p - 1] >> 10) == row) continue;
        double fused = 0.0;
        uint32_t bits = 0;
        for (int t = p; t < slots; ++t) {
            const u64 kt = ka[t];
            if (kt == ~0ull || (uint32_t)(kt >> 10) != row) break;
            const int r = (int)(kt >> 7) & 7, j = (int)kt & 127;
            fused = fused + hybrid_term(a, r, j, a.st_scores[base + (size_t)r * a.lmax + j]);
            bits |= 1u << r;
        }
        fa[e] = ~order_f64(fused);                    // ascending sort = fused descending
        fb[e] = ((u64)row << 8) | (u64)bits;          // ... then row ascending (rows are distinct among the heads)
        ++mine;
    }
    if (mine) atomicAdd(&nheads, mine);
    __syncthreads();   // (every read of the (row, r) order is done)
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const int p = tid + e * HY_THREADS;
        if (p < slots) { ka[p] = fa[e]; kb[p] = fb[e]; }
    }
    // 4. order the heads by (fused desc, row asc); everything else sorts behind them
    hybrid_bitonic<true>(ka, kb, slots, tid);

    // 5. outputs: raw (fused) order, or the level weight in double and ONE stable descending re-sort (emit_outputs' step)
    const int k = a.k;
    const int nres = min(min(k, nheads), slots);
    const size_t o = (size_t)q * k;
    double fused = -INFINITY, adj = -INFINITY;
    int row = -1, lvl = 0;
    uint32_t bits = 0;
    if (tid < nres) {
        fused = unorder_f64(~ka[tid]);
        row = (int)(kb[tid] >> 8);
        bits = (uint32_t)kb[tid] & 0xFFu;
        lvl = a.levels ? a.levels[row] : 1;
        adj = fused * level_weight(lvl);
        adjbuf[tid] = adj;
    }
    __syncthreads();
    if (tid >= k) return;
    int pos = tid;
    if (a.reweighted && tid < nres) {
        pos = 0;
        for (int i = 0; i < nres; ++i) {
            const double ai = adjbuf[i];
            pos += (ai > adj || (ai == adj && i < tid)) ? 1 : 0;
        }
    }
    const size_t w = o + pos;
    if (a.reweighted) a.out_adj[w] = adj;
    a.out_fused[w] = fused;
    a.out_ids[w] = row >= 0 ? (a.row_map ? a.row_map[row] : a.id_base + row) : -1ll;
    if (a.out_levels) a.out_levels[w] = lvl;
    if (a.out_reqbits) a.out_reqbits[w] = bits;
}
// ---- grouped fuse (rules H1 - H4) ----------------------------------------------------------------------------
struct HybridGroupedArgs {
    HybridArgs h;             // k = the number of GROUPS; limits[r] = L_r in runs of equal group ids; lmax <= HY_MAX_L slots per list
    const int *dense_of;      // [n] dense group (0 .. G-1) of every local row
    const int *group_of;      // [n] the caller's group id of every local row
    int s;                    // members per group; k * s <= FIN_MAX_K
    int *out_groups;          // [nq][k * s], nullable
};

// One work-group per query. List r is cut in front of its (L_r + 1)-th run of equal group ids (a slot without a row of the index is
// a run of its own and no hit), then hybrid_fuse_kernel's (row, r) network and run sums give the fused heads, ordered by
// (fused desc, row asc): a head's place p in that order stands for its key from there on. The heads are ordered again by
// (dense group, p) - each group's first head is its best - the group heads by p, and the first k groups' first s members are
// written group-rank-major, hits contiguous; the reweighted form ranks the winners as hybrid_fuse_kernel does.
// LDS: four u64 arrays of 1024 slots, 1024 ints, the winners and their adjusted scores = 38.5 KB, static; no scratch.
__global__ __launch_bounds__(HY_THREADS) void hybrid_fuse_grouped_kernel(const HybridGroupedArgs g) {
    __shared__ u64 ka[HY_SLOTS];
    __shared__ u64 kb[HY_SLOTS];
    __shared__ u64 kc[HY_SLOTS];
    __shared__ u64 kd[HY_SLOTS];
    __shared__ int sg[HY_SLOTS];          // dense group of every staged slot, -1 = no row
    __shared__ double adjbuf[FIN_MAX_K];
    __shared__ int win[FIN_MAX_K], gcnt[FIN_MAX_K];
    __shared__ int nheads, ngroups;
    const HybridArgs &a = g.h;
    const int tid = threadIdx.x;
    const int q = blockIdx.x;
    const int slots = a.slots;
    const size_t base = (size_t)q * a.R * a.lmax;
    if (tid == 0) { nheads = 0; ngroups = 0; }

    // 0. the staged slots' rows (kept in kc until the gather) and groups
    for (int i = tid; i < slots; i += HY_THREADS) {
        const int r = i / a.lmax, j = i - r * a.lmax;
        int row = -1;
        if (r < a.R) row = hybrid_local_row(a, a.st_ids[base + (size_t)r * a.lmax + j]);
        kc[i] = (u64)(uint32_t)row;
        sg[i] = row >= 0 ? g.dense_of[row] : -1;
    }
    __syncthreads();
    // 1. gather with the cut by runs: slot (r, j) lies in run number 1 + #{1 <= i <= j : group(i) != group(i - 1) or no row at i}
    for (int i = tid; i < slots; i += HY_THREADS) {
        const int r = i / a.lmax, j = i - r * a.lmax;
        u64 key = ~0ull;
        const int row = (int)(uint32_t)kc[i];
        if (r < a.R && row >= 0) {
            const int *lg = sg + r * a.lmax;
            int runs = 1;
            for (int t = 1; t <= j; ++t) runs += (lg[t] != lg[t - 1] || lg[t] < 0) ? 1 : 0;
            if (runs <= a.limits[r]) key = ((u64)(uint32_t)row << 10) | ((u64)r << 7) | (u64)j;
        }
        ka[i] = key;
    }
    // 2. order by (row, r)
    hybrid_bitonic<false>(ka, kb, slots, tid);

    // 3. the first entry of every run of equal rows sums the run (hybrid_fuse_kernel's step 3)
    constexpr int PER = HY_SLOTS / HY_THREADS;
    u64 fa[PER], fb[PER];
    int mine = 0;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const int p = tid + e * HY_THREADS;
        fa[e] = ~0ull; fb[e] = ~0ull;
        if (p >= slots) continue;
        const u64 key = ka[p];
        if (key == ~0ull) continue;
        const uint32_t row = (uint32_t)(key >> 10);
        if (p > 0 && (uint32_t)(ka[p - 1] >> 10) == row) continue;
        double fused = 0.0;
        uint32_t bits = 0;
        for (int t = p; t < slots; ++t) {
            const u64 kt = ka[t];
            if (kt == ~0ull || (uint32_t)(kt >> 10) != row) break;
            const int r = (int)(kt >> 7) & 7, j = (int)kt & 127;
            fused = fused + hybrid_term(a, r, j, a.st_scores[base + (size_t)r * a.lmax + j]);
            bits |= 1u << r;
        }
        fa[e] = ~order_f64(fused);
        fb[e] = ((u64)row << 8) | (u64)bits;
        ++mine;
    }
    if (mine) atomicAdd(&nheads, mine);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const int p = tid + e * HY_THREADS;
        if (p < slots) { ka[p] = fa[e]; kb[p] = fb[e]; }
    }
    // 4. the heads by (fused desc, row asc): head p of that order keeps its data at ka[p] / kb[p] to the end
    hybrid_bitonic<true>(ka, kb, slots, tid);
    const int nh = min(nheads, slots);

    // 5. the heads by (dense group, p)
    for (int i = tid; i < slots; i += HY_THREADS)
        kc[i] = i < nh ? (((u64)(uint32_t)g.dense_of[(int)(kb[i] >> 8)] << 10) | (u64)i) : ~0ull;
    hybrid_bitonic<false>(kc, kc, slots, tid);
    // 6. every group's first head is its best: the group heads by p, with where the group starts
    int heads_here = 0;
    for (int t = tid; t < slots; t += HY_THREADS) {
        u64 key = ~0ull;
        if (t < nh && (t == 0 || (kc[t - 1] >> 10) != (kc[t] >> 10))) { key = ((kc[t] & 1023ull) << 10) | (u64)t; ++heads_here; }
        kd[t] = key;
    }
    if (heads_here) atomicAdd(&ngroups, heads_here);
    hybrid_bitonic<false>(kd, kd, slots, tid);

    // 7. the first k groups' first s members, group-rank-major, hits contiguous
    const int kg = min(a.k, ngroups), ks = a.k * g.s;
    if (tid < kg) {
        const int t0 = (int)(kd[tid] & 1023ull);
        const u64 grp = kc[t0] >> 10;
        int c = 1;
        while (c < g.s && t0 + c < nh && (kc[t0 + c] >> 10) == grp) ++c;
        gcnt[tid] = c;
    }
    __syncthreads();
    int nres = 0;
    for (int i = 0; i < kg; ++i) nres += gcnt[i];
    if (tid < kg) {
        int off = 0;
        for (int i = 0; i < tid; ++i) off += gcnt[i];
        const int t0 = (int)(kd[tid] & 1023ull);
        for (int m = 0; m < gcnt[tid]; ++m) win[off + m] = (int)(kc[t0 + m] & 1023ull);
    }
    __syncthreads();

    // 8. outputs: raw order, or the level weight in double and ONE stable descending re-sort (hybrid_fuse_kernel's step 5)
    const size_t o = (size_t)q * ks;
    double fused = -INFINITY, adj = -INFINITY;
    int row = -1, lvl = 0;
    uint32_t bits = 0;
    if (tid < nres) {
        const int p = win[tid];
        fused = unorder_f64(~ka[p]);
        row = (int)(kb[p] >> 8);
        bits = (uint32_t)kb[p] & 0xFFu;
        lvl = a.levels ? a.levels[row] : 1;
        adj = fused * level_weight(lvl);
        adjbuf[tid] = adj;
    }
    __syncthreads();
    if (tid >= ks) return;
    int pos = tid;
    if (a.reweighted && tid < nres) {
        pos = 0;
        for (int i = 0; i < nres; ++i) {
            const double ai = adjbuf[i];
            pos += (ai > adj || (ai == adj && i < tid)) ? 1 : 0;
        }
    }
    const size_t w = o + pos;
    if (a.reweighted) a.out_adj[w] = adj;
    a.out_fused[w] = fused;
    a.out_ids[w] = row >= 0 ? (a.row_map ? a.row_map[row] : a.id_base + row) : -1ll;
    if (a.out_levels) a.out_levels[w] = lvl;
    if (a.out_reqbits) a.out_reqbits[w] = bits;
    if (g.out_groups) g.out_groups[w] = row >= 0 ? g.group_of[row] : -1;
}
#pragma clang fp contract(fast)

}  // namespace icd
