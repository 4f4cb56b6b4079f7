// sparse_kernel.hpp - exact sparse-vector search: the inner product of a sparse query with every sparse row
// of the index, over an inverted index, and the best k rows that share a term with the query.
//
// Replaces, on the device, what a caller of Milvus gets from a SPARSE_FLOAT_VECTOR field searched with metric IP (usually filled
// by its BM25 function); the reference has no sparse field and no code of its own for one (services/milvus_service.py:280-285 is
// its only search call).
//
// sparse_accumulate_select_kernel: one work-group of 256 lanes per (query, tile of SP_TILE consecutive rows). The tile's fp32
// accumulators and its touched bitset live in LDS. The query's terms are walked in ascending order, one barrier per term: the
// lanes stride over the term's postings inside the tile (found by a binary search per bound, all terms' bounds searched at once)
// and do acc[row] = acc[row] + q_t * d_t - a plain LDS read-modify-write (rows are distinct within a term), product and sum
// rounded separately (contract off). That order IS the canonical summation order. The touched rows that pass the query's row
// mask - and, in the BAND = true form (section 16), lie inside the query's band - are the candidates; lane l owns rows l, l + 256,
// ... of the tile (conflict-free LDS reads), one bit each. The k-th best
// 64-bit key (make_key: score desc, row asc) is found by a radix select over the keys' bytes, most significant first - an LDS
// histogram per byte, at most eight passes, correct for any number of candidates up to SP_TILE - and the at most k keys at or
// above it are ranked by counting. Output: [tile][query][k] keys best first, 0 = padding.
//
// sparse_merge_kernel: one work-group per query merges the tiles' lists (a bitonic network over 128 carried + up to 896 new keys
// per round), then writes raw order, or the level weight in double and ONE stable descending re-sort (emit_outputs' step).
//
// LDS: 32 KB accumulators + 1 KB bitset + 1 KB histogram + 1 KB survivors + 1.5 KB of the query = 36.6 KB: four work-groups per
// CU. No scratch.
//
// sparse_store_kernel (grouped sparse search): the same accumulate phase (sparse_accumulate_tile), then the
// tile's sums - a NaN where a row is no hit - go to the score block of a grouping, where group_topk.hpp's reduction kernels pick
// the k best groups and their s best rows. grouping_invert_kernel builds the row -> position table that store needs, once.
#pragma once
#include "hybrid_fuse.hpp"

namespace icd {

constexpr int SP_TILE = 8192;       // rows per tile (a power of two, a multiple of 32 * SP_THREADS / 32)
constexpr int SP_THREADS = 256;
constexpr int SP_MAX_TERMS = 64;    // ICD_SPARSE_MAX_QUERY_TERMS
constexpr int SP_PER = SP_TILE / SP_THREADS;   // rows per lane: lane l owns rows l + SP_THREADS * j of the tile
constexpr int SP_CARRY = FIN_MAX_K;            // merge: the best keys so far
constexpr int SP_MERGE_SLOTS = 1024;
static_assert(SP_PER == 32, "a lane's candidate rows are one 32-bit word");
static_assert((SP_TILE & (SP_TILE - 1)) == 0 && SP_THREADS == HY_THREADS, "tile a power of two; the merge sorts with hybrid_bitonic");

struct SparseArgs {
    const long long *post_off;   // [vocab + 1]
    const uint32_t *post_row;    // [nnz] ascending within a term
    const float *post_val;       // [nnz]
    long long vocab;
    const long long *q_off;      // [nq + 1]
    const uint32_t *q_terms;     // ascending within a query
    const float *q_vals;
    RowMasks masks;              // nullable: [query] -> bitset over the index's rows (topk_select.hpp)
    long long mask_words;        // rowmask_tile_words(n)
    int tiles, nq, k;
    u64 *part;                   // [tiles][nq][k]
};

#pragma clang fp contract(off)
// The accumulate phase both kernels run: on return (behind a barrier) acc[l] holds the canonical sum of row tile0 + l and touched
// its hit bit. The arrays are the caller's LDS.
__device__ __forceinline__ void sparse_accumulate_tile(const SparseArgs &a, int q, uint32_t tile0, float *acc, uint32_t *touched, long long *seg,
                                                       uint32_t *qt, float *qv, int tid) {
    // 0. an empty tile; the query's terms (a device caller's offsets are clamped: never more than SP_MAX_TERMS, never backwards)
    for (int i = tid; i < SP_TILE; i += SP_THREADS) acc[i] = 0.0f;
    touched[tid] = 0u;
    const long long qa = a.q_off[q];
    long long qn = a.q_off[q + 1] - qa;
    qn = qn < 0 ? 0 : (qn > SP_MAX_TERMS ? SP_MAX_TERMS : qn);
    const int nt = (int)qn;
    if (tid < nt) { qt[tid] = a.q_terms[qa + tid]; qv[tid] = a.q_vals[qa + tid]; }
    __syncthreads();

    // 1. the tile's segment of every term's postings: lane 2 t finds its begin, lane 2 t + 1 its end (a term outside the
    //    vocabulary has none)
    if (tid < 2 * nt) {
        const uint32_t term = qt[tid >> 1];
        const u64 target = (u64)tile0 + ((tid & 1) ? (u64)SP_TILE : 0ull);
        long long lo = 0, hi = 0;
        if ((long long)term < a.vocab) { lo = a.post_off[term]; hi = a.post_off[term + 1]; }
        while (lo < hi) {   // first posting whose row is at or behind target
            const long long mid = (lo + hi) >> 1;
            if ((u64)a.post_row[mid] < target) lo = mid + 1; else hi = mid;
        }
        seg[tid] = lo;
    }
    __syncthreads();

    // 2. the walk: terms in ascending order, one barrier per term
    for (int t = 0; t < nt; ++t) {
        const long long lo = seg[2 * t], hi = seg[2 * t + 1];
        const float w = qv[t];
        for (long long i = lo + tid; i < hi; i += SP_THREADS) {
            const uint32_t l = a.post_row[i] - tile0;
            if (l < (uint32_t)SP_TILE) {   // (always, for postings icd_sparse_pack built)
                const float prod = w * a.post_val[i];
                acc[l] = acc[l] + prod;
                atomicOr(&touched[l >> 5], 1u << (l & 31));
            }
        }
        __syncthreads();
    }
}

// The bands of a banded launch's queries: an argument of the BAND = true form only - the BAND = false form
// takes SparseArgs as it always has.
template <bool BAND>
struct SparseBands {};
template <>
struct SparseBands<true> {
    const BandQ *q;   // [nq] in device memory (topk_select.hpp)
};

// BAND: only touched rows inside the query's band (lo < score <= hi, ranked strictly behind the cursor) are candidates: the band is
// applied where `mine` is built, so the radix select, the counting rank and the output see band candidates only.
template <bool BAND>
__global__ __launch_bounds__(SP_THREADS) void sparse_accumulate_select_kernel(const SparseArgs a, const SparseBands<BAND> bands) {
    __shared__ float acc[SP_TILE];
    __shared__ uint32_t touched[SP_TILE / 32];
    __shared__ uint32_t hist[256];
    __shared__ u64 skey[FIN_MAX_K];
    __shared__ long long seg[2 * SP_MAX_TERMS];
    __shared__ uint32_t qt[SP_MAX_TERMS];
    __shared__ float qv[SP_MAX_TERMS];
    __shared__ int sh_cnt, sh_kept, sh_sel, sh_left, sh_bucket;
    const int tid = threadIdx.x;
    const int q = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x - (unsigned)q * (unsigned)a.tiles);
    const uint32_t tile0 = (uint32_t)tile * (uint32_t)SP_TILE;
    if (tid == 0) { sh_cnt = 0; sh_kept = 0; }
    sparse_accumulate_tile(a, q, tile0, acc, touched, seg, qt, qv, tid);

    // 3. candidates = touched rows inside the query's mask; bit j of `mine` = row tid + SP_THREADS * j of the tile
    const uint32_t *mask = a.masks ? a.masks[q] : nullptr;
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < SP_PER; ++j) {
        const int wi = (tid >> 5) + (SP_THREADS / 32) * j;
        uint32_t word = touched[wi];
        if (mask && word) {
            const long long mw = (long long)(tile0 >> 5) + wi;
            word &= mw < a.mask_words ? mask[mw] : 0u;
        }
        mine |= ((word >> (tid & 31)) & 1u) << j;
    }
    if constexpr (BAND) {   // the query's band, uniform across the work-group: loaded once; lo < NaN is false, a NaN sum is no hit
        const BandQ b = bands.q[q];
        uint32_t in = 0;
        for (uint32_t m = mine; m; m &= m - 1) {
            const int j = __ffs((int)m) - 1;
            const int l = tid + SP_THREADS * j;
            const float v = acc[l];
            in |= (uint32_t)((b.lo < v) & band_under(v, tile0 + (uint32_t)l, b.hi, b.below)) << j;
        }
        mine = in;
    }
    if (mine) atomicAdd(&sh_cnt, __popc(mine));
    __syncthreads();
    const int cnt = sh_cnt, k = a.k;

    // 4. more candidates than k: the k-th best key, byte by byte from the top. `prefix` holds the bytes found so far, `left` how
    //    many of the keys that share them are wanted. A pass ends the search early when its bucket is wanted whole.
    u64 thr = 0ull;
    if (cnt > k) {
        u64 prefix = 0ull;
        int left = k;
        for (int shift = 56; shift >= 0; shift -= 8) {
            hist[tid] = 0u;
            __syncthreads();
            for (uint32_t m = mine; m; m &= m - 1) {
                const int l = tid + SP_THREADS * (__ffs((int)m) - 1);
                const u64 key = make_key(acc[l], tile0 + (uint32_t)l);
                if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(uint32_t)(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            int above = 0;
            for (int d = tid + 1; d < 256; ++d) above += (int)hist[d];
            const int h = (int)hist[tid];
            if (above < left && above + h >= left) { sh_sel = tid; sh_left = left - above; sh_bucket = h; }
            __syncthreads();
            prefix |= (u64)(uint32_t)sh_sel << shift;
            left = sh_left;
            if (sh_bucket == left) break;   // (uniform; at shift 0 a bucket holds one key)
        }
        thr = prefix;
    }

    // 5. the keys at or above it (all of them when there are at most k), ranked by counting
    for (uint32_t m = mine; m; m &= m - 1) {
        const int l = tid + SP_THREADS * (__ffs((int)m) - 1);
        const u64 key = make_key(acc[l], tile0 + (uint32_t)l);
        if (key >= thr) {
            const int slot = atomicAdd(&sh_kept, 1);
            if (slot < FIN_MAX_K) skey[slot] = key;
        }
    }
    __syncthreads();
    const int nres = min(min(sh_kept, k), FIN_MAX_K);
    u64 *out = a.part + ((size_t)tile * a.nq + q) * k;
    if (tid < nres) {
        const u64 key = skey[tid];
        int rank = 0;
        for (int j = 0; j < nres; ++j) rank += skey[j] > key ? 1 : 0;
        out[rank] = key;
    } else if (tid < k) {
        out[tid] = 0ull;
    }
}

// ---- grouped sparse search: the tile's sums go to the grouping's score block, not to a top-k ----------------
struct SparseStoreArgs {
    SparseArgs sp;        // part / k unused; nq = the queries of this pass; q_off, masks indexed by q_base + query
    int q_base;           // first query of the pass
    int n;                // rows of the index
    const int *pos_of;    // [n] position of every row in the grouping's (group, row) order
    float *S;             // [queries of the pass][ldS] the grouping's score block
    long long ldS;
};

// position -> row becomes row -> position: one launch when a grouping first meets a sparse index
__global__ void grouping_invert_kernel(const int *order, int *pos_of, int n) {
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p < n) pos_of[order[p]] = p;
}

// One work-group per (query of the pass, tile): the accumulate phase, then S[query][pos_of[row]] for EVERY row of the tile below
// n - the sum of a hit inside the query's mask, a quiet NaN otherwise (group_topk.hpp reads NaN as "no hit": key 0). The block is
// reused between passes, so nothing of it is assumed. LDS: 32 KB + 1 KB + 1.5 KB of the query; no scratch.
__global__ __launch_bounds__(SP_THREADS) void sparse_store_kernel(const SparseStoreArgs a) {
    __shared__ float acc[SP_TILE];
    __shared__ uint32_t touched[SP_TILE / 32];
    __shared__ long long seg[2 * SP_MAX_TERMS];
    __shared__ uint32_t qt[SP_MAX_TERMS];
    __shared__ float qv[SP_MAX_TERMS];
    const int tid = threadIdx.x;
    const int ql = (int)(blockIdx.x / (unsigned)a.sp.tiles), tile = (int)(blockIdx.x - (unsigned)ql * (unsigned)a.sp.tiles);
    const int q = a.q_base + ql;
    const uint32_t tile0 = (uint32_t)tile * (uint32_t)SP_TILE;
    sparse_accumulate_tile(a.sp, q, tile0, acc, touched, seg, qt, qv, tid);

    const uint32_t *mask = a.sp.masks ? a.sp.masks[q] : nullptr;
    float *srow = a.S + (size_t)ql * a.ldS;
#pragma unroll 4
    for (int j = 0; j < SP_PER; ++j) {
        const int l = tid + SP_THREADS * j;   // consecutive lanes, consecutive rows: pos_of is read coalesced
        const long long row = (long long)tile0 + l;
        if (row >= a.n) break;
        const int wi = l >> 5;
        uint32_t word = touched[wi];
        if (mask && word) {
            const long long mw = (long long)(tile0 >> 5) + wi;
            word &= mw < a.sp.mask_words ? mask[mw] : 0u;
        }
        srow[a.pos_of[row]] = ((word >> (l & 31)) & 1u) ? acc[l] : __int_as_float(0x7FC00000);
    }
}

struct SparseMergeArgs {
    const u64 *part;        // [tiles][nq][k]
    int tiles, nq, k, reweighted;
    long long id_base;
    const int *levels;      // nullable
    double *out_adj;        // reweighted only
    float *out_raw;
    long long *out_ids;
    int *out_levels;        // nullable
};

__global__ __launch_bounds__(SP_THREADS) void sparse_merge_kernel(const SparseMergeArgs a) {
    __shared__ u64 buf[SP_MERGE_SLOTS];   // ~key: ascending sort = best first; ~0 = nothing
    __shared__ double adjbuf[FIN_MAX_K];
    const int tid = threadIdx.x, q = blockIdx.x, k = a.k;
    const long long total = (long long)a.tiles * k;
    for (long long base = 0; base < total; base += SP_MERGE_SLOTS - SP_CARRY) {
        const int chunk = (int)min((long long)(SP_MERGE_SLOTS - SP_CARRY), total - base);
        int slots = 2 * SP_CARRY;
        while (slots < SP_CARRY + chunk) slots <<= 1;
        for (int i = tid; i < slots; i += SP_THREADS) {
            if (i < SP_CARRY) {
                if (base == 0) buf[i] = ~0ull;   // (later rounds: the best so far stay where the sort left them)
            } else {
                u64 v = ~0ull;
                if (i - SP_CARRY < chunk) {
                    const long long c = base + (i - SP_CARRY);
                    const long long g = c / k;
                    v = ~a.part[((size_t)g * a.nq + q) * k + (size_t)(c - g * k)];
                }
                buf[i] = v;
            }
        }
        hybrid_bitonic<false>(buf, buf, slots, tid);
    }
    const size_t o = (size_t)q * k;
    const bool hit = tid < k && buf[tid] != ~0ull;
    float raw = -INFINITY;
    double adj = -INFINITY;
    int row = -1, lvl = 0;
    if (hit) {
        const u64 key = ~buf[tid];
        raw = key_score(key);
        row = (int)key_row(key);
        lvl = a.levels ? a.levels[row] : 1;
        adj = (double)raw * level_weight(lvl);
        adjbuf[tid] = adj;
    }
    __syncthreads();
    if (tid >= k) return;
    int pos = tid;
    if (a.reweighted && hit) {
        pos = 0;
        for (int i = 0; i < k && buf[i] != ~0ull; ++i) {
            const double ai = adjbuf[i];
            pos += (ai > adj || (ai == adj && i < tid)) ? 1 : 0;
        }
    }
    const size_t w = o + pos;
    if (a.reweighted) a.out_adj[w] = adj;
    a.out_raw[w] = raw;
    a.out_ids[w] = row >= 0 ? a.id_base + row : -1ll;
    if (a.out_levels) a.out_levels[w] = lvl;
}
#pragma clang fp contract(fast)

}  // namespace icd
