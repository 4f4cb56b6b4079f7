// filter_mask_kernel.hpp - filter expressions on the device: the row masks of a batch of filter programs
// (filter_program.hpp: postfix programs over int32 columns and the sparse index's postings), one mask per query, in one launch.
//
// Replaces, on the device, the bitset a Milvus query node builds from a boolean expression before the scan; the reference has no
// filter and no code of its own for one (services/milvus_service.py:280-285 is its only search call).
//
// filter_mask_kernel: text_match_mask_kernel's geometry - one work-group of 256 lanes per (query, tile of SP_TILE consecutive rows),
// lane l owns mask word l of the tile (rows 32 l .. 32 l + 31). The work-group walks the query's program once; every program word
// is the same for all lanes (read through readfirstlane: the walk's branches are scalar).
//   RANGE, SET   wave w reads rows 2048 w + 64 s .. + 63 of the column in step s (one coalesced 256-byte read), tests them and
//                takes the ballot: its low half is mask word 64 w + 2 s, its high half word 64 w + 2 s + 1 - both owned by lanes of
//                the SAME wave, so the two halves go to their owners with one select and nothing crosses waves. A SET's ids are
//                staged in LDS behind INT32_MAX padding and searched with six halving steps.
//   TEXT         section 17's byte counters in LDS, through text_match_kernel.hpp's own device functions (tm_segment_search,
//                tm_counter_walk, tm_threshold_word, unguarded: the checker vouches for terms and m): cleared here, filled and
//                tested there. The leaves of a program run one after another on the same counters, behind a barrier.
//   AND, OR, NOT on 32-bit words in registers: the stack is eight registers with its TOP at position 0 - a push moves every entry
//                one position down, a pop one up, all at compile-time positions, so nothing is indexed at run time (no scratch).
// NOT sets the bits of rows at or behind n as well; they are cleared ONCE, on the final word, by text_match_kernel.hpp's
// tm_store_word, which also ANDs the base mask's word, stores and counts the rows as it does for a keyword mask. Every word below
// rowmask_tile_words(n) is written for every query.
//
// Programs come from the host and were checked there (filter_check_programs): the kernel trusts their structure.
//
// LDS: 8 KB counters + 1 KB segment bounds + 256 B ids / terms = 9.3 KB. No scratch.
#pragma once
#include "filter_program.hpp"
#include "text_match_kernel.hpp"

namespace icd {

static_assert(FP_MAX_SET <= SP_MAX_TERMS && FP_MAX_TERMS == SP_MAX_TERMS, "a SET's ids and a TEXT's terms share one LDS array");
static_assert(SP_TILE == 32 * SP_THREADS && SP_THREADS == 256, "wave w covers rows 2048 w .. 2048 w + 2047 of the tile in 32 steps of 64");

struct FilterMaskArgs {
    const int *cols;             // [ncols][n]
    const long long *prog_off;   // [nq + 1]
    const uint32_t *prog;
    const long long *post_off;   // the sparse index's postings (nullptr: no program holds a TEXT leaf)
    const uint32_t *post_row;
    const uint32_t *const *base; // nullable: [query] -> base bitset (nullable entries: unfiltered)
    uint32_t *bits;              // [nq][stride] the produced bitsets
    long long stride;            // words between two queries' bitsets
    int *count;                  // [nq] rows of every produced mask (zeroed by the caller)
    long long n;                 // rows of the index (below 2^31)
    long long mask_words;        // rowmask_tile_words(n)
    int tiles;
};

// One scalar leaf: the tile's rows of `col` under `pred`, as lane `lane`'s mask word. Rows at or behind n are not read (and not set).
template <typename Pred>
__device__ __forceinline__ uint32_t filter_column_leaf(const int *__restrict__ col, long long n, uint32_t tile0, int wave, int lane, Pred pred) {
    uint32_t word = 0u;
    const long long row0 = (long long)tile0 + wave * (SP_TILE / 4) + lane;
#pragma unroll 8
    for (int s = 0; s < SP_TILE / 4 / 64; ++s) {
        const long long r = row0 + 64 * s;
        bool hit = false;
        if (r < n) hit = pred(col[r]);
        const u64 b = __ballot(hit);
        if ((lane >> 1) == s) word = (lane & 1) ? (uint32_t)(b >> 32) : (uint32_t)b;
    }
    return word;
}

__global__ __launch_bounds__(SP_THREADS) void filter_mask_kernel(const FilterMaskArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t cnt[TM_COUNT_WORDS];
    __shared__ long long seg[2 * SP_MAX_TERMS];
    __shared__ uint32_t ids[SP_MAX_TERMS];   // a SET's ids (as int32 bits, padded) or a TEXT's terms
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int q = (int)(blockIdx.x / (unsigned)a.tiles), tile = (int)(blockIdx.x - (unsigned)q * (unsigned)a.tiles);
    const uint32_t tile0 = (uint32_t)tile * (uint32_t)SP_TILE;
    const long long pa = a.prog_off[q];
    const uint32_t *__restrict__ p = a.prog + pa;
    const int len = __builtin_amdgcn_readfirstlane((int)(a.prog_off[q + 1] - pa));

    uint32_t st[FP_MAX_STACK];   // st[0] is the top
#pragma unroll
    for (int i = 0; i < FP_MAX_STACK; ++i) st[i] = 0u;

    int pc = 0;
    while (pc < len) {
        const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)p[pc]);
        const uint32_t op = w & 0xFFu;
        const int count = (int)((w >> 8) & 0xFFu);
        if (op == FOP_AND || op == FOP_OR) {
            st[0] = op == FOP_AND ? (st[0] & st[1]) : (st[0] | st[1]);
#pragma unroll
            for (int i = 1; i < FP_MAX_STACK - 1; ++i) st[i] = st[i + 1];
            st[FP_MAX_STACK - 1] = 0u;
            pc += 1;
            continue;
        }
        if (op == FOP_NOT) {
            st[0] = ~st[0];
            pc += 1;
            continue;
        }
        uint32_t word = 0u;
        if (op == FOP_RANGE) {
            const int c = __builtin_amdgcn_readfirstlane((int)p[pc + 1]);
            const int lo = __builtin_amdgcn_readfirstlane((int)p[pc + 2]), hi = __builtin_amdgcn_readfirstlane((int)p[pc + 3]);
            word = filter_column_leaf(a.cols + (long long)c * a.n, a.n, tile0, wave, lane, [lo, hi](int v) { return v >= lo && v < hi; });
            pc += 4;
        } else if (op == FOP_SET) {
            const int c = __builtin_amdgcn_readfirstlane((int)p[pc + 1]);
            __syncthreads();   // (whoever still reads ids or the counters of the leaf before)
            if (tid < SP_MAX_TERMS) ids[tid] = tid < count ? p[pc + 2 + tid] : 0x7FFFFFFFu;
            __syncthreads();
            const int *sid = reinterpret_cast<const int *>(ids);
            word = filter_column_leaf(a.cols + (long long)c * a.n, a.n, tile0, wave, lane, [sid, count](int v) {
                int pos = 0;   // the first position whose id is not below v (ids ascending, INT32_MAX behind count)
#pragma unroll
                for (int h = SP_MAX_TERMS / 2; h >= 1; h >>= 1)
                    if (sid[pos + h - 1] < v) pos += h;
                return pos < count && sid[pos] == v;
            });
            pc += 2 + count;
        } else {   // FOP_TEXT: section 17's walk, on counters this leaf clears
            const int m = (int)(w >> 16);
            __syncthreads();
            for (int i = tid; i < TM_COUNT_WORDS; i += SP_THREADS) cnt[i] = 0u;
            if (tid < count) ids[tid] = p[pc + 1 + tid];
            __syncthreads();
            tm_segment_search<false>(a, ids, count, tile0, tid, seg);
            __syncthreads();
            tm_counter_walk(a, seg, count, tile0, wave, lane, cnt);
            __syncthreads();
            word = tm_threshold_word<false>(cnt, m, count, tid);
            pc += 1 + count;
        }
        // push
#pragma unroll
        for (int i = FP_MAX_STACK - 1; i >= 1; --i) st[i] = st[i - 1];
        st[0] = word;
    }

    // the final word: rows at or behind n cleared once (a NOT set them), the base mask, the store, the count
    tm_store_word(a, st[0], q, tile0, tid, lane);
}

}  // namespace icd
