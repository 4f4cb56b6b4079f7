// wide_select_kernel.hpp - wide search: the exact ranks first .. first + k - 1 of a query's ranking for
// first + k up to 16 384, in one call. Replaces what a caller does today for more than 128 hits: paging the banded search with a
// cursor through the host (ceil(k / 128) full sweeps), or all n scores per query pulled to the host and sorted there.
//
// wide_scores_kernel      the geometry of rankof_sweep_kernel (rankof_kernel.hpp; exact_topk_kernel<.., BAND, MASK>'s): RK_QUERIES
//                         queries x a chunk of RK_TILE-row tiles per work-group, the corpus rows of a stage through LDS, the queries
//                         straight into the MFMA's operand registers, v_mfma_f32_32x32x2_f32 with k mapped to d ascending - the
//                         canonical bits. Behind a tile's MFMAs lane (c, h) holds 64 scores of query c in runs of four consecutive
//                         rows: each run leaves as ONE 16-byte store of order_f32(score) into the query's run of the score block S,
//                         0 for a row that does not rank (outside the mask, past n, NaN, outside the band - order_f32 is 0 only for
//                         a NaN pattern, which never ranks). Every word of S[query][0, n padded) is written, none twice.
// wide_threshold_kernel   one work-group per query: a radix select over the query's run, 11 + 11 + 10 bits, most significant first,
//                         an LDS histogram of integer adds per pass and a suffix scan by one wave. Leaves T (the ordered score of
//                         rank first + k - 1, or of the last ranking row), above, need and selected (WideRec).
// wide_collect_kernel     one work-group per query walks the run in ascending row order, 1 024 rows a step: every row above T and
//                         the `need` rows equal to T with the SMALLEST ids go to C[query] as make_key(score, row). Positions come
//                         from wave ballots and the prefix of the waves' counts, never from an atomic; the walk ends as soon as
//                         everything is found.
// wide_sort_emit_kernel   one work-group per query: a bitonic sort of the keys, descending, in LDS (tiers of 1 024 / 4 096 / 16 384
//                         keys: 8 / 32 / 128 KiB), then the outputs. Raw: ranks first .. in order. Reweighted: adj = (double)raw *
//                         w[level] and ONE stable descending sort of the slice, done as a merge by rank: w takes three values, and
//                         multiplying by a positive constant is monotone, so the hits of one weight class are already in adj
//                         order. Their positions are compacted class by class (ballots, in order) into the query's row of C -
//                         free once the keys are in LDS - and every hit counts, by binary search on (adj, position), how many of
//                         each class stand ahead of it. The sum is its final position.
// No scratch, no printf or assert, vector stores only; the only atomics are integer adds on LDS histograms and counters, which
// commute: the same bytes on every run. LDS: the sweep's two stages (33 792 bytes dynamic); the select's histogram (8 KiB); the
// sort's tier.
#pragma once
#include "finalize.hpp"
#include "topk_select.hpp"
#include "wide_select_plan.hpp"

namespace icd {

struct WideScoreArgs {
    const float *corpus;     // [n][dim]
    const float *queries;    // [nq][dim] the block's queries
    RowMasks mask;           // nullable: no query of the call is masked; else the block's entries
    const float *lo, *hi;    // nullable each: [nq] radius / range_filter of the block's queries
    uint32_t *S;             // [nq][n_pad]
    long long n_pad;
    int nq, n, dim;
    int chunks, rows_per_chunk;   // rk_plan
};

__global__ __launch_bounds__(RK_THREADS, 1) void wide_scores_kernel(const WideScoreArgs a) {
    constexpr int BK = RK_BK, BN = RK_TILE, LDT = BK + 1, NT = RK_THREADS;
    constexpr int C4 = BK / 4, CL = (BN * C4) / NT, QH = BK / 2, Q4 = QH / 4;
    static_assert(CL >= 1 && (BN * C4) % NT == 0, "stage loads divide over the threads");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *Cs = reinterpret_cast<float *>(smem);

    const int nq = a.nq;
    const int mtile = blockIdx.x / a.chunks, chunk = blockIdx.x % a.chunks;
    const int slot0 = mtile * RK_QUERIES;
    const int row_begin = chunk * a.rows_per_chunk;
    const int row_end = (int)min((long long)a.n, (long long)row_begin + a.rows_per_chunk);   // (the sum may pass 2^31)
    if (slot0 >= nq || row_begin >= row_end) return;   // (work-group-uniform; rk_plan makes neither)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int dim = a.dim, nks = dim / BK;
    const int h = lane >> 5, c = lane & 31;

    int cdst[CL], crow_off[CL], ccol[CL];
#pragma unroll
    for (int i = 0; i < CL; ++i) {
        const int idx = tid + NT * i;
        crow_off[i] = idx / C4;
        ccol[i] = (idx % C4) * 4;
        cdst[i] = crow_off[i] * LDT + ccol[i];
    }

    // this lane's query (slots past the end read the last query; nothing of theirs is stored), its mask, its band and its run of S
    const int my_slot = slot0 + wave * 32 + c;
    const bool my_valid = my_slot < nq;
    const int sq = min(my_slot, nq - 1);
    const float *qsrc = a.queries + (size_t)sq * dim + h * QH;
    const uint32_t *mask_words = a.mask ? a.mask[sq] : nullptr;
    const bool open_lo = a.lo == nullptr;   // (no radius: a score of -inf ranks; an explicit radius of -inf leaves it out, as the band's strict compare does)
    const float lo = a.lo ? a.lo[sq] : -INFINITY, hi = a.hi ? a.hi[sq] : INFINITY;
    uint32_t *run = a.S + ws_s_offset(sq, a.n_pad);

    float bq[QH];   // the stage's k-step pairs of the query operand: bq[s] = (k = 2 s | 2 s + 1)
    auto q_pairs = [&](const float4 (&qreg)[Q4]) {
        float r[QH];
#pragma unroll
        for (int i = 0; i < Q4; ++i) { r[4 * i] = qreg[i].x; r[4 * i + 1] = qreg[i].y; r[4 * i + 2] = qreg[i].z; r[4 * i + 3] = qreg[i].w; }
#pragma unroll
        for (int i = 0; i < QH / 2; ++i) {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(r[2 * i]), __float_as_uint(r[2 * i + 1]), false, false);
            bq[i] = __uint_as_float(sw[0]);
            bq[QH / 2 + i] = __uint_as_float(sw[1]);
        }
    };

    for (int tile_row0 = row_begin; tile_row0 < row_end; tile_row0 += BN) {
        f32x16 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

        const float *csrc[CL];
#pragma unroll
        for (int i = 0; i < CL; ++i) csrc[i] = a.corpus + (size_t)min(tile_row0 + crow_off[i], a.n - 1) * dim + ccol[i];
        float4 qreg[Q4], creg[CL];
#pragma unroll
        for (int i = 0; i < Q4; ++i) qreg[i] = *reinterpret_cast<const float4 *>(qsrc + 4 * i);
#pragma unroll
        for (int i = 0; i < CL; ++i) creg[i] = *reinterpret_cast<const float4 *>(csrc[i]);
        __syncthreads();  // previous tile's readers are done with buffer 0
#pragma unroll
        for (int i = 0; i < CL; ++i) {
            float *d = Cs + cdst[i];
            d[0] = creg[i].x; d[1] = creg[i].y; d[2] = creg[i].z; d[3] = creg[i].w;
        }
        q_pairs(qreg);
        __syncthreads();

        for (int ks = 0; ks < nks; ++ks) {
            const int cur = ks & 1;
            const bool more = ks + 1 < nks;
            if (more) {
                const int k0 = (ks + 1) * BK;
#pragma unroll
                for (int i = 0; i < Q4; ++i) qreg[i] = *reinterpret_cast<const float4 *>(qsrc + k0 + 4 * i);
#pragma unroll
                for (int i = 0; i < CL; ++i) creg[i] = *reinterpret_cast<const float4 *>(csrc[i] + k0);
            }
            const float *crow = Cs + cur * BN * LDT + c * LDT + h;
            // (the corpus operands of k-step pair g + 1 are read before the eight MFMAs of pair g are issued, as in exact_topk_kernel)
            float av[2][2][4];
            auto load_pair = [&](int g, int set) {
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int t = 0; t < 4; ++t) av[set][j][t] = crow[t * 32 * LDT + 2 * (2 * g + j)];
            };
            load_pair(0, 0);
#pragma unroll
            for (int g = 0; g < BK / 4; ++g) {
                if (g + 1 < BK / 4) load_pair(g + 1, (g + 1) & 1);
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[g & 1][j][t], bq[2 * g + j], acc[t], 0, 0, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
            }
            if (more) {
                float *cd = Cs + (cur ^ 1) * BN * LDT;
#pragma unroll
                for (int i = 0; i < CL; ++i) {
                    float *d = cd + cdst[i];
                    d[0] = creg[i].x; d[1] = creg[i].y; d[2] = creg[i].z; d[3] = creg[i].w;
                }
                q_pairs(qreg);
            }
            __syncthreads();
        }

        // the store epilogue: the tile's four mask words (one aligned 16-byte load, where the exact kernel reads them), cut at n -
        // a row at or past n never ranks, so the partial last tile stores zeros up to n padded (tile_row0 + 128 <= n_pad)
        uint4 m4 = {~0u, ~0u, ~0u, ~0u};
        if (mask_words) m4 = *reinterpret_cast<const uint4 *>(mask_words + (tile_row0 >> 5));   // (tile_row0 is a multiple of 128)
        const uint32_t w[4] = {m4.x & rk_valid_bits(tile_row0, a.n), m4.y & rk_valid_bits(tile_row0 + 32, a.n),
                               m4.z & rk_valid_bits(tile_row0 + 64, a.n), m4.w & rk_valid_bits(tile_row0 + 96, a.n)};
        if (my_valid) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {   // registers 4 g .. 4 g + 3: rows t 32 + 8 g + 4 h + (0 .. 3)
                    uint32_t o[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float s = acc[t][4 * g + e];
                        const bool in = (((w[t] >> (8 * g + 4 * h + e)) & 1u) != 0u) & (s == s) & (open_lo | (lo < s)) & (s <= hi);
                        o[e] = in ? order_f32(s) : 0u;
                    }
                    *reinterpret_cast<uint4 *>(run + tile_row0 + t * 32 + 8 * g + 4 * h) = make_uint4(o[0], o[1], o[2], o[3]);
                }
            }
        }
    }
}

// ---- the select over one query's run ---------------------------------------------------------------------------------------------
struct WideSelectArgs {
    const uint32_t *S;    // [nq][n_pad]
    WideRec *rec;         // [nq]
    u64 *C;               // [nq][width]
    long long n_pad;
    int width;            // first + k
};

__global__ __launch_bounds__(WS_SELECT_THREADS) void wide_threshold_kernel(const WideSelectArgs a) {
    __shared__ uint32_t hist[WS_BINS];
    __shared__ uint32_t found[3];   // the pass's digit, the rows above it inside the prefix, the rows inside the prefix
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t *run = a.S + ws_s_offset(q, a.n_pad);
    uint32_t prefix = 0u, pmask = 0u, above = 0u, remaining = 0u, selected = 0u;
    for (int pass = 0; pass < WS_PASSES; ++pass) {
        const int shift = ws_digit_shift(pass), bins = 1 << ws_digit_bits(pass);
        for (int b = tid; b < bins; b += WS_SELECT_THREADS) hist[b] = 0u;
        __syncthreads();
        for (long long i = (long long)tid * 4; i < a.n_pad; i += (long long)WS_SELECT_THREADS * 4) {   // (n_pad is a multiple of 128)
            const uint4 v = *reinterpret_cast<const uint4 *>(run + i);
            const uint32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e[j] != 0u && (e[j] & pmask) == prefix) atomicAdd(&hist[(e[j] >> shift) & (uint32_t)(bins - 1)], 1u);
        }
        __syncthreads();
        if (wave == 0) {   // lane L owns the bins [bins - (L + 1) per, bins - L per): lane 0 the highest digits
            const int per = bins / 64, top = bins - 1 - lane * per;
            uint32_t sum = 0u;
            for (int j = 0; j < per; ++j) sum += hist[top - j];
            uint32_t incl = sum;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(incl, d);
                if (lane >= d) incl += up;
            }
            const uint32_t total = __shfl(incl, 63), excl = incl - sum;
            const uint32_t want = pass == 0 ? min((uint32_t)a.width, total) : remaining;
            if (lane == 0) { found[0] = 0u; found[1] = 0u; found[2] = total; }
            if (want > 0u && excl < want && want <= incl) {   // exactly one lane
                uint32_t ahead = excl;
                int digit = top;
                for (int j = 0; j < per; ++j) {
                    const uint32_t cnt = hist[top - j];
                    if (ahead + cnt >= want) { digit = top - j; break; }
                    ahead += cnt;
                }
                found[0] = (uint32_t)digit;
                found[1] = ahead;
            }
        }
        __syncthreads();
        if (pass == 0) { selected = found[2]; remaining = min((uint32_t)a.width, selected); }
        if (remaining == 0u) break;   // (work-group-uniform: nothing ranks)
        above += found[1];
        remaining -= found[1];
        prefix |= found[0] << shift;
        pmask |= ws_digit_mask(pass);
        __syncthreads();   // (found and hist are rewritten by the next pass)
    }
    if (tid == 0) {
        WideRec r;
        r.T = remaining == 0u ? 0xFFFFFFFFu : prefix;
        r.above = remaining == 0u ? 0u : above;
        r.need = remaining;
        r.selected = selected;
        a.rec[q] = r;
    }
}

__global__ __launch_bounds__(WS_SELECT_THREADS) void wide_collect_kernel(const WideSelectArgs a) {
    constexpr int WAVES = WS_SELECT_THREADS / 64;
    __shared__ uint32_t wa[WAVES], we[WAVES];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const WideRec r = a.rec[q];
    if (r.above + r.need == 0u) return;   // (work-group-uniform)
    const uint32_t *run = a.S + ws_s_offset(q, a.n_pad);
    u64 *C = a.C + ws_c_offset(q, a.width);
    const u64 below = (1ull << lane) - 1ull;
    uint32_t base_a = 0u, base_e = 0u;
    for (long long row0 = 0; row0 < a.n_pad; row0 += WS_SELECT_THREADS) {
        const long long row = row0 + tid;
        const uint32_t v = row < a.n_pad ? run[row] : 0u;
        const bool is_a = v > r.T, is_e = v == r.T;   // (T is no sentinel here: a zero word is neither)
        const u64 ba = __ballot(is_a), be = __ballot(is_e);
        if (lane == 0) { wa[wave] = (uint32_t)__popcll(ba); we[wave] = (uint32_t)__popcll(be); }
        __syncthreads();
        uint32_t pre_a = base_a, pre_e = base_e, tot_a = 0u, tot_e = 0u;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const uint32_t xa = wa[w], xe = we[w];
            if (w < wave) { pre_a += xa; pre_e += xe; }
            tot_a += xa; tot_e += xe;
        }
        const u64 key = ((u64)v << 32) | (u64)(~(uint32_t)row);   // make_key(score, row) from the ordered score
        if (is_a) C[pre_a + (uint32_t)__popcll(ba & below)] = key;   // (fewer than r.above rows stand before it)
        if (is_e) {
            const uint32_t e = pre_e + (uint32_t)__popcll(be & below);
            if (e < r.need) C[r.above + e] = key;
        }
        base_a += tot_a;
        base_e += tot_e;
        if (base_a == r.above && base_e >= r.need) break;   // (work-group-uniform: everything is found)
        __syncthreads();   // (wa, we are rewritten by the next step)
    }
}

// ---- sort and emit ---------------------------------------------------------------------------------------------------------------
struct WideEmitArgs {
    u64 *C;                 // [nq][width] the collected keys; a query's row is its scratch once the keys are in LDS
    const WideRec *rec;     // [nq]
    const int *levels;      // nullable: [n]
    double *out_adj;        // reweighted only: [nq][k]
    float *out_raw;         // [nq][k]
    long long *out_ids;
    int *out_levels;
    int *out_count;         // [nq]
    long long *out_selected;
    long long id_base;
    int width, first, k, reweighted;
};

__device__ __forceinline__ int wide_class(int level) { return level == 1 ? 0 : (level == 3 ? 1 : 2); }
__device__ __forceinline__ double wide_class_weight(int cls) { return level_weight(cls == 0 ? 1 : (cls == 1 ? 3 : 0)); }

template <int TIER>
__global__ __launch_bounds__(TIER == 0 ? 256 : 1024) void wide_sort_emit_kernel(const WideEmitArgs a) {
    constexpr int THREADS = TIER == 0 ? 256 : 1024, WAVES = THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64 *keys = reinterpret_cast<u64 *>(smem);
    __shared__ int cls_count[3];
    __shared__ int wave_count[3][WAVES];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const WideRec rec = a.rec[q];
    const int total = (int)(rec.above + rec.need);   // <= width <= the tier's keys
    u64 *C = a.C + ws_c_offset(q, a.width);
    int m = 2;
    while (m < total) m <<= 1;
    for (int i = tid; i < m; i += THREADS) keys[i] = i < total ? C[i] : 0ull;   // (0 is below every real key)
    if (tid < 3) cls_count[tid] = 0;
    __syncthreads();
    for (int size = 2; size <= m; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (m >> 1); t += THREADS) {
                const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i + stride;
                const bool desc = (i & size) == 0;
                const u64 x = keys[i], y = keys[j];
                if ((x < y) == desc) { keys[i] = y; keys[j] = x; }
            }
            __syncthreads();
        }
    }

    const int k = a.k, first = a.first;
    const int cnt = total > first ? total - first : 0;
    if (tid == 0) { a.out_count[q] = cnt; a.out_selected[q] = (long long)rec.selected; }
    if (!a.reweighted) {
        for (int j = tid; j < k; j += THREADS) {
            const size_t o = ws_out_offset(q, k, j);
            if (j < cnt) {
                const u64 key = keys[first + j];
                const uint32_t row = key_row(key);
                a.out_raw[o] = key_score(key);
                a.out_ids[o] = (long long)row + a.id_base;
                a.out_levels[o] = a.levels ? a.levels[row] : 1;
            } else {
                a.out_raw[o] = -INFINITY; a.out_ids[o] = -1ll; a.out_levels[o] = 0;
            }
        }
        return;
    }

    // the stable re-sort as a merge by rank. Step 1: the hits of every weight class
    int mine[3] = {0, 0, 0};
    for (int j = tid; j < cnt; j += THREADS) {
        const uint32_t row = key_row(keys[first + j]);
        const int cls = wide_class(a.levels ? a.levels[row] : 1);
        mine[0] += cls == 0; mine[1] += cls == 1; mine[2] += cls == 2;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (mine[c]) atomicAdd(&cls_count[c], mine[c]);   // (integer adds on LDS commute)
    __syncthreads();
    const int n_cls[3] = {cls_count[0], cls_count[1], cls_count[2]};
    const int cls_base[3] = {0, n_cls[0], n_cls[0] + n_cls[1]};
    // step 2: their positions in the slice, class by class in raw order, into the query's row of C (4 bytes a hit; every key was
    // read into LDS before the first barrier)
    uint32_t *P = reinterpret_cast<uint32_t *>(C);
    const u64 below = (1ull << lane) - 1ull;
    int run_base[3] = {cls_base[0], cls_base[1], cls_base[2]};
    for (int j0 = 0; j0 < cnt; j0 += THREADS) {
        const int j = j0 + tid;
        int cls = -1;
        if (j < cnt) cls = wide_class(a.levels ? a.levels[key_row(keys[first + j])] : 1);
        u64 bal[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            bal[c] = __ballot(cls == c);
            if (lane == 0) wave_count[c][wave] = __popcll(bal[c]);
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int pre = run_base[c], tot = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) {
                const int x = wave_count[c][w];
                if (w < wave) pre += x;
                tot += x;
            }
            if (cls == c) P[pre + __popcll(bal[c] & below)] = (uint32_t)j;
            run_base[c] += tot;
        }
        __syncthreads();   // (wave_count is rewritten by the next step; behind the last one P is complete and visible)
    }
    // step 3: every hit's final position: the hits of each class that stand ahead of it. Within a class adj falls (weakly) with
    // the position, so "ahead" - a larger adj, or the same adj at a smaller position - holds for a prefix of the class's list.
    for (int j = tid; j < k; j += THREADS) {
        if (j >= cnt) {
            const size_t o = ws_out_offset(q, k, j);
            a.out_adj[o] = -INFINITY; a.out_raw[o] = -INFINITY; a.out_ids[o] = -1ll; a.out_levels[o] = 0;
            continue;
        }
        const u64 key = keys[first + j];
        const uint32_t row = key_row(key);
        const float raw = key_score(key);
        const int lv = a.levels ? a.levels[row] : 1;
        const double adj = (double)raw * level_weight(lv);
        int pos = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double wc = wide_class_weight(c);
            const uint32_t *list = P + cls_base[c];
            int lo = 0, hi = n_cls[c];   // the first entry that is NOT ahead
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const int hj = (int)list[mid];
                const double hadj = (double)key_score(keys[first + hj]) * wc;
                if (hadj > adj || (hadj == adj && hj < j)) lo = mid + 1; else hi = mid;
            }
            pos += lo;
        }
        const size_t o = ws_out_offset(q, k, pos);
        a.out_adj[o] = adj; a.out_raw[o] = raw; a.out_ids[o] = (long long)row + a.id_base; a.out_levels[o] = lv;
    }
}

}  // namespace icd
