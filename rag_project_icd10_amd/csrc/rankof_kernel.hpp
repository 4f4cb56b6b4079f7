// rankof_kernel.hpp - rank-of search: where do given rows land in a query's exact ranking? Replaces what an
// evaluation does by hand today: a search at the largest k and a lookup (every rank past 128 is lost), or all n scores per query
// pulled to the host and sorted there.
//
// rankof_targets_kernel  four lanes per (query, target): the target's canonical score by mmr_quad_chain (mmr_select_kernel.hpp:
//                        the strict d-ascending fmaf chain from +0.0f, the bits of oracle/icd_oracle.c chain_score and of every
//                        exact kernel), its (score, row) key as topk_select.hpp builds it, its adjusted score and level, and
//                        the preset of its rank: 0, or -1 where there is none (a padding slot, an id outside the index, a row
//                        outside the query's mask, a NaN score - the exact kernels never return such a row). Slot 0 of a query
//                        also zeroes its `selected`. The row address is formed only from a row inside [0, n).
// rankof_sweep_kernel    the geometry of exact_topk_kernel<.., BAND, MASK>: RK_QUERIES queries x a chunk of RK_TILE-row tiles per
//                        work-group, the corpus rows of a stage through LDS, the queries straight into the MFMA's operand
//                        registers, v_mfma_f32_32x32x2_f32 with k mapped to d ascending - the same bits. Behind a tile's MFMAs
//                        lane (c, h) holds 64 scores of query c; where the exact kernel overwrites masked-out rows and appends the
//                        others to its candidate lists, this one turns every admitted, non-NaN score into its key and makes ONE
//                        64-bit compare per (row, target): a row whose key is larger stands strictly ahead of the target. Counts
//                        stay in registers over the chunk (16 per lane), the two lanes of a query add theirs (one shuffle), and
//                        one lane issues ONE integer add per (work-group, query, target) into the output. A wave's 32 queries
//                        are its own, so there is nothing to add across waves. `selected` is the popcount of the tile's mask
//                        words, cut at n, added the same way. Integer adds commute: the same bytes on every run.
// No scratch, no printf or assert, vector stores and vector atomics only. LDS: the sweep's two stages, 33 792 bytes dynamic.
#pragma once
#include "mmr_select_kernel.hpp"
#include "rankof_plan.hpp"
#include "topk_select.hpp"

namespace icd {

constexpr u64 RK_NO_KEY = ~0ull;   // the key of a target without a rank: no row's key is larger, nothing is ever added

struct RankOfTargetArgs {
    const float *corpus;        // [n][dim] the canonical fp32 rows
    const float *queries;       // [nq][dim]
    const long long *targets;   // [nq][nt] global ids, -1 = padding
    const int *levels;          // nullable: [n]
    RowMasks mask;              // nullable: no query of the call is masked
    u64 *tkey;                  // [nq][nt]
    long long *rank;            // [nq][nt]
    double *adj;
    float *raw;
    int *out_levels;
    long long *selected;        // [nq]
    long long n, id_base;
    int dim, nq, nt;
};

#pragma clang fp contract(off)
__global__ __launch_bounds__(RK_TARGET_THREADS) void rankof_targets_kernel(const RankOfTargetArgs a) {
    const int qi = threadIdx.x & 3;
    const long long slot = (long long)blockIdx.x * RK_TARGET_SLOTS + (threadIdx.x >> 2);
    const long long total = (long long)a.nq * a.nt;
    const bool live = slot < total;            // (the same in the four lanes of a quad)
    const long long s = live ? slot : total - 1;
    const long long q = s / a.nt;
    const long long id = a.targets[s];
    const long long row = id == -1ll ? -1ll : br_row_of(id, a.id_base, a.n);
    bool in = row >= 0;
    if (in && a.mask) in = ((a.mask[q][row >> 5] >> (row & 31)) & 1u) != 0u;
    // (every lane runs the chain - its quad broadcasts need all four - on row 0 where there is no row)
    const float sc = mmr_quad_chain(a.corpus, in ? row : 0ll, a.dim, a.queries + (size_t)q * a.dim, qi);
    if (!live || qi != 0) return;
    const bool ranked = in && sc == sc;
    const int lv = in ? (a.levels ? a.levels[row] : 1) : 0;
    a.tkey[s] = ranked ? make_key(sc, (uint32_t)row) : RK_NO_KEY;
    a.rank[s] = ranked ? 0ll : -1ll;
    a.raw[s] = in ? sc : __builtin_nanf("");
    a.adj[s] = in ? (double)sc * level_weight(lv) : __builtin_nan("");
    a.out_levels[s] = lv;
    if (s == q * a.nt) a.selected[q] = 0ll;
}
#pragma clang fp contract(fast)

struct RankOfSweepArgs {
    const float *corpus;     // [n][dim]
    const float *queries;    // [nq][dim]
    RowMasks mask;           // nullable: no query of the call is masked
    const u64 *tkey;         // [nq][nt] the targets' keys (RK_NO_KEY: no rank)
    long long *rank;         // [nq][nt] preset by rankof_targets_kernel
    long long *selected;     // [nq] zeroed by rankof_targets_kernel
    int nq, nt, n, dim;
    int chunks, rows_per_chunk;   // rk_plan
};

__global__ __launch_bounds__(RK_THREADS, 1) void rankof_sweep_kernel(const RankOfSweepArgs a) {
    constexpr int BK = RK_BK, BN = RK_TILE, LDT = BK + 1, NT = RK_THREADS;
    constexpr int C4 = BK / 4, CL = (BN * C4) / NT, QH = BK / 2, Q4 = QH / 4;
    static_assert(CL >= 1 && (BN * C4) % NT == 0, "stage loads divide over the threads");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *Cs = reinterpret_cast<float *>(smem);

    const int nq = a.nq, nt = a.nt;
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

    // this lane's query (slots past the end read the last query; nothing of theirs is added), its mask and its targets' keys
    const int my_slot = slot0 + wave * 32 + c;
    const bool my_valid = my_slot < nq;
    const int sq = min(my_slot, nq - 1);
    const float *qsrc = a.queries + (size_t)sq * dim + h * QH;
    const uint32_t *mask_words = a.mask ? a.mask[sq] : nullptr;
    u64 tk[RK_MAX_TARGETS];
    int cnt[RK_MAX_TARGETS];
#pragma unroll
    for (int j = 0; j < RK_MAX_TARGETS; ++j) {
        tk[j] = (my_valid && j < nt) ? a.tkey[rk_slot(sq, j, nt)] : RK_NO_KEY;
        cnt[j] = 0;
    }
    int sel = 0;

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

        // the count: the tile's four mask words (one aligned 16-byte load, where the exact kernel reads them), cut at n - a row at
        // or past n is never admitted, so the partial last tile needs no other test
        uint4 m4 = {~0u, ~0u, ~0u, ~0u};
        if (mask_words) m4 = *reinterpret_cast<const uint4 *>(mask_words + (tile_row0 >> 5));   // (tile_row0 is a multiple of 128)
        const uint32_t w[4] = {m4.x & rk_valid_bits(tile_row0, a.n), m4.y & rk_valid_bits(tile_row0 + 32, a.n),
                               m4.z & rk_valid_bits(tile_row0 + 64, a.n), m4.w & rk_valid_bits(tile_row0 + 96, a.n)};
        if (h == 0) sel += __popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            u64 key[16];   // 0: not admitted, or a NaN score - below every target's key
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int off = 4 * h + (r & 3) + 8 * (r >> 2);
                const float s = acc[t][r];
                const bool in = (((w[t] >> off) & 1u) != 0u) & (s == s);
                key[r] = in ? make_key(s, (uint32_t)(tile_row0 + t * 32 + off)) : 0ull;
            }
#pragma unroll
            for (int j = 0; j < RK_MAX_TARGETS; ++j) {
                if (j < nt) {   // (work-group-uniform)
#pragma unroll
                    for (int r = 0; r < 16; ++r) cnt[j] += key[r] > tk[j] ? 1 : 0;
                }
            }
        }
    }

    // the two lanes of a query hold the halves of its counts; lane h = 0 adds the sum once per (work-group, query, target)
#pragma unroll
    for (int j = 0; j < RK_MAX_TARGETS; ++j) {
        const int both = cnt[j] + __shfl_xor(cnt[j], 32);
        if (j < nt && h == 0 && my_valid && both > 0)
            atomicAdd(reinterpret_cast<unsigned long long *>(a.rank + rk_slot(my_slot, j, nt)), (unsigned long long)both);
    }
    if (h == 0 && my_valid && sel > 0) atomicAdd(reinterpret_cast<unsigned long long *>(a.selected + my_slot), (unsigned long long)sel);
}

}  // namespace icd
