// group_topk.hpp — Milvus grouping search (`group_by_field` / `group_size`), exact, on the device: the k best GROUPS of a query
// and the s best rows of each. A top-k list cannot answer that - an ICD family fills a top-128 with
// siblings of two or three categories - so every row is scored and reduced per group:
//
//   1. group_scores_kernel  canonical scores of ALL rows for a block of queries -> S[query][position], the exact_topk main loop
//                           (exact_kernel.hpp: rows through LDS, queries from registers, v_mfma_f32_32x32x2_f32 = the d-ascending
//                           fmaf chain) with a plain store epilogue. The rows are read THROUGH the grouping's `order`
//                           (rows sorted by (group, row)), so a group's scores are one contiguous run of S.
//   2. group_best_kernel    segmented maximum of the 64-bit key over those runs -> best[query][group] (the group scorers SUM /
//                           AVG put group_aggregate_kernel.hpp's reduction here instead: DESIGN.md section 24)
//   3. group_finish_kernel  one wave per query: the k best groups of best[query][.], of each its s best members (a second
//                           pass over its run of S, only when s > 1), then emit_outputs (finalize.hpp): raw order, the level
//                           reweight in double, the stable re-sort, row_map, with the group id travelling next to the level.
//
// Replaces MilvusClient.search(..., group_by_field=, group_size=) - the reference itself does not pass them
// (services/milvus_service.py:280-285); the hit list it would get back is re-sorted by :290-314 like any other.
#pragma once
#include "finalize.hpp"
#include "topk_select.hpp"

namespace icd {

constexpr int GROUP_TILE = 128;   // queries per work-group and rows per work-group of the scoring pass; S rows are padded to it

struct GroupScoreArgs {
    const float *corpus;   // [n][dim]
    const float *queries;  // [nq][dim]
    const int *order;      // [n] row at every position of the (group, row) order
    int nq, n, dim, mtiles;
    float *S;              // [nq rounded up to 128][ldS]
    long long ldS;         // n rounded up to 128: a tile's stores need no bound
};

// Work-group = 4 waves = 128 queries x ONE tile of 128 positions; block b -> (tile b / mtiles, query tile b % mtiles): the
// work-groups in flight share their corpus rows. Operand layout, staging and MFMA order are exact_topk_kernel's.
__global__ __launch_bounds__(256, 2) void group_scores_kernel(GroupScoreArgs a) {
    constexpr int NW = 4, BK = 32, BN = GROUP_TILE, LDT = BK + 1, NT = NW * 64;
    constexpr int C4 = BK / 4, CL = (BN * C4) / NT, QH = BK / 2, Q4 = QH / 4;
    __shared__ float Cs[2 * BN * LDT];

    const int mtile = blockIdx.x % a.mtiles, tile_row0 = (blockIdx.x / a.mtiles) * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int dim = a.dim, nks = dim / BK;
    const int h = lane >> 5, c = lane & 31;
    const int my_slot = mtile * (NW * 32) + wave * 32 + c;
    const bool my_valid = my_slot < a.nq;

    int cdst[CL];
    const float *csrc[CL];
#pragma unroll
    for (int i = 0; i < CL; ++i) {
        const int idx = tid + NT * i;
        const int ro = idx / C4, col = (idx % C4) * 4;
        cdst[i] = ro * LDT + col;
        const int row = a.order[min(tile_row0 + ro, a.n - 1)];   // (past the end: the last position again, its scores land in S's padding)
        csrc[i] = a.corpus + (size_t)row * dim + col;
    }
    const float *qsrc = a.queries + (size_t)min(my_slot, a.nq - 1) * dim + h * QH;

    float bq[QH];
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

    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    float4 qreg[Q4], creg[CL];
#pragma unroll
    for (int i = 0; i < Q4; ++i) qreg[i] = *reinterpret_cast<const float4 *>(qsrc + 4 * i);
#pragma unroll
    for (int i = 0; i < CL; ++i) creg[i] = *reinterpret_cast<const float4 *>(csrc[i]);
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

    // store epilogue: register r of tile t is position tile_row0 + 32 t + 8 (r >> 2) + 4 h + (r & 3) of query my_slot
    if (my_valid) {
        float *dst = a.S + (size_t)my_slot * a.ldS + tile_row0 + 4 * h;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                *reinterpret_cast<float4 *>(dst + 32 * t + 8 * j) = make_float4(acc[t][4 * j], acc[t][4 * j + 1], acc[t][4 * j + 2], acc[t][4 * j + 3]);
    }
}

__device__ __forceinline__ u64 shfl_up_u64(u64 v, int off) {
    return ((u64)(uint32_t)__shfl_up((int)(v >> 32), off) << 32) | (uint32_t)__shfl_up((int)v, off);
}

struct GroupBestArgs {
    const float *S;
    long long ldS;
    const int *order;    // [n] row at every position
    const int *gpos;     // [n] dense group at every position (non-decreasing)
    const int *seg;      // [G + 1] first position of every group
    int nq, n, G;
    int R, nranges;      // positions per wave (a multiple of 64) and waves per query quad
    u64 *best;           // [nq][G], zero on entry (0 is below every key)
};

// A wave walks R consecutive positions for QW queries at once (the group boundaries are the same for all of them): per
// 64 positions a segmented max-scan of the keys, one store per run that ends inside the chunk, the open run carried in
// registers. A group that lies inside the wave's range is written with a plain store by the one lane that closes it; a group
// cut by a range boundary (large groups: a few per wave) is combined with a 64-bit atomic maximum - order-independent, so the
// result is deterministic.
template <int QW>
__global__ __launch_bounds__(256) void group_best_kernel(GroupBestArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long w = (long long)blockIdx.x * 4 + wave;
    const int rng = (int)(w % a.nranges), q0 = (int)(w / a.nranges) * QW;
    if (q0 >= a.nq) return;
    const int p_begin = rng * a.R, p_end = min(a.n, p_begin + a.R);
    auto flush = [&](int g, int i, u64 key) {
        if (q0 + i >= a.nq) return;
        u64 *dst = a.best + (size_t)(q0 + i) * a.G + g;
        if (a.seg[g] >= p_begin && a.seg[g + 1] <= p_end) *dst = key;
        else if (key != 0ull) atomicMax(dst, key);
    };
    int cg = -1;
    u64 ck[QW];
#pragma unroll
    for (int i = 0; i < QW; ++i) ck[i] = 0ull;
    for (int p0 = p_begin; p0 < p_end; p0 += 64) {
        const int p = p0 + lane;
        const bool in = p < p_end;
        const int last = min(63, p_end - 1 - p0);   // last lane that holds a position (wave-uniform)
        const int g = in ? a.gpos[p] : -2;
        const uint32_t row = in ? (uint32_t)a.order[p] : 0u;
        u64 key[QW];
#pragma unroll
        for (int i = 0; i < QW; ++i) {
            key[i] = 0ull;
            if (in && q0 + i < a.nq) {
                const float sc = a.S[(size_t)(q0 + i) * a.ldS + p];
                if (sc == sc) key[i] = make_key(sc, row);   // (a NaN score is no hit, as everywhere else)
            }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int go = __shfl_up(g, off);
            const bool same = lane >= off && go == g;
#pragma unroll
            for (int i = 0; i < QW; ++i) {
                const u64 o = shfl_up_u64(key[i], off);
                if (same && o > key[i]) key[i] = o;
            }
        }
        const int g_first = readlane<int>(g, 0);
        if (cg >= 0 && cg != g_first) {
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < QW; ++i) flush(cg, i, ck[i]);
            }
        } else if (cg >= 0 && g == cg) {
#pragma unroll
            for (int i = 0; i < QW; ++i) key[i] = ck[i] > key[i] ? ck[i] : key[i];
        }
        const int g_next = __shfl_down(g, 1);
        if (in && lane < last && g_next != g) {
#pragma unroll
            for (int i = 0; i < QW; ++i) flush(g, i, key[i]);
        }
        cg = readlane<int>(g, last);
#pragma unroll
        for (int i = 0; i < QW; ++i) ck[i] = readlane_u64(key[i], last);
    }
    if (cg >= 0 && lane == 0) {
#pragma unroll
        for (int i = 0; i < QW; ++i) flush(cg, i, ck[i]);
    }
}

// The KP best of `count` keys (key_at(i), 0 = none), sorted best first at buf[0 ..); returns how many. Streaming form of the
// candidate buffers of topk_select.hpp: keys above the running KP-th best are appended, compact_one ranks the buffer
// whenever another 64 might not fit.
template <int KP, int E, typename F>
__device__ __forceinline__ int wave_select(F key_at, int count, u64 *buf, int lane) {
    constexpr int CAP = 64 * E;
    static_assert(CAP - 64 >= KP, "a full buffer still takes one more chunk");
    const u64 lt = (1ull << lane) - 1ull;
    u64 thr = 0ull, kth;
    int cnt = 0;
    for (int i0 = 0; i0 < count; i0 += 64) {
        const int i = i0 + lane;
        const u64 key = i < count ? key_at(i) : 0ull;
        const bool pass = key > thr;
        const u64 m = __ballot(pass);
        if (pass) buf[cnt + __popcll(m & lt)] = key;
        cnt += __popcll(m);
        if (cnt > CAP - 64) {
            compact_one<KP, E>(buf, cnt, lane, kth);
            if (cnt >= KP) { thr = kth; cnt = KP; }
        }
    }
    compact_one<KP, E>(buf, cnt, lane, kth);
    return min(cnt, KP);
}

struct GroupFinishArgs {
    const u64 *best;      // [nq][G] of this block of queries
    const float *S;
    long long ldS;
    const int *order;     // [n]
    const int *seg;       // [G + 1]
    const int *dense_of;  // [n] dense group of every row
    int nq, G, k, s;
    int q_base;           // first query of the block: the outputs are indexed by q_base + query
    FinArgs fin;          // k = k * s, levels, id_base, row_map, groups, the outputs (emit_outputs)
    // GS instantiations only (the scored entry point), either may be null: the winning groups in rank order
    float *out_group_scores;   // [query][k] the score the group ranked by; -inf in padding
    int *out_group_ids;        // [query][k] the caller's id of the group; -1 in padding
};

constexpr int GROUP_FIN_WAVE_LDS = (256 + 128 + 128) * 8 + 128 * 8;   // select buffer | winning groups | hits | adjbuf

// GS = false is the kernel as it always was; GS = true also writes the winning groups' own scores and ids
template <int KP, int E, bool GS = false>
__global__ __launch_bounds__(256) void group_finish_kernel(GroupFinishArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[4 * GROUP_FIN_WAVE_LDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + wave;
    if (q >= a.nq) return;
    u64 *buf = reinterpret_cast<u64 *>(smem + (size_t)wave * GROUP_FIN_WAVE_LDS);
    u64 *gsel = buf + 256, *hits = gsel + 128;
    double *adjbuf = reinterpret_cast<double *>(hits + 128);

    const u64 *bq = a.best + (size_t)q * a.G;
    const int ng = min(a.k, wave_select<KP, E>([&](int i) { return bq[i]; }, a.G, buf, lane));
    if constexpr (GS) {
        const size_t o = (size_t)(a.q_base + q) * a.k;
        for (int j = lane; j < a.k; j += 64) {
            if (a.out_group_scores) a.out_group_scores[o + j] = j < ng ? key_score(buf[j]) : -INFINITY;
            if (a.out_group_ids) a.out_group_ids[o + j] = j < ng ? a.fin.groups[key_row(buf[j])] : -1;
        }
    }
    const u64 *sorted = buf;
    int nres = ng;
    if (a.s > 1) {
        for (int j = lane; j < ng; j += 64) gsel[j] = buf[j];
        nres = 0;
        const float *sq = a.S + (size_t)q * a.ldS;
        for (int j = 0; j < ng; ++j) {
            const int g = a.dense_of[key_row(gsel[j])];
            const int b = a.seg[g], e = a.seg[g + 1];
            const int m = min(a.s, wave_select<KP, E>([&](int i) {
                const float sc = sq[b + i];
                return sc == sc ? make_key(sc, (uint32_t)a.order[b + i]) : 0ull;
            }, e - b, buf, lane));
            for (int i = lane; i < m; i += 64) hits[nres + i] = buf[i];
            nres += m;
        }
        sorted = hits;
    }
    emit_outputs(a.fin, a.q_base + q, sorted, nres, adjbuf, lane);
}

}  // namespace icd
