// flat_partition.hpp — index arithmetic of the flat (query tile x corpus tile) partition of coarse_flat_kernel.hpp.
// Plain C++ (no HIP types): shared by the kernel, the host launcher and tests/test_flat_partition.py (g++).
//
// Units are numbered u = mtile * ctiles + tile; work-group w takes [w U, (w+1) U). Its run inside one query tile is cut
// into lists of at most `list_tiles` tiles; ordinals count the lists of a query tile in row order.
#pragma once
#include <algorithm>
#if defined(__HIPCC__)
#define ICD_HD __host__ __device__
#else
#define ICD_HD
#endif

namespace icd {

constexpr int FLAT_SPARE_TILES = 7;   // zero tiles allocated behind the fp16 corpus image (plan_flat_tiles may sweep them)

// number of lists a run of `len` tiles is cut into
ICD_HD inline int flat_lists_of_run(int len, int list_tiles) { return (len + list_tiles - 1) / list_tiles; }

// ordinal (within query tile m) of the first list of work-group w's run: the lists of the earlier work-groups
ICD_HD inline int flat_first_ordinal(int m, int w, int ctiles, int U, int list_tiles) {
    const long long m0 = (long long)m * ctiles, m1 = m0 + ctiles;
    int ord = 0;
    for (long long wp = m0 / U; wp < w; ++wp) {
        const long long r0 = wp * U > m0 ? wp * U : m0;
        const long long r1 = (wp + 1) * U < m1 ? (wp + 1) * U : m1;
        if (r1 > r0) ord += flat_lists_of_run((int)(r1 - r0), list_tiles);
    }
    return ord;
}


// Work-groups l and l + T start on the same corpus tile, T = ctiles / gcd(U mod ctiles, ctiles): they stream the same
// tiles at the same time and, placed on one XCD (flat_workgroup_of_block), share its L2.
ICD_HD inline int flat_class_period(int U, int ctiles) {
    int g = U % ctiles, h = ctiles;   // gcd(0, c) = c
    while (g) { const int t = h % g; h = g; g = t; }
    return ctiles / h;
}

// Tiles per work-group U and the corpus tile count to sweep (ctiles_min .. ctiles_min + spare; the tiles past the corpus
// are zero rows that never pass the select). The smallest U leaves every CU the same number of tiles, but when it is
// coprime to the tile count no two work-groups ever stream the same tile together and every XCD fetches the corpus for
// itself (measured: 40 474 rows = 317 tiles, U = 98: 0.771 ms; 320 tiles, U = 100: 0.721 ms, the rate of the 37 000-row
// case). Cost model: time ~ U, +7 % when classes have fewer than two members, +3 % below four.
struct FlatPlan { int ctiles, U; };
ICD_HD inline FlatPlan plan_flat_tiles(int mtc, int ctiles_min, int spare, int num_cu) {
    FlatPlan best{ctiles_min, 1};
    double best_cost = 1e300;
    for (int ce = ctiles_min; ce <= ctiles_min + spare; ++ce) {
        const long long units = (long long)mtc * ce;
        const int umin = (int)((units + num_cu - 1) / num_cu) > 1 ? (int)((units + num_cu - 1) / num_cu) : 1;
        const int umax = umin + (umin / 16 > 1 ? umin / 16 : 1);
        for (int U = umin; U <= umax; ++U) {
            const int nwg = (int)((units + U - 1) / U);
            const int members = nwg / flat_class_period(U, ce);
            const double cost = (double)U * (members >= 4 ? 1.0 : (members >= 2 ? 1.03 : 1.07));
            if (cost < best_cost - 1e-9) { best_cost = cost; best.ctiles = ce; best.U = U; }
        }
    }
    return best;
}

// work-group index of hardware block `w` of a grid of G: every XCD (blockIdx mod 8) gets a contiguous stretch of the
// class-major order of the logical indices (class = index mod T: work-groups of a class start on the same corpus
// tile); T <= 0: identity. A bijection of [0, G).
ICD_HD inline int flat_workgroup_of_block(int w, int G, int T) {
    if (T <= 0) return w;
    const int xcd = w & 7, q8 = G >> 3, r8 = G & 7;
    const int jx = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (w >> 3);   // contiguous per XCD
    const int qT = G / T, rT = G - qT * T;
    if (qT == 0) return jx;
    if (jx < rT * (qT + 1)) return jx / (qT + 1) + (jx % (qT + 1)) * T;
    const int jj = jx - rT * (qT + 1);
    return rT + jj / qT + (jj % qT) * T;
}


// ---- list plan of the coarse pass (icd_search.hip search_device) ----------------------------------------------------
constexpr int FLAT_TILE_ROWS = 128;      // rows of a corpus tile (CO_BN)
constexpr int COARSE_MAX_P = 32;         // lists per query of the first pass (P * KP <= FIN_MAX_CAND)
constexpr int PASS2_CHUNKS = 20;         // second coarse pass (and wide mode): about this many candidate lists per query
constexpr int PASS2_MAX_P = 24;          // ... at most this many (workspace); 24 x 16 candidates < FIN_MAX_CAND
constexpr int PASS2_BELOW = 320;         // the second pass runs when the first gave a query fewer candidates than this
constexpr long long FLAT_DESC_MAX_BYTES = 0x7FFFFFFFLL;   // num_records of the kernel's per-list buffer descriptor (a signed int)

// The longest list one buffer descriptor reaches. coarse_flat_kernel bases its descriptor at a list's first tile and
// addresses tile t of the list with the 32-bit soffset t * 128 * dim * 2; num_records is capped at 2^31 - 1 bytes. A list
// of this many tiles ends inside num_records, and the one tile the ring prefetches past its end (never consumed) still has
// an soffset below 2^32: 10 922 tiles (1.4 M rows) at dim 768, 8 191 at 1024.
ICD_HD inline int flat_max_list_tiles(int dim) { return (int)(FLAT_DESC_MAX_BYTES / ((long long)FLAT_TILE_ROWS * dim * 2)); }

// largest number of lists of any query tile (the kernel's rule, flat_first_ordinal)
inline int flat_lists_needed(int mtc, int ctiles, int U, int list_tiles) {
    int worst = 0;
    for (int m = 0; m < mtc; ++m) {
        const long long m1 = (long long)(m + 1) * ctiles;
        const int wl = (int)((m1 - 1) / U);   // last work-group touching the query tile
        const int p = flat_first_ordinal(m, wl + 1, ctiles, U, list_tiles);
        if (p > worst) worst = p;
    }
    return worst;
}

struct CoarsePlanIn {
    int mtc, ctiles, U;            // query tiles, corpus tiles to sweep and tiles per work-group (plan_flat_tiles)
    int nq, k;
    int kp;                        // candidates per list of the first pass (CO_KP, or CO_KP_WIDE with wide_lists)
    int kp2;                       // ... of the second pass (CO_KP)
    int max_cand;                  // finalize's candidate window (FIN_MAX_CAND)
    int wide_lists;                // the first pass keeps kp_wide candidates per list: about k / 6 lists
    int wide_now;                  // wide mode: about PASS2_CHUNKS lists per query
    int chunks_override;           // test hook (> 0): about this many lists per query, every work-group's run one list
    int list_override;             // A/B (> 0): tiles per list of the narrow plan
    int pass2;                     // the second pass may run (enabled, not disarmed, its workspace allocated)
    long long partc_cap, part2_cap;   // workspace entries of the two passes
    int max_list_tiles;            // flat_max_list_tiles(dim)
};
struct CoarsePlan {
    int ok;                        // 0: no first-pass plan fits the workspace and finalize's window
    int U, list_tiles, P;          // first pass
    int U2, list_tiles2, P2;       // second pass (P2 = 0: none)
};

// The list plan of both coarse passes: a pure function of the shape, the workspace and the options. Lists never grow past
// max_list_tiles; a shape that would need longer ones to fit the workspace gets more tiles per work-group, or no plan.
inline CoarsePlan plan_coarse_lists(const CoarsePlanIn &in) {
    const int ctiles = in.ctiles, lcap = std::min(in.max_list_tiles, ctiles);
    CoarsePlan r{};
    int U = in.U;
    // A query's lists should number at least two of comparable length: the certificate compares against the largest
    // score any list may have dropped, and with one list that is the query's own 16th best (8 % of Gaussian queries then
    // fail, profiles/r01_sizes_before_pmin2.log); with two or more it is about rank 32.
    int L = std::max(1, (ctiles + 1) / 2);
    // Larger k: every list keeps KP candidates and ends on its own KP-th best, so the bound the certificate compares the
    // k-th best against sits near rank KP P / 2 of the whole corpus: ask for about k / 4 lists of 16. Above k = 64 (dim
    // 768) the lists keep 24: a query fails the certificate when ONE list holds more than KP of the ~1.3 k rows around its
    // top-k - with 16 that happens to 3-5 of 10 000 queries at k = 100 and costs an exact corpus sweep per batch
    // (0.34 ms); with 24 per list and about k / 6 lists it did not happen. The wider lists make the coarse pass ~20 %
    // slower (lower thresholds, more appends), so they only pay where that sweep is the larger cost: k = 100
    // 1.69 -> 1.54 ms, k = 32 would go 0.87 -> 0.99 (profiles/r02_tile_planner_and_shapes.log).
    if (in.wide_lists) L = std::max(1, std::min(L, ctiles / ((in.k + 5) / 6)));
    else if (in.k > 8) L = std::max(1, std::min(L, ctiles / ((in.k + 3) / 4)));
    if (in.list_override > 0) L = in.list_override;
    if (in.chunks_override > 0) {
        U = std::max(1, (ctiles + in.chunks_override - 1) / in.chunks_override);
        L = ctiles;
    } else if (in.wide_now) {
        // Wide mode: about PASS2_CHUNKS lists per query, cut out of the SAME long sweeps as the narrow plan (a work-group
        // keeps its queries in registers and its ring running over ~100 tiles and closes a list every 16)
        L = std::max(1, (ctiles + PASS2_CHUNKS - 1) / PASS2_CHUNKS);
    }
    L = std::min(L, lcap);
    auto fits = [&](int p) { return p <= COARSE_MAX_P && p * in.kp <= in.max_cand && (long long)in.nq * p * in.kp <= in.partc_cap; };
    int P = flat_lists_needed(in.mtc, ctiles, U, L);
    // too many lists for the workspace or for finalize's candidate window: longer lists first (the balance of the
    // partition is untouched), more tiles per work-group once a list spans the corpus or reaches the descriptor's reach
    while (!fits(P)) {
        if (L < lcap) L = std::min(lcap, L + std::max(1, L / 8));
        else if (U < ctiles) U = std::min(ctiles, U + std::max(1, U / 4));
        else break;
        P = flat_lists_needed(in.mtc, ctiles, U, L);
    }
    r.ok = fits(P) ? 1 : 0;
    r.U = U; r.list_tiles = L; r.P = P;
    if (!r.ok) return r;
    // The second pass: the same sweep cut into about PASS2_CHUNKS lists per query, every work-group's run one list (cut
    // at the descriptor's reach), sized for the full batch: the kernel sizes the sweep from the flagged count on the device.
    if (in.pass2 && P * in.kp < PASS2_BELOW) {
        int U2 = std::max(1, (ctiles + PASS2_CHUNKS - 1) / PASS2_CHUNKS);
        const int L2 = lcap;
        int p2 = flat_lists_needed(in.mtc, ctiles, U2, L2);
        while ((p2 > PASS2_MAX_P || (long long)in.nq * p2 * in.kp2 > in.part2_cap) && U2 < ctiles) {
            U2 = std::min(ctiles, U2 + std::max(1, U2 / 8));
            p2 = flat_lists_needed(in.mtc, ctiles, U2, L2);
        }
        if (p2 <= PASS2_MAX_P && (long long)in.nq * p2 * in.kp2 <= in.part2_cap && p2 * in.kp2 > P * in.kp) {
            r.U2 = U2; r.list_tiles2 = L2; r.P2 = p2;
        }
    }
    return r;
}

// Entries per candidate workspace of the first pass (icd_index_create): about k / 4 lists of kp up to k = 64, about k / 6
// lists of kp_wide above (+ the lists that work-group boundaries add), and the wide partition of large batches on
// family-shaped corpora (wide mode: PASS2_MAX_P lists of kp). The second pass's workspace holds PASS2_MAX_P lists of kp.
inline long long coarse_partc_entries(int max_nq_pad, int kcap, int kp, int kp_wide, int max_cand) {
    const int lists = std::min(COARSE_MAX_P, std::max(6, (std::min(kcap, 64) + 3) / 4 + 4));
    const int wide = kcap > 64 ? std::min(max_cand / kp_wide, (kcap + 5) / 6 + 4) : 0;
    return std::max((long long)max_nq_pad * std::max(std::max(lists, PASS2_MAX_P) * kp, wide * kp_wide), 1LL << 20);
}
inline long long coarse_part2_entries(int max_nq_pad, int kp) { return (long long)max_nq_pad * PASS2_MAX_P * kp; }

// Rows per work-group of the streaming exact kernel (stream_kernel.hpp), whose buffer descriptor spans one work-group's
// rows (fp32, at most rows_per_wg * dim * 4 bytes from its base): the multi-list form ...
inline int stream_rows_per_wg(int n, int num_cu) {
    const int nwg_max = std::max(1, std::min(num_cu, 256));
    return ((n + nwg_max - 1) / nwg_max + 255) / 256 * 256;
}
// ... and the single-launch form: rows per wave and step (whole 8-row pieces, at most 64), rows and count of work-groups
struct StreamOneRows { int rps, rows_per_wg, nwg; };
inline StreamOneRows plan_stream_one_rows(int n, int num_cu) {
    const int ncu = std::max(1, std::min(num_cu, 256));
    const int per_cu = (n + ncu - 1) / ncu;
    const int rps = std::min(64, ((per_cu + 3) / 4 + 7) / 8 * 8);
    const int steps = (per_cu + 4 * rps - 1) / (4 * rps);
    StreamOneRows p;
    p.rps = rps; p.rows_per_wg = 4 * rps * steps; p.nwg = (n + p.rows_per_wg - 1) / p.rows_per_wg;
    return p;
}

// List counts after every reduction level of the streaming kernel's 4 * nwg per-wave lists: a reduce wave merges at most
// per_max lists, the last level must leave p_final lists (p_final = 0: as few as one more level gives), and the number
// of levels must be ODD because the levels ping-pong between the two list workspaces and finalize reads the second one.
// (Round 1 sized the sweep so that ONE level sufficed: 16 work-groups at k > 16, 4 at k > 64 - a 0.45 / 1.6 ms fallback
// for a single uncertified query at k = 64 / 100, profiles/r02_shapes_before.log. Now the sweep always fills the chip.)
ICD_HD inline int plan_reduce_levels(int nlists, int per_max, int p_final, int p_cap, int *plan /* [8] */) {
    const int target = p_final > 0 ? p_final : p_cap;
    int levels = 1;
    long long reach = (long long)per_max * target;          // lists that `levels` levels can bring down to `target`
    while (reach < nlists) { reach *= per_max; ++levels; }
    const bool extra = levels % 2 == 0;                      // an even count gets one more level, of fan-in 2, in front
    if (levels + (extra ? 1 : 0) > 8) return 0;
    int cnt = 0, cur = nlists;
    if (extra) { cur = (cur + 1) / 2; plan[cnt++] = cur; }
    for (int l = 1; l < levels; ++l) { cur = (cur + per_max - 1) / per_max; plan[cnt++] = cur; }
    plan[cnt++] = p_final > 0 ? p_final : ((cur + per_max - 1) / per_max > 1 ? (cur + per_max - 1) / per_max : 1);
    return cnt;
}

}  // namespace icd
