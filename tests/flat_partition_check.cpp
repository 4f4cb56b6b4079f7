// Checker for rag_project_icd10_amd/csrc/flat_partition.hpp (built by tests/test_flat_partition.py with g++).
// For (query tiles, corpus tiles, units per work-group, list length): walks every work-group's range exactly like
// coarse_flat_kernel does and verifies
//   * every (query tile, corpus tile) unit is covered exactly once,
//   * the lists of a query tile get the ordinals 0, 1, 2, ... in row order, each used once, all below P,
//   * the hardware-block -> work-group map is a bijection for every class period.
// Then the list plan of both coarse passes (plan_coarse_lists) over realistic shard shapes, up to the rows a shard can hold
// in HBM: every list of every plan lies inside the reach of the kernel's per-list buffer descriptor; the plans of the
// measured shapes are pinned. `flat_partition_check plan N DIM NQ K [WIDE_NOW [MAX_LIST_TILES]]` prints one plan as JSON.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "flat_partition.hpp"

using namespace icd;

static int check(int mtc, int ctiles, int U, int L) {
    const long long total = (long long)mtc * ctiles;
    const int G = (int)((total + U - 1) / U);
    int P = 0;
    for (int m = 0; m < mtc; ++m) {
        const long long m1 = (long long)(m + 1) * ctiles;
        const int wl = (int)((m1 - 1) / U);
        const int p = flat_first_ordinal(m, wl + 1, ctiles, U, L);
        if (p > P) P = p;
    }
    std::vector<int> covered((size_t)total, 0);
    std::vector<std::vector<int>> ord_first((size_t)mtc);   // [mtile][ordinal] = first tile of that list
    for (int m = 0; m < mtc; ++m) ord_first[m].assign((size_t)P, -1);
    for (int w = 0; w < G; ++w) {
        const long long u_begin = (long long)w * U, u_end = u_begin + U < total ? u_begin + U : total;
        long long u = u_begin;
        while (u < u_end) {
            const int mtile = (int)(u / ctiles), t0 = (int)(u - (long long)mtile * ctiles);
            const long long mb = (long long)mtile * ctiles;
            const int run0 = (int)(u_begin > mb ? u_begin - mb : 0);
            const int run1 = (int)(u_end - mb < ctiles ? u_end - mb : ctiles);
            const int j = (t0 - run0) / L;
            const int t1 = run1 < run0 + (j + 1) * L ? run1 : run0 + (j + 1) * L;
            const int ord = flat_first_ordinal(mtile, w, ctiles, U, L) + j;
            if (ord < 0 || ord >= P) { printf("ordinal %d out of range P=%d (m=%d w=%d)\n", ord, P, mtile, w); return 1; }
            if (ord_first[mtile][ord] != -1) { printf("ordinal %d used twice (m=%d)\n", ord, mtile); return 1; }
            ord_first[mtile][ord] = t0;
            if (t1 <= t0) { printf("empty list (m=%d w=%d)\n", mtile, w); return 1; }
            for (int t = t0; t < t1; ++t) covered[(size_t)(mb + t)] += 1;
            u += t1 - t0;
        }
    }
    for (long long i = 0; i < total; ++i)
        if (covered[(size_t)i] != 1) { printf("unit %lld covered %d times\n", i, covered[(size_t)i]); return 1; }
    for (int m = 0; m < mtc; ++m) {   // ordinals are dense and in row order
        int prev = -1;
        bool ended = false;
        for (int o = 0; o < P; ++o) {
            const int f = ord_first[m][o];
            if (f == -1) { ended = true; continue; }
            if (ended || f <= prev) { printf("ordinals of query tile %d not dense / not in row order\n", m); return 1; }
            prev = f;
        }
        if (ord_first[m][0] != 0) { printf("query tile %d: first list does not start at tile 0\n", m); return 1; }
    }
    return 0;
}

// ---- the coarse list plan at a search shape, with the launcher's inputs (icd_search.hip search_device) ----------------
// (restated here: the kernel-side constants coarse_common.hpp / finalize.hpp hold and the launcher's defaults)
constexpr int NUM_CU = 256;          // MI355X
constexpr int KP = 16, KP_WIDE = 24; // CO_KP, CO_KP_WIDE
constexpr int MAX_CAND = 512;        // FIN_MAX_CAND
constexpr int FAST_MAX_K = 100;
constexpr int WIDE_FROM = 48;        // icd_index opt_wide_from: k above it keeps KP_WIDE per list (dim 768)
constexpr long long HBM_BYTES = 288LL << 30;

struct Shape { long long n; int dim, nq, k, max_nq, max_k, wide_now, pass2; };
struct Full { FlatPlan fp; CoarsePlan cp; int mtc; };

static Full plan_at(const Shape &s, int max_list_tiles) {
    Full f{};
    const int nq_pad = (s.nq + 127) / 128 * 128, max_nq_pad = (s.max_nq + 127) / 128 * 128;
    f.mtc = nq_pad / 128;
    const int ctiles_min = (int)((s.n + 127) / 128);
    static std::map<std::pair<int, int>, FlatPlan> memo;   // (the sweep asks for the same tile plan at every k)
    const auto key = std::make_pair(f.mtc, ctiles_min);
    auto it = memo.find(key);
    if (it == memo.end()) it = memo.emplace(key, plan_flat_tiles(f.mtc, ctiles_min, FLAT_SPARE_TILES, NUM_CU)).first;
    f.fp = it->second;
    const bool wide_lists = s.k > WIDE_FROM && s.dim == 768;
    CoarsePlanIn in{};
    in.mtc = f.mtc; in.ctiles = f.fp.ctiles; in.U = f.fp.U; in.nq = s.nq; in.k = s.k;
    in.kp = wide_lists ? KP_WIDE : KP; in.kp2 = KP; in.max_cand = MAX_CAND;
    in.wide_lists = wide_lists; in.wide_now = s.wide_now; in.pass2 = s.pass2;
    in.partc_cap = coarse_partc_entries(max_nq_pad, s.max_k < FAST_MAX_K ? s.max_k : FAST_MAX_K, KP, KP_WIDE, MAX_CAND);
    in.part2_cap = coarse_part2_entries(max_nq_pad, KP);
    in.max_list_tiles = max_list_tiles;
    f.cp = plan_coarse_lists(in);
    return f;
}

// Walks every list of a pass exactly like coarse_flat_kernel (without a per-unit array: shards of tens of millions of rows)
// and checks: the lists of a query tile get the ordinals 0 .. in row order, below P, and chain into [0, ctiles) without gap
// or overlap; each list's tiles lie inside num_records of the descriptor based at its first tile; the soffset of every
// stage the ring issues (up to one tile past the list, clamped to the last tile) stays below 2^32. *longest: tiles of the
// longest list seen (up to the first error). Returns 0 or an error text.
static const char *walk_lists(int mtc, int ctiles, int U, int L, int P, int dim, int *longest) {
    static char err[256];
    const long long tile_bytes = (long long)FLAT_TILE_ROWS * dim * 2, total = (long long)mtc * ctiles;
    const long long G = (total + U - 1) / U;
    std::vector<int> first((size_t)P), end((size_t)P);
    int cur_m = -1, base_m = -1, base = 0;   // (base: ordinal of the first list of work-group base_w's run in query tile base_m)
    long long base_w = -1;
    *longest = 0;
    auto close_tile = [&](int m) -> const char * {
        int expect = 0;
        for (int o = 0; o < P; ++o) {
            if (first[(size_t)o] == -1) { for (int r = o; r < P; ++r) if (first[(size_t)r] != -1) { snprintf(err, sizeof err, "query tile %d: ordinals not dense", m); return err; } break; }
            if (first[(size_t)o] != expect) { snprintf(err, sizeof err, "query tile %d: list %d starts at tile %d, not %d", m, o, first[(size_t)o], expect); return err; }
            expect = end[(size_t)o];
        }
        if (expect != ctiles) { snprintf(err, sizeof err, "query tile %d: lists end at tile %d of %d", m, expect, ctiles); return err; }
        return nullptr;
    };
    for (long long w = 0; w < G; ++w) {
        const long long u_begin = w * U, u_end = u_begin + U < total ? u_begin + U : total;
        long long u = u_begin;
        while (u < u_end) {
            const int mtile = (int)(u / ctiles), t0 = (int)(u - (long long)mtile * ctiles);
            if (mtile != cur_m) {   // work-groups run in unit order: a query tile's lists are all seen before the next one's
                if (cur_m >= 0) if (const char *e = close_tile(cur_m)) return e;
                std::fill(first.begin(), first.end(), -1);
                cur_m = mtile;
            }
            const long long mb = (long long)mtile * ctiles;
            const int run0 = (int)(u_begin > mb ? u_begin - mb : 0);
            const int run1 = (int)(u_end - mb < ctiles ? u_end - mb : ctiles);
            const int j = (t0 - run0) / L;
            const int t1 = run1 < run0 + (j + 1) * L ? run1 : run0 + (j + 1) * L;
            if (mtile != base_m || w != base_w) { base = flat_first_ordinal(mtile, (int)w, ctiles, U, L); base_m = mtile; base_w = w; }
            const int ord = base + j;
            if (t1 <= t0) { snprintf(err, sizeof err, "empty list (m=%d w=%lld)", mtile, w); return err; }
            if (ord < 0 || ord >= P || first[(size_t)ord] != -1) { snprintf(err, sizeof err, "ordinal %d out of range or reused (P=%d m=%d)", ord, P, mtile); return err; }
            first[(size_t)ord] = t0; end[(size_t)ord] = t1;
            const long long ntiles = t1 - t0;
            const long long num_records = std::min((long long)(ctiles - t0) * tile_bytes, FLAT_DESC_MAX_BYTES);
            const long long issued = std::min(ntiles, (long long)(ctiles - 1 - t0)) + 1;   // tiles the ring touches
            if (ntiles > *longest) *longest = (int)ntiles;
            if (ntiles * tile_bytes > num_records || issued * tile_bytes > (1LL << 32)) {
                snprintf(err, sizeof err, "list of %lld tiles (%.2f GiB) at tile %d beyond the descriptor's reach (dim %d)", ntiles,
                         (double)(ntiles * tile_bytes) / (1 << 30), t0, dim);
                return err;
            }
            u += ntiles;
        }
    }
    return cur_m >= 0 ? close_tile(cur_m) : nullptr;
}

// both passes of a plan; 0 or an error text
static const char *check_plan(const Shape &s, const Full &f, int *longest) {
    const char *e = walk_lists(f.mtc, f.fp.ctiles, f.cp.U, f.cp.list_tiles, f.cp.P, s.dim, longest);
    if (e || f.cp.P2 == 0) return e;
    int l2 = 0;
    e = walk_lists(f.mtc, f.fp.ctiles, f.cp.U2, f.cp.list_tiles2, f.cp.P2, s.dim, &l2);
    if (l2 > *longest) *longest = l2;
    return e;
}

static int print_plan(int argc, char **argv) {
    if (argc < 6) { printf("usage: %s plan N DIM NQ K [WIDE_NOW [MAX_LIST_TILES (-1: uncapped)]]\n", argv[0]); return 2; }
    Shape s{atoll(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), 0, 0, argc > 6 ? atoi(argv[6]) : 0, 1};
    s.max_nq = s.nq; s.max_k = s.k > 10 ? s.k : 10;
    const int cap = argc > 7 && atoi(argv[7]) >= 0 ? atoi(argv[7]) : (argc > 7 ? INT_MAX : flat_max_list_tiles(s.dim));
    const Full f = plan_at(s, cap);
    int longest = 0;
    const char *e = f.cp.ok ? check_plan(s, f, &longest) : "no plan";
    printf("{\"ok\": %d, \"ctiles\": %d, \"U\": %d, \"list_tiles\": %d, \"P\": %d, \"U2\": %d, \"list_tiles2\": %d, \"P2\": %d, "
           "\"max_list_tiles\": %d, \"longest_list_tiles\": %d, \"longest_list_bytes\": %lld, \"in_reach\": %d, \"error\": \"%s\"}\n",
           f.cp.ok, f.fp.ctiles, f.cp.U, f.cp.list_tiles, f.cp.P, f.cp.U2, f.cp.list_tiles2, f.cp.P2, flat_max_list_tiles(s.dim), longest,
           (long long)longest * FLAT_TILE_ROWS * s.dim * 2, e ? 0 : 1, e ? e : "");
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "plan")) return print_plan(argc, argv);
    int cases = 0;
    const int mtcs[] = {1, 2, 8, 79, 128}, cts[] = {1, 2, 32, 290, 317, 1000};
    for (int mtc : mtcs)
        for (int ct : cts)
            for (int U : {1, 2, 3, 12, 90, 97, 145, 290, 500, 4883})
                for (int L : {1, 5, 24, 145, 290, 100000}) {
                    if (check(mtc, ct, U, L)) { printf("FAILED at mtc=%d ctiles=%d U=%d L=%d\n", mtc, ct, U, L); return 1; }
                    ++cases;
                }
    for (int G : {1, 7, 8, 9, 64, 255, 256, 300})   // block -> work-group map: a bijection
        for (int T : {0, 1, 2, 3, 29, 58, 290, 1 << 30}) {
            std::vector<int> seen((size_t)G, 0);
            for (int w = 0; w < G; ++w) {
                const int l = flat_workgroup_of_block(w, G, T);
                if (l < 0 || l >= G || seen[(size_t)l]++) { printf("not a bijection: G=%d T=%d w=%d -> %d\n", G, T, w, l); return 1; }
            }
            ++cases;
        }
    // reduction plan of the streaming kernel's per-wave lists: odd number of levels (the levels ping-pong between two
    // workspaces and finalize reads the second), fan-in <= per_max at every level, the requested final list count (or as few
    // as possible), at most 512 lists after the first of several levels (workspace sizing)
    for (int m : {32, 8, 4})
        for (int pf : {0, m})
            for (int n = 1; n <= 1024; ++n) {
                int plan[8];
                const int c = plan_reduce_levels(n, m, pf, m, plan);
                bool ok = c > 0 && c <= 8 && c % 2 == 1;
                int cur = n;
                for (int i = 0; i < c && ok; ++i) {
                    const int per = (cur + plan[i] - 1) / plan[i];
                    if (per > m || plan[i] < 1 || (i == 0 && c > 1 && plan[0] > 512)) ok = false;
                    cur = plan[i];
                }
                if (ok && pf > 0 && plan[c - 1] != pf) ok = false;
                if (ok && pf == 0 && plan[c - 1] > m) ok = false;
                if (!ok) { printf("bad reduction plan: nlists=%d per_max=%d p_final=%d\n", n, m, pf); return 1; }
                ++cases;
            }
    // tile planner: U never below the balanced minimum nor more than ~6 % (+1) above it, the swept tile count inside the
    // allocation, the class period consistent with gcd; the planned partition itself is a valid one; the two measured cases
    for (int mtc : {1, 2, 3, 8, 40, 79, 128, 782, 977})
        for (int ct : {1, 2, 3, 33, 100, 289, 290, 317, 320, 1000, 9766, 78125})
            for (int spare : {0, 7})
                for (int cus : {1, 8, 256}) {
                    const FlatPlan p = plan_flat_tiles(mtc, ct, spare, cus);
                    const long long units = (long long)mtc * p.ctiles;
                    const long long umin = (units + cus - 1) / cus > 1 ? (units + cus - 1) / cus : 1;
                    bool ok = p.ctiles >= ct && p.ctiles <= ct + spare && p.U >= umin && p.U <= umin + (umin / 16 > 1 ? umin / 16 : 1);
                    const int T = flat_class_period(p.U, p.ctiles);
                    ok = ok && T >= 1 && p.ctiles % T == 0 && ((long long)p.U * T) % p.ctiles == 0;
                    if (!ok) { printf("bad tile plan: mtc=%d ctiles=%d spare=%d cus=%d -> ctiles=%d U=%d\n", mtc, ct, spare, cus, p.ctiles, p.U); return 1; }
                    if (units <= 400000 && check(mtc, p.ctiles, p.U, (p.ctiles + 1) / 2)) { printf("planned partition invalid\n"); return 1; }
                    ++cases;
                }
    {
        const FlatPlan a = plan_flat_tiles(79, 290, 7, 256), b = plan_flat_tiles(79, 317, 7, 256);
        if (a.ctiles != 290 || a.U != 90 || b.ctiles != 319 || b.U != 99) {
            printf("tile plan changed: 37 000 rows -> (%d, %d), 40 474 rows -> (%d, %d)\n", a.ctiles, a.U, b.ctiles, b.U);
            return 1;
        }
    }
    // ---- the coarse list plan over realistic shard shapes ----------------------------------------------------------
    // rows up to what one shard of dim 768 / 1024 holds in HBM (fp32 rows + the fp16 image: 6 bytes per element), batches up
    // to 100 000 queries, k up to 128, all three plans (narrow, wide mode, the second pass of each)
    int unsupported = 0;
    long long first_unsupported[2][200] = {};
    const long long ns[] = {1, 127, 129, 1000, 37000, 40474, 65536, 1250000, 2100000, 4200000, 5000000, 7000000, 10000000,
                            15000000, 20000000, 25000000, 33000000, 40000000, 46000000, 52000000, 62000000};
    const int nqs[] = {1, 17, 128, 129, 300, 1000, 2048, 10000, 16384, 50000, 100000};
    const int ks[] = {1, 5, 8, 9, 10, 16, 20, 32, 33, 48, 49, 64, 100, 128};
    for (int di = 0; di < 2; ++di) {
        const int dim = di ? 1024 : 768;
        for (long long n : ns) {
            if (n * dim * 6 > HBM_BYTES) continue;
            for (int nq : nqs)
                for (int k : ks)
                    for (int wide_now : {0, 1}) {
                        const Shape sh{n, dim, nq, k, nq, k > 10 ? k : 10, wide_now, 1};
                        const Full f = plan_at(sh, flat_max_list_tiles(dim));
                        ++cases;
                        if (!f.cp.ok) {   // no plan: the search returns ICD_ERR_UNSUPPORTED; record the smallest such shard
                            ++unsupported;
                            if (!first_unsupported[di][k] || n < first_unsupported[di][k]) first_unsupported[di][k] = n;
                            continue;
                        }
                        int longest = 0;
                        if (const char *e = check_plan(sh, f, &longest)) {
                            printf("FAILED plan n=%lld dim=%d nq=%d k=%d wide=%d (ctiles %d U %d list %d P %d / U2 %d P2 %d): %s\n", n, dim, nq, k,
                                   wide_now, f.fp.ctiles, f.cp.U, f.cp.list_tiles, f.cp.P, f.cp.U2, f.cp.P2, e);
                            return 1;
                        }
                        if (f.cp.P > COARSE_MAX_P || f.cp.P2 > PASS2_MAX_P) { printf("plan past its list bounds\n"); return 1; }
                    }
        }
    }
    // every shard of up to 20 M rows has a plan at every batch size and k (a larger one may get ICD_ERR_UNSUPPORTED)
    for (int di = 0; di < 2; ++di)
        for (int k : ks)
            if (first_unsupported[di][k] && first_unsupported[di][k] <= 20000000) {
                printf("no coarse plan for %lld rows at dim %d, k = %d\n", first_unsupported[di][k], di ? 1024 : 768, k);
                return 1;
            }
    // the sweep finds the descriptor bound: the plan without the cap (lists only limited by the corpus) puts a list past it at
    // BASELINE configs[4] on one GPU (10 M x 768 rows, 16 384-query slices, k = 10)
    {
        const Shape sh{10000000, 768, 16384, 10, 16384, 10, 0, 1};
        const Full f = plan_at(sh, INT_MAX);
        int longest = 0;
        if (!f.cp.ok || !check_plan(sh, f, &longest)) { printf("the uncapped plan at 10 M x 768 should leave the descriptor's reach\n"); return 1; }
    }
    // plans of the measured shapes (bench.py legs and the test suite), identical with and without the cap:
    // (n, dim, nq, k, wide mode) -> (ctiles, U, list_tiles, P, U2, P2)
    struct Pin { long long n; int dim, nq, k, wide_now; int ctiles, U, list_tiles, P, U2, P2; };
    const Pin pins[] = {
        {37000, 768, 10000, 10, 0, 290, 90, 96, 5, 15, 20},      // BASELINE configs[1], the headline
        {37000, 768, 10000, 10, 1, 290, 90, 15, 20, 0, 0},       // ... in wide mode (the family leg)
        {37000, 768, 10000, 20, 0, 290, 90, 58, 8, 15, 20},      // the serving path's k = 20
        {37000, 768, 10000, 100, 0, 290, 90, 17, 20, 0, 0},      // k = 100: lists of 24
        {37000, 1024, 10000, 10, 0, 290, 90, 96, 5, 15, 20},     // 1024-d leg
        {40474, 768, 10000, 10, 0, 319, 99, 106, 5, 16, 21},     // the real CSV's size
        {40474, 768, 1000, 10, 0, 320, 10, 106, 32, 0, 0},       // configs[2]'s batch of 1 000 diagnoses
        {40474, 768, 1000, 20, 0, 320, 10, 64, 32, 0, 0},
        {37000, 768, 1000, 10, 0, 290, 10, 96, 29, 0, 0},
        {1250000, 768, 16384, 10, 0, 9766, 4883, 3255, 4, 489, 21},   // configs[4]'s 1.25 M-row shard, 16 384-query slices
        {1250000, 768, 1696, 10, 0, 9768, 555, 3256, 19, 489, 21},    // ... its last slice
        {1250000, 768, 300, 10, 0, 9766, 346, 9766, 29, 0, 0},        // test_config5_shard_size_properties
    };
    for (const Pin &pn : pins) {
        const Shape sh{pn.n, pn.dim, pn.nq, pn.k, pn.nq, pn.k > 10 ? pn.k : 10, pn.wide_now, 1};
        for (int cap : {flat_max_list_tiles(pn.dim), INT_MAX}) {
            const Full f = plan_at(sh, cap);
            if (!f.cp.ok || f.fp.ctiles != pn.ctiles || f.cp.U != pn.U || f.cp.list_tiles != pn.list_tiles || f.cp.P != pn.P ||
                f.cp.U2 != pn.U2 || f.cp.P2 != pn.P2) {
                printf("plan changed at n=%lld dim=%d nq=%d k=%d wide=%d (cap %d): (%d, %d, %d, %d, %d, %d)\n", pn.n, pn.dim, pn.nq, pn.k,
                       pn.wide_now, cap, f.fp.ctiles, f.cp.U, f.cp.list_tiles, f.cp.P, f.cp.U2, f.cp.P2);
                return 1;
            }
        }
        ++cases;
    }
    // the streaming exact kernel's descriptor spans one work-group's fp32 rows: inside num_records for every shard that fits
    // HBM, at dims up to 4096
    for (int dim : {768, 1024, 2048, 4096})
        for (long long n = 1; n * dim * 4 <= HBM_BYTES && n < INT_MAX; n = n * 3 / 2 + 1) {
            const long long a = (long long)stream_rows_per_wg((int)n, NUM_CU) * dim * 4;
            const long long b = (long long)plan_stream_one_rows((int)n, NUM_CU).rows_per_wg * dim * 4;
            if (a > FLAT_DESC_MAX_BYTES || b > FLAT_DESC_MAX_BYTES) { printf("stream descriptor past num_records: n=%lld dim=%d\n", n, dim); return 1; }
            ++cases;
        }
    printf("coarse plans: %d shapes without a plan (largest shards only); smallest such shard at k = 10: %lld rows (768), %lld (1024)\n",
           unsupported, first_unsupported[0][10], first_unsupported[1][10]);
    printf("flat_partition: %d cases ok\n", cases);
    return 0;
}
