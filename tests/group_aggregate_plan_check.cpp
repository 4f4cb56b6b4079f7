// group_aggregate_plan_check.cpp - host check of rag_project_icd10_amd/csrc/group_aggregate_plan.hpp, built
// with -fsanitize=address,undefined and run by tests/test_group_scorer_cpu.py. The plan decides which positions a wave of
// group_aggregate_pack_kernel / group_aggregate_long_kernel reads and which cell of `best` it writes, so: every position lies in
// exactly one pack or long item, no pack exceeds 64 positions or splits a group, the long items are exactly the runs above 64 -
// on the edge shapes by hand and on seeded random groupings. The marks live in a heap array of EXACTLY n entries: a pack that
// reaches past the last position is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "group_aggregate_plan.hpp"

using namespace icd;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// seg from run lengths
static std::vector<int> seg_of(const std::vector<int> &runs) {
    std::vector<int> seg(1, 0);
    for (int r : runs) seg.push_back(seg.back() + r);
    return seg;
}

static GaPlan check(const std::vector<int> &runs) {
    const std::vector<int> seg = seg_of(runs);
    const int G = (int)runs.size(), n = seg.back();
    const GaPlan plan = ga_plan(seg.data(), G);
    std::vector<int> covered((size_t)n, 0), group_done((size_t)G, 0), start_group((size_t)n + 1, -1);
    for (int g = 0; g <= G; ++g) start_group[(size_t)seg[(size_t)g]] = g;   // (groups are non-empty: the starts are distinct)
    int prev_end = 0;
    for (const GaPack &pk : plan.packs) {
        CHECK(pk.len >= 1 && pk.len <= GA_PACK);
        CHECK(pk.p0 >= prev_end && pk.p0 + pk.len <= n);   // ascending, in bounds
        prev_end = pk.p0 + pk.len;
        // starts and ends on group boundaries, and every group inside is a short one
        CHECK(start_group[(size_t)pk.p0] >= 0 && start_group[(size_t)(pk.p0 + pk.len)] >= 0);
        for (int g = start_group[(size_t)pk.p0]; g < start_group[(size_t)(pk.p0 + pk.len)]; ++g) {
            CHECK(runs[(size_t)g] <= GA_PACK);
            ++group_done[(size_t)g];
        }
        for (int p = pk.p0; p < pk.p0 + pk.len; ++p) ++covered[(size_t)p];
    }
    int prev_g = -1;
    for (int g : plan.long_groups) {
        CHECK(g > prev_g && g < G);
        prev_g = g;
        CHECK(runs[(size_t)g] > GA_PACK);
        ++group_done[(size_t)g];
        for (int p = seg[(size_t)g]; p < seg[(size_t)g + 1]; ++p) ++covered[(size_t)p];
    }
    for (int p = 0; p < n; ++p) CHECK(covered[(size_t)p] == 1);
    int nlong = 0;
    for (int g = 0; g < G; ++g) {
        CHECK(group_done[(size_t)g] == 1);
        nlong += runs[(size_t)g] > GA_PACK ? 1 : 0;
    }
    CHECK((int)plan.long_groups.size() == nlong);
    CHECK(plan.bytes() == plan.packs.size() * 8 + plan.long_groups.size() * 4);
    // greedy: two neighbouring packs with no long group between them could not have been one
    for (size_t i = 0; i + 1 < plan.packs.size(); ++i) {
        const GaPack &a = plan.packs[i], &b = plan.packs[i + 1];
        if (a.p0 + a.len != b.p0) continue;
        const int g = start_group[(size_t)b.p0];
        CHECK(a.len + runs[(size_t)g] > GA_PACK);
    }
    return plan;
}

int main() {
    {   // n = 1
        const GaPlan p = check({1});
        CHECK(p.packs.size() == 1 && p.packs[0].p0 == 0 && p.packs[0].len == 1 && p.long_groups.empty());
    }
    {   // one group: short, exactly a pack, one more than a pack, long
        CHECK(check({63}).packs.size() == 1);
        const GaPlan p64 = check({64});
        CHECK(p64.packs.size() == 1 && p64.packs[0].len == 64 && p64.long_groups.empty());
        const GaPlan p65 = check({65});
        CHECK(p65.packs.empty() && p65.long_groups.size() == 1 && p65.long_groups[0] == 0);
        CHECK(check({1000}).long_groups.size() == 1);
    }
    {   // all singletons: full packs and a rest
        const GaPlan p = check(std::vector<int>(1000, 1));
        CHECK(p.packs.size() == 16 && p.packs[0].len == 64 && p.packs[15].len == 1000 - 15 * 64 && p.long_groups.empty());
        CHECK(check(std::vector<int>(64, 1)).packs.size() == 1);
        CHECK(check(std::vector<int>(65, 1)).packs.size() == 2);
    }
    {   // a run of 64 followed by a run of 1: the single row gets a pack of its own
        const GaPlan p = check({64, 1});
        CHECK(p.packs.size() == 2 && p.packs[0].len == 64 && p.packs[1].p0 == 64 && p.packs[1].len == 1);
        const GaPlan r = check({1, 64});
        CHECK(r.packs.size() == 2 && r.packs[0].len == 1 && r.packs[1].p0 == 1 && r.packs[1].len == 64);
        const GaPlan s = check({63, 1, 1});
        CHECK(s.packs.size() == 2 && s.packs[0].len == 64 && s.packs[1].len == 1);
    }
    {   // long groups cut the packs: singletons, 200, singletons, 600, singletons
        std::vector<int> runs(10, 1);
        runs.push_back(200);
        runs.insert(runs.end(), 70, 1);
        runs.push_back(600);
        runs.insert(runs.end(), 3, 1);
        const GaPlan p = check(runs);
        CHECK(p.long_groups.size() == 2 && p.long_groups[0] == 10 && p.long_groups[1] == 81);
        CHECK(p.packs.size() == 4 && p.packs[0].len == 10 && p.packs[1].len == 64 && p.packs[2].len == 6 && p.packs[3].len == 3);
        CHECK(check({65, 65, 65}).packs.empty());
        CHECK(check({65, 1, 65}).packs.size() == 1);
    }
    // seeded random groupings: run lengths 1 - 70, then mostly short with a few very long
    unsigned long long state = 88172645463325252ull;
    auto next = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
    for (int trial = 0; trial < 200; ++trial) {
        std::vector<int> runs;
        const int G = 1 + (int)(next() % 300);
        for (int g = 0; g < G; ++g) {
            const unsigned long long r = next();
            runs.push_back(trial % 2 ? 1 + (int)(r % 70) : (r % 50 == 0 ? 65 + (int)((r >> 8) % 2000) : 1 + (int)((r >> 8) % 20)));
        }
        check(runs);
    }
    CHECK(ga_pack_blocks(0, 5) == 0 && ga_pack_blocks(1, 1) == 1 && ga_pack_blocks(3, 5) == 2 && ga_pack_blocks(16, 512) == 512);
    CHECK(ga_long_blocks(0, 7) == 0 && ga_long_blocks(1, 1) == 1 && ga_long_blocks(3, 3) == 3);
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("group aggregate plan ok\n");
    return 0;
}
