// maxsim_plan_check.cpp - host check of rag_project_icd10_amd/csrc/maxsim_plan.hpp, built with
// -fsanitize=address,undefined and run by tests/test_maxsim_cpu.py. The plan decides which rows of `best` a lane of
// maxsim_reduce_kernel walks and which rows of the outputs a wave of maxsim_finish_kernel writes, so: every vector and every list
// lies in exactly one pass, no pass exceeds the score block or splits a list, a pass ends only in front of a list that no longer
// fits, the launches of a pass cover its lists once with offsets inside the pass - on the edge shapes by hand and on seeded random
// batches. The marks live in heap arrays of EXACTLY as many entries as there are vectors and lists: a pass that reaches past the
// end is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "maxsim_plan.hpp"

using namespace icd;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static std::vector<int64_t> off_of(const std::vector<int> &sizes) {
    std::vector<int64_t> off(1, 0);
    for (int t : sizes) off.push_back(off.back() + t);
    return off;
}

static std::vector<MaxsimPass> check(const std::vector<int> &sizes, int B) {
    const std::vector<int64_t> off = off_of(sizes);
    const int64_t nl = (int64_t)sizes.size(), nv = off.back();
    std::vector<MaxsimPass> passes;
    CHECK(maxsim_plan(off.data(), nl, B, passes));
    std::vector<int> vec_seen((size_t)nv, 0), list_seen((size_t)nl, 0);
    int64_t next_v = 0, next_l = 0;
    for (size_t pi = 0; pi < passes.size(); ++pi) {
        const MaxsimPass &p = passes[pi];
        CHECK(p.v0 == next_v && p.l0 == next_l);                     // in order, nothing skipped
        CHECK(p.nv >= 1 && p.nv <= B && p.nl >= 1);
        CHECK((int)p.off.size() == p.nl + 1 && p.off[0] == 0 && p.off[(size_t)p.nl] == p.nv);
        CHECK(p.v0 + p.nv <= nv && p.l0 + p.nl <= nl);
        if (p.v0 + p.nv > nv || p.l0 + p.nl > nl) break;
        for (int i = 0; i < p.nl; ++i) {                             // whole lists, at their own offsets
            CHECK(p.v0 + p.off[(size_t)i] == off[(size_t)(p.l0 + i)] && p.v0 + p.off[(size_t)i + 1] == off[(size_t)(p.l0 + i) + 1]);
            ++list_seen[(size_t)(p.l0 + i)];
        }
        for (int v = 0; v < p.nv; ++v) ++vec_seen[(size_t)(p.v0 + v)];
        if (p.l0 + p.nl < nl) CHECK(p.nv + sizes[(size_t)(p.l0 + p.nl)] > B);     // greedy: the next list did not fit
        // the launches: consecutive, at most MAXSIM_LAUNCH_LISTS lists each, the pass's offsets
        int covered = 0;
        CHECK(p.launches() == (p.nl + MAXSIM_LAUNCH_LISTS - 1) / MAXSIM_LAUNCH_LISTS);
        for (int i = 0; i < p.launches(); ++i) {
            const MaxsimLists m = p.launch(i);
            CHECK(m.first == covered && m.n >= 1 && m.n <= MAXSIM_LAUNCH_LISTS && m.first + m.n <= p.nl);
            for (int j = 0; j <= m.n && m.first + j <= p.nl; ++j) CHECK(m.off[j] == p.off[(size_t)(m.first + j)]);
            covered += m.n;
        }
        CHECK(covered == p.nl);
        next_v += p.nv;
        next_l += p.nl;
    }
    CHECK(next_v == nv && next_l == nl);
    for (int64_t v = 0; v < nv; ++v) CHECK(vec_seen[(size_t)v] == 1);
    for (int64_t l = 0; l < nl; ++l) CHECK(list_seen[(size_t)l] == 1);
    return passes;
}

int main() {
    const int B = 512;
    {   // one list: of one vector, of 64
        const auto p = check({1}, B);
        CHECK(p.size() == 1 && p[0].nv == 1 && p[0].nl == 1);
        const auto q = check({64}, B);
        CHECK(q.size() == 1 && q[0].nv == 64);
        CHECK(check({64}, 64).size() == 1);                          // a block of exactly one full list
    }
    {   // lists that end exactly at B, at B - 1 and at B + 1
        const auto e = check(std::vector<int>(8, 64), B);
        CHECK(e.size() == 1 && e[0].nv == B && e[0].nl == 8);
        std::vector<int> m(7, 64);
        m.push_back(63);
        const auto f = check(m, B);
        CHECK(f.size() == 1 && f[0].nv == B - 1);
        m.push_back(1);                                              // ... and one more vector fills the block
        CHECK(check(m, B).size() == 1);
        m.push_back(1);                                              // ... and the next one opens a pass
        const auto g = check(m, B);
        CHECK(g.size() == 2 && g[0].nv == B && g[1].nv == 1 && g[1].v0 == B && g[1].l0 == 9);
        std::vector<int> o(7, 64);
        o.push_back(63);
        o.push_back(2);                                              // would end at B + 1: moves to the next pass whole
        const auto h = check(o, B);
        CHECK(h.size() == 2 && h[0].nv == B - 1 && h[1].nv == 2 && h[1].v0 == B - 1);
    }
    {   // a list of 64 that does not fit the remainder
        std::vector<int> s(7, 64);
        s.push_back(1);
        s.push_back(64);
        s.push_back(3);
        const auto p = check(s, B);
        CHECK(p.size() == 2 && p[0].nv == 449 && p[0].nl == 8 && p[1].nv == 67 && p[1].nl == 2 && p[1].off[1] == 64);
    }
    {   // 512 lists of one vector: one pass, four launches; 513: two passes
        const auto p = check(std::vector<int>(512, 1), B);
        CHECK(p.size() == 1 && p[0].launches() == 4 && p[0].launch(3).first == 384 && p[0].launch(3).n == 128);
        const auto q = check(std::vector<int>(513, 1), B);
        CHECK(q.size() == 2 && q[1].nl == 1 && q[1].launches() == 1);
        const auto r = check(std::vector<int>(129, 1), B);
        CHECK(r.size() == 1 && r[0].launches() == 2 && r[0].launch(1).n == 1 && r[0].launch(1).off[0] == 128 && r[0].launch(1).off[1] == 129);
    }
    {   // refused: empty input, a null table, an empty list, a list above 64 or above the block, offsets that do not start at 0
        std::vector<MaxsimPass> out(3);
        const int64_t zero[1] = {0};
        CHECK(!maxsim_plan(zero, 0, B, out) && out.empty());
        CHECK(!maxsim_plan(nullptr, 1, B, out));
        const int64_t empty_list[3] = {0, 0, 4};
        CHECK(!maxsim_plan(empty_list, 2, B, out));
        const int64_t down[3] = {0, 5, 3};
        CHECK(!maxsim_plan(down, 2, B, out));
        const int64_t big[2] = {0, 65};
        CHECK(!maxsim_plan(big, 1, B, out));
        const int64_t wide[2] = {0, 40};
        CHECK(!maxsim_plan(wide, 1, 32, out) && maxsim_plan(wide, 1, 40, out));
        const int64_t late[2] = {1, 3};
        CHECK(!maxsim_plan(late, 1, B, out));
        CHECK(!maxsim_plan(zero, 1, 0, out));
    }
    // seeded random batches: sizes 1 - 64, mostly short, at several block sizes
    unsigned long long state = 88172645463325252ull;
    auto next = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
    for (int trial = 0; trial < 300; ++trial) {
        std::vector<int> sizes;
        const int nl = 1 + (int)(next() % 700);
        for (int l = 0; l < nl; ++l) {
            const unsigned long long r = next();
            sizes.push_back(trial % 3 == 0 ? 1 + (int)(r % 64) : (r % 9 == 0 ? 64 - (int)((r >> 8) % 3) : 1 + (int)((r >> 8) % 6)));
        }
        const int blocks[4] = {128, 256, 384, 512};
        check(sizes, blocks[trial % 4]);
    }
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("maxsim plan ok\n");
    return 0;
}
