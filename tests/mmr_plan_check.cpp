// mmr_plan_check.cpp - the host-visible arithmetic of the MMR select (csrc/mmr_plan.hpp) in a program of its own, built with
// -fsanitize=address,undefined by tests/test_mmr_cpu.py: the value, the pen update and the winner rule against a plain loop that
// is written here from the contract's words, not from the header.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "mmr_plan.hpp"

using namespace icd;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static const double NaN = std::numeric_limits<double>::quiet_NaN();
static const double INF = std::numeric_limits<double>::infinity();

// the contract's words: the unpicked candidate of the greatest value under plain `>`, ties to the lower index (a later equal value
// does not replace); a NaN value never wins; no comparable value: the lowest unpicked index; everything picked: none
static int plain_winner(const std::vector<double> &v, const std::vector<unsigned char> &picked) {
    int best = -1;
    for (int i = 0; i < (int)v.size(); ++i) {
        if (picked[i] || v[i] != v[i]) continue;
        if (best < 0 || v[i] > v[best]) best = i;
    }
    if (best >= 0) return best;
    for (int i = 0; i < (int)v.size(); ++i)
        if (!picked[i]) return i;
    return MMR_NONE;
}

// the same entries folded as the kernel folds them: two per lane, then a butterfly over 64 lanes
static int butterfly_winner(const std::vector<double> &v, const std::vector<unsigned char> &picked) {
    const int C = (int)v.size();
    MmrEntry lane[64];
    for (int l = 0; l < 64; ++l) {
        const int i0 = l, i1 = l + 64;
        MmrEntry e = mmr_entry(i0 < C ? v[i0] : 0.0, i0, i0 >= C || picked[i0]);
        lane[l] = mmr_fold(e, mmr_entry(i1 < C ? v[i1] : 0.0, i1, i1 >= C || picked[i1]));
    }
    for (int m = 1; m < 64; m <<= 1) {
        MmrEntry next[64];
        for (int l = 0; l < 64; ++l) next[l] = mmr_fold(lane[l], lane[l ^ m]);
        std::memcpy(lane, next, sizeof lane);
    }
    for (int l = 1; l < 64; ++l) CHECK(lane[l].idx == lane[0].idx);   // every lane holds the same winner
    return lane[0].idx;
}

static void check_winner(const std::vector<double> &v, const std::vector<unsigned char> &picked, int want) {
    CHECK(plain_winner(v, picked) == want);
    CHECK(mmr_winner(v.data(), picked.data(), (int)v.size()) == want);
    CHECK(butterfly_winner(v, picked) == want);
    // a right-to-left fold: the order of the fold does not matter
    MmrEntry best = mmr_entry(0.0, 0, true);
    for (int i = (int)v.size() - 1; i >= 0; --i) best = mmr_fold(mmr_entry(v[i], i, picked[i] != 0), best);
    CHECK(best.idx == want);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

int main() {
    // ---- the winner rule ----
    check_winner({1.0, 3.0, 3.0, 2.0}, {0, 0, 0, 0}, 1);                 // ties go to the lower index
    check_winner({1.0, 3.0, 3.0, 2.0}, {0, 1, 0, 0}, 2);                 // ... among the unpicked
    check_winner({0.0, -0.0, -0.0}, {1, 0, 0}, 1);                       // +0.0 == -0.0: a tie
    check_winner({-0.0, 0.0}, {0, 0}, 0);
    check_winner({NaN, -5.0, NaN}, {0, 0, 0}, 1);                        // a NaN never wins
    check_winner({NaN, -INF, NaN}, {0, 0, 0}, 1);                        // -inf is comparable
    check_winner({-INF, -INF}, {0, 0}, 0);
    check_winner({INF, INF, 1.0}, {1, 0, 0}, 1);
    check_winner({NaN, NaN, NaN}, {0, 0, 0}, 0);                         // nothing comparable: the lowest unpicked index
    check_winner({NaN, NaN, NaN}, {1, 0, 0}, 1);
    check_winner({NaN, NaN, 7.0}, {0, 0, 1}, 0);                         // (the comparable one is picked)
    check_winner({1.0, 2.0}, {1, 1}, MMR_NONE);
    check_winner({}, {}, MMR_NONE);
    check_winner({4.0}, {0}, 0);
    {   // 128 candidates, the winner in the upper half
        std::vector<double> v(128, 1.0);
        std::vector<unsigned char> p(128, 0);
        v[100] = 2.0; v[127] = 2.0;
        check_winner(v, p, 100);
        p[100] = 1;
        check_winner(v, p, 127);
        p[127] = 1;
        check_winner(v, p, 0);
    }

    // ---- the value: two products and one difference, each rounded once ----
    {
        volatile double a, b, c;
        const double lam = 0.3, om = 1.0 - 0.3;
        const float rel = 0.123456789f, pen = 0.987654321f;
        a = lam * (double)rel; b = om * (double)pen; c = a - b;
        CHECK(mmr_value(lam, om, rel, pen) == c);
        a = lam * (double)rel;
        CHECK(mmr_first_value(lam, rel) == a);
    }
    // lambda = 1: the value IS the relevance (the penalty's product is +-0.0); lambda = 0: minus the penalty
    for (float rel : {0.5f, -0.25f, 0.0f, 1e-40f, -1e-40f})
        for (float pen : {0.75f, -0.5f, 0.0f, -0.0f, 1e-41f}) {
            CHECK(mmr_value(1.0, 1.0 - 1.0, rel, pen) == (double)rel);
            CHECK(mmr_value(0.0, 1.0 - 0.0, rel, pen) == 0.0 * (double)rel - (double)pen);
            CHECK(mmr_value(0.0, 1.0, rel, pen) == -(double)pen);
            CHECK(mmr_first_value(1.0, rel) == (double)rel && mmr_first_value(0.0, rel) == 0.0);
        }
    CHECK(std::isnan(mmr_value(0.0, 1.0, (float)INF, 0.5f)));            // 0 * inf: a NaN value (it never wins)
    CHECK(std::isnan(mmr_value(0.5, 0.5, 1.0f, (float)NaN)));

    // ---- the pen update: plain `s > pen ? s : pen` ----
    CHECK(mmr_pen_update(0.25f, 0.5f) == 0.5f && mmr_pen_update(0.5f, 0.25f) == 0.5f && mmr_pen_update(0.5f, 0.5f) == 0.5f);
    CHECK(mmr_pen_update(0.5f, (float)NaN) == 0.5f);                      // a NaN similarity never replaces
    CHECK(std::isnan(mmr_pen_update((float)NaN, 0.5f)));                  // a NaN penalty stays
    CHECK(std::signbit(mmr_pen_update(-0.0f, 0.0f)) && !std::signbit(mmr_pen_update(0.0f, -0.0f)));   // equal: the old one stays
    CHECK(mmr_pen_update(-(float)INF, -1.0f) == -1.0f);

    // ---- random arrays against the plain loop ----
    for (int round = 0; round < 4000; ++round) {
        const int n = (int)(rnd() % (MMR_MAX_FETCH + 1));
        std::vector<double> v((size_t)n);
        std::vector<unsigned char> p((size_t)n);
        const int kinds = (int)(rnd() % 4);   // few distinct values (ties), NaN-heavy, all picked but a few, anything
        for (int i = 0; i < n; ++i) {
            const uint64_t r = rnd();
            double x = (double)(int)(r % 7) - 3.0;
            if (kinds == 3) x = (double)(int64_t)(r >> 11) / 9007199254740992.0 - 0.5;
            if ((kinds == 1 && (r >> 32) % 3 != 0) || (r >> 40) % 23 == 0) x = NaN;
            if ((r >> 48) % 29 == 0) x = (r >> 60) & 1 ? INF : -INF;
            if ((r >> 52) % 17 == 0) x = -0.0;
            v[(size_t)i] = x;
            p[(size_t)i] = kinds == 2 ? (unsigned char)((r >> 20) % 8 != 0) : (unsigned char)((r >> 20) % 3 == 0);
        }
        check_winner(v, p, plain_winner(v, p));
    }

    // ---- a whole greedy run on a small case, every step against the loop ----
    {
        const int C = 6;
        const float rel[C] = {0.9f, 0.9f, 0.8f, 0.8f, 0.5f, 0.1f};
        const float sim[C][C] = {{1, 1, .2f, .2f, .1f, 0}, {1, 1, .2f, .2f, .1f, 0}, {.2f, .2f, 1, 1, .3f, 0},
                                 {.2f, .2f, 1, 1, .3f, 0}, {.1f, .1f, .3f, .3f, 1, 0}, {0, 0, 0, 0, 0, 1}};
        std::vector<unsigned char> picked(C, 0);
        std::vector<float> pen(C, 0.f);
        std::vector<double> val(C, 0.0);
        std::vector<int> order{0};
        picked[0] = 1;
        for (int t = 1; t < C; ++t) {
            const int last = order.back();
            for (int i = 0; i < C; ++i) {
                if (picked[i]) continue;
                pen[i] = t == 1 ? sim[i][last] : mmr_pen_update(pen[i], sim[i][last]);
                val[i] = mmr_value(0.5, 0.5, rel[i], pen[i]);
            }
            const int w = mmr_winner(val.data(), picked.data(), C);
            CHECK(w == plain_winner(val, picked));
            picked[w] = 1;
            order.push_back(w);
        }
        const int want[C] = {0, 2, 4, 5, 1, 3};   // the tie 2 / 3 goes to 2; the copies (1 of 0, 3 of 2) come last
        for (int t = 0; t < C; ++t) CHECK(order[(size_t)t] == want[t]);
    }

    if (failures) {
        std::printf("mmr plan: %d checks FAILED\n", failures);
        return 1;
    }
    std::printf("mmr plan ok\n");
    return 0;
}
