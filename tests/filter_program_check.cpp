// Checker for rag_project_icd10_amd/csrc/filter_program.hpp (host only; built by tests/test_filter_device_cpu.py with g++ and
// -fsanitize=address,undefined). Walks well-formed programs at the limits, the malformed streams of the Python test, and random
// word streams from a fixed seed: the checker must answer every one of them without reading outside the stream (every stream sits
// in a heap block of exactly its size, so a read past the end is an ASan report).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "filter_program.hpp"

using namespace icd;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++fails; } } while (0)

typedef std::vector<uint32_t> Words;

// one program in a heap block of exactly its size (and one behind a good program)
static int check_one(const Words &w, int64_t ncols, int64_t vocab, char *msg, size_t msg_len) {
    uint32_t *exact = w.empty() ? nullptr : new uint32_t[w.size()];
    if (!w.empty()) memcpy(exact, w.data(), w.size() * sizeof(uint32_t));
    const int64_t off[2] = {0, (int64_t)w.size()};
    const int rc = filter_check_programs(off, exact, 1, ncols, vocab, msg, msg_len);
    delete[] exact;
    return rc;
}

static void refused(const char *name, const Words &w) {
    char msg[200] = "";
    EXPECT(check_one(w, 8, 100, msg, sizeof msg) == FILTER_BAD);
    if (!msg[0]) { printf("FAILED: %s gave no message\n", name); ++fails; }
    Words two = {FOP_RANGE, 0, 0, 1};
    two.insert(two.end(), w.begin(), w.end());
    const int64_t off[3] = {0, 4, (int64_t)two.size()};
    EXPECT(filter_check_programs(off, two.data(), 2, 8, 100, msg, sizeof msg) == FILTER_BAD);
}

static Words repeat(const Words &unit, int times, const Words &tail = {}) {
    Words out;
    for (int i = 0; i < times; ++i) out.insert(out.end(), unit.begin(), unit.end());
    out.insert(out.end(), tail.begin(), tail.end());
    return out;
}

int main() {
    const uint32_t R = FOP_RANGE, S = FOP_SET, T = FOP_TEXT, AND = FOP_AND, OR = FOP_OR, NOT = FOP_NOT;
    char msg[200] = "";
    // well-formed, at the limits
    Words full = {S | 64u << 8, 7};
    for (uint32_t i = 0; i < 64; ++i) full.push_back(i);
    full.push_back(T | 64u << 8 | 64u << 16);
    for (uint32_t i = 36; i < 100; ++i) full.push_back(i);
    full.push_back(AND); full.push_back(NOT);
    EXPECT(check_one(full, 8, 100, msg, sizeof msg) == FILTER_OK && msg[0] == 0);
    Words deep = repeat({R, 0, 0x80000000u, 0x7FFFFFFFu}, 8, repeat({AND}, 7));
    const Words second = repeat({R, 1, 5, 5}, 7, repeat({OR}, 7, {R, 2, 0, 9, OR}));
    deep.insert(deep.end(), second.begin(), second.end());
    EXPECT(check_one(deep, 8, 100, msg, sizeof msg) == FILTER_OK);
    EXPECT(check_one({S, 0}, 1, 0, msg, sizeof msg) == FILTER_OK);                       // the empty set, no vocabulary
    EXPECT(check_one({S | 2u << 8, 0, 0x80000000u, 0x7FFFFFFFu}, 1, 0, msg, sizeof msg) == FILTER_OK);   // INT32_MIN < INT32_MAX
    bool any_text = false;
    {
        const int64_t off[3] = {0, 4, 4 + (int64_t)full.size()};
        Words two = {R, 0, 0, 1};
        two.insert(two.end(), full.begin(), full.end());
        EXPECT(filter_check_programs(off, two.data(), 2, 8, 100, msg, sizeof msg, &any_text) == FILTER_OK && any_text);
        EXPECT(filter_check_programs(off, two.data(), 1, 8, 100, msg, sizeof msg, &any_text) == FILTER_OK && !any_text);
        EXPECT(filter_check_programs(off, two.data(), 2, 8, 0, msg, sizeof msg) == FILTER_BAD);   // a TEXT leaf without a vocabulary
        EXPECT(filter_check_programs(off, two.data(), 2, 8, 100, nullptr, 0) == FILTER_OK);        // no message buffer
        EXPECT(filter_check_programs(off, two.data(), 2, 7, 100, nullptr, 0) == FILTER_BAD);
        EXPECT(filter_check_programs(off, two.data(), 2, 7, 100, msg, 1) == FILTER_BAD && msg[0] == 0);   // a one-byte buffer
        EXPECT(filter_check_programs(nullptr, nullptr, 1, 8, 100, msg, sizeof msg) == FILTER_BAD);
        EXPECT(filter_check_programs(off, nullptr, 2, 8, 100, msg, sizeof msg) == FILTER_BAD);
        EXPECT(filter_check_programs(off, two.data(), 0, 8, 100, msg, sizeof msg) == FILTER_OK);
        EXPECT(filter_check_programs(off, two.data(), -1, 8, 100, msg, sizeof msg) == FILTER_BAD);
        const int64_t back[3] = {0, 4, 2}, late[2] = {1, 4};
        EXPECT(filter_check_programs(back, two.data(), 2, 8, 100, msg, sizeof msg) == FILTER_BAD);
        EXPECT(filter_check_programs(late, two.data(), 1, 8, 100, msg, sizeof msg) == FILTER_BAD);
    }
    // the malformed streams
    refused("a RANGE cut off", {R, 0, 1});
    refused("a SET cut off", {S | 3u << 8, 0, 1, 2});
    refused("a TEXT cut off", {T | 2u << 8 | 1u << 16, 5});
    refused("AND on one set", {R, 0, 0, 1, AND});
    refused("NOT on none", {NOT});
    refused("a leftover stack", {R, 0, 0, 1, R, 1, 0, 1});
    refused("an empty program", {});
    refused("a column >= ncols", {R, 8, 0, 1});
    refused("a SET column >= ncols", {S | 1u << 8, 9, 1});
    refused("unsorted set ids", {S | 2u << 8, 0, 5, 5});
    refused("set ids unsorted as int32", {S | 2u << 8, 0, 1, 0xFFFFFFFFu});
    refused("a term >= vocab", {T | 1u << 8 | 1u << 16, 100});
    refused("unsorted terms", {T | 2u << 8 | 1u << 16, 7, 3});
    refused("m = 0", {T | 1u << 8, 5});
    refused("m = 65", {T | 1u << 8 | 65u << 16, 5});
    refused("5 TEXT leaves", repeat({T | 1u << 8 | 1u << 16, 5}, 5, repeat({OR}, 4)));
    Words big = {S | 65u << 8, 0};
    for (uint32_t i = 0; i < 65; ++i) big.push_back(i);
    refused("65 set ids", big);
    refused("17 leaves", repeat({R, 0, 0, 1, R, 0, 0, 1, OR}, 8, {R, 0, 0, 1, OR}));
    refused("9 sets on the stack", repeat({R, 0, 0, 1}, 9, repeat({OR}, 8)));
    Words nots = {R, 0, 0, 1};
    nots.insert(nots.end(), 32, NOT);
    refused("33 operations", nots);
    refused("an unknown operation", {7});
    refused("stray bits on a RANGE", {R | 1u << 8, 0, 0, 1});
    refused("stray bits on a NOT", {R, 0, 0, 1, NOT | 1u << 16});
    refused("too long", repeat({R, 0, 0, 1, NOT}, 400));
    // random word streams: raw words, and words biased towards operation codes with small arguments - any answer, no bad read
    int ok = 0;
    for (int round = 0; round < 20000; ++round) {
        Words w(rnd() % 40);
        for (uint32_t &x : w) {
            const uint32_t r = rnd();
            x = (round & 1) ? r : ((r % 7) | ((r >> 8) % 4) << 8 | ((r >> 16) % 3) << 16);
            if ((round & 3) == 2) x = r % 9;
        }
        ok += check_one(w, 1 + rnd() % 8, rnd() % 3 ? 100 : 0, msg, sizeof msg) == FILTER_OK;
    }
    EXPECT(ok > 0 && ok < 20000);   // (the biased streams do hit well-formed programs)
    if (fails) { printf("%d failures\n", fails); return 1; }
    printf("filter program cases ok (%d of 20000 random streams were well-formed)\n", ok);
    return 0;
}
