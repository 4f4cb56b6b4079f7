// filter_program.hpp - host only (no HIP, no handle): the encoding of a filter program and its checker.
// Included by icd_search.hip (icd_filter.hpp), by filter_mask_kernel.hpp (the constants) and by tests/filter_program_check.cpp,
// which runs the checker under the host sanitizers.
//
// One query's filter is a postfix sequence of operations over a stack of row sets; the program of query q is the uint32 words
// prog[prog_off[q] .. prog_off[q + 1]). The first word of an operation holds its kind in bits 0 .. 7:
//
//   FOP_RANGE  { 1,                      col, lo, hi }          push the rows with lo <= column[col][row] < hi (lo, hi: int32 bits;
//                                                               lo >= hi is the empty set)
//   FOP_SET    { 2 | count << 8,         col, ids[count] }      push the rows whose column value is one of ids: int32 bits, strictly
//                                                               increasing as int32, count 0 .. 64 (0: the empty set)
//   FOP_TEXT   { 3 | count << 8 | m << 16, terms[count] }       push the rows that hold at least m of the terms (icd_sparse_match_rowmasks'
//                                                               rules: strictly increasing, below the vocabulary, count 0 .. 64, m 1 .. 64;
//                                                               m above count is the empty set)
//   FOP_AND { 4 }, FOP_OR { 5 }                                 pop two sets, push their intersection / union
//   FOP_NOT { 6 }                                               replace the top set by its complement within the index's rows
//
// Every other bit of a first word is 0. A program holds 1 .. 32 operations, at most 16 leaves (RANGE, SET, TEXT) of which at most
// 4 are TEXT, never more than 8 sets on the stack, never pops an empty stack and ends with exactly one set: the query's mask.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace icd {

enum : uint32_t { FOP_RANGE = 1, FOP_SET = 2, FOP_TEXT = 3, FOP_AND = 4, FOP_OR = 5, FOP_NOT = 6 };
constexpr int FP_MAX_OPS = 32, FP_MAX_LEAVES = 16, FP_MAX_STACK = 8, FP_MAX_TEXT = 4, FP_MAX_SET = 64, FP_MAX_TERMS = 64;

enum { FILTER_OK = 0, FILTER_BAD = -1 };

// `nq` programs against `ncols` columns and a vocabulary of `vocab` terms (0: no sparse index, a TEXT leaf is refused). On a
// violation: FILTER_BAD and its description in msg. *any_text (nullable): a TEXT leaf occurs.
inline int filter_check_programs(const int64_t *prog_off, const uint32_t *prog, int64_t nq, int64_t ncols, int64_t vocab, char *msg,
                                 size_t msg_len, bool *any_text = nullptr) {
    char none[8];
    if (!msg || msg_len == 0) { msg = none; msg_len = sizeof none; }
    msg[0] = 0;
    if (any_text) *any_text = false;
    if (nq < 0 || ncols < 0 || vocab < 0 || vocab > 0xFFFFFFFFll || !prog_off) {
        snprintf(msg, msg_len, "program offsets NULL, nq=%lld, ncols=%lld or vocab=%lld", (long long)nq, (long long)ncols, (long long)vocab);
        return FILTER_BAD;
    }
    if (prog_off[0] != 0) { snprintf(msg, msg_len, "program offsets start at %lld, not 0", (long long)prog_off[0]); return FILTER_BAD; }
    for (int64_t q = 0; q < nq; ++q) {
        const int64_t a = prog_off[q], b = prog_off[q + 1];
        if (b < a) { snprintf(msg, msg_len, "program %lld: offsets decrease", (long long)q); return FILTER_BAD; }
        if (b > a && !prog) { snprintf(msg, msg_len, "prog is NULL"); return FILTER_BAD; }
        // (the longest legal program: 16 leaves of 2 + 64 words and 16 one-word operations)
        if (b - a > FP_MAX_LEAVES * (2 + FP_MAX_SET) + FP_MAX_OPS) { snprintf(msg, msg_len, "program %lld holds %lld words: too long", (long long)q, (long long)(b - a)); return FILTER_BAD; }
        int ops = 0, leaves = 0, texts = 0, depth = 0;
        int64_t p = a;
        while (p < b) {
            const uint32_t w = prog[p];
            const uint32_t op = w & 0xFFu, count = (w >> 8) & 0xFFu, m = w >> 16;
            if (++ops > FP_MAX_OPS) { snprintf(msg, msg_len, "program %lld holds more than %d operations", (long long)q, FP_MAX_OPS); return FILTER_BAD; }
            int64_t len = 1;
            if (op == FOP_RANGE || op == FOP_SET || op == FOP_TEXT) {
                if (++leaves > FP_MAX_LEAVES) { snprintf(msg, msg_len, "program %lld holds more than %d leaves", (long long)q, FP_MAX_LEAVES); return FILTER_BAD; }
                if (op == FOP_RANGE) {
                    if (w != FOP_RANGE) { snprintf(msg, msg_len, "program %lld, word %lld: a RANGE carries no count", (long long)q, (long long)(p - a)); return FILTER_BAD; }
                    len = 4;
                } else if (op == FOP_SET) {
                    if (m != 0 || count > (uint32_t)FP_MAX_SET) { snprintf(msg, msg_len, "program %lld, word %lld: a SET holds 0 .. %d ids", (long long)q, (long long)(p - a), FP_MAX_SET); return FILTER_BAD; }
                    len = 2 + (int64_t)count;
                } else {
                    if (count > (uint32_t)FP_MAX_TERMS) { snprintf(msg, msg_len, "program %lld, word %lld: a TEXT holds 0 .. %d terms", (long long)q, (long long)(p - a), FP_MAX_TERMS); return FILTER_BAD; }
                    if (m < 1 || m > (uint32_t)FP_MAX_TERMS) { snprintf(msg, msg_len, "program %lld, word %lld: min_match=%u outside 1 .. %d", (long long)q, (long long)(p - a), m, FP_MAX_TERMS); return FILTER_BAD; }
                    if (++texts > FP_MAX_TEXT) { snprintf(msg, msg_len, "program %lld holds more than %d TEXT leaves", (long long)q, FP_MAX_TEXT); return FILTER_BAD; }
                    if (vocab < 1) { snprintf(msg, msg_len, "program %lld holds a TEXT leaf: it needs a sparse index", (long long)q); return FILTER_BAD; }
                    len = 1 + (int64_t)count;
                }
                if (p + len > b) { snprintf(msg, msg_len, "program %lld, word %lld: the leaf is cut off by the program's end", (long long)q, (long long)(p - a)); return FILTER_BAD; }
                if (op != FOP_TEXT && (int64_t)prog[p + 1] >= ncols) {
                    snprintf(msg, msg_len, "program %lld, word %lld: column %u outside [0, %lld)", (long long)q, (long long)(p - a), prog[p + 1], (long long)ncols);
                    return FILTER_BAD;
                }
                const int64_t first = p + (op == FOP_TEXT ? 1 : 2);
                for (int64_t i = first; op != FOP_RANGE && i < p + len; ++i) {
                    if (op == FOP_TEXT && (int64_t)prog[i] >= vocab) {
                        snprintf(msg, msg_len, "program %lld: term %u outside the vocabulary's [0, %lld)", (long long)q, prog[i], (long long)vocab);
                        return FILTER_BAD;
                    }
                    const bool rising = i == first || (op == FOP_TEXT ? prog[i] > prog[i - 1] : (int32_t)prog[i] > (int32_t)prog[i - 1]);
                    if (!rising) { snprintf(msg, msg_len, "program %lld, word %lld: %s must be strictly increasing", (long long)q, (long long)(i - a), op == FOP_TEXT ? "terms" : "set ids"); return FILTER_BAD; }
                }
                if (++depth > FP_MAX_STACK) { snprintf(msg, msg_len, "program %lld, word %lld: more than %d sets on the stack", (long long)q, (long long)(p - a), FP_MAX_STACK); return FILTER_BAD; }
                if (op == FOP_TEXT && any_text) *any_text = true;
            } else if (op == FOP_AND || op == FOP_OR || op == FOP_NOT) {
                if (w != op) { snprintf(msg, msg_len, "program %lld, word %lld: operation %u carries no argument", (long long)q, (long long)(p - a), op); return FILTER_BAD; }
                const int need = op == FOP_NOT ? 1 : 2;
                if (depth < need) { snprintf(msg, msg_len, "program %lld, word %lld: the stack holds %d sets, the operation pops %d", (long long)q, (long long)(p - a), depth, need); return FILTER_BAD; }
                depth -= need - 1;
            } else {
                snprintf(msg, msg_len, "program %lld, word %lld: unknown operation %u", (long long)q, (long long)(p - a), op);
                return FILTER_BAD;
            }
            p += len;
        }
        if (depth != 1) { snprintf(msg, msg_len, "program %lld leaves %d sets on the stack, not 1", (long long)q, depth); return FILTER_BAD; }
    }
    return FILTER_OK;
}

}  // namespace icd
