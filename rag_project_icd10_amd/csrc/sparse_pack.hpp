// sparse_pack.hpp - host only (no HIP, no handle): the checks of sparse rows / queries in CSR form and the stable counting sort that
// turns the rows into the inverted index sparse_kernel.hpp walks. Included by icd_search.hip (icd_sparse.hpp) and by
// tests/sparse_pack_check.cpp, which runs it under the host sanitizers.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace icd {

enum { SPARSE_OK = 0, SPARSE_BAD = -1 };

// `count` CSR rows (row_off[count + 1], terms, vals): offsets start at 0 and never decrease, a row's terms are strictly increasing
// and below vocab, its values finite and non-zero; max_terms > 0 bounds a row's length (a query). On a violation: SPARSE_BAD and
// its description in msg.
inline int sparse_check_csr(const int64_t *row_off, const uint32_t *terms, const float *vals, int64_t count, int64_t vocab,
                            int64_t max_terms, const char *unit, char *msg, size_t msg_len) {
    if (count < 0 || vocab < 1 || vocab > 0xFFFFFFFFll || !row_off) {
        snprintf(msg, msg_len, "%s offsets NULL, count=%lld or vocab=%lld", unit, (long long)count, (long long)vocab);
        return SPARSE_BAD;
    }
    if (row_off[0] != 0) { snprintf(msg, msg_len, "%s offsets start at %lld, not 0", unit, (long long)row_off[0]); return SPARSE_BAD; }
    for (int64_t i = 0; i < count; ++i) {
        const int64_t a = row_off[i], b = row_off[i + 1];
        if (b < a) { snprintf(msg, msg_len, "%s %lld: offsets decrease", unit, (long long)i); return SPARSE_BAD; }
        if (max_terms > 0 && b - a > max_terms) {
            snprintf(msg, msg_len, "%s %lld carries %lld terms (at most %lld)", unit, (long long)i, (long long)(b - a), (long long)max_terms);
            return SPARSE_BAD;
        }
        if (b > a && (!terms || !vals)) { snprintf(msg, msg_len, "terms / vals NULL"); return SPARSE_BAD; }
        for (int64_t p = a; p < b; ++p) {
            if ((int64_t)terms[p] >= vocab) {
                snprintf(msg, msg_len, "%s %lld: term %u outside the vocabulary's [0, %lld)", unit, (long long)i, terms[p], (long long)vocab);
                return SPARSE_BAD;
            }
            if (p > a && terms[p] <= terms[p - 1]) {
                snprintf(msg, msg_len, "%s %lld: terms must be strictly increasing (%u after %u)", unit, (long long)i, terms[p], terms[p - 1]);
                return SPARSE_BAD;
            }
            if (!std::isfinite(vals[p]) || vals[p] == 0.0f) {
                snprintf(msg, msg_len, "%s %lld: the value of term %u must be finite and non-zero", unit, (long long)i, terms[p]);
                return SPARSE_BAD;
            }
        }
    }
    return SPARSE_OK;
}

// The queries of a keyword match: `count` term lists without values (q_off[count + 1], terms) under
// sparse_check_csr's rules for offsets and terms, at most max_terms terms each, and min_match[q] in 1 .. max_terms.
inline int sparse_check_match_queries(const int64_t *q_off, const uint32_t *terms, const int32_t *min_match, int64_t count, int64_t vocab,
                                      int64_t max_terms, char *msg, size_t msg_len) {
    if (count < 0 || vocab < 1 || vocab > 0xFFFFFFFFll || !q_off || !min_match) {
        snprintf(msg, msg_len, "query offsets or min_match NULL, count=%lld or vocab=%lld", (long long)count, (long long)vocab);
        return SPARSE_BAD;
    }
    if (q_off[0] != 0) { snprintf(msg, msg_len, "query offsets start at %lld, not 0", (long long)q_off[0]); return SPARSE_BAD; }
    for (int64_t i = 0; i < count; ++i) {
        const int64_t a = q_off[i], b = q_off[i + 1];
        if (b < a) { snprintf(msg, msg_len, "query %lld: offsets decrease", (long long)i); return SPARSE_BAD; }
        if (b - a > max_terms) {
            snprintf(msg, msg_len, "query %lld carries %lld terms (at most %lld)", (long long)i, (long long)(b - a), (long long)max_terms);
            return SPARSE_BAD;
        }
        if (min_match[i] < 1 || min_match[i] > max_terms) {
            snprintf(msg, msg_len, "query %lld: min_match=%d outside 1 .. %lld", (long long)i, min_match[i], (long long)max_terms);
            return SPARSE_BAD;
        }
        if (b > a && !terms) { snprintf(msg, msg_len, "terms NULL"); return SPARSE_BAD; }
        for (int64_t p = a; p < b; ++p) {
            if ((int64_t)terms[p] >= vocab) {
                snprintf(msg, msg_len, "query %lld: term %u outside the vocabulary's [0, %lld)", (long long)i, terms[p], (long long)vocab);
                return SPARSE_BAD;
            }
            if (p > a && terms[p] <= terms[p - 1]) {
                snprintf(msg, msg_len, "query %lld: terms must be strictly increasing (%u after %u)", (long long)i, terms[p], terms[p - 1]);
                return SPARSE_BAD;
            }
        }
    }
    return SPARSE_OK;
}

// CSR rows that sparse_check_csr has passed -> postings: post_off[vocab + 1], post_row / post_val [nnz]. A stable counting sort by
// term: rows are visited in ascending order, so every term's postings come out with ascending rows.
inline void sparse_pack_checked(const int64_t *row_off, const uint32_t *terms, const float *vals, int64_t n, int64_t vocab,
                                int64_t *post_off, uint32_t *post_row, float *post_val) {
    const int64_t nnz = row_off[n];
    memset(post_off, 0, (size_t)(vocab + 1) * sizeof(int64_t));
    for (int64_t p = 0; p < nnz; ++p) ++post_off[(int64_t)terms[p] + 1];
    for (int64_t t = 0; t < vocab; ++t) post_off[t + 1] += post_off[t];
    // post_off[t] is term t's cursor while the rows are placed, and its start again once shifted back
    for (int64_t i = 0; i < n; ++i)
        for (int64_t p = row_off[i]; p < row_off[i + 1]; ++p) {
            const int64_t at = post_off[terms[p]]++;
            post_row[at] = (uint32_t)i;
            post_val[at] = vals[p];
        }
    for (int64_t t = vocab; t > 0; --t) post_off[t] = post_off[t - 1];
    post_off[0] = 0;
}

// The rows of a sparse index: 1 <= n < 2^31 of them, under sparse_check_csr's rules.
inline int sparse_check_rows(const int64_t *row_off, const uint32_t *terms, const float *vals, int64_t n, int64_t vocab, char *msg, size_t msg_len) {
    if (n < 1 || n > 0x7FFFFFFFll) { snprintf(msg, msg_len, "n=%lld: a sparse index holds 1 .. 2^31 - 1 rows", (long long)n); return SPARSE_BAD; }
    return sparse_check_csr(row_off, terms, vals, n, vocab, 0, "row", msg, msg_len);
}

// check, then pack: nothing is written when the input is refused
inline int sparse_pack_rows(const int64_t *row_off, const uint32_t *terms, const float *vals, int64_t n, int64_t vocab,
                            int64_t *post_off, uint32_t *post_row, float *post_val, char *msg, size_t msg_len) {
    if (!post_off) { snprintf(msg, msg_len, "post_off is NULL"); return SPARSE_BAD; }
    if (const int rc = sparse_check_rows(row_off, terms, vals, n, vocab, msg, msg_len)) return rc;
    if (row_off[n] > 0 && (!post_row || !post_val)) { snprintf(msg, msg_len, "post_row / post_val NULL"); return SPARSE_BAD; }
    sparse_pack_checked(row_off, terms, vals, n, vocab, post_off, post_row, post_val);
    return SPARSE_OK;
}

}  // namespace icd
