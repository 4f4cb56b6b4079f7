// mmr_plan.hpp - the host-visible arithmetic of the MMR select: a candidate's value, the update of its
// penalty, and the winner rule over an array of (value, index). No HIP header and no handle: included by mmr_select_kernel.hpp
// (the kernel calls these very functions) and by tests/mmr_plan_check.cpp, which runs them under the host sanitizers.
//
// The value is two products and one difference, each rounded once in double. The compiler's default contraction would fuse the
// second product into the difference (one rounding less), so the functions sit between `#pragma clang fp contract(off)` and
// `contract(fast)`, as hybrid_fuse.hpp's sums do; gcc and clang on the host honour the same pragma or do not contract across
// statements at all (the check compares against volatile temporaries).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MMR_HD __host__ __device__
#else
#define MMR_HD
#endif

namespace icd {

constexpr int MMR_MAX_FETCH = 128;          // candidates of a query (ICD_MAX_K)
constexpr int MMR_NONE = 0x7FFFFFFF;        // the index of "no candidate" in a reduction: loses to every real entry

#if defined(__clang__)
#pragma clang fp contract(off)
#endif
// value_i = lambda * (double)rel_i - (1 - lambda) * (double)pen_i; `one_minus` is 1 - lambda, computed once by the caller
MMR_HD inline double mmr_value(double lambda, double one_minus, float rel, float pen) {
    const double a = lambda * (double)rel;
    const double b = one_minus * (double)pen;
    return a - b;
}
// the value pick 0 carries: it has no penalty yet
MMR_HD inline double mmr_first_value(double lambda, float rel) { return lambda * (double)rel; }
#if defined(__clang__)
#pragma clang fp contract(fast)
#endif

// pen_i = the float maximum of sim(i, s) over the picked s, by plain comparison: a NaN similarity never replaces a penalty, a NaN
// penalty (the first similarity was NaN) stays
MMR_HD inline float mmr_pen_update(float pen, float s) { return s > pen ? s : pen; }

// One entry of the winner's reduction. idx = MMR_NONE: no candidate (a picked slot, a lane without one).
struct MmrEntry {
    double value;
    int idx;
};

// a beats b. Comparable values (not NaN) come first, the greater value wins under plain `>`, equal values (+0.0 and -0.0 are
// equal) go to the lower index; among values that are all NaN the lower index wins. A strict total order over entries of
// distinct indices, so folding in any order - a loop, a tree, a butterfly across lanes - yields the same entry.
MMR_HD inline bool mmr_better(const MmrEntry &a, const MmrEntry &b) {
    const bool an = a.value != a.value, bn = b.value != b.value;
    if (an != bn) return bn;
    if (an) return a.idx < b.idx;
    return a.value > b.value || (a.value == b.value && a.idx < b.idx);
}
MMR_HD inline MmrEntry mmr_fold(const MmrEntry &a, const MmrEntry &b) { return mmr_better(b, a) ? b : a; }

// the entry candidate i brings to the reduction
MMR_HD inline MmrEntry mmr_entry(double value, int i, bool picked) {
    MmrEntry e;
    e.value = picked ? (double)__builtin_nan("") : value;   // (a picked slot's value is never read)
    e.idx = picked ? MMR_NONE : i;
    return e;
}

// The winner among candidates [0, n): left fold of the entries. Returns MMR_NONE when every candidate is picked.
MMR_HD inline int mmr_winner(const double *values, const unsigned char *picked, int n) {
    MmrEntry best;
    best.value = (double)__builtin_nan("");
    best.idx = MMR_NONE;
    for (int i = 0; i < n; ++i) best = mmr_fold(best, mmr_entry(values[i], i, picked[i] != 0));
    return best.idx;
}

}  // namespace icd
