// maxsim_plan.hpp - the host-made plan of the embedding-list search: how a batch of lists is cut into
// passes over the grouping's score block, and a pass into launches of maxsim_kernel.hpp. A list's aggregate is ONE ordered chain
// over its vectors' rows of `best`, which all have to be there at once, so the cuts are list boundaries:
//
//   pass     consecutive WHOLE lists whose vectors together fit the score block (B vectors). Greedy, in list order: a pass ends in
//            front of the first list that no longer fits.
//   launch   at most MAXSIM_LAUNCH_LISTS consecutive lists of one pass: their offsets inside the pass travel in the launch's
//            arguments (MaxsimLists), so a search copies no table to the device and stays graph-capturable.
//
// No HIP header and no handle: included by maxsim_kernel.hpp and by tests/maxsim_plan_check.cpp, which runs maxsim_plan under the
// host sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace icd {

constexpr int MAXSIM_MAX_T = 64;            // vectors of one list (include/icd_search.h ICD_MAXSIM_MAX_T)
constexpr int MAXSIM_LAUNCH_LISTS = 128;    // lists of one launch
constexpr int MAXSIM_SUM = 1, MAXSIM_MEAN = 2;   // ICD_MAXSIM_*

// the lists of one launch: list i owns the vectors off[i] .. off[i + 1] of the pass, and cell row `first + i` of the aggregates
struct MaxsimLists {
    int n, first;
    int off[MAXSIM_LAUNCH_LISTS + 1];
};

struct MaxsimPass {
    int64_t v0, l0;          // first vector and first list of the pass, in the call's numbering
    int nv, nl;              // vectors (1 .. B) and lists of the pass
    std::vector<int> off;    // [nl + 1] every list's first vector inside the pass; off[0] = 0, off[nl] = nv
    int launches() const { return (nl + MAXSIM_LAUNCH_LISTS - 1) / MAXSIM_LAUNCH_LISTS; }
    MaxsimLists launch(int i) const {
        MaxsimLists m{};
        m.first = i * MAXSIM_LAUNCH_LISTS;
        m.n = nl - m.first < MAXSIM_LAUNCH_LISTS ? nl - m.first : MAXSIM_LAUNCH_LISTS;
        for (int j = 0; j <= m.n; ++j) m.off[j] = off[(size_t)(m.first + j)];
        return m;
    }
};

// list_off: [nl + 1], must start at 0 and every list hold 1 .. min(MAXSIM_MAX_T, B) vectors; anything else, nl < 1 and B < 1 are
// refused (false, `out` empty). Every vector and every list lies in exactly one pass.
inline bool maxsim_plan(const int64_t *list_off, int64_t nl, int B, std::vector<MaxsimPass> &out) {
    out.clear();
    if (!list_off || nl < 1 || B < 1 || list_off[0] != 0) return false;
    for (int64_t l = 0; l < nl; ++l) {
        const int64_t t = list_off[l + 1] - list_off[l];
        if (t < 1 || t > MAXSIM_MAX_T || t > B) return false;
    }
    MaxsimPass open{0, 0, 0, 0, {0}};
    for (int64_t l = 0; l < nl; ++l) {
        const int t = (int)(list_off[l + 1] - list_off[l]);
        if (open.nv + t > B) {
            out.push_back(open);
            open = MaxsimPass{list_off[l], l, 0, 0, {0}};
        }
        open.nv += t;
        open.nl += 1;
        open.off.push_back(open.nv);
    }
    out.push_back(open);
    return true;
}

}  // namespace icd
