"""The keyword-match contract in plain numpy: which rows TEXT_MATCH selects. No device, no library code
under test - the expected bitset comes from the existing host packer (icd_rowmask_pack), which this feature does not touch.

    rows' CSR     row_off int64 [n + 1], terms uint32 (a row's distinct terms; the values of the sparse index play no part)
    query         the distinct KNOWN term ids of the predicate's text and m = minimum_should_match
    answer        the sorted row ids that hold at least m of the query's terms and, with a base, lie in the base row set
"""
import numpy as np


def match_rows(row_off, terms, q_terms, m, base=None):
    """sorted int64 row ids; base: None or an array of row ids (any order) the answer is restricted to"""
    row_off = np.asarray(row_off, np.int64)
    n = len(row_off) - 1
    wanted = set(int(t) for t in np.asarray(q_terms).reshape(-1))
    t = np.asarray(terms).astype(np.int64)
    count = np.zeros(n, np.int64)
    for r in range(n):   # (a Python loop on purpose: nothing here shares a line of thought with the code under test)
        a, b = int(row_off[r]), int(row_off[r + 1])
        if a < b:
            count[r] = sum(1 for x in t[a:b].tolist() if x in wanted)
    hit = (count >= int(m)) if int(m) >= 1 else np.zeros(n, bool)
    if base is not None:
        keep = np.zeros(n, bool)
        keep[np.asarray(base, np.int64)] = True
        hit &= keep
    return np.flatnonzero(hit).astype(np.int64)


def match_text(texts, analyze, text, m):
    """The same rule from the texts themselves: row i matches when analyze(texts[i]) holds at least m of the distinct terms of
    analyze(text); m = "all": every one of them (an unknown term included, so it matches nothing)."""
    want = set(analyze(text))
    need = len(want) if m == "all" else int(m)
    if not want or need < 1:
        return np.zeros(0, np.int64)
    return np.array([i for i, t in enumerate(texts) if len(want & set(analyze(t))) >= need], np.int64)
