"""The contract of the sparse search in numpy, written independently of the package: the score and the
answer of icd_sparse_search, a numpy counting sort for icd_sparse_pack, and the analyzer / BM25 weighting of
services/sparse_text.py restated."""
import math
import unicodedata

import numpy as np

LEVEL_WEIGHT = {1: 1.2, 3: 0.8}


def rows_as_dicts(row_off, terms, vals):
    return [{int(terms[p]): np.float32(vals[p]) for p in range(int(row_off[i]), int(row_off[i + 1]))} for i in range(len(row_off) - 1)]


def postings(row_off, terms, vals, vocab):
    """term -> (rows ascending, values): what a stable counting sort of the CSR rows by term gives"""
    terms = np.asarray(terms, np.int64)
    rows = np.repeat(np.arange(len(row_off) - 1, dtype=np.int64), np.diff(row_off))
    order = np.argsort(terms, kind="stable")
    post_off = np.zeros(vocab + 1, np.int64)
    np.add.at(post_off, terms + 1, 1)
    return np.cumsum(post_off), rows[order].astype(np.uint32), np.asarray(vals, np.float32)[order]


def search(row_off, terms, vals, vocab, q_off, q_terms, q_vals, k, levels=None, id_base=0, masks=None, reweighted=False):
    """-> (raw f32, ids i64, levels i32) [nq][k], or (adj f64, raw, ids, levels) in the re-sorted order. masks: None or per
    query None / a boolean array over the rows."""
    n, nq = len(row_off) - 1, len(q_off) - 1
    post_off, post_row, post_val = postings(row_off, terms, vals, vocab)
    raw = np.full((nq, k), -np.inf, np.float32)
    ids = np.full((nq, k), -1, np.int64)
    lv = np.zeros((nq, k), np.int32)
    adj = np.full((nq, k), -np.inf, np.float64)
    for q in range(nq):
        acc = np.zeros(n, np.float32)
        hit = np.zeros(n, bool)
        for p in range(int(q_off[q]), int(q_off[q + 1])):   # ascending terms: the canonical order of the sum
            t = int(q_terms[p])
            r = post_row[post_off[t]:post_off[t + 1]].astype(np.int64)
            prod = np.float32(q_vals[p]) * post_val[post_off[t]:post_off[t + 1]]   # float32 * float32, rounded once
            acc[r] = acc[r] + prod.astype(np.float32)
            hit[r] = True
        if masks is not None and masks[q] is not None:
            hit &= np.asarray(masks[q], bool)
        cand = np.flatnonzero(hit)
        order = cand[np.lexsort((cand, -acc[cand].astype(np.float64)))][:k]
        m = len(order)
        r_, i_ = acc[order], order + id_base
        l_ = np.ones(m, np.int32) if levels is None else np.asarray(levels, np.int32)[order]
        if reweighted:
            a_ = r_.astype(np.float64) * np.array([LEVEL_WEIGHT.get(int(x), 1.0) for x in l_], np.float64)
            re = np.argsort(-a_, kind="stable")
            r_, i_, l_, a_ = r_[re], i_[re], l_[re], a_[re]
            adj[q, :m] = a_
        raw[q, :m], ids[q, :m], lv[q, :m] = r_, i_, l_
    return (adj, raw, ids, lv) if reweighted else (raw, ids, lv)


# ---- the analyzer and BM25, restated ------------------------------------------------------------------------------------------
def _is_cjk(ch):
    c = ord(ch)
    return 0x3400 <= c <= 0x4DBF or 0x4E00 <= c <= 0x9FFF or 0xF900 <= c <= 0xFAFF or 0x20000 <= c <= 0x3134F


def _is_alnum(ch):
    return ("a" <= ch <= "z") or ("0" <= ch <= "9")


def analyze(text):
    s = unicodedata.normalize("NFKC", text).lower()
    out, i = [], 0
    while i < len(s):
        if _is_cjk(s[i]):
            j = i
            while j < len(s) and _is_cjk(s[j]):
                j += 1
            out += list(s[i:j]) + [s[p:p + 2] for p in range(i, j - 1)]
            i = j
        elif _is_alnum(s[i]):
            j = i
            while j < len(s) and (_is_alnum(s[j]) or (s[j] == "." and j + 1 < len(s) and _is_alnum(s[j + 1]) and _is_alnum(s[j - 1]))):
                j += 1
            out.append(s[i:j])
            i = j
        else:
            i += 1
    return out


def bm25(texts, k1=1.2, b=0.75):
    """-> (vocab list, row_off, terms, vals fp32, idf float64) of the corpus"""
    docs = [analyze(t) for t in texts]
    vocab = sorted({t for d in docs for t in d})
    where = {t: i for i, t in enumerate(vocab)}
    n = len(docs)
    total = sum(len(d) for d in docs)
    avgdl = total / n if total > 0 else 1.0
    df = [0] * len(vocab)
    row_off, terms, vals = [0], [], []
    for d in docs:
        tf = {}
        for t in d:
            tf[where[t]] = tf.get(where[t], 0) + 1
        for t in sorted(tf):
            f = float(tf[t])
            df[t] += 1
            terms.append(t)
            vals.append(np.float32(f * (k1 + 1) / (f + k1 * (1 - b + b * float(len(d)) / avgdl))))
        row_off.append(len(terms))
    idf = np.array([math.log(1 + (n - d + 0.5) / (d + 0.5)) for d in df], np.float64)
    return vocab, np.array(row_off, np.int64), np.array(terms, np.uint32), np.array(vals, np.float32), idf


def bm25_query(text, vocab, idf, max_terms=64):
    where = {t: i for i, t in enumerate(vocab)}
    qtf = {}
    for t in analyze(text):
        if t in where:
            qtf[where[t]] = qtf.get(where[t], 0) + 1
    pairs = [(t, float(idf[t]) * float(c)) for t, c in qtf.items()]
    if len(pairs) > max_terms:
        pairs = sorted(pairs, key=lambda p: (-p[1], p[0]))[:max_terms]
    pairs = [(t, np.float32(w)) for t, w in sorted(pairs) if np.float32(w) != 0]
    return np.array([t for t, _ in pairs], np.uint32), np.array([w for _, w in pairs], np.float32)
