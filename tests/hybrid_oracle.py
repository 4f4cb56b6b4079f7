"""What a hybrid search must return (rules 1-6 of DESIGN.md section 13), from the FULL ranking of every request's vector
(oracle.flat_ip_topk at k = n: scores and ids, best first by (score desc, id asc)): every sub-list is the ranking restricted to
its mask (mask_oracle.restrict) and band (range_oracle.in_band), cut at the request's limit; the fused score of an id is the
left-to-right float64 sum over the requests, ascending, whose list holds it.

No device code and nothing of the package under test: numpy and Python floats (IEEE doubles, one rounding per operation) only.
"""
import math

import numpy as np

from mask_oracle import restrict
from range_oracle import W, in_band


def sub_list(scores, ids, limit, mask=None, radius=None, range_filter=None, id_base=0):
    """rule 1: one request's hits for one query, (scores f32, ids i64) of at most `limit` entries, raw order, no padding; a mask
    is over rows (id - id_base)"""
    s, i = (np.asarray(scores, np.float32), np.asarray(ids, np.int64)) if mask is None else restrict(scores, ids, mask, id_base)
    keep = in_band(s, i, radius, range_filter)
    return s[keep][:limit], i[keep][:limit]


def term(ranker, j, score, c=60.0, weight=1.0, norm="none"):
    """one request's contribution to an id at rank j (from 0) with raw score `score` (rules 2 and 3)"""
    if ranker == "rrf":
        return 1.0 / (float(c) + j + 1)
    s = float(np.float32(score))   # (double)score
    if norm == "cosine":
        s = (1.0 + s) * 0.5
    elif norm == "atan":
        s = 0.5 + math.atan(s) / math.pi
    else:
        assert norm == "none"
    return float(weight) * s


def fuse_query(lists, levels, k, ranker="rrf", c=60.0, weights=None, norm="none", id_base=0, n=None):
    """lists: R (scores, ids) sub-lists of one query. Returns ((fused, ids, levels, bits) best fused first, (adj, fused, ids,
    levels, bits) reweighted), each of length k and padded (-inf, id -1, level 0, bits 0); rules 2-6. levels is indexed by
    id - id_base. n: the index's rows - a caller's list (fuse_lists) may hold padding (-1) and ids outside [id_base, id_base + n):
    they are skipped and keep their slot, a hit's rank is its slot."""
    fused, bits = {}, {}
    for r, (s, ids) in enumerate(lists):   # r ascending: the order of the sum
        for j in range(len(ids)):
            i = int(ids[j])
            if n is not None and not id_base <= i < id_base + n:
                continue
            t = term(ranker, j, s[j], c, 1.0 if weights is None else weights[r], norm)
            fused[i] = fused.get(i, 0.0) + t
            bits[i] = bits.get(i, 0) | (1 << r)
    best = sorted(fused, key=lambda i: (-fused[i], i))[:k]
    m = len(best)
    o_f, o_i = np.full(k, -np.inf, np.float64), np.full(k, -1, np.int64)
    o_l, o_b = np.zeros(k, np.int32), np.zeros(k, np.uint32)
    for p, i in enumerate(best):
        o_f[p], o_i[p], o_l[p], o_b[p] = fused[i], i, levels[i - id_base], bits[i]
    adj = [float(o_f[p] * W.get(int(o_l[p]), 1.0)) for p in range(m)]
    order = sorted(range(m), key=lambda p: -adj[p])   # (sorted is stable)
    a_a, a_f, a_i = np.full(k, -np.inf, np.float64), np.full(k, -np.inf, np.float64), np.full(k, -1, np.int64)
    a_l, a_b = np.zeros(k, np.int32), np.zeros(k, np.uint32)
    for p, j in enumerate(order):
        a_a[p], a_f[p], a_i[p], a_l[p], a_b[p] = adj[j], o_f[j], o_i[j], o_l[j], o_b[j]
    return (o_f, o_i, o_l, o_b), (a_a, a_f, a_i, a_l, a_b)


def hybrid_batch(scores, ids, levels, sel, limits, k, ranker="rrf", c=60.0, weights=None, norm="none", masks=None, radius=None,
                 range_filter=None, id_base=0):
    """a batch. scores / ids: the full rankings of a POOL of vectors; sel int [nq][R]: which pool vector request r of query q is.
    limits: R ints. masks: None or [nq][R] entries (None, boolean array or row list); radius / range_filter: None or float
    [nq][R] (-inf / +inf: no bound). Returns (raw tuple, reweighted tuple) of [nq, k] arrays."""
    sel = np.asarray(sel)
    nq, R = sel.shape
    raws, adjs = [], []
    for q in range(nq):
        lists = []
        for r in range(R):
            p = int(sel[q, r])
            lo = None if radius is None else np.asarray(radius, np.float32).reshape(nq, R)[q, r]
            hi = None if range_filter is None else np.asarray(range_filter, np.float32).reshape(nq, R)[q, r]
            lists.append(sub_list(scores[p], ids[p], int(limits[r]), None if masks is None else masks[q][r], lo, hi, id_base))
        raw, adj = fuse_query(lists, levels, k, ranker, c, weights, norm, id_base)
        raws.append(raw)
        adjs.append(adj)
    return tuple(np.stack([x[j] for x in raws]) for j in range(4)), tuple(np.stack([x[j] for x in adjs]) for j in range(5))


def brute_force(corpus, vectors, limits, k, ranker="rrf", c=60.0, weights=None, norm="none", rows=None):
    """one query by plain dictionaries over ALL rows (a yardstick for the walk above on small well-separated data): vectors [R][dim],
    rows: None or R row lists the requests are restricted to. Returns [(id, fused)] best first."""
    n = len(corpus)
    acc = {}
    for r, v in enumerate(vectors):
        cand = range(n) if rows is None or rows[r] is None else [int(x) for x in rows[r]]
        sc = {i: np.float32(np.dot(corpus[i].astype(np.float64), v.astype(np.float64))) for i in cand}
        top = sorted(sc, key=lambda i: (-float(sc[i]), i))[:limits[r]]
        for j, i in enumerate(top):
            acc.setdefault(i, []).append(term(ranker, j, sc[i], c, 1.0 if weights is None else weights[r], norm))
    tot = {}
    for i, ts in acc.items():
        s = 0.0
        for t in ts:
            s = s + t
        tot[i] = s
    return [(i, tot[i]) for i in sorted(tot, key=lambda i: (-tot[i], i))[:k]]
