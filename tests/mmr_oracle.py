"""What an MMR search must return, from the oracle's FULL ranking of every query (oracle.flat_ip_topk at
k = n): the candidates are the existing walkers' lists (range_oracle / mask_oracle at k = fetch_k, raw order), the similarity of
two candidates is oracle.scores of one stored row against the other (the canonical chain), the value is computed in Python floats
(IEEE doubles: two products and a difference, each rounded once) with one_minus = 1.0 - lam computed once, and the reweighted form
goes through oracle.reweight. Everything is exact: there is no tolerance anywhere.

`orc` is the oracle module (the `oracle` fixture). numpy and the oracle only: nothing of the package under test.
"""
import math

import numpy as np

from mask_oracle import masked_batch


def greedy(rel, sim_to, k, lam):
    """The picks of one query. rel: the candidates' float32 scores (C of them, best first); sim_to(i) -> float32 [C], the
    similarity of every candidate to candidate i. Returns (picks, values): candidate indices in pick order and the Python-float
    value each was picked with (pick 0: lam * rel_0)."""
    C = len(rel)
    npick = min(int(k), C)
    if npick == 0:
        return [], []
    lam = float(lam)
    one_minus = 1.0 - lam
    picks, values = [0], [lam * float(rel[0])]
    picked = np.zeros(C, bool)
    picked[0] = True
    pen = None
    while len(picks) < npick:
        s = np.asarray(sim_to(picks[-1]), np.float32)
        if pen is None:
            pen = s.copy()
        else:
            pen = np.where(s > pen, s, pen).astype(np.float32)   # plain `s > pen ? s : pen`: a NaN never replaces, a NaN pen stays
        best, best_v = -1, 0.0
        for i in range(C):
            if picked[i]:
                continue
            v = lam * float(rel[i]) - one_minus * float(pen[i])
            if math.isnan(v):
                continue
            if best < 0 or v > best_v:
                best, best_v = i, v
        if best < 0:   # no comparable value: the lowest unpicked index, with the (NaN) value it has
            best = int(np.flatnonzero(~picked)[0])
            best_v = lam * float(rel[best]) - one_minus * float(pen[best])
        picks.append(best)
        values.append(best_v)
        picked[best] = True
    return picks, values


def mmr_batch(orc, corpus, levels, full_scores, full_ids, k, fetch_k, lam, masks=None, radius=None, range_filter=None, id_base=0):
    """A batch. full_scores / full_ids: oracle.flat_ip_topk(corpus, queries, n, id_base) (slots without a row - NaN scores - hold
    id -1). masks: None or one entry per query (None, boolean array over rows, row list); radius / range_filter: None, scalars or
    one value per query. Returns (pick, rew): pick = (raw f32, ids i64, levels i32, mmr f64) in pick order, rew = (adj f64, raw,
    ids, levels, mmr) through the reweight, each [nq, k], padded (-inf, -1, 0, -inf)."""
    corpus = np.ascontiguousarray(corpus, np.float32)
    levels = np.asarray(levels, np.int32)
    nq = len(full_scores)
    fs = [np.asarray(full_scores[q])[np.asarray(full_ids[q]) >= 0] for q in range(nq)]
    fi = [np.asarray(full_ids[q])[np.asarray(full_ids[q]) >= 0] for q in range(nq)]
    every = np.ones(len(corpus), bool)   # (one entry per ROW: a ranking that left NaN rows out is shorter than the corpus)
    per_row = [every if m is None else m for m in (masks if masks is not None else [None] * nq)]
    (c_raw, c_ids, c_lv), _ = masked_batch(fs, fi, levels, per_row, fetch_k, radius, range_filter, id_base=id_base)
    o_raw = np.full((nq, k), -np.inf, np.float32)
    o_ids = np.full((nq, k), -1, np.int64)
    o_lv = np.zeros((nq, k), np.int32)
    o_mmr = np.full((nq, k), -np.inf, np.float64)
    r_mmr = np.full((nq, k), -np.inf, np.float64)
    for q in range(nq):
        C = int((c_ids[q] >= 0).sum())
        rows = c_ids[q][:C] - id_base
        sub = corpus[rows]
        picks, values = greedy(c_raw[q][:C], lambda i: orc.scores(sub[i], sub), k, lam)
        t = len(picks)
        o_raw[q, :t], o_ids[q, :t], o_lv[q, :t], o_mmr[q, :t] = c_raw[q][picks], c_ids[q][picks], c_lv[q][picks], values
    adj, r_raw, r_ids, r_lv = orc.reweight(o_raw, o_ids, levels, id_base)
    # the mmr value travels with its hit: the reweight is one stable descending sort of the adjusted scores
    for q in range(nq):
        t = int((o_ids[q] >= 0).sum())
        a = [float(np.float64(o_raw[q, j]) * orc.level_weight(o_lv[q, j])) for j in range(t)]
        order = sorted(range(t), key=lambda j: -a[j])
        r_mmr[q, :t] = o_mmr[q][order]
        assert np.array_equal(r_ids[q, :t], o_ids[q][order])
    return (o_raw, o_ids, o_lv, o_mmr), (adj, r_raw, r_ids, r_lv, r_mmr)


def brute_force(corpus, levels, query, k, fetch_k, lam, keep=None, id_base=0):
    """One query by a plain Python loop with chains of its own: the product of two float32 is exact in float64, the sum is taken
    there and rounded to float32. That is fmaf whenever the float64 sum is exact - the test feeds rows of small dyadic values
    (multiples of 1/8), where every step is. Returns (ids, values) in pick order."""
    corpus = np.asarray(corpus, np.float32)

    def chain(a, b):
        acc = np.float32(0.0)
        for x, y in zip(a, b):
            acc = np.float32(np.float64(x) * np.float64(y) + np.float64(acc))
        return acc
    n = len(corpus)
    cand = []
    for r in range(n):
        if keep is not None and not keep[r]:
            continue
        s = chain(query, corpus[r])
        if not np.isnan(s):
            cand.append((s, r))
    cand.sort(key=lambda t: (-float(t[0]), t[1]))
    cand = cand[:fetch_k]
    rel = np.array([c[0] for c in cand], np.float32)
    rows = [c[1] for c in cand]
    picks, values = greedy(rel, lambda i: np.array([chain(corpus[rows[i]], corpus[r]) for r in rows], np.float32), k, lam)
    return [rows[p] + id_base for p in picks], values
