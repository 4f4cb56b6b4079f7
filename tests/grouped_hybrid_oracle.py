"""The contract of the grouped sparse and the grouped hybrid search in numpy and Python floats, composed from
the oracles that exist: sparse hits and scores are sparse_oracle's (rule G1), the choice of groups and members is
grouped_oracle's walk over a full ranking (rule G2, and the sub-lists of rule H1), the fused score is hybrid_oracle's term
(rule H2); masks are sparse_oracle's (the sparse index has no other filter). Nothing of the package is imported."""
import numpy as np

import grouped_oracle as go
import sparse_oracle as so


def sparse_ranking(row_off, terms, vals, vocab, q_off, q_terms, q_vals, masks=None):
    """(raw f32, local rows i64) [nq][n]: EVERY hit of every query in (score desc, row asc) order, -inf / -1 behind the last one -
    sparse_oracle.search at k = n. Computed once per corpus and batch and shared by the groupings and (k, s) tested on it."""
    n = len(row_off) - 1
    raw, ids, _ = so.search(row_off, terms, vals, vocab, q_off, q_terms, q_vals, n, masks=masks)
    return raw, ids


class Ranking:
    """grouped_oracle.Ranking over the queries that have a hit at all (a dense ranking always has; a sparse one need not): the
    others answer with padding"""

    def __init__(self, scores, ids, group_of):
        ids = np.asarray(ids, np.int64)
        self.group_of = np.asarray(group_of, np.int64)
        self.nq = ids.shape[0]
        self.some = np.flatnonzero(ids[:, 0] >= 0) if ids.shape[1] else np.zeros(0, np.int64)
        self.inner = go.Ranking(np.asarray(scores)[self.some], ids[self.some], group_of) if self.some.size else None

    def raw(self, k, s):
        sc = np.full((self.nq, k * s), -np.inf, np.float32)
        ids = np.full((self.nq, k * s), -1, np.int64)
        grp = np.full((self.nq, k * s), -1, np.int32)
        if self.inner is not None:
            sc[self.some], ids[self.some], grp[self.some] = self.inner.raw(k, s)
        return sc, ids, grp


def grouped_from_ranking(raw, rows, group_of, k, s, levels=None, id_base=0, reweighted=False):
    return grouped_from(Ranking(raw, rows, group_of), k, s, levels, id_base, reweighted)


def grouped_from(ranking, k, s, levels=None, id_base=0, reweighted=False):
    """ranking: a Ranking of a full ranking under a grouping (built once, shared by every (k, s))
    -> (raw f32, ids i64, levels i32, groups i32) [nq][k * s], group-rank-major, or (adj f64, raw, ids, levels, groups) after
    the level weight in double and ONE stable descending re-sort of the query's hits; padding -inf, -1, 0, -1"""
    sc, rid, grp = ranking.raw(k, s)
    group_of = ranking.group_of
    hit = rid >= 0
    n = len(group_of)
    lv_all = np.ones(n, np.int32) if levels is None else np.asarray(levels, np.int32)
    lv = np.where(hit, lv_all[np.clip(rid, 0, None)], 0).astype(np.int32)
    ids = np.where(hit, rid + id_base, -1).astype(np.int64)
    if not reweighted:
        return sc, ids, lv, grp
    w = np.ones(int(lv_all.max()) + 2, np.float64)
    for level, weight in so.LEVEL_WEIGHT.items():
        if level < len(w):
            w[level] = weight
    adj = np.where(hit, sc.astype(np.float64) * w[lv], -np.inf)
    out = [np.full(adj.shape, -np.inf, np.float64), np.full(sc.shape, -np.inf, np.float32), np.full(ids.shape, -1, np.int64),
           np.zeros(lv.shape, np.int32), np.full(grp.shape, -1, np.int32)]
    for q in range(adj.shape[0]):
        m = int(hit[q].sum())   # (hits are contiguous)
        order = np.argsort(-adj[q, :m], kind="stable")
        for dst, src in zip(out, (adj, sc, ids, lv, grp)):
            dst[q, :m] = src[q, :m][order]
    return tuple(out)


def sparse_search_grouped(row_off, terms, vals, vocab, q_off, q_terms, q_vals, group_of, k, s, levels=None, id_base=0, masks=None,
                          reweighted=False):
    raw, rows = sparse_ranking(row_off, terms, vals, vocab, q_off, q_terms, q_vals, masks)
    return grouped_from_ranking(raw, rows, group_of, k, s, levels, id_base, reweighted)


# ---- grouped hybrid search (rules H1 - H4) -----------------------------------------------------------------------------------------
import hybrid_oracle as ho   # noqa: E402
from range_oracle import W   # noqa: E402


def run_cut(ids, group_of, limit):
    """rule H1: how many leading slots of a list lie in front of its (limit + 1)-th RUN of equal group ids. group_of is indexed by
    id; an id that is no row (negative, past the end, or group -1: outside a view) is a run of its own."""
    runs, prev = 0, None
    for j, i in enumerate(np.asarray(ids, np.int64).tolist()):
        g = int(group_of[i]) if 0 <= i < len(group_of) else -1
        if j == 0 or g != prev or g < 0:
            runs += 1
        if runs > limit:
            return j
        prev = g
    return len(ids)


def fuse_query_grouped(lists, group_of, levels, limits, k, s, ranker="rrf", c=60.0, weights=None, norm="none"):
    """lists: R (scores, ids) of one query, every slot kept (rank j IS the slot index; ids that are no row are no hit). Returns
    (raw, reweighted, gap): raw = (fused f64, ids, levels, bits, groups) [k * s] group-rank-major, reweighted = (adj,) + the same
    after ONE stable descending re-sort, padding -inf / -1 / 0 / 0 / -1; gap = the smallest distance of two fused heads."""
    fused, bits = {}, {}
    for r, (sc, ids) in enumerate(lists):   # r ascending: the order of the sum
        for j in range(run_cut(ids, group_of, int(limits[r]))):
            i = int(ids[j])
            if not (0 <= i < len(group_of)) or group_of[i] < 0:
                continue
            t = ho.term(ranker, j, sc[j], c, 1.0 if weights is None else weights[r], norm)
            fused[i] = fused.get(i, 0.0) + t
            bits[i] = bits.get(i, 0) | (1 << r)
    members = {}
    for i in sorted(fused, key=lambda i: (-fused[i], i)):
        members.setdefault(int(group_of[i]), []).append(i)          # (dicts keep insertion order: groups by their best member)
    best = [i for g in list(members)[:k] for i in members[g][:s]]
    vals = sorted(fused.values())
    gap = min((b - a for a, b in zip(vals, vals[1:])), default=np.inf)
    n = k * s
    raw = [np.full(n, -np.inf, np.float64), np.full(n, -1, np.int64), np.zeros(n, np.int32), np.zeros(n, np.uint32), np.full(n, -1, np.int32)]
    for p, i in enumerate(best):
        raw[0][p], raw[1][p], raw[2][p], raw[3][p], raw[4][p] = fused[i], i, levels[i], bits[i], group_of[i]
    m = len(best)
    adj = [float(raw[0][p] * W.get(int(raw[2][p]), 1.0)) for p in range(m)]
    order = sorted(range(m), key=lambda p: -adj[p])   # (sorted is stable)
    out = [np.full(n, -np.inf, np.float64)] + [x.copy() for x in raw]
    for x, pad in zip(out[1:], (-np.inf, -1, 0, 0, -1)):
        x[:] = pad
    for p, j in enumerate(order):
        out[0][p] = adj[j]
        for x, src in zip(out[1:], raw):
            x[p] = src[j]
    return tuple(raw), tuple(out), gap


def hybrid_grouped_batch(scores, ids, group_of, levels, sel, limits, k, s, ranker="rrf", c=60.0, weights=None, norm="none", row_map=None):
    """scores / ids: the full rankings of a POOL of vectors over the index (a view: over its local rows, row_map their global ids,
    group_of per local row, levels the parent's); sel int [nq][R]. Sub-list (q, r) is the grouped search's raw output at
    max(limits) groups of s members (H1). Returns (raw tuple, reweighted tuple, gaps [nq]) of [nq, k * s] arrays."""
    sel = np.asarray(sel)
    nq, R = sel.shape
    sub_s, sub_i, _ = go.Ranking(scores, ids, group_of).raw(int(max(limits)), s)
    g_of = np.asarray(group_of, np.int64)
    if row_map is not None:
        row_map = np.asarray(row_map, np.int64)
        sub_i = np.where(sub_i >= 0, row_map[np.clip(sub_i, 0, None)], -1)
        g_of = np.full(len(levels), -1, np.int64)
        g_of[row_map] = np.asarray(group_of, np.int64)
    outs = [fuse_query_grouped([(sub_s[int(sel[q, r])], sub_i[int(sel[q, r])]) for r in range(R)], g_of, levels, limits, k, s, ranker, c, weights, norm)
            for q in range(nq)]
    return (tuple(np.stack([o[0][j] for o in outs]) for j in range(5)), tuple(np.stack([o[1][j] for o in outs]) for j in range(6)),
            np.array([o[2] for o in outs]))
