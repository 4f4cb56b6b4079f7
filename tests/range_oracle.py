"""What a range search / offset / iterator page must return, as a walk over the FULL ranking of every query
(oracle.flat_ip_topk at k = n: scores and ids, best first by (score desc, id asc)). Rules 1-8 of DESIGN.md section 11.

No device code and nothing of the package under test: numpy only.
"""
import numpy as np

W = {1: 1.2, 3: 0.8}


def in_band(scores, ids, radius=None, range_filter=None, after=None):
    """mask over one query's ranking: radius < score <= range_filter (plain float compares), strictly behind the cursor
    after = (score, id): score < after score, or equal score BITS and id > after id; NaN scores are never hits"""
    scores = np.asarray(scores, np.float32)
    ids = np.asarray(ids, np.int64)
    m = ~np.isnan(scores)
    if radius is not None:
        m &= scores > np.float32(radius)
    if range_filter is not None:
        m &= scores <= np.float32(range_filter)
    if after is not None:
        a_s, a_id = np.float32(after[0]), int(after[1])
        same = scores.view(np.uint32) == np.array([a_s], np.float32).view(np.uint32)[0]
        m &= (scores < a_s) | (same & (ids > a_id))
    return m


def reweight(raw, ids, levels_of_hits):
    """adj = float64(raw) * w[level], ONE stable descending re-sort of the valid hits, padding (-inf, -inf, -1, 0) behind"""
    k = len(raw)
    m = int((ids >= 0).sum())
    adj = np.array([float(np.float64(raw[j]) * W.get(int(levels_of_hits[j]), 1.0)) for j in range(m)], np.float64)
    order = sorted(range(m), key=lambda j: -adj[j])   # (sorted is stable)
    o_adj, o_raw = np.full(k, -np.inf, np.float64), np.full(k, -np.inf, np.float32)
    o_ids, o_lv = np.full(k, -1, np.int64), np.zeros(k, np.int32)
    for p, j in enumerate(order):
        o_adj[p], o_raw[p], o_ids[p], o_lv[p] = adj[j], raw[j], ids[j], levels_of_hits[j]
    return o_adj, o_raw, o_ids, o_lv


def band_query(scores, ids, levels, k, radius=None, range_filter=None, after=None, offset=0, id_base=0):
    """one query: ((raw, ids, levels) in raw order, (adj, raw, ids, levels) reweighted), each of length k, padded. `ids` are the
    ids searches return (global: id_base + row; on a view the parent's); levels is indexed by id - id_base."""
    scores = np.asarray(scores, np.float32)
    ids = np.asarray(ids, np.int64)
    pos = np.nonzero(in_band(scores, ids, radius, range_filter, after))[0][offset:offset + k]
    raw = np.full(k, -np.inf, np.float32)
    rid = np.full(k, -1, np.int64)
    lv = np.zeros(k, np.int32)
    raw[:len(pos)], rid[:len(pos)] = scores[pos], ids[pos]
    lv[:len(pos)] = np.asarray(levels)[ids[pos] - id_base]
    return (raw, rid, lv), reweight(raw, rid, lv)


def _per_query(v, q):
    if v is None:
        return None
    v = np.asarray(v)
    return v.reshape(-1)[q] if v.size > 1 else v.reshape(-1)[0]


def band_batch(scores, ids, levels, k, radius=None, range_filter=None, after=None, offset=0, id_base=0):
    """a batch: bounds are None, scalars or one value per query; after = (scores [nq], ids [nq]) or None"""
    nq = len(scores)
    raws, adjs = [], []
    for q in range(nq):
        a = None if after is None else (_per_query(after[0], q), _per_query(after[1], q))
        r, a2 = band_query(scores[q], ids[q], levels, k, _per_query(radius, q), _per_query(range_filter, q), a, offset, id_base)
        raws.append(r)
        adjs.append(a2)
    return tuple(np.stack([r[i] for r in raws]) for i in range(3)), tuple(np.stack([a[i] for a in adjs]) for i in range(4))


def pages(scores, ids, batch_size, radius=None, range_filter=None, limit=-1):
    """one query: the iterator's pages as lists of ids in RAW order (rule 8: page i + 1 starts behind the raw-order last hit of
    page i); stops behind a short page or at `limit` hits"""
    scores = np.asarray(scores, np.float32)
    ids = np.asarray(ids, np.int64)
    out, after, left = [], None, (None if limit == -1 else limit)
    while left is None or left > 0:
        want = batch_size if left is None else min(batch_size, left)
        pos = np.nonzero(in_band(scores, ids, radius, range_filter, after))[0][:want]
        if len(pos) == 0:
            break
        out.append(ids[pos].tolist())
        after = (scores[pos[-1]], ids[pos[-1]])
        if left is not None:
            left -= len(pos)
        if len(pos) < want:
            break
    return out
