"""What a masked search must return, as a walk over the FULL ranking of every query (oracle.flat_ip_topk at k = n: scores and
ids, best first by (score desc, id asc)): keep the rows of the query's mask, then apply range_oracle.band_query to what is
left. Rules 1-8 of DESIGN.md section 12.

No device code and nothing of the package under test: numpy only.
"""
import numpy as np

from range_oracle import band_query, pages


def as_bool(mask, n):
    """None (unfiltered), a boolean array [n] or a list of row indices -> boolean array [n]"""
    if mask is None:
        return np.ones(n, bool)
    m = np.asarray(mask)
    if m.dtype == bool:
        assert m.shape == (n,)
        return m
    out = np.zeros(n, bool)
    out[m.astype(np.int64)] = True
    return out


def restrict(scores, ids, mask, id_base=0):
    """one query's ranking restricted to its mask: (scores, ids) of the kept positions, order unchanged"""
    ids = np.asarray(ids, np.int64)
    m = None if mask is None else np.asarray(mask)
    if m is not None and m.dtype == bool:   # one entry per ROW of the index: a ranking that left NaN rows out is shorter than that
        keep = m[ids - id_base]
    else:
        keep = as_bool(mask, len(ids))[ids - id_base]
    return np.asarray(scores, np.float32)[keep], ids[keep]


def _per_query(v, q):
    if v is None:
        return None
    v = np.asarray(v)
    return v.reshape(-1)[q] if v.size > 1 else v.reshape(-1)[0]


def masked_batch(scores, ids, levels, masks, k, radius=None, range_filter=None, after=None, offset=0, id_base=0):
    """a batch: masks is one entry per query (None, boolean array or row list, over ROWS: id - id_base); bounds are None, scalars
    or one value per query; after = (scores [nq], ids [nq]) or None. Returns ((raw, ids, levels) in raw order, (adj, raw, ids, levels) reweighted),
    each [nq, k], padded (-inf, -1, level 0)."""
    nq = len(scores)
    assert len(masks) == nq
    raws, adjs = [], []
    for q in range(nq):
        s, i = restrict(scores[q], ids[q], masks[q], id_base)
        a = None if after is None else (_per_query(after[0], q), _per_query(after[1], q))
        r, a2 = band_query(s, i, levels, k, _per_query(radius, q), _per_query(range_filter, q), a, offset, id_base)
        raws.append(r)
        adjs.append(a2)
    return tuple(np.stack([r[j] for r in raws]) for j in range(3)), tuple(np.stack([a[j] for a in adjs]) for j in range(4))


def masked_pages(scores, ids, mask, batch_size, radius=None, range_filter=None, limit=-1):
    """one query: the iterator's pages (lists of ids in raw order) over the ranking restricted to the mask"""
    s, i = restrict(scores, ids, mask)
    return pages(s, i, batch_size, radius, range_filter, limit)


def brute_force_topk(corpus, query, rows, k):
    """the k best of `rows` for one query by plain numpy (float64 products rounded once - a yardstick for the helper on tiny
    well-separated data, not the canonical chain): ids best first by (score desc, id asc)"""
    rows = np.asarray(rows, np.int64)
    sc = corpus[rows].astype(np.float64) @ query.astype(np.float64)
    order = np.lexsort((rows, -sc))
    return rows[order][:k]
