"""The contract of the sparse range search in numpy, written independently of the package: section 11's band
on section 14's ranking. A query's hits are the rows that share a term with it inside its mask; they are ranked by
(order_f32(score) descending, id ascending); the band (radius < score <= range_filter as plain float compares, strictly behind the
cursor's key) is applied to the hits; the answer is ranks offset .. offset + k of what is left. The reweighted form is
sparse_oracle.search's: adj = float64(raw) * w[level], one stable descending re-sort of those k.

Test inputs keep every product a normal float, so signed zeros do not enter (a sum of normal floats from +0 is never -0)."""
import numpy as np

from sparse_oracle import LEVEL_WEIGHT, postings


def order_f32(x):
    """make_key's score half: a uint32 that orders as the floats do (and tells -0 from +0, NaNs by their bits)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def score_queries(row_off, terms, vals, vocab, q_off, q_terms, q_vals):
    """[(acc float32 [n], hit bool [n])] per query: the canonical sums (ascending terms, product and sum rounded separately) and
    the rows that share a term with the query"""
    n = len(row_off) - 1
    post_off, post_row, post_val = postings(row_off, terms, vals, vocab)
    out = []
    for q in range(len(q_off) - 1):
        acc, hit = np.zeros(n, np.float32), np.zeros(n, bool)
        for p in range(int(q_off[q]), int(q_off[q + 1])):
            t = int(q_terms[p])
            r = post_row[post_off[t]:post_off[t + 1]].astype(np.int64)
            prod = (np.float32(q_vals[p]) * post_val[post_off[t]:post_off[t + 1]]).astype(np.float32)
            acc[r] = acc[r] + prod
            hit[r] = True
        out.append((acc, hit))
    return out


def _per_query(v, nq, dtype):
    if v is None:
        return None
    v = np.asarray(v, dtype).reshape(-1)
    return np.broadcast_to(v, (nq,)) if v.size == 1 else v


def band_rows(acc, hit, id_base=0, mask=None, radius=None, range_filter=None, after=None):
    """the rows of ONE query's band, ranked: hits (inside the mask) by (order_f32 desc, id asc), then the band on them"""
    if mask is not None:
        hit = hit & np.asarray(mask, bool)
    rows = np.flatnonzero(hit)
    o = order_f32(acc[rows]).astype(np.int64)
    rows = rows[np.lexsort((rows, -o))]
    s = acc[rows]
    keep = np.ones(len(rows), bool)
    if radius is not None:
        keep &= s > np.float32(radius)
    if range_filter is not None:
        keep &= s <= np.float32(range_filter)
    if after is not None:
        o, ao = order_f32(s).astype(np.int64), int(order_f32(np.float32(after[0])).reshape(-1)[0])
        keep &= (o < ao) | ((o == ao) & (rows + id_base > int(after[1])))
    return rows[keep]


def rankings(scored, id_base=0, masks=None, radius=None, range_filter=None, after=None):
    """per query the FULL ranking of its band: [(raw float32, ids int64)]. Bounds: None, one value, or one value per query;
    after = (scores, ids) likewise."""
    nq = len(scored)
    rad, rf = _per_query(radius, nq, np.float32), _per_query(range_filter, nq, np.float32)
    a_s = None if after is None else _per_query(after[0], nq, np.float32)
    a_i = None if after is None else _per_query(after[1], nq, np.int64)
    out = []
    for q, (acc, hit) in enumerate(scored):
        rows = band_rows(acc, hit, id_base, None if masks is None else masks[q], None if rad is None else rad[q], None if rf is None else rf[q],
                         None if a_s is None else (a_s[q], a_i[q]))
        out.append((acc[rows], rows + id_base))
    return out


def search(scored, k, levels=None, id_base=0, masks=None, radius=None, range_filter=None, after=None, reweighted=False, offset=0):
    """-> (raw f32, ids i64, levels i32) [nq][k] of ranks offset .. offset + k of every band's ranking, or (adj f64, raw, ids,
    levels) with those k reweighted and re-sorted; padding -inf, -1, 0"""
    nq = len(scored)
    raw = np.full((nq, k), -np.inf, np.float32)
    ids = np.full((nq, k), -1, np.int64)
    lv = np.zeros((nq, k), np.int32)
    adj = np.full((nq, k), -np.inf, np.float64)
    for q, (r_, i_) in enumerate(rankings(scored, id_base, masks, radius, range_filter, after)):
        r_, i_ = r_[offset:offset + k], i_[offset:offset + k]
        m = len(i_)
        l_ = np.ones(m, np.int32) if levels is None else np.asarray(levels, np.int32)[i_ - id_base]
        if reweighted:
            a_ = r_.astype(np.float64) * np.array([LEVEL_WEIGHT.get(int(x), 1.0) for x in l_], np.float64)
            re = np.argsort(-a_, kind="stable")
            r_, i_, l_, a_ = r_[re], i_[re], l_[re], a_[re]
            adj[q, :m] = a_
        raw[q, :m], ids[q, :m], lv[q, :m] = r_, i_, l_
    return (adj, raw, ids, lv) if reweighted else (raw, ids, lv)


def pages(acc, hit, batch, id_base=0, mask=None, radius=None, range_filter=None, limit=-1):
    """the iterator's pages of ONE query by cursor: page i + 1 is the band behind the last hit of page i -> [[ids]]"""
    out, after, left = [], None, (None if limit == -1 else limit)
    while left is None or left > 0:
        want = batch if left is None else min(batch, left)
        rows = band_rows(acc, hit, id_base, mask, radius, range_filter, after)[:want]
        if len(rows):
            out.append([int(r) + id_base for r in rows])
            after = (acc[rows[-1]], int(rows[-1]) + id_base)
            if left is not None:
                left -= len(rows)
        if len(rows) < want:
            break
    return out
