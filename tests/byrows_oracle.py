"""What a search by stored rows must return, as a walk over the FULL ranking of every query
(oracle.flat_ip_topk at k = n of the named rows' own stored values: scores and ids, best first by (score desc, id asc)).

Query q names row ids[q] of the index. Two statements of its answer, which must agree:

  without_self   the masked / range search (mask_oracle: keep the mask's rows, then the band, the k best, then the level reweight
                 of those k) over the ranking with the entry of id ids[q] taken out first;
  drop_self      the masked search's RAW list at k + 1; the entry of id ids[q] removed and the gap closed, or - the id is not in
                 the list: the row is outside its own mask or band, or holds a NaN - the last entry dropped; then the level
                 reweight of the k that stay.

include_self: the masked search at k itself. Everything is exact: there is no tolerance anywhere.

No device code and nothing of the package under test: numpy only.
"""
import numpy as np

from mask_oracle import _per_query, restrict
from range_oracle import band_query, reweight


def _rows(mask, levels):
    """no mask: every ROW of the index (levels holds one entry per row; a ranking that left NaN rows out is shorter than that)"""
    return np.ones(len(levels), bool) if mask is None else mask


def without_self(scores, ids, levels, self_id, k, mask=None, radius=None, range_filter=None, id_base=0, include_self=False):
    """one query, statement 1: ((raw, ids, levels) in raw order, (adj, raw, ids, levels) reweighted), each of length k, padded"""
    s, i = restrict(scores, ids, _rows(mask, levels), id_base)
    if not include_self:
        keep = i != int(self_id)
        s, i = s[keep], i[keep]
    return band_query(s, i, levels, k, radius, range_filter, None, 0, id_base)


def drop_from_list(raw, ids, lv, self_id):
    """the (k + 1)-wide raw list of one query -> the k-wide one: self removed and the gap closed, else the last entry dropped"""
    raw, ids, lv = np.asarray(raw, np.float32), np.asarray(ids, np.int64), np.asarray(lv, np.int32)
    at = np.flatnonzero(ids == int(self_id))
    gap = int(at[0]) if len(at) else len(ids) - 1
    keep = np.arange(len(ids)) != gap
    return raw[keep], ids[keep], lv[keep]


def drop_self(scores, ids, levels, self_id, k, mask=None, radius=None, range_filter=None, id_base=0, include_self=False):
    """one query, statement 2"""
    s, i = restrict(scores, ids, _rows(mask, levels), id_base)
    if include_self:
        return band_query(s, i, levels, k, radius, range_filter, None, 0, id_base)
    (raw, rid, lv), _ = band_query(s, i, levels, k + 1, radius, range_filter, None, 0, id_base)
    raw, rid, lv = drop_from_list(raw, rid, lv, self_id)
    return (raw, rid, lv), reweight(raw, rid, lv)


def byrows_batch(scores, ids, levels, self_ids, k, masks=None, radius=None, range_filter=None, id_base=0, include_self=False,
                 statement=without_self):
    """A batch. scores / ids: the full ranking of every query (the named row's stored values against the corpus; slots without a
    row - NaN scores - may hold id -1 and are dropped). masks: None or one entry per query (None, boolean array over rows, row
    list); radius / range_filter: None, scalars or one value per query. Returns ((raw f32, ids i64, levels i32) in raw order,
    (adj f64, raw, ids, levels) reweighted), each [nq, k], padded (-inf, -1, 0)."""
    nq = len(self_ids)
    raws, adjs = [], []
    for q in range(nq):
        valid = np.asarray(ids[q]) >= 0
        s, i = np.asarray(scores[q], np.float32)[valid], np.asarray(ids[q], np.int64)[valid]
        r, a = statement(s, i, levels, self_ids[q], k, None if masks is None else masks[q], _per_query(radius, q),
                         _per_query(range_filter, q), id_base, include_self)
        raws.append(r)
        adjs.append(a)
    if nq == 0:
        return ((np.zeros((0, k), np.float32), np.zeros((0, k), np.int64), np.zeros((0, k), np.int32)),
                (np.zeros((0, k), np.float64), np.zeros((0, k), np.float32), np.zeros((0, k), np.int64), np.zeros((0, k), np.int32)))
    return tuple(np.stack([r[j] for r in raws]) for j in range(3)), tuple(np.stack([a[j] for a in adjs]) for j in range(4))


def drop_reweighted_list(adj, raw, ids, lv, self_id):
    """The REWEIGHTED (k + 1)-wide list of the masked search -> the reweighted k-wide answer, for the equality the device test
    holds against icd_index_search_masked at k + 1. Self present: removed, the gap closed (a stable sort of a subset is the
    subset of the stable sort). Self absent: the entry that is last in RAW order goes - the last padding slot when there is one,
    else the hit of the smallest (score, then largest id) - because the answer is the k best by raw score, re-sorted."""
    adj, raw, ids, lv = np.asarray(adj), np.asarray(raw), np.asarray(ids), np.asarray(lv)
    at = np.flatnonzero(ids == int(self_id))
    if len(at):
        gap = int(at[0])
    elif (ids < 0).any():
        gap = len(ids) - 1
    else:
        gap = max(range(len(ids)), key=lambda j: (-float(raw[j]), int(ids[j])))
    keep = np.arange(len(ids)) != gap
    return adj[keep], raw[keep], ids[keep], lv[keep]
