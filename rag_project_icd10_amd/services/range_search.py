"""Range search, offset and the search iterator of MilvusService.

One definition serves all three: "the k best rows strictly inside a band of a query's (score desc, id asc) ranking" -
_native.IcdIndex.search_range / icd_index_search_range. This module holds what sits on top of that call and needs no device:
the argument rules (Milvus's `radius` / `range_filter`, also spelled search_params={"params": {...}}; `offset`), the level
reweight of a page on the host (the arithmetic of icd_index_search_reweighted: adj = float64(raw) * w[level], one stable
descending re-sort), the cursor walk of a large offset, and the iterator.

The reference passes none of these arguments (services/milvus_service.py:280-285).
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

MAX_WINDOW = 16384   # Milvus's limit on offset + limit
PAGE = 128           # include/icd_search.h ICD_MAX_K: the hits of one call


def level_weights(levels: np.ndarray) -> np.ndarray:
    """w[level] of services/milvus_service.py:550-558 (1 -> 1.2, 3 -> 0.8, anything else 1.0) as float64"""
    lv = np.asarray(levels)
    return np.where(lv == 1, 1.2, np.where(lv == 3, 0.8, 1.0))


def check_bounds(radius=None, range_filter=None, search_params: Optional[Dict[str, Any]] = None) -> Tuple[Optional[float], Optional[float]]:
    """(radius, range_filter) as floats or None, from the keyword arguments or Milvus's search_params={"params": {...}} (also
    accepted flat: {"radius": ...}); hits have radius < score <= range_filter. ValueError: a bound given twice with different
    values, a non-number, NaN, or radius >= range_filter."""
    if search_params is not None:
        if not isinstance(search_params, dict):
            raise ValueError("search_params must be a dict")
        inner = search_params.get("params", search_params)
        if not isinstance(inner, dict):
            raise ValueError('search_params["params"] must be a dict')
        for name in ("radius", "range_filter"):
            if inner.get(name) is None:
                continue
            given = radius if name == "radius" else range_filter
            if given is not None and float(given) != float(inner[name]):
                raise ValueError(f"{name} given twice with different values")
            if name == "radius":
                radius = inner[name]
            else:
                range_filter = inner[name]
    out = []
    for name, v in (("radius", radius), ("range_filter", range_filter)):
        if v is None:
            out.append(None)
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{name} must be a number")
        v = float(np.float32(v))   # (the comparison runs on the fp32 score)
        if math.isnan(v):
            raise ValueError(f"{name} is NaN")
        out.append(v)
    if out[0] is not None and out[1] is not None and not out[0] < out[1]:
        raise ValueError(f"radius={out[0]} must be below range_filter={out[1]} (hits have radius < score <= range_filter)")
    return out[0], out[1]


def check_offset(offset, top_k: int) -> int:
    if isinstance(offset, bool) or not isinstance(offset, (int, np.integer)):
        raise ValueError("offset must be an integer")
    offset = int(offset)
    if offset < 0 or offset + int(top_k) > MAX_WINDOW:
        raise ValueError(f"offset={offset}, top_k={top_k}: need offset >= 0 and offset + top_k <= {MAX_WINDOW}")
    return offset


def reweight_page(raw: np.ndarray, ids: np.ndarray, levels: np.ndarray):
    """A raw-order page [nq, k] (padding: -inf, -1, 0) -> (adj f64, raw, ids, levels) in icd_index_search_reweighted's order:
    adj = float64(raw) * w[level], one stable descending re-sort of every query's hits (padding stays behind them)"""
    raw, ids, levels = np.asarray(raw), np.asarray(ids), np.asarray(levels)
    adj = raw.astype(np.float64) * level_weights(levels)
    adj[ids < 0] = -np.inf
    order = np.argsort(-adj, axis=1, kind="stable")
    take = lambda a: np.take_along_axis(a, order, axis=1)
    return take(adj), take(raw), take(ids), take(levels)


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _cursor_of(raw: np.ndarray, ids: np.ndarray, want: int):
    """per query: the raw-order LAST hit of a page (its smallest key) as the next cursor, and whether the page was full. A query
    whose band is exhausted gets the cursor nothing ranks behind (-inf, the largest id)."""
    valid = (ids >= 0).sum(axis=1)
    full = valid >= want
    last = np.maximum(valid - 1, 0)
    rows = np.arange(len(ids))
    sc = np.where(full, raw[rows, last], -np.inf).astype(np.float32)
    cid = np.where(full, ids[rows, last], np.iinfo(np.int64).max).astype(np.int64)
    return sc, cid


class MaskedIndex:
    """An (index, masks) pair with an index's band-search surface: search_range runs IcdIndex.search_masked with the pair's
    masks - ONE IcdRowMask for every query, or one entry (IcdRowMask or None) per query. Holds a reference
    to its masks: a mask evicted from a cache lives as long as a pair that pages over it."""

    def __init__(self, index, masks):
        self.index, self.masks = index, masks

    @property
    def max_k(self) -> int:
        return self.index.max_k

    @property
    def closed(self) -> bool:
        ms = self.masks if isinstance(self.masks, (list, tuple)) else [self.masks]
        return self.index.closed or any(m is not None and m.closed for m in ms)

    def search_range(self, queries, k, **kw):
        return self.index.search_masked(queries, k, self.masks, **kw)


class SparseBandIndex:
    """An (index, sparse index, masks) triple with an index's band-search surface: search_range runs
    IcdIndex.search_sparse with the band, its `queries` are the CSR triple (q_off, q_terms, q_vals) of host arrays. masks: None,
    ONE IcdRowMask for every query, or one entry (IcdRowMask or None) per query. A batch longer than the sparse index's max_nq
    is sent in pieces, per-query bounds sliced with it. Holds references to the sparse index and the masks it pages over."""

    def __init__(self, index, sparse, masks=None):
        self.index, self.sparse, self.masks = index, sparse, masks

    @property
    def max_k(self) -> int:
        return min(int(self.index.max_k), int(self.sparse.max_k))

    @property
    def closed(self) -> bool:
        ms = self.masks if isinstance(self.masks, (list, tuple)) else [self.masks]
        return self.index.closed or self.sparse.closed or any(m is not None and m.closed for m in ms)

    def search_range(self, queries, k, *, radius=None, range_filter=None, after=None, reweighted: bool = True):
        q_off, q_terms, q_vals = queries
        q_off = np.asarray(q_off, np.int64).reshape(-1)
        nq, step = len(q_off) - 1, int(self.sparse.max_nq)
        if nq <= step:
            return self.index.search_sparse(self.sparse, q_off, q_terms, q_vals, k, masks=self.masks, reweighted=reweighted,
                                            radius=radius, range_filter=range_filter, after=after)
        per_query = isinstance(self.masks, (list, tuple))

        def part(v, s0, s1):   # a per-query bound's slice (a scalar serves every piece)
            return v if v is None or np.ndim(v) == 0 or np.size(v) == 1 else np.asarray(v).reshape(-1)[s0:s1]
        outs = []
        for s0 in range(0, nq, step):
            s1 = min(nq, s0 + step)
            a, b = int(q_off[s0]), int(q_off[s1])
            outs.append(self.index.search_sparse(
                self.sparse, q_off[s0:s1 + 1] - a, q_terms[a:b], q_vals[a:b], k, masks=self.masks[s0:s1] if per_query else self.masks,
                reweighted=reweighted, radius=part(radius, s0, s1), range_filter=part(range_filter, s0, s1),
                after=None if after is None else (part(after[0], s0, s1), part(after[1], s0, s1))))
        return tuple(np.concatenate([o[i] for o in outs]) for i in range(len(outs[0])))


def check_bounds_per_query(radius, range_filter, nq: int, search_params: Optional[Dict[str, Any]] = None):
    """check_bounds for bounds that may hold one value PER QUERY (arrays of nq numbers): every query's pair goes through
    check_bounds. -> (radius, range_filter), each None, a float, or a float32 array [nq]."""
    def scalar(v):
        return v is None or np.ndim(v) == 0
    if scalar(radius) and scalar(range_filter):
        return check_bounds(radius, range_filter, search_params)
    if search_params is not None:
        raise ValueError("per-query bounds are given as radius / range_filter arrays, not through search_params")
    cols = []
    for name, v in (("radius", radius), ("range_filter", range_filter)):
        if not scalar(v):
            v = _host(v).reshape(-1)
            if len(v) != nq:
                raise ValueError(f"{name} holds {len(v)} values for {nq} queries")
            v = [x.item() if isinstance(x, np.generic) else x for x in v]
        cols.append(v)
    pairs = [check_bounds(cols[0] if scalar(cols[0]) else cols[0][q], cols[1] if scalar(cols[1]) else cols[1][q]) for q in range(nq)]
    return tuple(None if cols[i] is None else (pairs[0][i] if scalar(cols[i]) and pairs else np.array([p[i] for p in pairs], np.float32))
                 for i in range(2))


def _band_index(index):
    """an index, a view, or the pair (index, masks) -> the object whose search_range serves it"""
    return MaskedIndex(*index) if isinstance(index, tuple) else index


def search_band(index, queries, k: int, radius=None, range_filter=None, offset: int = 0):
    """(adj, raw, ids, levels), each [nq, k], of ranks offset .. offset + k of every query's band ranking (raw order), then
    reweighted and re-sorted. offset + k <= the index's page: ONE search and a slice; beyond: the skipped ranks are walked with raw
    pages (`after` cursor) and only the last page is reweighted - ceil(offset / page) extra searches. Device tensors in -> device
    tensors out (offset = 0 never leaves the device). index: an IcdIndex (or view), or the pair (index, masks) of a masked search -
    the ranking is then every query's own mask's."""
    index = _band_index(index)
    k, offset = int(k), int(offset)
    if offset == 0:
        return index.search_range(queries, k, radius=radius, range_filter=range_filter)
    page = min(PAGE, int(index.max_k))
    device = queries.device if hasattr(queries, "is_cuda") and queries.is_cuda else None
    if offset + k <= page:
        raw, ids, lv = (_host(t) for t in index.search_range(queries, offset + k, radius=radius, range_filter=range_filter, reweighted=False))
        out = reweight_page(raw[:, offset:], ids[:, offset:], lv[:, offset:])
    else:
        sc, cid, left = None, None, offset
        while left > 0:
            step = min(page, left)
            after = None if sc is None else (sc, cid)
            raw, ids, _ = (_host(t) for t in index.search_range(queries, step, radius=radius, range_filter=range_filter, after=after, reweighted=False))
            sc, cid = _cursor_of(raw, ids, step)
            left -= step
        out = tuple(_host(t) for t in index.search_range(queries, k, radius=radius, range_filter=range_filter, after=(sc, cid)))
    if device is not None:
        import torch
        return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in out)
    return tuple(np.ascontiguousarray(a) for a in out)


class SearchIterator:
    """pymilvus's iterator surface: next() -> a `search`-shaped hit list of up to batch_size hits ([] when exhausted), close().
    Page i + 1 is the band search behind the raw-order LAST hit of page i, so pages are disjoint and their raw-order concatenation
    is the band's full ranking; every page is handed out re-sorted by adjusted score like any hit list. The iterator pins the
    index (or filter view, or the pair (index, mask) of a masked search, or the SparseBandIndex of a sparse search - the query
    is then the CSR triple of ONE query) and the store generation it started on: after a mutation
    of the store next() raises RuntimeError instead of paging through two different corpora. One launch per next() at
    batch_size <= 16."""

    def __init__(self, index, query_vector, batch_size: int, limit: int, radius, range_filter, to_hits, generation_of):
        index = None if index is None else _band_index(index)
        if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
            raise ValueError("batch_size must be a positive integer")
        page = PAGE if index is None else min(PAGE, int(index.max_k))
        if batch_size > page:
            raise ValueError(f"batch_size={batch_size} exceeds the {page} hits of one search")
        if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or (limit < 0 and limit != -1):
            raise ValueError("limit must be -1 (no limit) or a non-negative integer")
        self._index = index
        if index is None:
            self._q = None
        elif isinstance(query_vector, tuple):   # ONE sparse query as its CSR triple (q_off, q_terms, q_vals): SparseBandIndex
            self._q = query_vector
        else:
            self._q = np.ascontiguousarray(query_vector, dtype=np.float32).reshape(1, -1)
        self._batch, self._left = int(batch_size), (None if limit == -1 else int(limit))
        self._radius, self._range_filter = radius, range_filter
        self._to_hits, self._generation_of = to_hits, generation_of
        self._generation = generation_of()
        self._cursor = None
        self._done = index is None
        self.last_raw_ids: List[int] = []   # the last page's ids in RAW order (its last entry is the cursor)

    def next(self) -> List[Dict[str, Any]]:   # noqa: A003 (pymilvus's name)
        if self._done or (self._left is not None and self._left <= 0):
            self._done = True
            return []
        if self._generation_of() != self._generation or self._index.closed:
            raise RuntimeError("the collection changed under the iterator: start a new search_iterator")
        want = self._batch if self._left is None else min(self._batch, self._left)
        raw, ids, lv = self._index.search_range(self._q, want, radius=self._radius, range_filter=self._range_filter,
                                                after=self._cursor, reweighted=False)
        valid = int((ids[0] >= 0).sum())
        self.last_raw_ids = [int(i) for i in ids[0][:valid]]
        if valid < want:
            self._done = True
        if valid == 0:
            return []
        self._cursor = (np.float32(raw[0][valid - 1]), np.int64(ids[0][valid - 1]))
        if self._left is not None:
            self._left -= valid
        adj, raw_s, ids_s, _ = reweight_page(raw[:, :valid], ids[:, :valid], lv[:, :valid])
        return self._to_hits(adj[0], raw_s[0], ids_s[0])

    def close(self):
        self._done = True
        self._index = None
