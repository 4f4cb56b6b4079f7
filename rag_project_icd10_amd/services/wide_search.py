"""Wide search on the service level: the exact top_k of a query for top_k up to 16 384 in ONE device call -
a candidate list for a re-ranker, recall@1000, a deep offset, everything above a similarity floor. `MilvusService.search` stops
at 128 hits and serves a deep offset by paging (services/range_search.py). Additive, beside MilvusService - whose public surface
is recorded and stays as it is - in the way services/rank_of.py stands beside it: WideSearch wraps a MilvusService and goes
through ITS helpers for everything the entry points share (the live index, the filter checks, the leased masks of the mask cache /
device programs / TEXT_MATCH route, the workspace cache, the hit dicts); nothing of them is copied here.

    wide = WideSearch(milvus_service)
    wide.search_wide(vector, top_k=1000, filter='level >= 2')
    lists, totals = wide.search_wide_batch(vectors, 2000, radius=0.3, as_dicts=True, with_totals=True)
"""
from __future__ import annotations

import logging
from typing import Any, Dict, List, Optional

import numpy as np

from . import range_search

logger = logging.getLogger(__name__)

MAX_TOP_K = range_search.MAX_WINDOW   # offset + top_k of one call (ICD_WIDE_MAX_K, Milvus's window)


def make_workspace(index, size: int):
    """the wide-search workspace of `index` for `size` queries per call (MilvusService._workspace_for's factory for the kind "wide")"""
    from .. import _native
    return _native.IcdWide(index, size, MAX_TOP_K)


def check_top_k(top_k) -> int:
    if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or not 1 <= int(top_k) <= MAX_TOP_K:
        raise ValueError(f"top_k={top_k!r}: an integer in 1 .. {MAX_TOP_K}")
    return int(top_k)


class WideSearch:
    """search_wide / search_wide_batch over one MilvusService"""

    def __init__(self, milvus_service):
        self.ms = milvus_service

    def search_wide_batch(self, query_vectors, top_k: int, filter=None, radius=None, range_filter=None, offset: int = 0,   # noqa: A002
                          search_params: Optional[Dict[str, Any]] = None, as_dicts: bool = False, with_totals: bool = False):
        """Additive: ranks offset .. offset + top_k - 1 of every query's exact ranking, 1 <= top_k and offset + top_k <= 16 384,
        re-sorted by adjusted score like any hit list. query_vectors: [nq, dim]; filter: one expression for the batch or a list
        with one (or None) per query - always as row masks of the store's index (device programs, TEXT_MATCH, the mask cache);
        radius / range_filter (or Milvus's search_params): only rows with radius < inner product <= range_filter rank. Returns
        (adj f64, raw f32, ids i64, levels i32), each [nq, top_k] and padded (-inf, -1, 0), or with as_dicts=True one
        `search`-shaped hit list per query; with_totals=True: a pair of that and the rows that rank per query (int64 [nq]; without
        a band: count(filter)). A bad argument raises ValueError before anything is loaded; a runtime failure is logged and gives
        empty lists, as `search_batch` does."""
        top_k = check_top_k(top_k)
        radius, range_filter = range_search.check_bounds(radius, range_filter, search_params)
        offset = range_search.check_offset(offset, top_k)
        q = np.asarray(query_vectors, dtype=np.float32)
        if q.ndim != 2:
            raise ValueError("query_vectors: [nq, dim]")
        q = np.ascontiguousarray(q)
        nq = int(q.shape[0])
        self.ms._check_filter_args(filter, "mask", None, nq)

        def shaped(adj, raw, ids, levels, totals):
            out = self.ms._hit_lists(adj, raw, ids) if as_dicts else (adj, raw, ids, levels)
            return (out, totals) if with_totals else out

        def empty():
            return shaped(np.full((nq, top_k), -np.inf, np.float64), np.full((nq, top_k), -np.inf, np.float32), np.full((nq, top_k), -1, np.int64),
                          np.zeros((nq, top_k), np.int32), np.zeros(nq, np.int64))
        try:
            index = self.ms._live_index()
            if index is None or nq == 0:
                return empty()
            if q.shape[-1] != index.dim:
                raise ValueError(f"query dim {q.shape[-1]} != index dim {index.dim}")
            with self.ms._leased_masks(index, filter, nq) as masks:
                adj, raw, ids, levels, _count, selected = self.ms._workspace_for("wide", index, nq).search_wide(
                    q, top_k, masks=masks, radius=radius, range_filter=range_filter, first=offset, reweighted=True)
            return shaped(adj, raw, ids, levels, np.asarray(selected, np.int64))
        except ValueError:
            raise
        except Exception as exc:
            logger.error("搜索失败: %s", exc)
            return empty()

    def search_wide(self, query_vector, top_k: int, filter: Optional[str] = None, radius: Optional[float] = None,   # noqa: A002
                    range_filter: Optional[float] = None, offset: int = 0, search_params: Optional[Dict[str, Any]] = None) -> List[Dict[str, Any]]:
        """the `search`-shaped hits of ONE query vector at top_k up to 16 384 (search_wide_batch)"""
        self.ms._one_filter(filter, "a list of filters needs a batch: one expression (or None) per query of search_wide_batch")
        if np.ndim(query_vector) != 1:
            raise ValueError("query_vector: one vector")
        return self.search_wide_batch(np.asarray(query_vector, dtype=np.float32).reshape(1, -1), top_k, filter=filter, radius=radius,
                                      range_filter=range_filter, offset=offset, search_params=search_params, as_dicts=True)[0]
