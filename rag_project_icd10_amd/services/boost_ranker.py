"""The boost ranker of MilvusService: Milvus 2.6's {"reranker": "boost", "filter": ..., "weight": ...}.

"Rows that match this filter count `weight` times as much": the score of a row the filter selects is multiplied by the weight
BEFORE the top-k is chosen (_native.IcdIndex.search_boosted / icd_index_search_boosted), so a row at raw rank 500 can land in
the top 10 - which no rescaling of a finished hit list can do. This module holds what needs no device: the ranker with its
argument checks, the rankers of a batch, and the band-search surface (range_search) of a boosted search.

The reference has no such call (services/milvus_service.py:280-285 passes a vector and a limit).
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np

from . import filter_expr

MAX_BOOSTS = 4                          # include/icd_search.h ICD_MAX_BOOSTS: rankers per query
_MIN_NORMAL = float(np.finfo(np.float32).tiny)
_MAX = float(np.finfo(np.float32).max)


class BoostRanker:
    """One boost: `filter` a Milvus filter expression (compiled here: ValueError on a bad one), `weight` a number that is a
    positive normal float32 - above 1 lifts the rows the filter selects, below 1 demotes them. Rankers of a query apply in list
    order, one fp32 multiply each."""

    __slots__ = ("filter", "weight")

    def __init__(self, filter: str, weight: float):   # noqa: A002 (Milvus's name)
        if not isinstance(filter, str) or not filter.strip():
            raise ValueError("BoostRanker: filter is a non-empty filter expression")
        filter_expr.compile(filter)
        if isinstance(weight, bool) or not isinstance(weight, (int, float, np.integer, np.floating)):
            raise ValueError(f"BoostRanker: weight={weight!r}: a number")
        w = float(weight)
        if math.isnan(w) or math.isinf(w) or w <= 0.0:
            raise ValueError(f"BoostRanker: weight={weight!r}: a positive finite number")
        with np.errstate(over="ignore"):
            w32 = float(np.float32(w))
        if not _MIN_NORMAL <= w32 <= _MAX:
            raise ValueError(f"BoostRanker: weight={weight!r} is not a normal float32 (between {_MIN_NORMAL:g} and {_MAX:g})")
        self.filter, self.weight = filter, w32

    @classmethod
    def from_dict(cls, d) -> "BoostRanker":
        """Milvus's function parameters: {"reranker": "boost", "filter": ..., "weight": ...} (the reranker key may be left out)"""
        if not isinstance(d, dict):
            raise ValueError("a boost is a BoostRanker or a dict with filter and weight")
        if d.get("reranker", "boost") != "boost":
            raise ValueError(f"reranker={d.get('reranker')!r}: only 'boost' is served")
        if "filter" not in d or "weight" not in d:
            raise ValueError("a boost needs filter and weight")
        return cls(d["filter"], d["weight"])

    def __repr__(self) -> str:
        return f"BoostRanker({self.filter!r}, {self.weight!r})"


def _one_list(boosts) -> List[BoostRanker]:
    if isinstance(boosts, (BoostRanker, dict)):
        boosts = [boosts]
    if not isinstance(boosts, (list, tuple)):
        raise ValueError("boosts: a list of BoostRanker")
    out = [b if isinstance(b, BoostRanker) else BoostRanker.from_dict(b) for b in boosts]
    if len(out) > MAX_BOOSTS:
        raise ValueError(f"{len(out)} boosts on one query: up to {MAX_BOOSTS}")
    return out


def rankers_per_query(boosts, nq: int) -> List[List[BoostRanker]]:
    """The rankers of a batch of nq queries: `boosts` is ONE list of rankers (or dicts) for every query, or a list of nq such
    lists (None or []: that query is not boosted). ValueError on anything else."""
    if boosts is None:
        return [[] for _ in range(nq)]
    if isinstance(boosts, (BoostRanker, dict)):
        boosts = [boosts]
    if not isinstance(boosts, (list, tuple)):
        raise ValueError("boosts: a list of BoostRanker, or one such list per query")
    if any(b is None or isinstance(b, (list, tuple)) for b in boosts):   # one list per query
        if len(boosts) != nq:
            raise ValueError(f"boosts holds {len(boosts)} lists for {nq} queries")
        return [[] if b is None else _one_list(b) for b in boosts]
    shared = _one_list(boosts)
    return [shared for _ in range(nq)]


class BoostedIndex:
    """An (index, workspace, boosts, masks) bundle with an index's band-search surface (range_search): search_range runs
    IcdIndex.search_boosted - bounds, cursor and pages are then those of the BOOSTED ranking. boosts: per query a list of
    (IcdRowMask, weight); masks: None or one entry (IcdRowMask or None) per query. Holds references to the masks it pages over."""

    def __init__(self, index, workspace, boosts: Sequence, masks: Optional[Sequence] = None):
        self.index, self.workspace, self.boosts, self.masks = index, workspace, boosts, masks

    @property
    def max_k(self) -> int:
        return self.index.max_k

    def all_masks(self):
        for per in self.boosts:
            for pair in per or ():
                if pair is not None:
                    yield pair[0]
        for m in self.masks or ():
            if m is not None:
                yield m

    @property
    def closed(self) -> bool:
        return self.index.closed or self.workspace.closed or any(m.closed for m in self.all_masks())

    def search_range(self, queries, k, **kw):
        return self.index.search_boosted(queries, k, self.boosts, self.masks, workspace=self.workspace, **kw)
