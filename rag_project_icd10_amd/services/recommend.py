"""Recommend search on the service level: "more like these, less like those" - the exact ranking of the whole
collection by positive and negative examples, in ONE device call. Every other entry point takes one thing per query; none can use
the verdicts a coder gives on a hit list. Additive, beside MilvusService - whose public surface is recorded and stays as it is -
in the way services/wide_search.py stands beside it: Recommend wraps a MilvusService and goes through ITS helpers for everything the
entry points share (the live index, the code -> row table of similar_codes, the filter checks, the leased masks of the mask cache /
device programs / TEXT_MATCH route, the workspace cache, the hit dicts); nothing of them is copied here.

    rec = Recommend(milvus_service)
    rec.recommend(positive=["K35.8", "急性阑尾炎伴腹膜炎"], negative=["K36"], strategy="best_score", top_k=10, filter='level >= 2')
    lists, totals = rec.recommend_batch(positive=[[12, 40], ["A01"]], negative=[[7], []], strategy="sum_scores", with_totals=True)

An example is a code (a string that is a stored code), an int id, a text (any other string: embedded, all texts of a batch in one
encode_query_batch) or a vector. A request's stored examples never come back as hits.
"""
from __future__ import annotations

import logging
from typing import Any, Dict, List, Optional

import numpy as np

from . import range_search, wide_search

logger = logging.getLogger(__name__)

MAX_EXAMPLES = 16                      # positive + negative examples of one request (ICD_RECOMMEND_MAX_EXAMPLES)
MAX_TOP_K = wide_search.MAX_TOP_K      # offset + top_k of one call (ICD_WIDE_MAX_K)
STRATEGIES = ("average_vector", "best_score", "sum_scores")


def make_workspace(index, size: int):
    """the recommend workspace of `index` for `size` requests per call (MilvusService._workspace_for's factory for the kind "recommend")"""
    from .. import _native
    return _native.IcdRecommend(index, size, None, MAX_TOP_K)


class Recommend:
    """recommend / recommend_batch over one MilvusService"""

    def __init__(self, milvus_service):
        self.ms = milvus_service

    def _examples(self, positive, negative, strategy):
        """the requests' examples checked without a store: per request (positives, negatives) as lists of str / int / float32
        vector; ValueError on a bad one"""
        if strategy not in STRATEGIES:
            raise ValueError(f"strategy={strategy!r}: one of {STRATEGIES}")
        if isinstance(positive, str) or not isinstance(positive, (list, tuple)):
            raise ValueError("positive: one list of examples per request")
        nr = len(positive)
        negative = [[] for _ in range(nr)] if negative is None else negative
        if isinstance(negative, str) or not isinstance(negative, (list, tuple)) or len(negative) != nr:
            raise ValueError(f"negative: one list of examples per request ({nr} requests)")

        def one(ex):
            if isinstance(ex, str):
                if not ex:
                    raise ValueError("examples: non-empty strings")
                return ex
            if self.ms._int_in(ex):
                if ex < 0:
                    raise ValueError(f"examples: id {ex} is negative")
                return int(ex)
            if isinstance(ex, bool) or np.ndim(ex) != 1 or not np.size(ex):
                raise ValueError("examples: a code, an int id, a text or a vector")
            return np.ascontiguousarray(ex, dtype=np.float32)

        out = []
        for pos, neg in zip(positive, negative):
            if isinstance(pos, str) or isinstance(neg, str) or not isinstance(pos, (list, tuple)) or not isinstance(neg, (list, tuple)):
                raise ValueError("positive / negative: a list of examples per request")
            if not 1 <= len(pos) + len(neg) <= MAX_EXAMPLES:
                raise ValueError(f"a request holds 1 .. {MAX_EXAMPLES} examples, got {len(pos) + len(neg)}")
            if strategy == "average_vector" and not pos:
                raise ValueError("average_vector needs a positive example")
            out.append(([one(e) for e in pos], [one(e) for e in neg]))
        return out

    def recommend_batch(self, positive, negative=None, strategy: str = "average_vector", top_k: int = 10, filter=None,   # noqa: A002
                        radius=None, range_filter=None, offset: int = 0, as_dicts: bool = True, with_totals: bool = False):
        """Additive: per request ranks offset .. offset + top_k - 1 of the collection's exact ranking by the request's examples
        (DESIGN.md section 28), 1 <= top_k and offset + top_k <= 16 384, re-sorted by adjusted score like any hit list.
        positive / negative: one list of examples per request (negative None: none anywhere), 1 .. 16 examples a request; an
        example is a stored code, an int id, a text or a vector. strategy: "average_vector" (one target vector: the positives'
        mean, pushed away from the negatives' mean), "best_score" (the best positive score, unless a negative scores at least as
        high) or "sum_scores" (positives' scores minus negatives'). filter: one expression for the batch or a list with one (or
        None) per request, as row masks; radius / range_filter: only rows with radius < combined score <= range_filter rank.
        Returns one `search`-shaped hit list per request (`original_score` is the combined score), or with as_dicts=False (adj,
        raw, ids, levels) [nr, top_k] padded; with_totals=True: a pair of that and the rows that rank per request. An id outside
        the collection raises KeyError. A bad argument raises ValueError before anything is loaded; a runtime failure is logged
        and gives empty lists, as `search_batch` does."""
        top_k = wide_search.check_top_k(top_k)
        radius, range_filter = range_search.check_bounds(radius, range_filter, None)
        offset = range_search.check_offset(offset, top_k)
        requests = self._examples(positive, negative, strategy)
        nr = len(requests)
        self.ms._check_filter_args(filter, "mask", None, nr)

        def shaped(adj, raw, ids, levels, totals):
            out = self.ms._hit_lists(adj, raw, ids) if as_dicts else (adj, raw, ids, levels)
            return (out, totals) if with_totals else out

        def empty():
            return shaped(np.full((nr, top_k), -np.inf, np.float64), np.full((nr, top_k), -np.inf, np.float32), np.full((nr, top_k), -1, np.int64),
                          np.zeros((nr, top_k), np.int32), np.zeros(nr, np.int64))
        index = self.ms._live_index()
        if index is None or nr == 0:
            return empty()
        # strings: a stored code is that row, anything else is a text - all texts of the batch in ONE encode_query_batch
        texts: List[str] = []
        resolved = []
        for pos, neg in requests:
            sides = []
            for side in (pos, neg):
                got = []
                for ex in side:
                    if isinstance(ex, str):
                        row = self.ms._row_of_code(ex)
                        if row is None:
                            texts.append(ex)
                            got.append(("text", len(texts) - 1))
                        else:
                            got.append(int(row))
                    elif isinstance(ex, int):
                        if ex >= index.n:
                            raise KeyError(ex)
                        got.append(ex)
                    else:
                        if ex.shape[0] != index.dim:
                            raise ValueError(f"example dim {ex.shape[0]} != index dim {index.dim}")
                        got.append(ex)
                sides.append(got)
            resolved.append(sides)
        if texts:
            if self.ms.embedding_service is None:
                raise ValueError("examples: texts need an embedding service")
            emb = np.ascontiguousarray(np.asarray(self.ms.embedding_service.encode_query_batch(texts), dtype=np.float32).reshape(len(texts), -1))
            if emb.shape[-1] != index.dim:
                raise ValueError(f"embedding dim {emb.shape[-1]} != index dim {index.dim}")
            resolved = [[[emb[e[1]] if isinstance(e, tuple) else e for e in side] for side in sides] for sides in resolved]
        try:
            with self.ms._leased_masks(index, filter, nr) as masks:
                adj, raw, ids, levels, _count, selected = self.ms._workspace_for("recommend", index, nr).recommend(
                    [s[0] for s in resolved], [s[1] for s in resolved], strategy, top_k, masks=masks, radius=radius, range_filter=range_filter,
                    first=offset, reweighted=True)
            return shaped(adj, raw, ids, levels, np.asarray(selected, np.int64))
        except ValueError:
            raise
        except Exception as exc:
            logger.error("搜索失败: %s", exc)
            return empty()

    def recommend(self, positive, negative=None, strategy: str = "average_vector", top_k: int = 10, filter: Optional[str] = None,   # noqa: A002
                  radius: Optional[float] = None, range_filter: Optional[float] = None, offset: int = 0) -> List[Dict[str, Any]]:
        """the `search`-shaped hits of ONE request: positive / negative are its lists of examples (recommend_batch)"""
        self.ms._one_filter(filter, "a list of filters needs a batch: one expression (or None) per request of recommend_batch")
        if isinstance(positive, str) or not isinstance(positive, (list, tuple)) or (negative is not None and (isinstance(negative, str) or not isinstance(negative, (list, tuple)))):
            raise ValueError("positive / negative: lists of examples")
        return self.recommend_batch([list(positive)], [list(negative or [])], strategy, top_k, filter=filter, radius=radius,
                                    range_filter=range_filter, offset=offset, as_dicts=True)[0]
