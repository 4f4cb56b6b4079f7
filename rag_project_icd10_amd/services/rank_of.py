"""Rank-of search on the service level: where do given codes land in a query's exact ranking over the whole
collection, and the evaluation metrics that follow from it. Additive, beside MilvusService - whose public surface is recorded
and stays as it is - in the way services/range_search.py and services/boost_ranker.py stand beside it: RankOf wraps a
MilvusService and goes through ITS helpers for everything the entry points share (the live index, the code -> row table of
similar_codes, the filter checks, the leased masks of the mask cache / device programs / TEXT_MATCH route, the workspace cache);
nothing of them is copied here.

    ranks = RankOf(milvus_service)
    ranks.rank_of("急性阑尾炎", ["K35.8"], filter='level >= 2')
    ranks.evaluate([(text, "K35.8"), (text2, ["A01.0", "A01"])], ks=(1, 5, 10))
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import numpy as np

MAX_CODES = 16   # codes per query of one call (ICD_RANKOF_MAX_TARGETS)


def make_workspace(index, size: int):
    """the rank-of workspace of `index` for `size` queries per call (MilvusService._workspace_for's factory for the kind "rankof")"""
    from .. import _native
    return _native.IcdRankOf(index, size)


class RankOf:
    """rank_of / rank_of_batch / evaluate over one MilvusService"""

    def __init__(self, milvus_service):
        self.ms = milvus_service


    def _rank_queries(self, queries) -> np.ndarray:
        """the queries of a rank-of batch as float32 [nq, dim]: vectors (one, or [nq, dim]) as they are, texts (one string, or a
        list of strings) through the embedding service's encode_query_batch; ValueError on anything else"""
        texts = [queries] if isinstance(queries, str) else (list(queries) if isinstance(queries, (list, tuple)) and queries and all(isinstance(q, str) for q in queries) else None)
        if texts is not None:
            if self.ms.embedding_service is None:
                raise ValueError("queries: texts need an embedding service")
            return np.ascontiguousarray(np.asarray(self.ms.embedding_service.encode_query_batch(texts), dtype=np.float32).reshape(len(texts), -1))
        if isinstance(queries, (list, tuple)) and any(isinstance(q, str) for q in queries):
            raise ValueError("queries: vectors or texts, not both")
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim == 1 and q.size:
            q = q.reshape(1, -1)
        if q.ndim != 2:
            raise ValueError("queries: [nq, dim] vectors (or one vector), a text or a list of texts")
        return np.ascontiguousarray(q)

    def _rank_codes(self, codes_per_query, nq: int):
        """codes_per_query checked without a store: one list of 1 .. MAX_CODES code strings per query (a bare string is a
        list of one); ValueError on a bad one"""
        if isinstance(codes_per_query, str) or not isinstance(codes_per_query, (list, tuple)) or len(codes_per_query) != nq:
            raise ValueError(f"codes_per_query: one list of codes per query ({nq} queries)")
        out = []
        for codes in codes_per_query:
            codes = [codes] if isinstance(codes, str) else codes
            if not isinstance(codes, (list, tuple)) or not 1 <= len(codes) <= MAX_CODES:
                raise ValueError(f"codes: 1 .. {MAX_CODES} codes per query")
            if any(not isinstance(c, str) or not c for c in codes):
                raise ValueError("codes: non-empty strings")
            out.append(list(codes))
        return out

    def rank_of_batch(self, queries, codes_per_query, filter=None) -> List[List[Dict[str, Any]]]:   # noqa: A002
        """Additive: for every query the EXACT rank of given codes in its ranking over the whole collection -
        the position `search_batch(..., filter_mode="mask")` in raw order would return the code at, for ranks past the largest k
        too. queries: [nq, dim] vectors (or one) or texts (a string or a list, through the embedding service); codes_per_query:
        per query a list of 1 .. 16 code strings (or one string), looked up as `similar_codes` does - an unknown code raises
        KeyError. filter: one expression for the batch or a list with one (or None) per query, as row masks. Returns per query a
        list of {code, rank, score, raw_score, level, selected}: rank counts the selected rows strictly ahead (0 = best) and is
        None - with score and raw_score None - where the filter leaves the code out; score is the level-adjusted score, raw_score
        the inner product, selected the rows the filter admits. Batches above the store's max_batch run in slices. An empty or
        unloaded collection answers [] per query. Bad arguments raise ValueError before anything is loaded."""
        q = self._rank_queries(queries)
        nq = int(q.shape[0])
        codes = self._rank_codes(codes_per_query, nq)
        self.ms._check_filter_args(filter, "mask", None, nq)
        index = self.ms._live_index()
        if index is None:
            return [[] for _ in range(nq)]
        if q.shape[-1] != index.dim:
            raise ValueError(f"query dim {q.shape[-1]} != index dim {index.dim}")
        nt = max(len(c) for c in codes)
        targets = np.full((nq, nt), -1, np.int64)
        for i, per in enumerate(codes):
            for j, code in enumerate(per):
                row = self.ms._row_of_code(code)
                if row is None:
                    raise KeyError(code)
                targets[i, j] = row
        with self.ms._leased_masks(index, filter, nq) as masks:
            rank, adj, raw, levels, selected = self.ms._workspace_for("rankof", index, nq).rank_of(q, targets, masks)
        out = []
        for i, per in enumerate(codes):
            hits = []
            for j, code in enumerate(per):
                ranked = int(rank[i, j]) >= 0
                hits.append({"code": code, "rank": int(rank[i, j]) if ranked else None, "score": float(adj[i, j]) if ranked else None,
                             "raw_score": float(raw[i, j]) if ranked else None, "level": int(levels[i, j]), "selected": int(selected[i])})
            out.append(hits)
        return out

    def rank_of(self, query, codes, filter: Optional[str] = None) -> List[Dict[str, Any]]:   # noqa: A002
        """the ranks of `codes` (a code or a list of up to 16) for ONE query, a vector or a text (rank_of_batch): a list of
        {code, rank, score, raw_score, level, selected}"""
        self.ms._one_filter(filter, "a list of filters needs a batch: one expression (or None) per query of rank_of_batch")
        if not isinstance(query, str) and np.ndim(query) != 1:
            raise ValueError("query: one vector or one text")
        return self.rank_of_batch([query] if isinstance(query, str) else np.asarray(query, dtype=np.float32).reshape(1, -1), [codes], filter=filter)[0]

    @staticmethod
    def rank_metrics(best_ranks, ks=(1, 5, 10)) -> Dict[str, Any]:
        """recall@k, MRR and the mean rank of `best_ranks` (per query the best rank among its acceptable codes, 0 = first; None or
        a negative value: not ranked at all - it counts in n, in no recall, as 0 in the MRR, and not in mean_rank). Host
        arithmetic in float64."""
        ranks = [None if r is None or int(r) < 0 else int(r) for r in best_ranks]
        n = len(ranks)
        found = np.asarray([r for r in ranks if r is not None], np.float64)
        out: Dict[str, Any] = {"n": n}
        for k in ks:
            out[f"recall@{int(k)}"] = float((found < int(k)).sum() / n) if n else 0.0
        out["mrr"] = float((1.0 / (found + 1.0)).sum() / n) if n else 0.0
        out["mean_rank"] = float(found.mean()) if found.size else None
        out["ranks"] = ranks
        return out

    def evaluate(self, pairs, ks=(1, 5, 10), filter=None) -> Dict[str, Any]:   # noqa: A002
        """Additive: recall@k, MRR and the mean rank of labelled pairs over the WHOLE ranking (rank_of_batch; no rank is lost past
        the largest k). pairs: a sequence of (text or vector, gold code or list of acceptable codes); ks: positive ints; filter: as
        in rank_of_batch. A query's rank is the best among its acceptable codes. Returns {"n", "recall@k" per k, "mrr", "mean_rank",
        "ranks"} (rank_metrics). An unknown code raises KeyError."""
        pairs = list(pairs)
        if any(not isinstance(p, (list, tuple)) or len(p) != 2 for p in pairs):
            raise ValueError("pairs: (text or vector, gold code or list of codes) each")
        ks = tuple(ks)
        if not ks or any(not self.ms._int_in(k, 1) for k in ks):
            raise ValueError(f"ks={ks!r}: positive ints")
        if not pairs:
            return self.rank_metrics([], ks)
        texts = [isinstance(p[0], str) for p in pairs]
        if any(texts) and not all(texts):
            raise ValueError("pairs: texts or vectors, not both")
        queries = [p[0] for p in pairs] if texts[0] else np.stack([np.asarray(p[0], dtype=np.float32).reshape(-1) for p in pairs])
        per = self.rank_of_batch(queries, [p[1] for p in pairs], filter=filter)
        best = []
        for hits in per:
            got = [h["rank"] for h in hits if h["rank"] is not None]
            best.append(min(got) if got else None)
        return self.rank_metrics(best, ks)
