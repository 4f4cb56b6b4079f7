"""Hybrid search: pymilvus's request and ranker classes for MilvusService.hybrid_search.

    reqs = [AnnSearchRequest(vec_a, limit=20), AnnSearchRequest(vec_b, limit=20, expr="level >= 2")]
    hits = milvus_service.hybrid_search(reqs, RRFRanker(60), limit=10)

The reference has no hybrid search (it sends one MilvusClient.search per phrasing, services/milvus_service.py:280-285); these are
the argument names and ValueErrors of pymilvus's AnnSearchRequest / RRFRanker / WeightedRanker, restricted to what the dense index
takes: one vector field (no anns_field), metric IP. No device code here: the classes only carry and check arguments.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Optional

import numpy as np

from . import filter_expr, range_search

MAX_REQUESTS = 8    # include/icd_search.h ICD_MAX_REQUESTS
MAX_LIMIT = 128     # ICD_MAX_K
NORMS = ("none", "cosine", "atan")
ANNS_FIELDS = ("vector", "sparse")   # the dense field; the sparse (BM25) field of DESIGN.md section 14


class AnnSearchRequest:
    """One request of a hybrid search.

    anns_field "vector" (the default), a dense request. data: the query vector(s) - [dim] or [nq, dim]; limit: hits this request
    contributes (1 .. 128); expr: a Milvus filter expression (services/filter_expr.py) or None; param: Milvus search params, of
    which {"params": {"radius": .., "range_filter": ..}} (or the two keys at the top level) are used.

    anns_field "sparse": data is a text or a {term_id: weight} dict (or a list of nq of them), searched in the store's sparse
    (BM25) index (MilvusService.build_sparse_index); limit and expr as above, no bounds."""

    def __init__(self, data, limit: int, expr: Optional[str] = None, param: Optional[Dict[str, Any]] = None, *, anns_field: str = "vector"):
        if anns_field not in ANNS_FIELDS:
            raise ValueError(f"anns_field={anns_field!r}: one of {ANNS_FIELDS}")
        if anns_field == "sparse":
            for d in (data if isinstance(data, (list, tuple)) else [data]):
                if not isinstance(d, (str, dict)):
                    raise ValueError(f"a sparse request's data is a text or a {{term_id: weight}} dict (or a list of them), not {type(d).__name__}")
        if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)):
            raise ValueError(f"limit={limit!r}: an int in 1 .. {MAX_LIMIT}")
        if not 1 <= int(limit) <= MAX_LIMIT:
            raise ValueError(f"limit={limit}: a request returns 1 .. {MAX_LIMIT} hits")
        if expr is not None and not isinstance(expr, str):
            raise ValueError(f"expr={expr!r}: a filter expression (str) or None")
        if expr is not None:
            filter_expr.compile(expr)
        if param is not None and not isinstance(param, dict):
            raise ValueError(f"param={param!r}: a dict or None")
        self.data, self.limit, self.expr, self.param = data, int(limit), expr, param
        self.anns_field = anns_field
        self.radius, self.range_filter = range_search.check_bounds(None, None, param)
        if anns_field == "sparse" and (self.radius is not None or self.range_filter is not None):
            raise ValueError("a sparse request takes no radius / range_filter")

    def __repr__(self):
        return f"AnnSearchRequest(anns_field={self.anns_field!r}, limit={self.limit}, expr={self.expr!r}, param={self.param!r})"


class RRFRanker:
    """Reciprocal rank fusion: fused(id) = sum over the requests whose list holds id of 1 / (k + rank + 1), rank from 0."""

    def __init__(self, k: float = 60):
        if isinstance(k, bool) or not isinstance(k, (int, float, np.integer, np.floating)):
            raise ValueError(f"k={k!r}: a number with 0 < k < 16384")
        if not (0 < float(k) < 16384):
            raise ValueError(f"k={k}: need 0 < k < 16384")
        self.k = float(k)

    def dict(self):
        return {"strategy": "rrf", "params": {"k": self.k}}


class WeightedRanker:
    """Weighted sum: fused(id) = sum over the requests whose list holds id of weight_r * norm(score_r). One weight per request,
    each in [0, 1]. norm_score: "atan" (Milvus's normalisation for metric IP, 0.5 + atan(s) / pi; also True), "cosine"
    ((1 + s) / 2), "none" (the raw inner product; also False)."""

    def __init__(self, *weights, norm_score="atan"):
        if not weights:
            raise ValueError("WeightedRanker needs one weight per request")
        for w in weights:
            if isinstance(w, bool) or not isinstance(w, (int, float, np.integer, np.floating)):
                raise ValueError(f"weight {w!r}: a number in [0, 1]")
            if math.isnan(float(w)) or not 0.0 <= float(w) <= 1.0:
                raise ValueError(f"weight {w}: a weight lies in [0, 1]")
        if norm_score is True:
            norm_score = "atan"
        elif norm_score is False:
            norm_score = "none"
        if norm_score not in NORMS:
            raise ValueError(f"norm_score={norm_score!r}: one of {NORMS}")
        self.weights = [float(w) for w in weights]
        self.norm_score = norm_score

    def dict(self):
        return {"strategy": "weighted", "params": {"weights": self.weights, "norm_score": self.norm_score}}


def ranker_from_dict(spec) -> "RRFRanker | WeightedRanker":
    """{"strategy": "rrf", "params": {"k": 60}} / {"strategy": "weighted", "params": {"weights": [..], "norm_score": ..}} (the
    shape of pymilvus's ranker.dict(); "type" is accepted for "strategy", the params also at the top level) -> ranker"""
    if not isinstance(spec, dict):
        raise ValueError(f"ranker={spec!r}: a dict with 'strategy'")
    kind = spec.get("strategy", spec.get("type"))
    params = dict(spec.get("params") or {})
    for key in ("k", "weights", "norm_score"):
        if key in spec and key not in params:
            params[key] = spec[key]
    if kind == "rrf":
        return RRFRanker(params.get("k", 60))
    if kind == "weighted":
        weights = params.get("weights")
        if not isinstance(weights, (list, tuple)):
            raise ValueError("a weighted ranker needs 'weights': one number per request")
        return WeightedRanker(*weights, norm_score=params.get("norm_score", "atan"))
    raise ValueError(f"ranker strategy {kind!r}: 'rrf' or 'weighted'")


def check_requests(reqs, ranker, limit):
    """the checks of a hybrid search that need no store and no device: ValueError on a bad request list, ranker or limit.
    Returns limit as an int."""
    if not isinstance(reqs, (list, tuple)) or not reqs:
        raise ValueError("reqs: a non-empty list of AnnSearchRequest")
    if len(reqs) > MAX_REQUESTS:
        raise ValueError(f"{len(reqs)} requests: a hybrid search takes 1 .. {MAX_REQUESTS}")
    for r in reqs:
        if not isinstance(r, AnnSearchRequest):
            raise ValueError(f"reqs holds {type(r).__name__}: AnnSearchRequest expected")
    if not isinstance(ranker, (RRFRanker, WeightedRanker)):
        raise ValueError(f"ranker={ranker!r}: RRFRanker or WeightedRanker")
    if isinstance(ranker, WeightedRanker) and len(ranker.weights) != len(reqs):
        raise ValueError(f"the ranker holds {len(ranker.weights)} weights for {len(reqs)} requests")
    if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or not 1 <= int(limit) <= MAX_LIMIT:
        raise ValueError(f"limit={limit!r}: an int in 1 .. {MAX_LIMIT}")
    return int(limit)


def sparse_queries(req):
    """a sparse request's data as a list of nq texts / {term_id: weight} dicts"""
    return list(req.data) if isinstance(req.data, (list, tuple)) else [req.data]


def stack_requests(reqs):
    """the DENSE requests' vectors as ONE [nq, R, dim] array (numpy, or a torch CUDA tensor when every request's data is one)"""
    if any(r.anns_field != "vector" for r in reqs):
        raise ValueError("stack_requests takes dense requests only")
    datas = [r.data for r in reqs]
    if all(hasattr(d, "is_cuda") and d.is_cuda for d in datas):
        import torch
        ds = [d if d.dim() == 2 else d.reshape(1, -1) for d in datas]
        if len({tuple(d.shape) for d in ds}) != 1:
            raise ValueError("the requests' data must share one shape [nq, dim]")
        return torch.stack([d.to(torch.float32) for d in ds], dim=1).contiguous()
    ds = []
    for d in datas:
        if hasattr(d, "cpu"):
            d = d.detach().cpu().numpy()
        d = np.asarray(d, dtype=np.float32)
        if d.ndim == 1:
            d = d[None, :]
        if d.ndim != 2:
            raise ValueError("a request's data is one vector [dim] or a batch [nq, dim]")
        ds.append(d)
    if len({d.shape for d in ds}) != 1:
        raise ValueError("the requests' data must share one shape [nq, dim]")
    return np.ascontiguousarray(np.stack(ds, axis=1))
