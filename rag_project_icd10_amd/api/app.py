"""FastAPI surface: POST /embed, POST /query, POST /segments_query, POST /hybrid_query, POST /diverse_query, POST /boosted_query, POST /codes/query, POST /codes/facets, GET /codes/{code}, GET /codes/{code}/similar, POST /codes/rank, POST /wide_query, POST /recommend, GET /health, GET /stats, GET /.

Mirrors the reference's main.py for these routes: lifespan-owned service globals (:25-105), `/`
(:250-258), `/health` (:261-289), `/query` (:292-363: candidates of all matches merged, sorted by score,
cut to top_k, every match's confidence metrics / factors / level copied as :325-330 does; 503 when services are missing, 500 with a `detail` string on any exception), `/embed`
(:505-530), `/stats` (:574-599). `/query` takes a Milvus `filter` expression (services/filter_expr.py; a bad one is a 400), `/stats`
lists the cached filter views, filter masks and groupings; `/query` takes `filter_mode` ("view" / "mask"; anything else is a 400); `/query` also takes Milvus's `group_by_field` / `group_size` and `radius` / `range_filter` (a bad pair is a 400). `/hybrid_query` takes several phrasings of one diagnosis and a ranker (Milvus hybrid_search, services/hybrid_search.py; bad arguments are a 400), and `group_by_field` / `group_size` as `/query` does (a bad combination is a 400). The LLM, NER, standardisation and resource routes are out of scope.

    uvicorn rag_project_icd10_amd.api.app:app --host 0.0.0.0 --port 8005
"""
from __future__ import annotations

import logging
import os
from contextlib import asynccontextmanager
from typing import List, Optional

import numpy as np
from fastapi import FastAPI, HTTPException

from ..dotenv_lite import load_dotenv
from ..services import rank_of as rank_search
from ..services import recommend as recommend_search
from ..services import wide_search
from .icd_models import (BoostedQueryRequest, CodeRankRequest, CodeRankResult, DiagnosisMatch, DiverseQueryRequest, EmbeddingRequest, EmbeddingResponse, FacetRequest, FacetResponse, HealthCheckResponse,
                         HybridQueryRequest, QueryRequest, QueryResponse, RecommendRequest, ScalarQueryRequest, ScalarQueryResponse, SegmentsQueryRequest, SegmentsQueryResponse,
                         SimilarCodesResponse, WideQueryRequest, WideQueryResponse, convert_numpy_types)

load_dotenv()   # main.py:11 of the reference; existing environment variables win

logger = logging.getLogger(__name__)

embedding_service = None
milvus_service = None
multi_diagnosis_service = None


def install_services(embedding, milvus, multi=None):
    """Wire service instances (used by the lifespan and by tests)."""
    global embedding_service, milvus_service, multi_diagnosis_service
    embedding_service, milvus_service = embedding, milvus
    if multi is None and embedding is not None and milvus is not None:
        from ..services.multi_diagnosis_service import MultiDiagnosisService
        multi = MultiDiagnosisService(embedding, milvus)
    multi_diagnosis_service = multi


@asynccontextmanager
async def lifespan(app: FastAPI):
    if embedding_service is None:
        from ..services.embedding_service import EmbeddingService
        from ..services.milvus_service import MilvusService
        emb = EmbeddingService()
        mil = MilvusService(emb)
        # like the reference's MultiDiagnosisService (services/multi_diagnosis_service.py:28,44-47): an NER service - its classifier when the
        # checkpoint resolves, its rules otherwise - and with it the ENHANCED text mode (entities fused with semantic boundaries);
        # ICD_QUERY_NER=0: neither (delimiter extraction, the whole request on the device)
        ner = None
        if os.getenv("ICD_QUERY_NER", "1") != "0":
            try:
                from ..services.medical_ner_service import MedicalNERService
                ner = MedicalNERService()
            except Exception as exc:
                logger.error("no NER service (%s): /query extracts by delimiters", exc)
        # ICD_QUERY_CONFIDENCE=multidimensional: match confidences from the reference's 12-factor service, with its metrics, factors
        # and level on every diagnosis match (services/multi_diagnosis_service.py:176-207); "match" (the default): the original formula
        confidence = os.getenv("ICD_QUERY_CONFIDENCE", "match")
        from ..services.multi_diagnosis_service import MultiDiagnosisService
        install_services(emb, mil, MultiDiagnosisService(emb, mil, ner_service=ner, confidence=confidence))
    try:
        yield
    finally:
        if milvus_service is not None:
            try:
                milvus_service.disconnect()
            except Exception as exc:
                logger.warning("disconnect failed: %s", exc)


app = FastAPI(title="ICD-10 诊断标准化API", description="基于RAG的ICD-10诊断内容标准化系统 (MI355X)",
              version="1.0.0", lifespan=lifespan)


@app.get("/")
async def root():
    return {"message": "ICD-10 诊断标准化API", "version": "1.0.0", "docs": "/docs", "health": "/health"}


@app.get("/health", response_model=HealthCheckResponse)
async def health_check():
    try:
        loaded = bool(embedding_service and embedding_service.get_model_info().get("loaded", False))
        connected, total = False, 0
        if milvus_service:
            connected = milvus_service.test_connection().get("connected", False)
            if connected:
                total = milvus_service.get_collection_stats().get("num_entities", 0)
        return HealthCheckResponse(status="healthy" if (loaded and connected) else "unhealthy",
                                   milvus_connected=connected, embedding_model_loaded=loaded, total_records=total)
    except Exception as exc:
        raise HTTPException(status_code=500, detail=f"健康检查失败: {exc}")


@app.post("/query", response_model=QueryResponse)
async def query_similar(request: QueryRequest):
    if request.filter is not None:
        # (a bad filter is the caller's error: 400 with the parser's message, before the catch-all below turns everything into a 500)
        from ..services import filter_expr
        try:
            filter_expr.compile(request.filter)
        except ValueError as exc:
            raise HTTPException(status_code=400, detail=str(exc))
    if request.filter_mode not in ("view", "mask"):
        raise HTTPException(status_code=400, detail=f"filter_mode={request.filter_mode!r}: one of ('view', 'mask')")
    if request.filter_mode == "mask" and request.filter is not None and request.group_by_field is not None:
        raise HTTPException(status_code=400, detail="filter_mode='mask' cannot be combined with group_by_field")
    mode = {} if request.filter_mode == "view" else {"filter_mode": request.filter_mode}
    grouped = request.group_by_field is not None or request.group_size != 1
    if grouped:
        # (a bad grouping is a 400 like a bad filter; /query searches top_k * 2, with grouping that is top_k * 2 GROUPS)
        from ..services import filter_expr
        try:
            if request.group_by_field is None:
                raise ValueError("group_size needs group_by_field")
            filter_expr.check_grouping(request.group_by_field, request.top_k * 2, request.group_size)
        except ValueError as exc:
            raise HTTPException(status_code=400, detail=str(exc))
    scorer = {}
    if request.group_scorer is not None:
        # (a name outside max / sum / avg, or one without group_by_field, is a 400 as well)
        from ..services import filter_expr
        try:
            filter_expr.check_group_scorer(request.group_by_field, request.group_scorer)
        except ValueError as exc:
            raise HTTPException(status_code=400, detail=str(exc))
        scorer = {"group_scorer": request.group_scorer}
    ranged = request.radius is not None or request.range_filter is not None
    if ranged:
        # (a bad band, or one next to grouping, is a 400 as well)
        from ..services import range_search
        try:
            radius, range_filter = range_search.check_bounds(request.radius, request.range_filter)
            if grouped:
                raise ValueError("radius / range_filter cannot be combined with group_by_field")
        except ValueError as exc:
            raise HTTPException(status_code=400, detail=str(exc))
    try:
        if not embedding_service or not milvus_service or not multi_diagnosis_service:
            raise HTTPException(status_code=503, detail="服务未就绪")
        if ranged:
            result = multi_diagnosis_service.match_multiple_diagnoses(text=request.text, top_k=request.top_k, filter=request.filter,
                                                                      radius=radius, range_filter=range_filter, **mode)
        elif grouped:
            result = multi_diagnosis_service.match_multiple_diagnoses(text=request.text, top_k=request.top_k, filter=request.filter,
                                                                      group_by_field=request.group_by_field, group_size=request.group_size, **mode, **scorer)
        elif request.filter is None:
            result = multi_diagnosis_service.match_multiple_diagnoses(text=request.text, top_k=request.top_k)
        else:
            result = multi_diagnosis_service.match_multiple_diagnoses(text=request.text, top_k=request.top_k, filter=request.filter, **mode)
        candidates, matches = [], []
        for m in result["matches"]:
            candidates.extend(m.candidates)
            dm = DiagnosisMatch(diagnosis_text=m.diagnosis_text, candidates=m.candidates, match_confidence=m.match_confidence)
            # main.py:325-330 of the reference: the confidence details ride along (None unless the multidimensional mode set them)
            for name in ("confidence_metrics", "confidence_factors", "confidence_level"):
                if getattr(m, name, None) is not None:
                    setattr(dm, name, getattr(m, name))
            matches.append(dm)
        candidates.sort(key=lambda c: c.score, reverse=True)
        response = QueryResponse(candidates=candidates[:request.top_k],
                                 is_multi_diagnosis=len(result["extracted_diagnoses"]) > 1,
                                 extracted_diagnoses=result["extracted_diagnoses"], diagnosis_matches=matches)
        try:
            response = QueryResponse(**convert_numpy_types(response.model_dump()))
        except Exception as exc:
            logger.warning("numpy conversion failed: %s", exc)
        return response
    except Exception as exc:
        # like the reference (:361-363) every failure, the 503 above included, surfaces as a 500
        raise HTTPException(status_code=500, detail=f"查询失败: {exc}")


@app.post("/hybrid_query", response_model=QueryResponse)
async def hybrid_query(request: HybridQueryRequest):
    """Several phrasings of ONE diagnosis (the clinician's wording, the NER entity text, a synonym, an English term): encoded in one
    call, one dense request each, fused on the device by the ranker (MilvusService.hybrid_search). Bad arguments are a 400, also
    those only the store can judge (a limit above its max_k). The response has /query's hit shape: `score` is the fused score
    times the level weight, `original_score` the ranker's own value, `similarity_factors.matched_requests` the indices of the
    texts that found the hit. `score` is non-negative in that shape; a weighted sum of raw inner products (norm_score "none") can
    be negative, and such a hit carries score 0 with the true value in `enhanced_score`, which always holds the unclamped score."""
    from ..services import hybrid_search as hybrid
    try:
        if not request.texts or any(not isinstance(t, str) or not t.strip() for t in request.texts):
            raise ValueError("texts: 1 .. 8 non-empty strings")
        if len(request.texts) > hybrid.MAX_REQUESTS:
            raise ValueError(f"{len(request.texts)} texts: a hybrid query takes 1 .. {hybrid.MAX_REQUESTS} phrasings")
        if not 1 <= request.top_k <= 50:
            raise ValueError(f"top_k={request.top_k}: 1 .. 50")
        ranker = hybrid.ranker_from_dict(request.ranker)
        n_reqs = len(request.texts) * (2 if request.sparse else 1)   # sparse: the dense requests first, then one sparse request per text
        if n_reqs > hybrid.MAX_REQUESTS:
            raise ValueError(f"{len(request.texts)} texts with sparse requests: at most {hybrid.MAX_REQUESTS // 2} phrasings")
        if isinstance(ranker, hybrid.WeightedRanker) and len(ranker.weights) != n_reqs:
            raise ValueError(f"the ranker holds {len(ranker.weights)} weights for {n_reqs} requests")
        hybrid.AnnSearchRequest(None, request.req_limit, request.filter)   # (the limit's and the filter's checks)
        if request.group_by_field is not None:   # Milvus's grouping on hybrid_search: the limits count groups
            from ..services import filter_expr
            filter_expr.check_grouping(request.group_by_field, request.top_k, request.group_size)
            filter_expr.check_grouping(request.group_by_field, request.req_limit, request.group_size)
        elif request.group_size != 1:
            raise ValueError("group_size needs group_by_field")
    except ValueError as exc:
        raise HTTPException(status_code=400, detail=str(exc))
    if not embedding_service or not milvus_service:
        raise HTTPException(status_code=500, detail="查询失败: 服务未就绪")   # (as /query: the 503 surfaces as a 500)
    try:
        import numpy as np
        vecs = np.asarray(embedding_service.encode_query_batch(list(request.texts)), dtype=np.float32)
        reqs = [hybrid.AnnSearchRequest(vecs[i], request.req_limit, request.filter) for i in range(len(request.texts))]
        if request.sparse:
            reqs += [hybrid.AnnSearchRequest(t, request.req_limit, request.filter, anns_field="sparse") for t in request.texts]
        try:
            if request.group_by_field is not None:
                hits = milvus_service.hybrid_search(reqs, ranker, request.top_k, group_by_field=request.group_by_field, group_size=request.group_size)
            else:
                hits = milvus_service.hybrid_search(reqs, ranker, request.top_k)
        except ValueError as exc:
            raise HTTPException(status_code=400, detail=str(exc))
        from .icd_models import Candidate
        candidates = [Candidate(code=h["code"], title=h["title"] or "", score=max(float(h["score"]), 0.0), enhanced_score=float(h["score"]),
                                level=h["metadata"].get("level", 1), parent_code=h["metadata"].get("parent_code", ""),
                                original_score=float(h["fused_score"]), similarity_factors={"matched_requests": h["matched_requests"]})
                      for h in hits]
        response = QueryResponse(candidates=candidates, is_multi_diagnosis=False, extracted_diagnoses=[request.texts[0]])
        return QueryResponse(**convert_numpy_types(response.model_dump()))
    except HTTPException:
        raise
    except Exception as exc:
        raise HTTPException(status_code=500, detail=f"查询失败: {exc}")


@app.post("/diverse_query", response_model=QueryResponse)
async def diverse_query(request: DiverseQueryRequest):
    """One text, the top_k hits that are not copies of each other (MilvusService.search_mmr): the text is
    encoded like /query's, its fetch_k best rows are the candidates, and the device picks top_k of them by maximal marginal
    relevance. The response has /hybrid_query's hit shape: `score` the adjusted score, `original_score` the raw inner product,
    `similarity_factors.mmr_score` the value the hit was picked with. Bad arguments are a 400."""
    try:
        if not isinstance(request.text, str) or not request.text.strip():
            raise ValueError("text: a non-empty string")
        if not 1 <= request.top_k <= 50:
            raise ValueError(f"top_k={request.top_k}: 1 .. 50")
        if request.fetch_k is not None and not request.top_k <= request.fetch_k <= 128:
            raise ValueError(f"fetch_k={request.fetch_k}: top_k={request.top_k} .. 128")
        if not 0.0 <= request.lambda_mult <= 1.0:
            raise ValueError(f"lambda_mult={request.lambda_mult}: 0 .. 1")
        from ..services import filter_expr, range_search
        if request.filter is not None:
            filter_expr.compile(request.filter)
        range_search.check_bounds(request.radius, request.range_filter)
    except ValueError as exc:
        raise HTTPException(status_code=400, detail=str(exc))
    if not embedding_service or not milvus_service:
        raise HTTPException(status_code=500, detail="查询失败: 服务未就绪")   # (as /query: the 503 surfaces as a 500)
    try:
        import numpy as np
        vec = np.asarray(embedding_service.encode_query(request.text), dtype=np.float32).reshape(-1)
        try:
            hits = milvus_service.search_mmr(vec, request.top_k, request.fetch_k, request.lambda_mult, filter=request.filter,
                                             radius=request.radius, range_filter=request.range_filter)
        except ValueError as exc:
            raise HTTPException(status_code=400, detail=str(exc))
        from .icd_models import Candidate
        candidates = [Candidate(code=h["code"], title=h["title"] or "", score=max(float(h["score"]), 0.0), enhanced_score=float(h["score"]),
                                level=h["metadata"].get("level", 1), parent_code=h["metadata"].get("parent_code", ""),
                                original_score=float(h["original_score"]), similarity_factors={"mmr_score": float(h["mmr_score"])})
                      for h in hits]
        response = QueryResponse(candidates=candidates, is_multi_diagnosis=False, extracted_diagnoses=[request.text])
        return QueryResponse(**convert_numpy_types(response.model_dump()))
    except HTTPException:
        raise
    except Exception as exc:
        raise HTTPException(status_code=500, detail=f"查询失败: {exc}")


@app.post("/boosted_query", response_model=QueryResponse)
async def boosted_query(request: BoostedQueryRequest):
    """Every text's top_k hits over the boosted ranking (MilvusService.search_boosted_batch): the texts are
    encoded like /query's, the score of every row a boost's filter selects is multiplied by its weight on the device BEFORE the
    top-k is chosen, and `filter` drops rows as everywhere. The response has /diverse_query's hit shape - `score` the adjusted
    score, `original_score` the boosted inner product: `candidates` are the first text's hits, `diagnosis_matches` holds one
    entry per text. Bad arguments are a 400."""
    try:
        if not request.texts or len(request.texts) > 16 or any(not isinstance(t, str) or not t.strip() for t in request.texts):
            raise ValueError("texts: 1 .. 16 non-empty strings")
        if not 1 <= request.top_k <= 50:
            raise ValueError(f"top_k={request.top_k}: 1 .. 50")
        from ..services import boost_ranker, filter_expr
        if len(request.boosts) > boost_ranker.MAX_BOOSTS:
            raise ValueError(f"{len(request.boosts)} boosts: up to {boost_ranker.MAX_BOOSTS}")
        rankers = [boost_ranker.BoostRanker(b.filter, b.weight) for b in request.boosts]
        if request.filter is not None:
            filter_expr.compile(request.filter)
    except ValueError as exc:
        raise HTTPException(status_code=400, detail=str(exc))
    if not embedding_service or not milvus_service:
        raise HTTPException(status_code=500, detail="查询失败: 服务未就绪")   # (as /query: the 503 surfaces as a 500)
    try:
        import numpy as np
        vecs = np.stack([np.asarray(embedding_service.encode_query(t), dtype=np.float32).reshape(-1) for t in request.texts])
        try:
            lists = milvus_service.search_boosted_batch(vecs, request.top_k, rankers, as_dicts=True, filter=request.filter)
        except ValueError as exc:
            raise HTTPException(status_code=400, detail=str(exc))
        from .icd_models import Candidate
        per_text = [[Candidate(code=h["code"], title=h["title"] or "", score=max(float(h["score"]), 0.0), enhanced_score=float(h["score"]),
                               level=h["metadata"].get("level", 1), parent_code=h["metadata"].get("parent_code", ""),
                               original_score=float(h["original_score"]))
                     for h in hits] for hits in lists]
        matches = [DiagnosisMatch(diagnosis_text=t, candidates=c, match_confidence=min(max(c[0].score, 0.0), 1.0) if c else 0.0)
                   for t, c in zip(request.texts, per_text)]
        response = QueryResponse(candidates=per_text[0], is_multi_diagnosis=len(request.texts) > 1, extracted_diagnoses=list(request.texts),
                                 diagnosis_matches=matches)
        return QueryResponse(**convert_numpy_types(response.model_dump()))
    except HTTPException:
        raise
    except Exception as exc:
        raise HTTPException(status_code=500, detail=f"查询失败: {exc}")


@app.post("/segments_query", response_model=SegmentsQueryResponse)
async def segments_query(request: SegmentsQueryRequest):
    """The segments of one text as an embedding list under MAX_SIM (MilvusService.search_embedding_list): the
    top_k groups - values of group_by_field, or single codes - whose best rows cover all segments best in sum, and per group the
    row that answers each segment. Bad arguments are a 400."""
    if not embedding_service or not milvus_service:
        raise HTTPException(status_code=503, detail="服务未就绪")
    try:
        if not 1 <= len(request.segments) <= milvus_service.LIST_MAX_VECTORS:
            raise ValueError(f"segments: {len(request.segments)} texts, need 1 .. {milvus_service.LIST_MAX_VECTORS}")
        import numpy as np
        vecs = np.asarray(embedding_service.encode_query_batch(list(request.segments)), dtype=np.float32)
        groups = milvus_service.search_embedding_list(vecs, request.top_k, request.group_by_field, request.filter or None, request.scorer)
    except ValueError as exc:
        raise HTTPException(status_code=400, detail=str(exc))
    except Exception as exc:
        raise HTTPException(status_code=500, detail=f"查询失败: {exc}")
    return SegmentsQueryResponse(**convert_numpy_types({"segments": len(request.segments), "groups": groups}))


@app.post("/codes/query", response_model=ScalarQueryResponse)
async def codes_query(request: ScalarQueryRequest):
    """MilvusClient.query over the scalar fields (MilvusService.query_batch / count): the rows a filter
    selects, in ascending id, and their number. `total` is always filled - the device counts the selection in the call that pages
    it. count=true returns the total alone. Bad arguments are a 400."""
    if not milvus_service:
        raise HTTPException(status_code=503, detail="服务未就绪")
    try:
        if not 1 <= request.limit <= 1000:
            raise ValueError(f"limit={request.limit}: 1 .. 1000")
        if request.count:
            return ScalarQueryResponse(total=milvus_service.count(request.filter), rows=[])
        lists, totals = milvus_service.query_batch([request.filter], request.limit, request.offset, request.output_fields, with_totals=True)
    except ValueError as exc:
        raise HTTPException(status_code=400, detail=str(exc))
    except Exception as exc:
        raise HTTPException(status_code=500, detail=f"查询失败: {exc}")
    return ScalarQueryResponse(total=totals[0], rows=convert_numpy_types(lists[0]))


@app.post("/codes/facets", response_model=FacetResponse)
async def codes_facets(request: FacetRequest):
    """The terms aggregation of a code browser (MilvusService.facet_batch): the rows a filter selects counted
    per value of `field`, most frequent first, and their number. Bad arguments are a 400."""
    if not milvus_service:
        raise HTTPException(status_code=503, detail="服务未就绪")
    try:
        lists, totals = milvus_service.facet_batch(request.field, [request.filter], request.limit, request.min_count, with_totals=True)
    except ValueError as exc:
        raise HTTPException(status_code=400, detail=str(exc))
    except Exception as exc:
        raise HTTPException(status_code=500, detail=f"查询失败: {exc}")
    return FacetResponse(field=request.field, total=totals[0], facets=convert_numpy_types(lists[0]))


@app.post("/codes/rank", response_model=List[CodeRankResult])
async def codes_rank(request: CodeRankRequest):
    """Where given codes land for one text, over the whole collection (services/rank_of.py, RankOf.rank_of): per code its
    exact rank (0 = best, null where the filter leaves it out), adjusted and raw score, level, and the rows the filter admits. An
    unknown code is a 404, bad arguments are a 400."""
    if not embedding_service or not milvus_service:
        raise HTTPException(status_code=503, detail="服务未就绪")
    try:
        if not request.text:
            raise ValueError("text: a non-empty string")
        if not 1 <= len(request.codes) <= rank_search.MAX_CODES:
            raise ValueError(f"codes: {len(request.codes)} codes, need 1 .. {rank_search.MAX_CODES}")
        results = rank_search.RankOf(milvus_service).rank_of(request.text, list(request.codes), filter=request.filter or None)
    except KeyError as exc:
        raise HTTPException(status_code=404, detail=f"no record with code {exc.args[0] if exc.args else ''}")
    except ValueError as exc:
        raise HTTPException(status_code=400, detail=str(exc))
    except Exception as exc:
        raise HTTPException(status_code=500, detail=f"查询失败: {exc}")
    return convert_numpy_types(results)


@app.post("/wide_query", response_model=WideQueryResponse)
async def wide_query(request: WideQueryRequest):
    """The exact top_k candidates of one text for top_k up to 16 384, in one device call (services/wide_search.py,
    WideSearch.search_wide_batch), and `total`, the rows that rank inside the filter and the band. Bad
    arguments are a 400."""
    if not embedding_service or not milvus_service:
        raise HTTPException(status_code=503, detail="服务未就绪")
    try:
        if not request.text:
            raise ValueError("text: a non-empty string")
        vector = np.asarray(embedding_service.encode_query(request.text), dtype=np.float32).reshape(1, -1)
        lists, totals = wide_search.WideSearch(milvus_service).search_wide_batch(
            vector, request.top_k, filter=request.filter or None, radius=request.radius, range_filter=request.range_filter,
            offset=request.offset, as_dicts=True, with_totals=True)
    except ValueError as exc:
        raise HTTPException(status_code=400, detail=str(exc))
    except Exception as exc:
        raise HTTPException(status_code=500, detail=f"查询失败: {exc}")
    return WideQueryResponse(candidates=convert_numpy_types(lists[0]), total=int(totals[0]))


@app.post("/recommend", response_model=WideQueryResponse)
async def recommend(request: RecommendRequest):
    """The exact top_k candidates by positive and negative examples - stored codes, ids, texts or vectors - under one of three
    strategies, in one device call (services/recommend.py, Recommend.recommend_batch), and `total`, the rows
    that rank inside the filter and the band: `/wide_query`'s response shape. An id outside the collection is a 404, bad
    arguments are a 400."""
    if not milvus_service:
        raise HTTPException(status_code=503, detail="服务未就绪")
    try:
        lists, totals = recommend_search.Recommend(milvus_service).recommend_batch(
            [list(request.positive)], [list(request.negative)], request.strategy, request.top_k, filter=request.filter or None,
            radius=request.radius, range_filter=request.range_filter, offset=request.offset, as_dicts=True, with_totals=True)
    except KeyError as exc:
        raise HTTPException(status_code=404, detail=f"no record with id {exc.args[0] if exc.args else ''}")
    except ValueError as exc:
        raise HTTPException(status_code=400, detail=str(exc))
    except Exception as exc:
        raise HTTPException(status_code=500, detail=f"查询失败: {exc}")
    return WideQueryResponse(candidates=convert_numpy_types(lists[0]), total=int(totals[0]))


@app.get("/codes/{code}/similar", response_model=SimilarCodesResponse)
async def codes_similar(code: str, top_k: int = 10, filter: Optional[str] = None):   # noqa: A002
    """The top_k codes closest to one stored code (MilvusService.similar_codes): the code's stored vector is
    the query, on the device, and the code itself is left out. Hits have /diverse_query's shape - `score` the adjusted score,
    `original_score` the raw inner product. An unknown code is a 404, bad arguments are a 400."""
    if not milvus_service:
        raise HTTPException(status_code=503, detail="服务未就绪")
    try:
        if '"' in code or "\\" in code:
            raise ValueError("code: no quotes or backslashes")
        if not 1 <= top_k <= 50:
            raise ValueError(f"top_k={top_k}: 1 .. 50")
        hits = milvus_service.similar_codes(code, top_k, filter=filter or None)
    except KeyError:
        raise HTTPException(status_code=404, detail=f"no record with code {code}")
    except ValueError as exc:
        raise HTTPException(status_code=400, detail=str(exc))
    except Exception as exc:
        raise HTTPException(status_code=500, detail=f"查询失败: {exc}")
    from .icd_models import Candidate
    candidates = [Candidate(code=h["code"], title=h["title"] or "", score=max(float(h["score"]), 0.0), enhanced_score=float(h["score"]),
                            level=h["metadata"].get("level", 1), parent_code=h["metadata"].get("parent_code", ""),
                            original_score=float(h["original_score"]))
                  for h in hits]
    return SimilarCodesResponse(**convert_numpy_types(SimilarCodesResponse(code=code, candidates=candidates).model_dump()))


@app.get("/codes/{code}")
async def codes_get(code: str):
    """The stored record of one ICD code (`code == "..."` through MilvusService.query); 404 when the collection holds none"""
    if not milvus_service:
        raise HTTPException(status_code=503, detail="服务未就绪")
    if '"' in code or "\\" in code:
        raise HTTPException(status_code=400, detail="code: no quotes or backslashes")
    try:
        rows = milvus_service.query(f'code == "{code}"', limit=10)
    except ValueError as exc:
        raise HTTPException(status_code=400, detail=str(exc))
    except Exception as exc:
        raise HTTPException(status_code=500, detail=f"查询失败: {exc}")
    if not rows:
        raise HTTPException(status_code=404, detail=f"no record with code {code}")
    return convert_numpy_types(rows[0])


@app.post("/embed", response_model=EmbeddingResponse)
async def embed_texts(request: EmbeddingRequest):
    try:
        if not embedding_service:
            raise HTTPException(status_code=503, detail="向量化服务未就绪")
        embeddings = embedding_service.encode_batch(request.texts, show_progress=False)
        name = embedding_service.get_model_info().get("model_name", "unknown")
        return EmbeddingResponse(embeddings=embeddings, model=name)
    except Exception as exc:
        raise HTTPException(status_code=500, detail=f"向量化失败: {exc}")


@app.get("/stats")
async def get_stats():
    try:
        stats = {}
        if milvus_service:
            stats["milvus"] = milvus_service.get_collection_stats()
            if hasattr(milvus_service, "filter_views"):   # the cached filter views: expression, rows, HBM bytes
                stats["filter_views"] = milvus_service.filter_views()
            if hasattr(milvus_service, "filter_masks"):   # the cached filter masks (filter_mode "mask", per-query filters): expression, rows, HBM bytes
                stats["filter_masks"] = milvus_service.filter_masks()
            if hasattr(milvus_service, "groupings"):      # the cached groupings: field, groups, largest group, HBM bytes
                stats["groupings"] = milvus_service.groupings()
            if hasattr(milvus_service, "fusions"):        # the hybrid-search workspace: sub-lists per call, HBM bytes
                stats["fusions"] = milvus_service.fusions()
            if hasattr(milvus_service, "sparse_indexes"):   # the sparse (BM25) index: field, vocabulary, postings, HBM bytes
                stats["sparse_indexes"] = milvus_service.sparse_indexes()
        if embedding_service:
            stats["embedding"] = embedding_service.get_model_info()
        return stats
    except Exception as exc:
        raise HTTPException(status_code=500, detail=f"获取统计信息失败: {exc}")
