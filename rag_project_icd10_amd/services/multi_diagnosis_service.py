"""Per-diagnosis embed -> search(2k) -> hierarchical rescoring -> top_k: the serving-time caller of the
hot path, reduced to the parts that are in scope.

Follows the reference's services/multi_diagnosis_service.py: match_multiple_diagnoses (:51-125) and
_match_single_diagnosis_enhanced steps 2-4 (:152-175). Match confidence: by default (confidence="match") the reference's
original formula _calculate_match_confidence (:276-304); with confidence="multidimensional" its step 5 (:176-207), the 12-factor
MultiDimensionalConfidenceService, whose overall confidence becomes match_confidence and whose metrics, factors and level ride
on the match. NOT reproduced (out of scope): the semantic-boundary splitter (delimiter split only). The NER service (row N4) is optional: without one, query_entities is {}; with one, the all-device batch path
(match_diagnoses_batch(..., entities=)) rescores with the diagnoses' entities. Difference by design (row N2): all diagnoses of a
request are embedded in ONE encoder batch and searched in ONE search_batch call.
"""
from __future__ import annotations

import gc
import logging
import threading
from typing import Any, Dict, List, Optional

import numpy as np

from ..api.icd_models import Candidate, DiagnosisMatch, trusted_candidate, trusted_candidates
from ..tools.text_processor import DiagnosisTextProcessor
from .hierarchical_similarity_service import HierarchicalSimilarityService
from .multidimensional_confidence_service import MultiDimensionalConfidenceService

logger = logging.getLogger(__name__)



# The collector is a PROCESS-WIDE switch: under a threaded server two requests must not toggle it for each other (one
# re-enabling it in the middle of the other's build, or leaving it off for good). A lock-protected depth counter: the
# first request in switches it off (if it was on), the last one out switches it back on.
_gc_lock = threading.Lock()
_gc_depth = 0
_gc_was_on = False


class _gc_paused:
    def __enter__(self):
        global _gc_depth, _gc_was_on
        with _gc_lock:
            if _gc_depth == 0:
                _gc_was_on = gc.isenabled()
                if _gc_was_on:
                    gc.disable()
            _gc_depth += 1

    def __exit__(self, *exc):
        global _gc_depth
        with _gc_lock:
            _gc_depth -= 1
            if _gc_depth == 0 and _gc_was_on:
                gc.enable()
        return False

CONFIDENCE_MODES = ("match", "multidimensional")


def _search_options(filter, group_by_field, group_size, radius=None, range_filter=None, filter_mode="view", group_scorer=None) -> Dict[str, Any]:   # noqa: A002
    """keyword arguments of MilvusService.search_batch for a request's filter / grouping / range: only the ones that were given"""
    opts: Dict[str, Any] = {}
    if filter_mode != "view":
        opts["filter_mode"] = filter_mode
    if radius is not None:
        opts["radius"] = radius
    if range_filter is not None:
        opts["range_filter"] = range_filter
    if filter is not None:
        opts["filter"] = filter
    if group_by_field is not None or group_size != 1:
        opts["group_by_field"], opts["group_size"] = group_by_field, group_size
    if group_scorer is not None:
        opts["group_scorer"] = group_scorer
    return opts


class MultiDiagnosisService:
    def __init__(self, embedding_service, milvus_service, ner_service=None, confidence: str = "match"):
        """ner_service: a MedicalNERService (row N4) or None. The reference always builds one (:28); here it is opt-in
        because its weights are not available offline - with one given, the per-request path extracts the entities of
        all diagnoses of a request in ONE classifier batch and hands them to the rescoring like the reference (:147-158).
        confidence: "match" (the default: _calculate_match_confidence) or "multidimensional" (the reference's enhanced match,
        :176-207; a diagnosis whose confidence step fails, or gives a value outside [0, 1], keeps the "match" answer)."""
        if confidence not in CONFIDENCE_MODES:
            raise ValueError(f"confidence={confidence!r}: one of {CONFIDENCE_MODES}")
        self.confidence = confidence
        self.embedding_service = embedding_service
        self.milvus_service = milvus_service
        self.ner_service = ner_service
        self.hierarchical_similarity = HierarchicalSimilarityService(embedding_service=embedding_service,
                                                                     ner_service=ner_service)
        # the reference's default text mode is "enhanced" (entities + semantic boundaries, :44-47): here whenever there is an NER service
        self.text_processor = DiagnosisTextProcessor(embedding_service=embedding_service, ner_service=ner_service)
        # like the reference (:37-41): the confidence service shares the embedding and NER services
        self.confidence_service = MultiDimensionalConfidenceService(
            embedding_service=embedding_service, ner_service=ner_service, hierarchical_similarity_service=self.hierarchical_similarity)

    def match_multiple_diagnoses(self, text: str, top_k: int = 5, filter: Optional[str] = None,   # noqa: A002
                                 group_by_field: Optional[str] = None, group_size: int = 1, radius: Optional[float] = None,
                                 range_filter: Optional[float] = None, filter_mode: str = "view",
                                 group_scorer: Optional[str] = None) -> Dict[str, Any]:
        """group_scorer ("max", "sum", "avg", next to group_by_field): what a group of the grouped search ranks by
        (MilvusService.search_batch); a value outside the three names, or one without group_by_field, is a ValueError.
        filter: a Milvus filter expression (services/filter_expr.py) - every diagnosis is searched among the rows it selects only
        (the search of 2 top_k, on the device path and the host path alike); None ranks the whole corpus. filter_mode: "view" (the
        default) or "mask" - how MilvusService.search_batch applies it (a cached view, or a row mask of the index itself).
        radius / range_filter: Milvus's range search - only rows with radius < inner product <= range_filter are ranked
        (MilvusService.search_batch); a diagnosis with fewer than 2 top_k such rows is rescored on the shorter list."""
        if group_scorer is not None:
            from . import filter_expr
            filter_expr.check_group_scorer(group_by_field, group_scorer)
        enhanced = self.text_processor.extract_diagnoses_enhanced(text)
        diagnoses = [d["text"] for d in enhanced]
        mode = self.text_processor.get_processing_mode()
        if not diagnoses:
            return {"original_text": text, "extracted_diagnoses": [], "matches": [], "total_matches": 0,
                    "processing_mode": mode,
                    "extraction_metadata": {"enhanced_results_count": 0, "avg_extraction_confidence": 0.0}}
        confs = [d.get("diagnosis_confidence", 0.5) for d in enhanced]
        # one encoder batch + one search batch for the whole request
        grouped = {} if group_by_field is None and group_size == 1 else {"group_by_field": group_by_field, "group_size": group_size}
        if radius is not None:
            grouped["radius"] = radius
        if range_filter is not None:
            grouped["range_filter"] = range_filter
        if filter_mode != "view":
            grouped["filter_mode"] = filter_mode
        if group_scorer is not None:
            grouped["group_scorer"] = group_scorer
        matches = None
        ner_job = vectors = None
        device = getattr(self.milvus_service, "supports_device_rescoring", lambda: False)()
        if self.ner_service is None and device:
            # no entities to match (the reference's rescoring then depends on the query string and the hits' codes only):
            # the whole request stays on the device - encode -> search(2 top_k) -> rescoring -> top_k winners come back.
            # Same DiagnosisMatch objects as the host path below (tests/test_gpu_parity.py, all 1 000 golden strings).
            try:
                matches = self.match_diagnoses_batch(diagnoses, top_k=top_k, filter=filter, **grouped)
            except Exception as exc:
                logger.error("device-side request path failed (%s): host path", exc)
                matches = None
        elif device:
            # with entities: on live hits they feed three factors that depend on the query and the hit's chapter letter only, so
            # the rescoring stays on the device as well (query_params_entities, icd_hier_rescore_entities). The classifier runs in
            # its worker thread while this thread embeds and searches; its entities are joined before the rescoring launch.
            ner_job = self._ner_pool().submit(self._entities_of, diagnoses)
            try:
                vectors = self._embed_diagnoses(diagnoses)
                matches = self.match_diagnoses_batch(diagnoses, top_k=top_k, vectors=vectors, entities=ner_job, filter=filter, **grouped)
            except Exception as exc:
                logger.error("device-side request path with entities failed (%s): host path", exc)
                matches = None
        if matches is not None:
            return {"original_text": text, "extracted_diagnoses": diagnoses, "matches": matches,
                    "total_matches": sum(len(m.candidates) for m in matches), "processing_mode": mode,
                    "extraction_metadata": {"enhanced_results_count": len(enhanced),
                                            "avg_extraction_confidence": sum(confs) / len(confs),
                                            "extraction_method": mode, "drug_filtering_enabled": mode == "enhanced"}}
        # The entities of the request's diagnoses do not depend on their embeddings: the token classifier runs in a worker thread on
        # its own stream WHILE this thread embeds and searches (both forwards are latency-bound - a few work-groups each, csrc/
        # encoder_small.hpp - and overlap almost entirely: a one-diagnosis request with NER 1.14 -> 0.8 ms). Same results either way.
        if ner_job is None and self.ner_service:
            ner_job = self._ner_pool().submit(self._entities_of, diagnoses)
        if vectors is None:
            vectors = self._embed_diagnoses(diagnoses)
        try:
            hit_lists = self.milvus_service.search_batch(vectors, top_k * 2, as_dicts=True, **_search_options(filter, group_by_field, group_size, radius, range_filter, filter_mode, group_scorer))
        except Exception as exc:
            logger.error("batch search failed: %s", exc)
            hit_lists = [[] for _ in diagnoses]
        entities = ner_job.result() if ner_job is not None else [{} for _ in diagnoses]
        matches = [self._match_from_hits(d, hits, top_k, ents) for d, hits, ents in zip(diagnoses, hit_lists, entities)]
        return {"original_text": text, "extracted_diagnoses": diagnoses, "matches": matches,
                "total_matches": sum(len(m.candidates) for m in matches), "processing_mode": mode,
                "extraction_metadata": {"enhanced_results_count": len(enhanced),
                                        "avg_extraction_confidence": sum(confs) / len(confs),
                                        "extraction_method": mode, "drug_filtering_enabled": mode == "enhanced"}}

    def _embed_diagnoses(self, diagnoses: List[str]):
        """the request's diagnoses embedded in one batch - minus those the enhanced text mode has embedded already: a diagnosis that is a
        boundary's text was embedded when the boundaries were scored (services/semantic_boundary_service.py), and the canonical batch
        arithmetic gives a string the same bits whatever shares its call"""
        detector = getattr(getattr(self.text_processor, "_enhanced_processor", None), "boundary_detector", None)
        known = [detector.cached_vector(d) if detector is not None else None for d in diagnoses]
        missing = [d for d, v in zip(diagnoses, known) if v is None]
        if len(missing) == len(diagnoses):
            return self.embedding_service.encode_query_batch(diagnoses)
        fresh = iter(self.embedding_service.encode_query_batch(missing)) if missing else iter(())
        return np.stack([np.asarray(v) if v is not None else np.asarray(next(fresh)) for v in known])

    def _ner_pool(self):
        pool = getattr(self, "_ner_executor", None)
        if pool is None:
            from concurrent.futures import ThreadPoolExecutor
            pool = self._ner_executor = ThreadPoolExecutor(max_workers=1, thread_name_prefix="icd-ner")
        return pool

    def _entities_of(self, diagnoses: List[str]) -> List[Dict[str, Any]]:
        """the entities of every diagnosis of a request, never raising (the reference extracts inside
        _match_single_diagnosis_enhanced's try, services/multi_diagnosis_service.py:147-158: a failing NER costs that diagnosis its
        entities, never the request - one batch here, so a failure of the batch retries string by string and only the strings that
        still fail go without entities). Runs in the worker thread of _ner_pool, on its own stream when the classifier is on a GPU."""
        entities = [{} for _ in diagnoses]
        stream_ctx = None
        try:
            import torch
            dev = getattr(getattr(self.ner_service, "ner_pipeline", None), "device", "cpu")
            if str(dev).startswith("cuda") and torch.cuda.is_available():
                if getattr(self, "_ner_stream", None) is None:
                    self._ner_stream = torch.cuda.Stream(device=dev)
                stream_ctx = torch.cuda.stream(self._ner_stream)
        except Exception:   # (no torch / no GPU: the caller's stream, which is then the CPU)
            stream_ctx = None
        import contextlib
        # a diagnosis that IS the request's text (the usual one-diagnosis request) was classified when the text was cut: the same string,
        # the same switches, the same entities - not a second forward
        last = getattr(getattr(self.text_processor, "_enhanced_processor", None), "last_text_entities", None)
        if last is not None and last[1] and last[2] is not None and any(d == last[0] for d in diagnoses):
            import copy
            rest = [d for d in diagnoses if d != last[0]]
            rest_entities = iter(self._entities_of(rest)) if rest else iter(())
            return [copy.deepcopy(last[2]) if d == last[0] else next(rest_entities) for d in diagnoses]
        with (stream_ctx if stream_ctx is not None else contextlib.nullcontext()):
            try:
                entities = self.ner_service.extract_medical_entities_batch(diagnoses, filter_drugs=True)
            except Exception as exc:
                logger.error("batch NER failed (%s): one string at a time", exc)
                for i, d in enumerate(diagnoses):
                    try:
                        entities[i] = self.ner_service.extract_medical_entities(d, filter_drugs=True)
                    except Exception as exc1:
                        logger.error("NER failed for %r: %s", d, exc1)
        return entities

    def match_diagnoses_batch(self, diagnoses: List[str], top_k: int = 5, vectors=None,
                              confidence_statistics: bool = False, entities=None, confidence: str = None,
                              filter: Optional[str] = None, group_by_field: Optional[str] = None,   # noqa: A002
                              group_size: int = 1, radius: Optional[float] = None,
                              range_filter: Optional[float] = None, filter_mode: str = "view",
                              group_scorer: Optional[str] = None) -> List[DiagnosisMatch]:
        """Additive (row N2): embed -> search(2 top_k) -> level reweight -> hierarchical rescoring for MANY diagnosis
        strings with everything between the tokenizer and the final top_k on the GPU: one encoder batch, one search_batch,
        one rescoring launch; only the top_k winners per string come back and become Candidate objects. Same results as
        _match_from_hits(d, milvus.search(encode_query(d), 2 top_k), top_k) per string (tests/test_gpu_parity.py).
        confidence_statistics=True (row N3) also fills DiagnosisMatch.confidence_factors with the three numbers of the
        reference's confidence service that are in scope - semantic_coherence (the live shape: cosine with the embedding
        of the empty string), model_uncertainty, prediction_variance - computed for the whole batch in two launches.
        entities: the NER entities of every diagnosis (a list of entity dicts, or a Future of one - joined once the search is
        enqueued): each string is then rescored as _match_from_hits(d, hits, top_k, entities[i]) rescores it, on the device
        (HierarchicalSimilarityService.query_params_entities, icd_hier_rescore_entities).
        confidence: "match" / "multidimensional" (None: the service's mode). "multidimensional" scores every match with
        MultiDimensionalConfidenceService.comprehensive_confidence_batch - the cosine, the score statistics and the terminology
        scan as one launch each - equal to _match_from_hits' per-call scores except the cosine (sklearn's, to ~1e-14).
        filter: a Milvus filter expression: the search of 2 top_k ranks the rows it selects only (MilvusService.search_batch);
        the rescoring, the entities and both confidence modes then run unchanged on those hits (ids stay the corpus's row ids).
        A list or tuple with one expression (or None) PER DIAGNOSIS ranks every string over its own selection in the same ONE
        search (row masks), also with entities; filter_mode="mask" applies a single expression that way.
        group_by_field / group_size: Milvus's grouping search (MilvusService.search_batch): the search of 2 top_k then returns the
        group_size best rows of the 2 top_k best GROUPS, and the rescoring runs on those hits (2 top_k group_size <= 128).
        group_scorer: what a group ranks by ("max", "sum", "avg"; MilvusService.search_batch); a bad value is a ValueError.
        radius / range_filter: Milvus's range search (MilvusService.search_batch): lists shorter than 2 top_k arrive padded, as a
        short filter selection's do."""
        if group_scorer is not None:
            from . import filter_expr
            filter_expr.check_group_scorer(group_by_field, group_scorer)
        from .hierarchical_similarity_service import trusted_factors_row
        confidence = self.confidence if confidence is None else confidence
        if confidence not in CONFIDENCE_MODES:
            raise ValueError(f"confidence={confidence!r}: one of {CONFIDENCE_MODES}")
        if not diagnoses:
            return []
        import torch
        if vectors is None:
            vectors = self.embedding_service.encode_query_batch(diagnoses, to_device=True)
        elif not torch.is_tensor(vectors):   # (host vectors, e.g. _embed_diagnoses': the search then keeps its results on the device)
            vectors = torch.from_numpy(np.ascontiguousarray(vectors, dtype=np.float32)).to(self.milvus_service.row_tags().device)
        hs = self.hierarchical_similarity
        if entities is None:
            qps = [hs.query_params(d) for d in diagnoses]   # ([1] is the context relevance the factors report)
        adj, raw, ids = self.milvus_service.search_batch(vectors, top_k * 2, **_search_options(filter, group_by_field, group_size, radius, range_filter, filter_mode, group_scorer))[:3]
        if entities is not None:
            if hasattr(entities, "result"):   # (the NER worker's Future: the classifier ran beside the embedding and the search)
                entities = entities.result()
            if len(entities) != len(diagnoses):
                raise ValueError(f"{len(entities)} entity dicts for {len(diagnoses)} diagnoses")
            qps = [hs.query_params_entities(d, e or {}) for d, e in zip(diagnoses, entities)]   # ([12] entity match, [13..21] alignment)
        order, enh, score, vs, hb, boost = hs.rescore_live_hits_batch(diagnoses, adj, ids, self.milvus_service.row_tags(),
                                                                       q_params=qps)
        # winners only: gather on the device, one copy to the host, plain Python lists for the object loop
        import torch
        kk = min(top_k, order.shape[1])
        # (ONE copy: eight .tolist() calls were eight stream synchronisations, ~20 us each - a fifth of a one-diagnosis request.
        #  Everything travels in 8-byte slots: float64 - exact for the int32 order and the float32 scores - except the int64 ids,
        #  whose bit patterns ride in plane 0 (an id_base of a shard may exceed 2^53))
        if adj.is_cuda:
            from .. import _native
            packed = _native.pack_winners(order, ids, raw, adj, enh, vs, hb, boost, kk).cpu()   # (one launch: gathers, slices, stack)
        else:
            o = order[:, :kk].long().clamp(min=0)
            packed = torch.stack([torch.gather(ids, 1, o).long().contiguous().view(torch.float64), torch.gather(raw, 1, o).double(), torch.gather(adj, 1, o).double()]
                                 + [t[:, :kk].double() for t in (order, enh, vs, hb, boost)], 0)
        h_ids, h_ord = packed[0].contiguous().view(torch.int64).tolist(), packed[3].long().tolist()
        h_raw, h_adj, h_enh, h_vs, h_hb, h_boost = (packed[i].tolist() for i in (1, 2, 4, 5, 6, 7))
        recs = self.milvus_service.client.records
        sc = 0.3 if hs.embedding_service else 0.5
        conf = None
        if confidence_statistics:
            cs = self.confidence_service
            stats = cs.score_statistics_batch(enh, order, top_k=kk).tolist()
            qv = vectors if torch.is_tensor(vectors) else torch.as_tensor(np.asarray(vectors, dtype=np.float32))
            coh = cs.semantic_coherence_batch(qv.to(adj.device)).tolist()
            conf = [{"semantic_coherence": coh[q], "model_uncertainty": stats[q][4], "prediction_variance": stats[q][5]}
                    for q in range(len(diagnoses))]
        out = []
        failed = set()
        # (tens of thousands of acyclic objects are born here: the collector's generation-0 passes over them are pure cost)
        with _gc_paused():
            self._build_matches(out, diagnoses, kk, h_ord, h_enh, h_adj, h_raw, h_boost, h_ids, h_vs, h_hb, recs, sc, qps, conf, trusted_factors_row,
                                with_entities=entities is not None, failed=failed)
        if confidence == "multidimensional":
            qv = vectors if torch.is_tensor(vectors) else torch.as_tensor(np.asarray(vectors, dtype=np.float32))
            stats = self.confidence_service.score_statistics_batch(enh, order, top_k=kk).tolist() if adj.is_cuda else None
            self._multidimensional_batch(out, diagnoses, qv.to(adj.device), entities, stats, failed)
        return out

    @staticmethod
    def _confidence_inputs(candidates):
        """the reference's inputs of the confidence step (:176-196): records of the top_k candidates with score = enhanced_score,
        and the top-ranked hit's three factors (None without hits)"""
        records = [{"code": c.code, "title": c.title, "score": c.enhanced_score if hasattr(c, "enhanced_score") else c.score,
                    "level": getattr(c, "level", 1)} for c in candidates]
        if not candidates:
            return records, None
        f = candidates[0].similarity_factors
        return records, {"vector_similarity": f.vector_similarity, "hierarchy_boost": f.hierarchy_boost,
                         "entity_match_score": f.entity_match_score}

    def _with_confidence(self, match: DiagnosisMatch, metrics, factors) -> DiagnosisMatch:
        """the match with the multidimensional confidence (:198-207); the match as it is when the value fails match_confidence's
        0 <= c <= 1"""
        try:
            mc = float(metrics.overall_confidence)
            if not 0.0 <= mc <= 1.0:
                raise ValueError(f"overall confidence {mc}")
            return DiagnosisMatch(diagnosis_text=match.diagnosis_text, candidates=match.candidates, match_confidence=mc,
                                  confidence_metrics=metrics, confidence_factors=factors,
                                  confidence_level=self.confidence_service.get_confidence_level(mc))
        except Exception as exc:
            logger.error("multidimensional confidence failed for %s (%s): the match confidence stays", match.diagnosis_text, exc)
            return match

    def _multidimensional_batch(self, out, diagnoses, query_vectors, entities, stats, failed):
        idx = [q for q in range(len(diagnoses)) if q not in failed]
        if not idx:
            return
        try:
            inputs = [self._confidence_inputs(out[q].candidates) for q in idx]
            scored = self.confidence_service.comprehensive_confidence_batch(
                [diagnoses[q] for q in idx], [r for r, _ in inputs], [f for _, f in inputs], query_vectors=query_vectors[idx],
                entities=None if entities is None else [entities[q] for q in idx],
                stats=None if stats is None else [stats[q] for q in idx])
        except Exception as exc:
            logger.error("batch multidimensional confidence failed (%s): match confidences stay", exc)
            return
        for q, (metrics, factors) in zip(idx, scored):
            out[q] = self._with_confidence(out[q], metrics, factors)

    def _build_matches(self, out, diagnoses, kk, h_ord, h_enh, h_adj, h_raw, h_boost, h_ids, h_vs, h_hb, recs, sc, qps, conf, trusted_factors_row,
                       with_entities=False, failed=None):
        from ..api.icd_models import bulk_candidates, trusted_match, trusted_matches_ready
        from .hierarchical_similarity_service import SimilarityFactors
        # the corpus' code / title columns (plain lists by row) where the store offers them, and the one-loop constructor once
        # trusted_candidate has checked this pydantic's object layout on a real hit (the first call of a process does)
        cols = getattr(getattr(self.milvus_service, "client", None), "code_title_columns", None)
        codes = titles = None
        if cols is not None and recs is getattr(self.milvus_service.client, "records", None):
            codes, titles = cols()
        chapters = HierarchicalSimilarityService.CHAPTER_ORDER
        for q, diagnosis in enumerate(diagnoses):
            try:
                # how many winners exist (order < 0 from there on); live hits carry level / parent_code under "metadata": the
                # top-level defaults apply (F8). The values are Python floats / str already (tolist() of the device results):
                # the trusted constructors skip the per-object validator but keep its one rule with teeth - a negative score
                # raises and degrades the whole match to an empty one, like the reference's
                n = kk
                row_ord = h_ord[q]
                if row_ord[kk - 1] < 0:   # (the winners come first: most queries have all kk)
                    for j in range(kk):
                        if row_ord[j] < 0:
                            n = j
                            break
                enh_q, adj_q, raw_q, boost_q = h_enh[q], h_adj[q], h_raw[q], h_boost[q]
                if max(boost_q) > 0:      # (an uncertainty marker in the query: the boosted hits report their reweighted score)
                    originals = [adj_q[j] if boost_q[j] > 0 else raw_q[j] for j in range(n)]
                else:
                    originals = raw_q
                em = ca = None
                if with_entities:
                    # the entity match score is one per query; a winner's category alignment is its chapter's entry of the table
                    # (0.0 for a letter outside it), the value the kernel added - looked up by the winner's code, as row_tag does
                    qp = qps[q]
                    em, ca_of = qp[12], dict(zip(chapters, qp[13:22]))
                    ca = [ca_of.get(((codes[i] if codes is not None else recs[i].get("code")) or "")[:1], 0.0) for i in h_ids[q][:n]]
                if codes is not None and trusted_matches_ready():
                    ids_q = h_ids[q] if n == kk else h_ids[q][:n]
                    if ca is None:
                        cands = bulk_candidates(codes, titles, SimilarityFactors, ids_q, enh_q, originals, h_vs[q], h_hb[q], sc, qps[q][1])
                    else:
                        cands = bulk_candidates(codes, titles, SimilarityFactors, ids_q, enh_q, originals, h_vs[q], h_hb[q], sc, qps[q][1], em, ca)
                else:
                    cands = trusted_candidates(recs, h_ids[q][:n], enh_q[:n], originals[:n],
                                               trusted_factors_row(h_vs[q][:n], h_hb[q][:n], sc, qps[q][1], *(() if ca is None else (em, ca))))
                out.append(trusted_match(diagnosis, cands, self._match_confidence_of_scores(enh_q if n == kk else enh_q[:n]), conf[q] if conf is not None else None))
            except Exception as exc:
                logger.error("match failed for %s: %s", diagnosis, exc)
                out.append(DiagnosisMatch(diagnosis_text=diagnosis, candidates=[], match_confidence=0.0))
                if failed is not None:
                    failed.add(q)

    def _match_from_hits(self, diagnosis: str, hits: List[Dict[str, Any]], top_k: int,
                         query_entities: Dict[str, Any] = None) -> DiagnosisMatch:
        try:
            rescored = self.hierarchical_similarity.batch_calculate_similarities(diagnosis, query_entities or {}, hits)
            candidates = []
            for rec, score, factors in rescored[:top_k]:
                cand = Candidate(code=rec.get("code", ""), title=rec.get("title", ""), score=float(score))
                cand.level = rec.get("level", 1)
                cand.parent_code = rec.get("parent_code", "")
                cand.enhanced_score = float(score)
                cand.original_score = float(rec.get("original_score", 0.0))
                cand.similarity_factors = factors
                candidates.append(cand)
            match = DiagnosisMatch(diagnosis_text=diagnosis, candidates=candidates,
                                   match_confidence=self._calculate_match_confidence(candidates))
        except Exception as exc:  # e.g. a negative score fails Candidate's ge=0 validator
            logger.error("match failed for %s: %s", diagnosis, exc)
            return DiagnosisMatch(diagnosis_text=diagnosis, candidates=[], match_confidence=0.0)
        if self.confidence != "multidimensional":
            return match
        try:
            records, sf = self._confidence_inputs(candidates)
            # (the request's entities are extract_medical_entities(diagnosis, filter_drugs=True): the call the confidence service makes)
            pre = {"query_entities": query_entities} if self.ner_service is not None and query_entities is not None else None
            metrics, factors = self.confidence_service.calculate_comprehensive_confidence(diagnosis, records, sf, pre=pre)
        except Exception as exc:
            logger.error("multidimensional confidence failed for %s (%s): the match confidence stays", diagnosis, exc)
            return match
        return self._with_confidence(match, metrics, factors)

    def _calculate_match_confidence(self, candidates: List[Candidate]) -> float:
        if not candidates:
            return 0.0
        return self._match_confidence_of_scores([c.score for c in candidates])

    @staticmethod
    def _match_confidence_of_scores(scores) -> float:
        """the reference's _calculate_match_confidence (services/multi_diagnosis_service.py:276-304) on the candidates' scores"""
        if not scores:
            return 0.0
        best = max(scores)
        if best > 0.9:
            conf = min(best, 0.95)
        elif len([s for s in scores if s > 0.7]) >= 2:
            conf = best * 0.8
        else:
            conf = best * 0.6
        return round(conf, 3)
