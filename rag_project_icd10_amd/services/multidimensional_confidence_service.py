"""The reference's 12-factor confidence service, per call on the host, and for a whole batch with its device pieces.

Follows the reference's services/multidimensional_confidence_service.py (:14-1260) as it behaves:
    ConfidenceFactors / ConfidenceMetrics   :14-74      same fields, defaults and __post_init__ coercions
    factor_weights, confidence_thresholds   :96-125
    _init_complexity_classifier             :138-156
    calculate_comprehensive_confidence      :158-213    and every factor method it reaches (:215-1019)
    ICD terminology cache                   :541-694    _calculate_term_weight, _load_icd_terminology_if_needed,
                                                        _parse_icd_level, _calculate_icd_base_score, _calculate_category_score,
                                                        _get_term_specificity_from_icd
    _merge_factors, _calculate_final_metrics :1021-1157  with the variance, interval, reliability and calibration scores
    get_confidence_level ... get_confidence_explanation  :1159-1258
Differences by design: stdlib logging instead of loguru; sklearn's cosine_similarity is restated by `_cosine` (bit for bit on
two rows); the CSV path is resolvable (`terminology_csv`, ICD_TERMINOLOGY_CSV, else where the reference's relative path lands
in this package) and may be xz-compressed.

Properties of the reference kept as they are:
  - the live /query path hands this service records WITHOUT 'preferred_zh' (services/multi_diagnosis_service.py:178-186
    builds them from code / title / score / level), so the candidate text is '' and "the candidate vector" is the
    embedding of the empty string - one constant vector. context_consistency, terminology_accuracy and the context term of
    clinical_relevance are then 0; this is computed, not special-cased.
  - the terminology cache is a dict filled in CSV order: a name keeps the position of its FIRST row and the score of its
    LAST one; a partial match is the first key in that order that contains the term or that the term contains.

Batch entry points (additive): `score_statistics_batch` (icd_score_stats: numpy-identical doubles),
`semantic_coherence_batch` (icd_cosine_rows), `term_specificity_batch` (exact hits on the host, the misses' scan in ONE
icd_term_first_match launch) and `comprehensive_confidence_batch`, which runs the per-call arithmetic with those values
filled in.
"""
from __future__ import annotations

import logging
import os
import re
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

logger = logging.getLogger(__name__)

STAT_COLUMNS = ("mean", "std", "var", "max", "model_uncertainty", "prediction_variance")

# where the reference's os.path.join(<services>, '..', 'data', 'ICD_10v601.csv') lands in this package
DEFAULT_TERMINOLOGY_CSV = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "ICD_10v601.csv")
TERM_MAX_CODEPOINTS = 32   # include/icd_search.h ICD_TERM_MAX_LEN: longer terms are scanned on the host

_DISEASE_PATTERNS = (   # _extract_medical_terms_from_text (:523-530)
    r'[^，。；\s]{2,10}病',
    r'[^，。；\s]{2,10}症',
    r'[^，。；\s]{2,10}炎',
    r'[^，。；\s]{2,10}综合征',
    r'急性[^，。；\s]{2,10}',
    r'慢性[^，。；\s]{2,10}',
)


@dataclass
class ConfidenceFactors:
    """:14-50"""
    vector_similarity: float = 0.0
    hierarchy_boost: float = 0.0
    entity_match_score: float = 0.0
    semantic_coherence: float = 0.0
    context_consistency: float = 0.0
    terminology_accuracy: float = 0.0
    diagnosis_complexity: float = 0.0
    professional_specificity: float = 0.0
    clinical_relevance: float = 0.0
    data_quality: float = 0.0
    model_uncertainty: float = 0.0
    cross_validation_score: float = 0.0

    def __post_init__(self):
        self.vector_similarity = float(self.vector_similarity)
        self.hierarchy_boost = float(self.hierarchy_boost)
        self.entity_match_score = float(self.entity_match_score)
        self.semantic_coherence = float(self.semantic_coherence)
        self.context_consistency = float(self.context_consistency)
        self.terminology_accuracy = float(self.terminology_accuracy)
        self.diagnosis_complexity = float(self.diagnosis_complexity)
        self.professional_specificity = float(self.professional_specificity)
        self.clinical_relevance = float(self.clinical_relevance)
        self.data_quality = float(self.data_quality)
        self.model_uncertainty = float(self.model_uncertainty)
        self.cross_validation_score = float(self.cross_validation_score)


@dataclass
class ConfidenceMetrics:
    """:54-74"""
    overall_confidence: float = 0.0
    confidence_interval: Tuple[float, float] = (0.0, 0.0)
    reliability_score: float = 0.0
    prediction_variance: float = 0.0
    calibration_score: float = 0.0

    def __post_init__(self):
        self.overall_confidence = float(self.overall_confidence)
        self.reliability_score = float(self.reliability_score)
        self.prediction_variance = float(self.prediction_variance)
        self.calibration_score = float(self.calibration_score)
        if self.confidence_interval:
            self.confidence_interval = (float(self.confidence_interval[0]), float(self.confidence_interval[1]))


class MultiDimensionalConfidenceService:
    def __init__(self, embedding_service=None, ner_service=None, hierarchical_similarity_service=None,
                 terminology_csv: Optional[str] = None):
        """:80-135. terminology_csv: the ICD CSV of the terminology cache (.csv or .csv.xz); else ICD_TERMINOLOGY_CSV, else
        DEFAULT_TERMINOLOGY_CSV."""
        self.embedding_service = embedding_service
        self.ner_service = ner_service
        self.hierarchical_similarity_service = hierarchical_similarity_service
        self.terminology_csv = terminology_csv
        self._empty_vector = None   # encode_query('') on the device, made on first use
        self._empty_entities = None  # the NER entities of the live candidate text '', made on first use
        self._term_table = None     # (device, key code points, key offsets) of icd_term_first_match, made on first use
        self._term_keys = None      # the cache's keys in scan order, made on first use
        self.factor_weights = {
            'vector_similarity': 0.20,
            'hierarchy_boost': 0.15,
            'entity_match_score': 0.15,
            'semantic_coherence': 0.12,
            'context_consistency': 0.10,
            'terminology_accuracy': 0.08,
            'diagnosis_complexity': 0.05,
            'professional_specificity': 0.05,
            'clinical_relevance': 0.05,
            'data_quality': 0.02,
            'model_uncertainty': 0.02,
            'cross_validation_score': 0.01,
        }
        self.confidence_thresholds = {
            'high_confidence': 0.80,
            'medium_confidence': 0.60,
            'low_confidence': 0.40,
            'reject_threshold': 0.20,
        }
        self.icd_terminology_cache: Dict[str, float] = {}
        self.icd_data_loaded = False
        self.complexity_classifier = self._init_complexity_classifier()
        logger.debug("confidence weights: %s", self.factor_weights)

    def _init_complexity_classifier(self) -> Dict[str, Any]:
        """:138-156 (the character classes written as the reference writes them)"""
        return {
            'simple_patterns': [
                r'^[^，。；]{2,8}病$',
                r'^[^，。；]{2,6}[痛|热|肿]$',
            ],
            'moderate_patterns': [
                r'伴[^，。；]{2,10}',
                r'[^，。；]{3,12}综合征',
                r'[急性|慢性][^，。；]{2,10}',
            ],
            'complex_patterns': [
                r'[^，。；]{5,}并[^，。；]{5,}',
                r'[^，。；]{3,}伴[^，。；]{3,}伴[^，。；]{3,}',
                r'[^，。；]{8,}酸中毒',
                r'多发性[^，。；]{3,}',
            ],
        }

    # ---- the comprehensive score (:158-213) ------------------------------------------------------------------------
    # `pre` (batch path only): values computed for a whole batch beforehand - 'coherence' (the cosine), 'query_entities',
    # 'candidate_entities' (NER results), 'spec' (term -> _get_term_specificity_from_icd), 'stats' (an icd_score_stats row).
    # Each replaces exactly the call that produces it; everything else is the per-call arithmetic.
    def calculate_comprehensive_confidence(self, query_text: str, candidate_records: List[Dict[str, Any]],
                                           similarity_factors: Optional[Dict] = None,
                                           pre: Optional[Dict[str, Any]] = None) -> Tuple[ConfidenceMetrics, ConfidenceFactors]:
        try:
            factors = self._calculate_base_factors(query_text, candidate_records, similarity_factors)
            semantic_factors = self._calculate_semantic_factors(query_text, candidate_records, pre)
            complexity_factors = self._calculate_complexity_factors(query_text, candidate_records, pre)
            quality_factors = self._calculate_quality_factors(query_text, candidate_records, pre)
            all_factors = self._merge_factors(factors, semantic_factors, complexity_factors, quality_factors)
            metrics = self._calculate_final_metrics(all_factors, candidate_records, pre)
            return metrics, all_factors
        except Exception as exc:
            logger.error("comprehensive confidence failed: %s", exc)
            return ConfidenceMetrics(overall_confidence=0.5), ConfidenceFactors()

    def _calculate_base_factors(self, query_text, candidate_records, similarity_factors=None) -> ConfidenceFactors:
        """:215-255"""
        factors = ConfidenceFactors()
        if not candidate_records:
            return factors
        try:
            best_candidate = candidate_records[0]
            if similarity_factors and 'vector_similarity' in similarity_factors:
                factors.vector_similarity = similarity_factors['vector_similarity']
            else:
                factors.vector_similarity = best_candidate.get('score', 0.0)
            if similarity_factors and 'hierarchy_boost' in similarity_factors:
                factors.hierarchy_boost = similarity_factors['hierarchy_boost']
            else:
                factors.hierarchy_boost = self._calculate_hierarchy_score(best_candidate)
            if similarity_factors and 'entity_match_score' in similarity_factors:
                factors.entity_match_score = similarity_factors['entity_match_score']
            else:
                factors.entity_match_score = self._calculate_entity_match(query_text, best_candidate)
            return factors
        except Exception as exc:
            logger.warning("base factors failed: %s", exc)
            return factors

    def _calculate_semantic_factors(self, query_text, candidate_records, pre=None) -> Dict[str, float]:
        """:257-296 (a failure keeps what was computed before it)"""
        semantic_factors = {'semantic_coherence': 0.0, 'context_consistency': 0.0, 'terminology_accuracy': 0.0}
        if not candidate_records:
            return semantic_factors
        try:
            best_candidate = candidate_records[0]
            candidate_text = best_candidate.get('preferred_zh', '')
            if self.embedding_service:
                if pre is not None and 'coherence' in pre:
                    semantic_factors['semantic_coherence'] = pre['coherence']
                else:
                    q = np.asarray(self.embedding_service.encode_query(query_text), dtype=np.float64)
                    c = np.asarray(self.embedding_service.encode_query(candidate_text), dtype=np.float64)
                    semantic_factors['semantic_coherence'] = _cosine(q, c)
            semantic_factors['context_consistency'] = self._calculate_context_consistency(query_text, candidate_text)
            semantic_factors['terminology_accuracy'] = self._calculate_terminology_accuracy(query_text, candidate_text, pre)
            return semantic_factors
        except Exception as exc:
            logger.warning("semantic factors failed: %s", exc)
            return semantic_factors

    def _calculate_complexity_factors(self, query_text, candidate_records, pre=None) -> Dict[str, float]:
        """:298-329"""
        complexity_factors = {'diagnosis_complexity': 0.0, 'professional_specificity': 0.0, 'clinical_relevance': 0.0}
        try:
            complexity_factors['diagnosis_complexity'] = self._assess_diagnosis_complexity(query_text)
            complexity_factors['professional_specificity'] = self._assess_professional_specificity(query_text, pre)
            if candidate_records:
                complexity_factors['clinical_relevance'] = self._assess_clinical_relevance(query_text, candidate_records[0])
            return complexity_factors
        except Exception as exc:
            logger.warning("complexity factors failed: %s", exc)
            return complexity_factors

    def _calculate_quality_factors(self, query_text, candidate_records, pre=None) -> Dict[str, float]:
        """:331-361"""
        quality_factors = {'data_quality': 0.0, 'model_uncertainty': 0.0, 'cross_validation_score': 0.0}
        try:
            quality_factors['data_quality'] = self._assess_data_quality(candidate_records)
            if pre is not None and 'stats' in pre:
                quality_factors['model_uncertainty'] = pre['stats'][4]
            else:
                quality_factors['model_uncertainty'] = self._assess_model_uncertainty(candidate_records)
            quality_factors['cross_validation_score'] = self._calculate_cross_validation(candidate_records)
            return quality_factors
        except Exception as exc:
            logger.warning("quality factors failed: %s", exc)
            return quality_factors

    def _calculate_context_consistency(self, query_text: str, candidate_text: str) -> float:
        """:363-388"""
        try:
            query_words = set(query_text.replace(' ', ''))
            candidate_words = set(candidate_text.replace(' ', ''))
            if not query_words or not candidate_words:
                return 0.0
            intersection = len(query_words & candidate_words)
            union = len(query_words | candidate_words)
            jaccard_score = intersection / union if union > 0 else 0.0
            length_similarity = 1.0 - abs(len(query_text) - len(candidate_text)) / max(len(query_text), len(candidate_text), 1)
            consistency = (jaccard_score * 0.7 + length_similarity * 0.3)
            return min(consistency, 1.0)
        except Exception as exc:
            logger.warning("context consistency failed: %s", exc)
            return 0.5

    def _calculate_terminology_accuracy(self, query_text: str, candidate_text: str, pre=None) -> float:
        """:390-402"""
        try:
            if self.ner_service:
                return self._calculate_terminology_accuracy_with_ner(query_text, candidate_text, pre)
            return self._calculate_terminology_accuracy_fallback(query_text, candidate_text, pre)
        except Exception as exc:
            logger.warning("terminology accuracy failed: %s", exc)
            return 0.5

    def _query_entities(self, query_text, pre):
        if pre is not None and 'query_entities' in pre:
            return pre['query_entities']
        return self.ner_service.extract_medical_entities(query_text)

    def _calculate_terminology_accuracy_with_ner(self, query_text: str, candidate_text: str, pre=None) -> float:
        """:404-439"""
        try:
            query_entities = self._query_entities(query_text, pre)
            if pre is not None and 'candidate_entities' in pre:
                candidate_entities = pre['candidate_entities']
            else:
                candidate_entities = self.ner_service.extract_medical_entities(candidate_text)
            total_weight = 0.0
            matched_weight = 0.0
            for entity_type, entities in query_entities.items():
                type_weight = self._get_entity_type_weight(entity_type)
                for entity in entities:
                    entity_weight = entity['confidence'] * type_weight
                    total_weight += entity_weight
                    if self._entity_matches_in_candidate(entity, candidate_entities):
                        matched_weight += entity_weight
            if total_weight > 0:
                accuracy = matched_weight / total_weight
            else:
                accuracy = self._calculate_char_level_similarity(query_text, candidate_text)
            return min(accuracy, 1.0)
        except Exception as exc:
            logger.warning("terminology accuracy with NER failed: %s", exc)
            return self._calculate_terminology_accuracy_fallback(query_text, candidate_text, pre)

    def _calculate_terminology_accuracy_fallback(self, query_text: str, candidate_text: str, pre=None) -> float:
        """:441-463"""
        try:
            query_terms = self._extract_medical_terms_from_text(query_text, pre)
            candidate_terms = self._extract_medical_terms_from_text(candidate_text, pre)
            if not query_terms:
                return self._calculate_char_level_similarity(query_text, candidate_text)
            total_score = 0.0
            matched_score = 0.0
            for term, weight in query_terms.items():
                total_score += weight
                if term in candidate_terms:
                    matched_score += weight
            return matched_score / total_score if total_score > 0 else 0.5
        except Exception as exc:
            logger.warning("terminology accuracy fallback failed: %s", exc)
            return 0.5

    def _get_entity_type_weight(self, entity_type: str) -> float:
        """:465-476"""
        type_weights = {'disease': 1.0, 'symptom': 0.8, 'anatomy': 0.6, 'pathology': 0.9, 'treatment': 0.5, 'drug': 0.3,
                        'equipment': 0.2}
        return type_weights.get(entity_type, 0.5)

    def _entity_matches_in_candidate(self, query_entity: Dict[str, Any], candidate_entities: Dict[str, List[Dict[str, Any]]]) -> bool:
        """:478-497"""
        query_text = query_entity['text']
        for entity_type, entities in candidate_entities.items():
            for entity in entities:
                candidate_text = entity['text']
                if query_text == candidate_text:
                    return True
                if query_text in candidate_text or candidate_text in query_text:
                    if len(query_text) >= 2 and len(candidate_text) >= 2:
                        return True
        return False

    def _calculate_char_level_similarity(self, text1: str, text2: str) -> float:
        """:499-513"""
        if not text1 or not text2:
            return 0.0
        chars1 = set(text1.replace(' ', ''))
        chars2 = set(text2.replace(' ', ''))
        if not chars1 or not chars2:
            return 0.0
        intersection = len(chars1 & chars2)
        union = len(chars1 | chars2)
        return intersection / union if union > 0 else 0.0

    @staticmethod
    def _terms_in(text: str) -> List[str]:
        """the matches of _extract_medical_terms_from_text's patterns, in the order it visits them (each at most 13 code points)"""
        return [m for pattern in _DISEASE_PATTERNS for m in re.findall(pattern, text)]

    def _extract_medical_terms_from_text(self, text: str, pre=None) -> Dict[str, float]:
        """:515-539"""
        terms = {}
        for match in self._terms_in(text):
            terms[match] = self._calculate_term_weight(match, pre)
        return terms

    def _calculate_term_weight(self, term: str, pre=None) -> float:
        """:541-569"""
        spec = pre.get('spec') if pre is not None else None
        if spec is not None and term in spec:
            icd_weight = spec[term]
        else:
            icd_weight = self._get_term_specificity_from_icd(term)
        if icd_weight > 0.5:
            return icd_weight
        weight = 0.5
        if len(term) >= 6:
            weight += 0.3
        elif len(term) >= 4:
            weight += 0.2
        professional_keywords = ['急性', '慢性', '综合征', '功能不全', '梗死', '出血', '肿瘤', '癌']
        for keyword in professional_keywords:
            if keyword in term:
                weight += 0.2
                break
        if icd_weight != 0.5:
            weight = (weight + icd_weight) / 2
        return min(weight, 1.0)

    # ---- the ICD terminology cache (:571-694) ----------------------------------------------------------------------
    def terminology_path(self) -> str:
        return self.terminology_csv or os.environ.get("ICD_TERMINOLOGY_CSV") or DEFAULT_TERMINOLOGY_CSV

    def _load_icd_terminology_if_needed(self):
        """:571-607: loaded once; a missing file (or a failing load) is retried on the next call"""
        if self.icd_data_loaded:
            return
        try:
            import pandas as pd
            icd_file_path = self.terminology_path()
            if os.path.exists(icd_file_path):
                if icd_file_path.endswith(".xz"):
                    import lzma
                    with lzma.open(icd_file_path, "rb") as fh:
                        df = pd.read_csv(fh)
                else:
                    df = pd.read_csv(icd_file_path)
                for _, row in df.iterrows():
                    code = row.get('code', '')
                    disease = row.get('disease', '')
                    if disease and len(disease.strip()) > 1:
                        level = self._parse_icd_level(code)
                        base_score = self._calculate_icd_base_score(level, disease)
                        category_score = self._calculate_category_score(code)
                        final_score = (base_score + category_score) / 2
                        self.icd_terminology_cache[disease.strip()] = final_score
                self.icd_data_loaded = True
                self._term_keys = self._term_table = None
                logger.info("%d ICD terms in the terminology cache", len(self.icd_terminology_cache))
            else:
                logger.warning("ICD terminology file not found: %s", icd_file_path)
        except Exception as exc:
            logger.warning("loading the ICD terminology failed: %s", exc)

    def _parse_icd_level(self, code: str) -> int:
        """:609-625"""
        if not code:
            return 1
        if '.' not in code:
            return 1
        dot_parts = code.split('.')
        if len(dot_parts) == 2:
            after_dot = dot_parts[1]
            if len(after_dot) == 1:
                return 2
            else:
                return 3
        return 1

    def _calculate_icd_base_score(self, level: int, disease_name: str) -> float:
        """:627-644 (disease_name as the CSV has it, not stripped)"""
        level_scores = {1: 0.6, 2: 0.75, 3: 0.9}
        level_score = level_scores.get(level, 0.6)
        name_complexity = min(len(disease_name) / 15.0, 0.3)
        professional_bonus = 0.0
        professional_terms = ['急性', '慢性', '综合征', '功能不全', '梗死', '出血', '肿瘤', '癌', '病毒', '细菌']
        for term in professional_terms:
            if term in disease_name:
                professional_bonus = 0.1
                break
        return min(level_score + name_complexity + professional_bonus, 1.0)

    def _calculate_category_score(self, code: str) -> float:
        """:646-675"""
        if not code:
            return 0.5
        main_category = code[0].upper()
        category_scores = {'A': 0.8, 'B': 0.8, 'C': 0.95, 'D': 0.9, 'E': 0.85, 'F': 0.8, 'G': 0.9, 'H': 0.75, 'I': 0.9,
                           'J': 0.75, 'K': 0.8, 'L': 0.7, 'M': 0.75, 'N': 0.8, 'O': 0.85, 'P': 0.9, 'Q': 0.85, 'R': 0.6,
                           'S': 0.7, 'T': 0.75, 'Z': 0.5}
        return category_scores.get(main_category, 0.6)

    def _get_term_specificity_from_icd(self, term: str) -> float:
        """:677-694: the exact name, else the first name in cache order that contains the term or that the term contains"""
        self._load_icd_terminology_if_needed()
        if term in self.icd_terminology_cache:
            return self.icd_terminology_cache[term]
        for icd_term, score in self.icd_terminology_cache.items():
            if term in icd_term or icd_term in term:
                if len(term) >= 2 and len(icd_term) >= 2:
                    match_ratio = min(len(term), len(icd_term)) / max(len(term), len(icd_term))
                    return score * match_ratio
        return 0.5

    def _partial_score(self, term: str, index: int) -> float:
        """what _get_term_specificity_from_icd returns when key `index` (cache order) is the first partial match; -1: 0.5"""
        if index < 0:
            return 0.5
        if self._term_keys is None:
            self._term_keys = list(self.icd_terminology_cache.keys())
        icd_term = self._term_keys[index]
        score = self.icd_terminology_cache[icd_term]
        match_ratio = min(len(term), len(icd_term)) / max(len(term), len(icd_term))
        return score * match_ratio

    def term_table(self, device):
        """the cache's keys in scan order as int32 code points + int32 offsets [n_keys + 1], on `device` (made once)"""
        import torch
        self._load_icd_terminology_if_needed()
        if self._term_keys is None:
            self._term_keys = list(self.icd_terminology_cache.keys())
        dev = torch.device(device)
        if self._term_table is None or self._term_table[0] != dev:
            from .._native import pack_strings
            cp, off = pack_strings(self._term_keys)
            self._term_table = (dev, torch.from_numpy(cp).to(dev), torch.from_numpy(off).to(dev))
        return self._term_table

    def term_specificity_batch(self, terms: Sequence[str], device=None) -> Dict[str, float]:
        """_get_term_specificity_from_icd of every term, as a dict. Exact names are dict lookups; the scan of the others runs
        in ONE icd_term_first_match launch on `device` (a GPU), or - device None, or a term longer than
        TERM_MAX_CODEPOINTS - as the reference's loop on the host."""
        self._load_icd_terminology_if_needed()
        cache = self.icd_terminology_cache
        out: Dict[str, float] = {}
        misses = []
        for t in dict.fromkeys(terms):
            if t in cache:
                out[t] = cache[t]
            elif len(t) < 2 or not cache:
                out[t] = 0.5                      # (the scan's condition needs len(term) >= 2)
            else:
                misses.append(t)
        if misses and device is not None:
            on_device = [t for t in misses if len(t) <= TERM_MAX_CODEPOINTS]
            if on_device:
                from .._native import term_first_match
                _dev, key_cp, key_off = self.term_table(device)
                first = term_first_match(key_cp, key_off, on_device)
                for t, i in zip(on_device, first):
                    out[t] = self._partial_score(t, i)
            misses = [t for t in misses if len(t) > TERM_MAX_CODEPOINTS]
        for t in misses:
            out[t] = self._get_term_specificity_from_icd(t)
        return out

    # ---- complexity, specificity, relevance, quality (:696-1019) ---------------------------------------------------
    def _assess_diagnosis_complexity(self, query_text: str) -> float:
        """:696-730"""
        try:
            complexity_score = 0.0
            for pattern in self.complexity_classifier['complex_patterns']:
                if re.search(pattern, query_text):
                    complexity_score += 0.8
            for pattern in self.complexity_classifier['moderate_patterns']:
                if re.search(pattern, query_text):
                    complexity_score += 0.5
            for pattern in self.complexity_classifier['simple_patterns']:
                if re.search(pattern, query_text):
                    complexity_score += 0.2
            length_factor = min(len(query_text) / 50.0, 1.0)
            complexity_score += length_factor * 0.3
            separator_count = query_text.count('，') + query_text.count('；') + query_text.count('伴')
            if separator_count > 0:
                complexity_score += min(separator_count * 0.2, 0.6)
            return min(complexity_score, 1.0)
        except Exception as exc:
            logger.warning("diagnosis complexity failed: %s", exc)
            return 0.5

    def _assess_professional_specificity(self, query_text: str, pre=None) -> float:
        """:732-744"""
        try:
            if self.ner_service:
                return self._assess_professional_specificity_with_ner(query_text, pre)
            return self._assess_professional_specificity_fallback(query_text, pre)
        except Exception as exc:
            logger.warning("professional specificity failed: %s", exc)
            return 0.5

    def _assess_professional_specificity_with_ner(self, query_text: str, pre=None) -> float:
        """:746-781"""
        try:
            entities = self._query_entities(query_text, pre)
            if not any(entities.values()):
                return self._assess_professional_specificity_fallback(query_text, pre)
            total_weight = 0.0
            specificity_sum = 0.0
            for entity_type, entity_list in entities.items():
                type_specificity = self._get_entity_type_specificity(entity_type)
                for entity in entity_list:
                    entity_weight = entity['confidence']
                    content_specificity = self._assess_entity_content_specificity(entity['text'])
                    final_specificity = (type_specificity + content_specificity) / 2
                    total_weight += entity_weight
                    specificity_sum += entity_weight * final_specificity
            if total_weight > 0:
                return min(specificity_sum / total_weight, 1.0)
            return self._assess_professional_specificity_fallback(query_text, pre)
        except Exception as exc:
            logger.warning("professional specificity with NER failed: %s", exc)
            return self._assess_professional_specificity_fallback(query_text, pre)

    def _assess_professional_specificity_fallback(self, query_text: str, pre=None) -> float:
        """:783-807"""
        try:
            terms = self._extract_medical_terms_from_text(query_text, pre)
            if not terms:
                if any(keyword in query_text for keyword in ['急性', '慢性', '并发', '综合征']):
                    return 0.6
                elif any(keyword in query_text for keyword in ['病', '症', '炎']):
                    return 0.4
                else:
                    return 0.2
            total_weight = sum(terms.values())
            if total_weight > 0:
                return min(total_weight / len(terms), 1.0)
            return 0.5
        except Exception as exc:
            logger.warning("professional specificity fallback failed: %s", exc)
            return 0.5

    def _get_entity_type_specificity(self, entity_type: str) -> float:
        """:809-820"""
        type_specificity = {'disease': 0.9, 'pathology': 0.85, 'symptom': 0.6, 'anatomy': 0.5, 'treatment': 0.8, 'drug': 0.7,
                            'equipment': 0.4}
        return type_specificity.get(entity_type, 0.5)

    def _assess_entity_content_specificity(self, entity_text: str) -> float:
        """:822-853"""
        specificity = 0.5
        if len(entity_text) >= 6:
            specificity += 0.2
        elif len(entity_text) >= 4:
            specificity += 0.1
        professional_prefixes = ['急性', '慢性', '原发性', '继发性', '复发性']
        professional_suffixes = ['综合征', '功能不全', '功能障碍', '梗死', '出血', '肿瘤', '癌症']
        for prefix in professional_prefixes:
            if entity_text.startswith(prefix):
                specificity += 0.15
                break
        for suffix in professional_suffixes:
            if entity_text.endswith(suffix):
                specificity += 0.15
                break
        complex_terms = ['酸中毒', '综合征', '功能不全', '动脉硬化', '心肌梗死']
        for term in complex_terms:
            if term in entity_text:
                specificity += 0.1
                break
        return min(specificity, 1.0)

    def _assess_clinical_relevance(self, query_text: str, candidate: Dict[str, Any]) -> float:
        """:855-896"""
        try:
            relevance_score = 0.0
            code = candidate.get('code', '')
            level = candidate.get('level', 1)
            if level == 3:
                relevance_score += 0.4
            elif level == 2:
                relevance_score += 0.3
            else:
                relevance_score += 0.2
            if code:
                main_category = code[0]
                category_relevance = {'I': 0.9, 'C': 0.9, 'E': 0.8, 'J': 0.7, 'K': 0.7, 'N': 0.7, 'S': 0.6}.get(main_category, 0.5)
                relevance_score += category_relevance * 0.4
            candidate_text = candidate.get('preferred_zh', '')
            context_match = self._calculate_context_consistency(query_text, candidate_text)
            relevance_score += context_match * 0.2
            return min(relevance_score, 1.0)
        except Exception as exc:
            logger.warning("clinical relevance failed: %s", exc)
            return 0.5

    def _assess_data_quality(self, candidate_records: List[Dict[str, Any]]) -> float:
        """:898-934"""
        try:
            if not candidate_records:
                return 0.0
            quality_score = 0.0
            complete_records = 0
            for record in candidate_records:
                if record.get('code') and record.get('preferred_zh') and record.get('score', 0) > 0:
                    complete_records += 1
            completeness = complete_records / len(candidate_records)
            quality_score += completeness * 0.4
            scores = [r.get('score', 0) for r in candidate_records]
            if scores:
                max_score = max(scores)
                min_score = min(scores)
                score_range = max_score - min_score
                if score_range > 0.1:
                    quality_score += 0.3
                if max_score > 0.7:
                    quality_score += 0.3
            return min(quality_score, 1.0)
        except Exception as exc:
            logger.warning("data quality failed: %s", exc)
            return 0.5

    def _assess_model_uncertainty(self, candidate_records: List[Dict[str, Any]]) -> float:
        """:936-963"""
        try:
            if not candidate_records:
                return 0.0
            scores = [r.get("score", 0) for r in candidate_records]
            if not scores:
                return 0.0
            std_score = float(np.std(scores))
            uncertainty_score = 1.0 - min(std_score, 0.5) / 0.5
            score_confidence = max(scores)
            final_uncertainty = (uncertainty_score * 0.6 + score_confidence * 0.4)
            return min(final_uncertainty, 1.0)
        except Exception as exc:
            logger.warning("model uncertainty failed: %s", exc)
            return 0.5

    def _calculate_cross_validation(self, candidate_records: List[Dict[str, Any]]) -> float:
        """:965-991"""
        try:
            if len(candidate_records) < 2:
                return 0.5
            top_scores = [r.get('score', 0) for r in candidate_records[:min(3, len(candidate_records))]]
            if not top_scores:
                return 0.0
            max_score = max(top_scores)
            min_score = min(top_scores)
            if max_score > 0.8 and (max_score - min_score) > 0.2:
                return 0.8
            elif max_score > 0.6 and (max_score - min_score) > 0.1:
                return 0.6
            else:
                return 0.4
        except Exception as exc:
            logger.warning("cross validation failed: %s", exc)
            return 0.5

    def _calculate_hierarchy_score(self, candidate: Dict[str, Any]) -> float:
        """:993-1001"""
        try:
            level = candidate.get('level', 1)
            level_scores = {1: 0.6, 2: 0.8, 3: 1.0}
            return level_scores.get(level, 0.5)
        except Exception:
            return 0.5

    def _calculate_entity_match(self, query_text: str, candidate: Dict[str, Any]) -> float:
        """:1003-1019"""
        try:
            candidate_text = candidate.get('preferred_zh', '')
            query_chars = set(query_text)
            candidate_chars = set(candidate_text)
            if not query_chars or not candidate_chars:
                return 0.0
            overlap = len(query_chars & candidate_chars)
            union = len(query_chars | candidate_chars)
            return overlap / union if union > 0 else 0.0
        except Exception:
            return 0.0

    # ---- merge and final metrics (:1021-1157) ----------------------------------------------------------------------
    def _merge_factors(self, *factor_dicts) -> ConfidenceFactors:
        """:1021-1036 (setattr: the values are not coerced again)"""
        factors = ConfidenceFactors()
        for factor_dict in factor_dicts:
            if isinstance(factor_dict, dict):
                for key, value in factor_dict.items():
                    if hasattr(factors, key):
                        setattr(factors, key, value)
            elif isinstance(factor_dict, ConfidenceFactors):
                for field in ['vector_similarity', 'hierarchy_boost', 'entity_match_score']:
                    if hasattr(factor_dict, field):
                        setattr(factors, field, getattr(factor_dict, field))
        return factors

    def _calculate_final_metrics(self, factors: ConfidenceFactors, candidate_records: List[Dict[str, Any]],
                                 pre=None) -> ConfidenceMetrics:
        """:1038-1085"""
        try:
            overall_confidence = 0.0
            factor_dict = {
                'vector_similarity': factors.vector_similarity,
                'hierarchy_boost': factors.hierarchy_boost,
                'entity_match_score': factors.entity_match_score,
                'semantic_coherence': factors.semantic_coherence,
                'context_consistency': factors.context_consistency,
                'terminology_accuracy': factors.terminology_accuracy,
                'diagnosis_complexity': factors.diagnosis_complexity,
                'professional_specificity': factors.professional_specificity,
                'clinical_relevance': factors.clinical_relevance,
                'data_quality': factors.data_quality,
                'model_uncertainty': factors.model_uncertainty,
                'cross_validation_score': factors.cross_validation_score,
            }
            for factor_name, factor_value in factor_dict.items():
                weight = self.factor_weights.get(factor_name, 0.0)
                overall_confidence += factor_value * weight
            if pre is not None and 'stats' in pre:
                variance = pre['stats'][5]
            else:
                variance = self._calculate_prediction_variance(factors, candidate_records)
            confidence_interval = self._calculate_confidence_interval(overall_confidence, variance)
            reliability_score = self._calculate_reliability_score(factors)
            calibration_score = self._calculate_calibration_score(overall_confidence, factors)
            return ConfidenceMetrics(overall_confidence=min(overall_confidence, 1.0), confidence_interval=confidence_interval,
                                     reliability_score=reliability_score, prediction_variance=variance,
                                     calibration_score=calibration_score)
        except Exception as exc:
            logger.error("final metrics failed: %s", exc)
            return ConfidenceMetrics(overall_confidence=0.5)

    def _calculate_prediction_variance(self, factors, candidate_records: List[Dict[str, Any]]) -> float:
        """:1087-1099"""
        try:
            scores = [r.get("score", 0) for r in candidate_records]
            if len(scores) > 1:
                return float(np.var(scores))
            return 0.1
        except Exception:
            return 0.1

    def _calculate_confidence_interval(self, confidence: float, variance: float) -> Tuple[float, float]:
        """:1101-1114"""
        try:
            margin = 1.96 * float(np.sqrt(variance))
            return (max(0.0, confidence - margin), min(1.0, confidence + margin))
        except Exception:
            return (max(0.0, confidence - 0.1), min(1.0, confidence + 0.1))

    def _calculate_reliability_score(self, factors: ConfidenceFactors) -> float:
        """:1116-1137"""
        try:
            key_factors = [factors.vector_similarity, factors.entity_match_score, factors.semantic_coherence,
                           factors.terminology_accuracy]
            if key_factors:
                std_factor = float(np.std(key_factors))
                return 1.0 - min(std_factor, 0.5) / 0.5
            return 0.5
        except Exception:
            return 0.5

    def _calculate_calibration_score(self, confidence: float, factors: ConfidenceFactors) -> float:
        """:1139-1157"""
        try:
            factor_values = [factors.vector_similarity, factors.semantic_coherence, factors.terminology_accuracy]
            if factor_values:
                avg_factor = float(np.mean(factor_values))
                calibration = 1.0 - abs(confidence - avg_factor)
                return max(calibration, 0.0)
            return 0.5
        except Exception:
            return 0.5

    # ---- levels and explanations (:1159-1258) ----------------------------------------------------------------------
    def get_confidence_level(self, confidence: float) -> str:
        if confidence >= self.confidence_thresholds['high_confidence']:
            return "高置信度"
        elif confidence >= self.confidence_thresholds['medium_confidence']:
            return "中等置信度"
        elif confidence >= self.confidence_thresholds['low_confidence']:
            return "低置信度"
        else:
            return "极低置信度"

    def should_reject_prediction(self, confidence: float) -> bool:
        return confidence < self.confidence_thresholds['reject_threshold']

    def adjust_thresholds(self, new_thresholds: Dict[str, float]):
        for threshold_name, value in new_thresholds.items():
            if threshold_name in self.confidence_thresholds:
                self.confidence_thresholds[threshold_name] = value
                logger.info("threshold %s = %s", threshold_name, value)

    def get_confidence_explanation(self, metrics: ConfidenceMetrics, factors: ConfidenceFactors) -> Dict[str, Any]:
        explanation = {
            'overall_confidence': metrics.overall_confidence,
            'confidence_level': self.get_confidence_level(metrics.overall_confidence),
            'confidence_interval': metrics.confidence_interval,
            'reliability_score': metrics.reliability_score,
            'should_reject': self.should_reject_prediction(metrics.overall_confidence),
            'factor_contributions': {},
            'top_contributing_factors': [],
            'improvement_suggestions': [],
        }
        factor_dict = {
            '向量相似度': factors.vector_similarity,
            '层级增强': factors.hierarchy_boost,
            '实体匹配': factors.entity_match_score,
            '语义一致性': factors.semantic_coherence,
            '上下文一致性': factors.context_consistency,
            '术语准确性': factors.terminology_accuracy,
            '诊断复杂度': factors.diagnosis_complexity,
            '专业特异性': factors.professional_specificity,
            '临床相关性': factors.clinical_relevance,
            '数据质量': factors.data_quality,
            '模型不确定性': factors.model_uncertainty,
            '交叉验证': factors.cross_validation_score,
        }
        weight_mapping = {
            '向量相似度': 'vector_similarity',
            '层级增强': 'hierarchy_boost',
            '实体匹配': 'entity_match_score',
            '语义一致性': 'semantic_coherence',
            '上下文一致性': 'context_consistency',
            '术语准确性': 'terminology_accuracy',
            '诊断复杂度': 'diagnosis_complexity',
            '专业特异性': 'professional_specificity',
            '临床相关性': 'clinical_relevance',
            '数据质量': 'data_quality',
            '模型不确定性': 'model_uncertainty',
            '交叉验证': 'cross_validation_score',
        }
        for factor_name_zh, factor_value in factor_dict.items():
            weight = self.factor_weights.get(weight_mapping[factor_name_zh], 0.0)
            explanation['factor_contributions'][factor_name_zh] = {'value': factor_value, 'weight': weight,
                                                                   'contribution': factor_value * weight}
        sorted_contributions = sorted(explanation['factor_contributions'].items(), key=lambda x: x[1]['contribution'], reverse=True)
        explanation['top_contributing_factors'] = [f"{name}: {info['contribution']:.4f}" for name, info in sorted_contributions[:3]]
        if metrics.overall_confidence < 0.6:
            explanation['improvement_suggestions'] = ["考虑补充更多医学术语信息", "检查查询文本的完整性和准确性", "增加上下文信息以提高匹配精度"]
        return explanation

    # ---- row N3 pieces, per call ------------------------------------------------------------------------------------
    def semantic_coherence(self, query_text: str, candidate_records: List[Dict[str, Any]]) -> float:
        """The 'semantic_coherence' entry of _calculate_semantic_factors (:257-296): 0.0 without candidates, without an
        embedding service, or when anything fails."""
        if not candidate_records or not self.embedding_service:
            return 0.0
        try:
            candidate_text = candidate_records[0].get("preferred_zh", "")
            q = np.asarray(self.embedding_service.encode_query(query_text), dtype=np.float64)
            c = np.asarray(self.embedding_service.encode_query(candidate_text), dtype=np.float64)
            return float(_cosine(q, c))
        except Exception as exc:
            logger.warning("semantic factors failed: %s", exc)
            return 0.0

    # ---- whole batch, on the device ------------------------------------------------------------------------------
    def score_statistics_batch(self, scores, order=None, top_k: Optional[int] = None):
        """scores f64 [nq, k] (device): every query's candidate scores in result order; order (i32 [nq, k], optional):
        entries below 0 mark hits that do not exist; top_k: the statistics run over each query's first top_k hits, like
        the reference's candidates[:top_k]. Returns f64 [nq, 6] (STAT_COLUMNS), bit-identical to the per-call methods."""
        from .._native import score_stats
        return score_stats(scores, order, top_k)

    def semantic_coherence_batch(self, query_vectors, candidate_texts: Optional[Sequence[str]] = None):
        """query_vectors f32 [nq, dim] (device, as encode_query_batch(..., to_device=True) returns them).
        candidate_texts None: the live /query shape, every query against encode_query('') (see the module docstring);
        else one text per query (the best candidates' 'preferred_zh'), embedded in ONE encoder batch. Returns f64 [nq]."""
        from .._native import cosine_rows
        if self.embedding_service is None:
            import torch
            return torch.zeros((query_vectors.shape[0],), dtype=torch.float64, device=query_vectors.device)
        if candidate_texts is None:
            if self._empty_vector is None or self._empty_vector.device != query_vectors.device:
                self._empty_vector = self.embedding_service.encode_query_batch([""], to_device=True)[0].to(query_vectors.device)
            return cosine_rows(query_vectors, self._empty_vector)
        assert len(candidate_texts) == query_vectors.shape[0]
        cand = self.embedding_service.encode_query_batch(list(candidate_texts), to_device=True).to(query_vectors.device)
        return cosine_rows(query_vectors, cand)

    def comprehensive_confidence_batch(self, queries: Sequence[str], candidate_records: Sequence[List[Dict[str, Any]]],
                                       similarity_factors: Sequence[Optional[Dict]], query_vectors=None, entities=None,
                                       stats=None) -> List[Tuple[ConfidenceMetrics, ConfidenceFactors]]:
        """calculate_comprehensive_confidence(queries[i], candidate_records[i], similarity_factors[i]) for every i, with the
        parts that are batch work done once for the batch:
          - semantic coherence: icd_cosine_rows of query_vectors (f32 [nq, dim] on a GPU; encode_query of every query) against
            encode_query(best candidate's 'preferred_zh') - the empty string's vector for live records. Equal to sklearn's
            cosine to ~1e-14, not bit for bit; without query_vectors the per-call cosine.
          - model uncertainty and prediction variance: `stats` (icd_score_stats rows [nq][6] over the records' scores), or
            one icd_score_stats launch here when query_vectors are on a GPU.
          - term specificity: term_specificity_batch over the terms whose weights can reach a factor (one launch).
          - NER: `entities` (entities[i]: extract_medical_entities(queries[i]), the filter_drugs=True call the rescoring
            makes) and the entities of the empty candidate text, extracted once per service.
        Returns one (ConfidenceMetrics, ConfidenceFactors) per query."""
        nq = len(queries)
        assert len(candidate_records) == nq and len(similarity_factors) == nq
        if entities is not None:
            assert len(entities) == nq
        pres: List[Dict[str, Any]] = [{} for _ in range(nq)]
        device = None
        import torch
        if query_vectors is not None and torch.is_tensor(query_vectors) and query_vectors.is_cuda:
            device = query_vectors.device
        # --- cosine
        if self.embedding_service and query_vectors is not None and any(candidate_records):
            texts = [r[0].get('preferred_zh', '') if r else '' for r in candidate_records]
            if device is not None:
                coh = self.semantic_coherence_batch(query_vectors, None if not any(texts) else texts).tolist()
            else:
                coh = None
            if coh is not None:
                for i in range(nq):
                    pres[i]['coherence'] = coh[i]
        # --- score statistics
        if stats is None and device is not None and nq:
            kmax = max((len(r) for r in candidate_records), default=0)
            if 0 < kmax <= 128:
                sc = np.zeros((nq, kmax), np.float64)
                order = np.full((nq, kmax), -1, np.int32)
                ok = True
                for i, recs in enumerate(candidate_records):
                    for j, r in enumerate(recs):
                        s = r.get('score', 0)
                        if not isinstance(s, (float, int)) or isinstance(s, bool):
                            ok = False
                        sc[i, j] = s
                        order[i, j] = j
                if ok:
                    stats = self.score_statistics_batch(torch.from_numpy(sc).to(device), torch.from_numpy(order).to(device),
                                                        top_k=kmax).tolist()
        if stats is not None:
            for i in range(nq):
                pres[i]['stats'] = stats[i]
        # --- NER
        if self.ner_service is not None and entities is not None:
            if self._empty_entities is None:
                self._empty_entities = self.ner_service.extract_medical_entities('')
            for i in range(nq):
                pres[i]['query_entities'] = entities[i] if entities[i] is not None else {}
                texts_c = candidate_records[i][0].get('preferred_zh', '') if candidate_records[i] else ''
                if texts_c == '':
                    pres[i]['candidate_entities'] = self._empty_entities
        # --- term specificity: the weights reach professional_specificity (no NER service, or no entities) and
        # terminology_accuracy (no NER service) - there only through matched / total, which is 0.0 when the candidate text has
        # no terms (every weight is positive), so those queries' terms need no lookup for it
        need = []
        for i, q in enumerate(queries):
            if self.ner_service is None:
                need.append(q)
                if candidate_records[i]:   # (an offline record's text: its terms decide what matches)
                    need.append(candidate_records[i][0].get('preferred_zh', ''))
            else:
                ents = pres[i].get('query_entities')
                if ents is None or not any(ents.values()):
                    need.append(q)
        terms = [t for q in need if isinstance(q, str) for t in self._terms_in(q)]
        if terms:
            spec = self.term_specificity_batch(terms, device=device)
            for p in pres:
                p['spec'] = spec
        return [self.calculate_comprehensive_confidence(q, recs, sf, pre=p)
                for q, recs, sf, p in zip(queries, candidate_records, similarity_factors, pres)]


def _cosine(x: np.ndarray, y: np.ndarray) -> float:
    """sklearn.metrics.pairwise.cosine_similarity of two rows: each divided by its Euclidean norm (a zero row is left
    alone), then the dot product, in float64."""
    nx = float(np.sqrt(np.einsum("i,i->", x, x)))
    ny = float(np.sqrt(np.einsum("i,i->", y, y)))
    xn = x / (nx if nx != 0.0 else 1.0)
    yn = y / (ny if ny != 0.0 else 1.0)
    return float(np.dot(xn, yn))
