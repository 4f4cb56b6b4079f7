#!/usr/bin/env python3
"""Golden fixture of the reference's 12-factor confidence service, produced by RUNNING THE REFERENCE'S OWN
services/multidimensional_confidence_service.py (unchanged, imported from /root/reference) on its own data/ICD_10v601.csv:

    python tests/golden/make_multidim_confidence_golden.py

Functions run: calculate_comprehensive_confidence (:158-213, every factor method it reaches), get_confidence_level,
should_reject_prediction, get_confidence_explanation (:1159-1258) and _get_term_specificity_from_icd (:677-694).

Only loguru is replaced (absent here; a no-op logger). The embedding service is a table of seeded unit vectors (16 wide:
the cosine is what is pinned, not the encoder); the NER service is a table of seeded entity dicts (text -> entities; {} for
texts outside it), so the with-NER cases need no classifier. Queries: the 1 000 golden diagnosis strings and hand-picked ones
(no terms, several terms, a duplicated CSV name as the exact hit and as the first partial hit, a term that contains a name, a
term with no hit, the complexity patterns). Records: the live shape (code / title / score / level, no 'preferred_zh') and
the offline one (with 'preferred_zh'), with 0, 1, 2 and k candidates; similarity_factors given and None; with and without NER.

Only DATA is written: multidim_confidence_cases.json.xz and multidim_confidence_vectors.npz. No case lies within 1e-9 of a
confidence threshold (asserted), so a 1e-12 difference in the cosine cannot change a level.
"""
import json
import lzma
import os
import re
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
DIM = 16
THRESHOLDS = (0.80, 0.60, 0.40, 0.20)
PATTERNS = (r'[^，。；\s]{2,10}病', r'[^，。；\s]{2,10}症', r'[^，。；\s]{2,10}炎', r'[^，。；\s]{2,10}综合征',
            r'急性[^，。；\s]{2,10}', r'慢性[^，。；\s]{2,10}')
ENTITY_TYPES = ("disease", "symptom", "anatomy", "pathology", "treatment", "drug", "equipment", "other")


def stub_modules():
    class _Logger:
        def __getattr__(self, name):
            return lambda *a, **k: None
    loguru = types.ModuleType("loguru")
    loguru.logger = _Logger()
    sys.modules["loguru"] = loguru


class TableEmbedding:
    def __init__(self, table):
        self.table = table

    def encode_query(self, text):
        return self.table[text].tolist()


class TableNER:
    def __init__(self, table):
        self.table = table

    def extract_medical_entities(self, text, filter_drugs=True):
        return json.loads(json.dumps(self.table.get(text, {})))


def terms_of(text):
    return [m for p in PATTERNS for m in re.findall(p, text)]


def seeded_entities(rng, text):
    """entity dicts drawn from the text's own substrings; some all-empty, some with no entities at all"""
    kind = rng.integers(0, 5)
    if kind == 0 or len(text) < 2:
        return {}
    if kind == 1:
        return {"disease": [], "symptom": []}
    out = {}
    for _ in range(int(rng.integers(1, 4))):
        a = int(rng.integers(0, max(1, len(text) - 1)))
        b = min(len(text), a + int(rng.integers(1, 7)))
        t = ENTITY_TYPES[int(rng.integers(0, len(ENTITY_TYPES)))]
        out.setdefault(t, []).append({"text": text[a:b], "confidence": float(rng.uniform(0.3, 1.0)), "start": a, "end": b})
    return out


def main():
    stub_modules()
    sys.path.insert(0, REF)
    from services.multidimensional_confidence_service import MultiDimensionalConfidenceService

    golden = [l.strip() for l in open(os.path.join(HERE, "diagnosis_strings.txt"), encoding="utf-8") if l.strip()]
    assert len(golden) == 1000
    plain = MultiDimensionalConfidenceService()
    plain._load_icd_terminology_if_needed()
    cache = plain.icd_terminology_cache
    keys = list(cache)

    def first_hit(term):
        for i, k in enumerate(keys):
            if (term in k or k in term) and len(term) >= 2 and len(k) >= 2:
                return i
        return -1

    # duplicated names of the CSV (a name at two codes: the dict keeps the first position and the last score)
    import pandas as pd
    df = pd.read_csv(os.path.join(REF, "data", "ICD_10v601.csv"))
    seen, dups = set(), []
    for d in df["disease"]:
        s = d.strip()
        if len(s) > 1:
            if s in seen and s not in dups:
                dups.append(s)
            seen.add(s)
    dup_set = set(dups)
    exact_dup = [k for k in dups if terms_of(k) == [k]][:4]
    partial_dup = []
    for k in dups:
        for t in ("慢性" + k[:-1] if len(k) > 2 else None, k[:-1] + "病"):
            if t and len(t) <= 12 and t not in cache and terms_of(t) and terms_of(t)[0] == t:
                i = first_hit(t)
                if i >= 0 and keys[i] in dup_set:
                    partial_dup.append(t)
        if len(partial_dup) >= 4:
            break
    contains_key = [k + "并发症" for k in exact_dup[:2]]
    hand = (["头晕", "", "发热三天", "急性胰腺炎伴糖尿病酮症酸中毒，慢性肾功能不全综合征", "龘龘龘病", "慢性龘龘龘"]
            + exact_dup + partial_dup + contains_key
            + ["高血压病伴冠状动脉粥样硬化性心脏病伴心力衰竭", "2型糖尿病并发糖尿病肾病", "严重的糖尿病性酮症酸中毒",
               "多发性骨髓瘤", "多发性硬化症", "腰痛", "胃肠炎", "急性上呼吸道感染", "急性心肌梗死伴心律失常",
               "慢性阻塞性肺疾病急性加重，肺部感染；呼吸衰竭", "肺炎伴胸腔积液并发呼吸衰竭"])
    assert len(exact_dup) >= 2 and len(partial_dup) >= 2, (exact_dup, partial_dup)
    queries = golden + hand

    rng = np.random.default_rng(20261016)
    letters = "ABCDEGIJKNRSZQX"
    cases_in = []
    for i, q in enumerate(queries):
        n = [0, 1, 2, 5, 10, 3][i % 6] if i < 1000 else [0, 1, 2, 10][i % 4]
        offline = i % 3 == 0
        scores = np.sort(rng.uniform(0.0, 1.3, n))[::-1]
        recs = []
        for j in range(n):
            L = letters[int(rng.integers(0, len(letters)))]
            tail = ["", ".9", f".{int(rng.integers(0, 9))}", f".{int(rng.integers(0, 9))}{int(rng.integers(10, 99))}"][int(rng.integers(0, 4))]
            rec = {"code": f"{L}{int(rng.integers(0, 99)):02d}{tail}", "title": "", "score": float(scores[j]), "level": 1 + tail.count(".") + (len(tail) > 2)}
            if offline:
                # an offline record names a disease: the query itself, another golden string, or a CSV name
                pick = int(rng.integers(0, 3))
                rec["preferred_zh"] = q if pick == 0 else (golden[int(rng.integers(0, 1000))] if pick == 1 else keys[int(rng.integers(0, len(keys)))])
                rec["title"] = rec["preferred_zh"]
            recs.append(rec)
        sf = None
        if i % 2 == 0 and n:
            sf = {"vector_similarity": float(rng.uniform(0.3, 1.0)), "hierarchy_boost": float(rng.uniform(0.0, 1.0)),
                  "entity_match_score": float(rng.uniform(0.0, 1.0)) if i % 4 == 0 else 0.0}
        cases_in.append((q, recs, sf))

    texts = sorted({q for q, _, _ in cases_in} | {r["preferred_zh"] for _, recs, _ in cases_in for r in recs if "preferred_zh" in r} | {""})
    erng = np.random.default_rng(77)
    base = erng.standard_normal(DIM).astype(np.float32)
    table = {}
    for t in texts:
        v = (0.8 * base + erng.standard_normal(DIM).astype(np.float32)).astype(np.float32)
        v /= np.linalg.norm(v)
        table[t] = v.astype(np.float32)
    nrng = np.random.default_rng(99)
    ner_table = {t: seeded_entities(nrng, t) for t in texts if t}
    ner_table = {t: e for t, e in ner_table.items() if e}
    emb = TableEmbedding(table)
    svc = {False: MultiDimensionalConfidenceService(embedding_service=emb),
           True: MultiDimensionalConfidenceService(embedding_service=emb, ner_service=TableNER(ner_table))}

    cases, near = [], []
    for idx, (q, recs, sf) in enumerate(cases_in):
        for with_ner in (False, True):
            s = svc[with_ner]
            metrics, factors = s.calculate_comprehensive_confidence(q, [dict(r) for r in recs], dict(sf) if sf else None)
            oc = float(metrics.overall_confidence)
            if any(abs(oc - th) < 1e-9 for th in THRESHOLDS):
                near.append((q, with_ner, oc))
            case = {"query": q, "records": recs, "similarity_factors": sf, "ner": with_ner,
                    "factors": {k: float(v) for k, v in vars(factors).items()},
                    "metrics": {"overall_confidence": oc, "confidence_interval": [float(x) for x in metrics.confidence_interval],
                                "reliability_score": float(metrics.reliability_score),
                                "prediction_variance": float(metrics.prediction_variance),
                                "calibration_score": float(metrics.calibration_score)},
                    "level": s.get_confidence_level(oc), "reject": bool(s.should_reject_prediction(oc))}
            if idx % 25 == 0 or idx >= 1000:
                case["explanation"] = json.loads(json.dumps(s.get_confidence_explanation(metrics, factors), ensure_ascii=False))
            cases.append(case)
    assert not near, near

    all_terms = sorted({t for q in texts for t in terms_of(q)})
    spec = {t: float(plain._get_term_specificity_from_icd(t)) for t in all_terms}
    first = {t: first_hit(t) for t in all_terms}
    out = {"cases": cases, "ner_table": ner_table, "term_specificity": spec, "term_first_hit": first,
           "hand_picked": {"exact_duplicate": exact_dup, "partial_duplicate": partial_dup, "contains_key": contains_key},
           "n_keys": len(keys), "numpy": np.__version__}
    with lzma.open(os.path.join(HERE, "multidim_confidence_cases.json.xz"), "wt", encoding="utf-8", preset=9) as f:
        json.dump(out, f, ensure_ascii=False)
    np.savez_compressed(os.path.join(HERE, "multidim_confidence_vectors.npz"),
                        vectors=np.stack([table[t] for t in texts]), texts=np.array(texts))
    print(f"{len(cases)} cases, {len(all_terms)} terms, {len(texts)} texts; duplicated names as exact hits {exact_dup}, "
          f"as first partial hits {partial_dup}")


if __name__ == "__main__":
    main()
