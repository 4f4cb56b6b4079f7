#!/usr/bin/env python3
"""The 12-factor match confidence on one MI355X: match_diagnoses_batch over the 1 000 golden strings with confidence off
("match") and on ("multidimensional"), without NER and with the rules NER, against the per-call host path
(_match_from_hits in the multidimensional mode, string by string); synthetic encoder weights, a 40 474-row corpus, top_k = 5,
the reference's CSV (tests/golden/ICD_10v601.csv.xz) as the terminology cache.
Run it under `rocprofv3 --kernel-trace --stats -- python scripts/probe/multidim_confidence.py --reps 1` for the time of
icd_term_first_match (term_first_match_kernel) and its launch count: one per confidence-on batch."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault("EMBEDDING_MODEL_NAME", "shibing624/text2vec-base-chinese")
os.environ.setdefault("ICD_EMBEDDING_ALLOW_SYNTHETIC", "1")
os.environ.setdefault("ICD_TERMINOLOGY_CSV", os.path.join(ROOT, "tests", "golden", "ICD_10v601.csv.xz"))
tmp = tempfile.mkdtemp(prefix="icd_conf_")
os.environ["MILVUS_DB_PATH"] = os.path.join(tmp, "db")
os.environ["MILVUS_COLLECTION_NAME"] = "icd10_conf"


def _median(x):
    x = sorted(x)
    return x[len(x) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    from rag_project_icd10_amd import _native
    from rag_project_icd10_amd.services.embedding_service import EmbeddingService
    from rag_project_icd10_amd.services.medical_ner_service import MedicalNERService
    from rag_project_icd10_amd.services.milvus_service import MilvusService
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    n, dim, top_k = 40474, 768, 5
    letters = "ABCEIJKNSZQ"
    es = EmbeddingService()
    ms = MilvusService(embedding_service=es)
    rng = np.random.default_rng(1234)
    corpus = rng.standard_normal((n, dim), dtype=np.float32)
    corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
    for s in range(0, n, 4096):
        recs = [{"code": f"{letters[i % 11]}{i % 100:02d}.{i % 10}{i:05d}", "preferred_zh": f"合成疾病{i}", "level": 1 + i % 3,
                 "parent_code": "", "category_path": "", "semantic_text": f"合成疾病{i}"} for i in range(s, min(n, s + 4096))]
        assert ms.insert_records(recs, list(corpus[s:s + 4096]))
    assert ms.load_collection() and ms.supports_device_rescoring()
    strings = [l.strip() for l in open(os.path.join(ROOT, "tests", "golden", "diagnosis_strings.txt"), encoding="utf-8") if l.strip()]
    launches = []
    inner = _native.term_first_match
    _native.term_first_match = lambda *a: launches.append(len(a[2])) or inner(*a)
    print(f"{len(strings)} golden strings, top_k {top_k}, {n} rows; medians of {args.reps} batches after one warm-up")
    for ner_name in ("no NER", "rules NER"):
        ner = MedicalNERService(use_model=False) if ner_name == "rules NER" else None
        ents = ner.extract_medical_entities_batch(strings, filter_drugs=True) if ner else None
        md = MultiDiagnosisService(es, ms, ner_service=ner, confidence="multidimensional")
        md.confidence_service._load_icd_terminology_if_needed()
        vecs = es.encode_query_batch(strings, to_device=True)
        row = {}
        for mode in ("match", "multidimensional"):
            md.match_diagnoses_batch(strings, top_k=top_k, vectors=vecs, entities=ents, confidence=mode)   # warm-up (+ table upload)
            torch.cuda.synchronize()
            before = len(launches)
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                out = md.match_diagnoses_batch(strings, top_k=top_k, vectors=vecs, entities=ents, confidence=mode)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            row[mode] = (_median(times), (len(launches) - before) / args.reps, sum(launches[before:]) // max(1, len(launches) - before))
        with_ents = sum(1 for e in ents if any(e.values())) if ents else 0
        levels = {}
        for m in out:
            levels[m.confidence_level] = levels.get(m.confidence_level, 0) + 1
        print(f"{ner_name} ({with_ents} strings with entities): match_diagnoses_batch confidence off {row['match'][0]:.1f} ms, "
              f"on {row['multidimensional'][0]:.1f} ms; term_first_match launches per confidence-on batch "
              f"{row['multidimensional'][1]:.0f} ({row['multidimensional'][2]} terms); levels {levels}")
        # the per-call host path for the same strings: search + host rescoring + calculate_comprehensive_confidence per string
        hv = es.encode_query_batch(strings)
        t0 = time.perf_counter()
        for i, s in enumerate(strings):
            md._match_from_hits(s, ms.search(hv[i], top_k=2 * top_k), top_k, ents[i] if ents else None)
        host = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        for i, s in enumerate(strings):
            ms.search(hv[i], top_k=2 * top_k)
        search = (time.perf_counter() - t0) * 1e3
        print(f"{ner_name}: per-call host path (search + rescoring + confidence per string) {host:.0f} ms, of which the "
              f"one-query searches {search:.0f} ms")


if __name__ == "__main__":
    main()
