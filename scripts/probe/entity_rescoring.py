#!/usr/bin/env python3
"""Rescoring of queries WITH NER entities on one MI355X: host (_match_from_hits per string: batch_calculate_similarities on
hit dicts) against the device (match_diagnoses_batch(..., entities=): query_params_entities + icd_hier_rescore_entities),
synthetic encoder / NER weights, 40 474-row corpus with codes of every chapter letter.
  1. the 1 000 golden strings with the synthetic-weight NER's entities, top_k = 5 (search k = 10): ms per 1 000 strings of
     the host rescoring, of the search + dict marshalling it needs, and of search + rescoring + winners on the device
     (checked equal, DiagnosisMatch by DiagnosisMatch)
  2. /query latency with NER on (match_multiple_diagnoses), 1 / 3 / 8 diagnoses per request: the old routing (host
     rescoring, forced by supports_device_rescoring = False) and the new one (device), alternated request by request."""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault("EMBEDDING_MODEL_NAME", "shibing624/text2vec-base-chinese")
os.environ.setdefault("ICD_EMBEDDING_ALLOW_SYNTHETIC", "1")
os.environ.setdefault("ICD_NER_ALLOW_SYNTHETIC", "1")
os.environ.setdefault("MEDICAL_NER_MODEL", "/nonexistent/ner")
tmp = tempfile.mkdtemp(prefix="icd_ent_")
os.environ["MILVUS_DB_PATH"] = os.path.join(tmp, "db")
os.environ["MILVUS_COLLECTION_NAME"] = "icd10_ent"


def _median(x):
    x = sorted(x)
    return x[len(x) // 2]


def main():
    import torch
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
    ner = MedicalNERService()
    print(f"NER: synthetic weights {ner.synthetic}, classifier on {getattr(ner.ner_pipeline, 'device', 'cpu')}")
    md = MultiDiagnosisService(es, ms, ner_service=ner)

    # ---- 1. 1 000 strings, host against device rescoring ----
    ents = ner.extract_medical_entities_batch(strings, filter_drugs=True)
    with_ents = sum(1 for e in ents if any(e.values()))
    vecs = es.encode_query_batch(strings, to_device=True)
    torch.cuda.synchronize()
    t_search, t_host, t_dev = [], [], []
    for rep in range(5):
        t0 = time.perf_counter()
        hit_lists = ms.search_batch(vecs, 2 * top_k, as_dicts=True)
        t1 = time.perf_counter()
        host = [md._match_from_hits(d, h, top_k, e) for d, h, e in zip(strings, hit_lists, ents)]
        t2 = time.perf_counter()
        dev = md.match_diagnoses_batch(strings, top_k=top_k, vectors=vecs, entities=ents)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if rep == 0:
            assert [m.model_dump() for m in dev] == [m.model_dump() for m in host], "device and host rescoring differ"
            ca = sum(1 for m in dev for c in m.candidates if c.similarity_factors.category_alignment > 0)
        else:
            t_search.append((t1 - t0) * 1e3)
            t_host.append((t2 - t1) * 1e3)
            t_dev.append((t3 - t2) * 1e3)
    print(f"1 000 golden strings, top_k {top_k}, {with_ents} with entities, {ca} winners with a category alignment; "
          f"equal DiagnosisMatch objects on both paths")
    print(f"  host rescoring (_match_from_hits per string): median {_median(t_host):.1f} ms")
    print(f"  search(2k) + dict marshalling for it:        median {_median(t_search):.1f} ms")
    print(f"  device: search(2k) + rescoring + winners:    median {_median(t_dev):.1f} ms")

    # ---- 2. /query latency with NER on, old routing against new, alternated ----
    md_new = MultiDiagnosisService(es, ms, ner_service=ner)
    md_old = MultiDiagnosisService(es, ms, ner_service=ner)

    def old(text):
        ms.supports_device_rescoring = lambda: False
        try:
            return md_old.match_multiple_diagnoses(text, top_k=top_k)
        finally:
            del ms.supports_device_rescoring

    for nd in (1, 3, 8):
        texts = ["，".join(strings[i * nd:(i + 1) * nd]) for i in range(40)]
        for t in texts[:5]:
            old(t)
            md_new.match_multiple_diagnoses(t, top_k=top_k)
        torch.cuda.synchronize()
        lat_old, lat_new = [], []
        for t in texts:
            t0 = time.perf_counter()
            a = old(t)
            t1 = time.perf_counter()
            b = md_new.match_multiple_diagnoses(t, top_k=top_k)
            t2 = time.perf_counter()
            assert [m.model_dump() for m in a["matches"]] == [m.model_dump() for m in b["matches"]], t
            lat_old.append((t1 - t0) * 1e3)
            lat_new.append((t2 - t1) * 1e3)
        lat_old.sort()
        lat_new.sort()
        print(f"/query NER on, {nd} diagnoses per request ({len(b['extracted_diagnoses'])} extracted): "
              f"old routing median {_median(lat_old):.2f} ms p90 {lat_old[int(len(lat_old) * 0.9)]:.2f} ms, "
              f"new routing median {_median(lat_new):.2f} ms p90 {lat_new[int(len(lat_new) * 0.9)]:.2f} ms")


if __name__ == "__main__":
    main()
