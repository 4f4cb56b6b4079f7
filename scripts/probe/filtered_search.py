#!/usr/bin/env python3
"""Filtered search on one MI355X: what a Milvus `filter` costs.

The store holds the 40 474 records of the real ICD-10 CSV (tests/golden/ICD_10v601.csv.xz) with random unit vectors (no model
weights offline: the synthetic encoder embeds the queries). Timed:
  * the build of a view for `code like "C%"` (1 850 rows), `level >= 2` (35 443) and `code like "E11%"` (154): the selection on
    the host, then icd_index_create_view (gather kernel + fp16 image + workspace + probe);
  * a search of 1 and of 10 000 queries at k = 10 against the whole corpus and against each view - the view cached, and the
    first call of an expression (selection + view build + search);
  * /query (MultiDiagnosisService + the FastAPI handler) with and without a filter.
Medians of wall-clock times (host calls: the time a caller sees). Prints a report; `> profiles/filtered_search_probe.log`.
"""
import lzma
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

EXPRS = ['code like "C%"', "level >= 2", 'code like "E11%"']


def med(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def main():
    import torch
    os.environ.setdefault("EMBEDDING_MODEL_NAME", "shibing624/text2vec-base-chinese")
    os.environ.setdefault("ICD_EMBEDDING_ALLOW_SYNTHETIC", "1")
    tmp = tempfile.mkdtemp(prefix="icd_filter_")
    os.environ["MILVUS_DB_PATH"] = os.path.join(tmp, "db")
    os.environ["MILVUS_COLLECTION_NAME"] = "icd10_filter_probe"
    csv = os.path.join(tmp, "ICD_10v601.csv")
    with open(csv, "wb") as f:
        f.write(lzma.open(os.path.join(ROOT, "tests", "golden", "ICD_10v601.csv.xz")).read())
    from rag_project_icd10_amd.services.embedding_service import EmbeddingService
    from rag_project_icd10_amd.services.milvus_service import MilvusService
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    from rag_project_icd10_amd.tools.build_database import DatabaseBuilder
    recs = DatabaseBuilder.__new__(DatabaseBuilder).load_csv_data(csv)
    n, dim, k = len(recs), 768, 10
    es = EmbeddingService()
    ms = MilvusService(embedding_service=es)
    rng = np.random.default_rng(77)
    corpus = rng.standard_normal((n, dim), dtype=np.float32)
    corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
    assert ms.insert_records(recs, list(corpus)) and ms.load_collection()
    index = ms._ready_index()
    print(f"corpus: {n} rows x {dim} (records of the ICD-10 CSV, random unit vectors); device {torch.cuda.get_device_name(0)}")
    q1 = corpus[rng.integers(0, n, 1)] + 0.1 * rng.standard_normal((1, dim), dtype=np.float32)
    qb = corpus[rng.integers(0, n, 10000)] + 0.1 * rng.standard_normal((10000, dim), dtype=np.float32)
    q1, qb = np.ascontiguousarray(q1, np.float32), np.ascontiguousarray(qb, np.float32)
    dqb = torch.from_numpy(qb).cuda()

    def dev_batch(idx):
        idx.search_reweighted(dqb, k)
        torch.cuda.synchronize()

    for _ in range(5):
        index.search_reweighted(q1, k)
        dev_batch(index)
    base1 = med(lambda: index.search_reweighted(q1, k), 200)
    baseb = med(lambda: dev_batch(index), 30)
    print(f"\nunfiltered: 1 query {base1:.3f} ms (host in/out), 10 000 queries {baseb:.3f} ms (device in/out), k = {k}")

    from rag_project_icd10_amd.services import filter_expr
    t0 = time.perf_counter()
    cols = ms._filter_columns()
    print(f"\nfilter columns of the store (once per store generation): {(time.perf_counter() - t0) * 1e3:.1f} ms")
    print("\nview builds (the expression evaluated over the columns uncached, then icd_index_create_view; first call = a fresh")
    print("expression through MilvusService.search_batch: selection + view + one query; medians of 3)")
    print(f"{'expression':<22}{'rows':>8}{'share':>8}{'select ms':>11}{'create ms':>11}{'first 1q ms':>13}{'1q ms':>9}"
          f"{'10k ms':>9}{'10k / unfiltered':>18}{'HBM MB':>9}")
    for expr in EXPRS:
        t_sel, t_create, t_first = [], [], []
        for rep in range(3):
            ms._clear_views()
            cols._sel.clear()
            t0 = time.perf_counter()
            rows = filter_expr.select(expr, cols)
            t1 = time.perf_counter()
            view = index.view(rows)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            t_sel.append((t1 - t0) * 1e3)
            t_create.append((t2 - t1) * 1e3)
            view.close()
            ms._clear_views()
            cols._sel.clear()
            t0 = time.perf_counter()
            ms.search_batch(q1, k, filter=expr)   # first call: selection + view + search
            t_first.append((time.perf_counter() - t0) * 1e3)
        view, _rows = ms._filtered_index(expr)
        for _ in range(5):
            view.search_reweighted(q1, k)
            dev_batch(view)
        v1 = med(lambda: ms.search_batch(q1, k, filter=expr), 200)
        vb = med(lambda: dev_batch(view), 30)
        st = view.stats()
        mb = (st["bytes_corpus_f32"] + st["bytes_corpus_f16"] + st["bytes_workspace"]) / 2 ** 20
        print(f"{expr:<22}{len(rows):>8}{len(rows) / n:>8.3f}{statistics.median(t_sel):>11.2f}{statistics.median(t_create):>11.2f}"
              f"{statistics.median(t_first):>13.2f}{v1:>9.3f}{vb:>9.3f}{vb / baseb:>18.3f}{mb:>9.1f}")

    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    appmod.install_services(es, ms, MultiDiagnosisService(es, ms))
    text = "2型糖尿病伴有肾的并发症，高血压，肺恶性肿瘤"
    print(f"\n/query latency (delimiter extraction, no NER; text {text!r}, top_k 5, median of 50)")
    with TestClient(appmod.app) as client:
        for flt in (None, 'code like "E11%"', "level >= 2", 'code like "C%" or code like "E%"'):
            body = {"text": text, "top_k": 5}
            if flt is not None:
                body["filter"] = flt
            for _ in range(5):
                assert client.post("/query", json=body).status_code == 200
            t = med(lambda: client.post("/query", json=body), 50)
            print(f"  filter {flt!s:<34} {t:8.3f} ms")
    appmod.install_services(None, None, None)
    ms.disconnect()


if __name__ == "__main__":
    main()
