"""services/recommend.py: Recommend.recommend / recommend_batch over a MilvusService on the golden CSV slice's
store, with the test encoder weights the neighbouring service tests use: codes, texts and ids as examples, a filter, `offset`, all
against tests/recommend_oracle.py over the CPU oracle's canonical scores, and the API route. Exact: every comparison is of equal
values, no tolerance."""
import os

import numpy as np
import pytest

import recommend_oracle as ro

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILTERS = ['level >= 2 and code like "A0%"', 'parent_code != "" and (level in [2] or secondary_code like "G%")']


@pytest.fixture(scope="module")
def services(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("MILVUS_DB_PATH", str(tmp_path_factory.mktemp("db")))
    mp.setenv("MILVUS_COLLECTION_NAME", "icd10_recommend")
    mp.setenv("EMBEDDING_MODEL_NAME", "shibing624/text2vec-base-chinese")
    mp.setenv("ICD_EMBEDDING_ALLOW_SYNTHETIC", "1")
    from rag_project_icd10_amd.tools.build_database import DatabaseBuilder
    b = DatabaseBuilder()
    b.initialize_services()
    recs = b.load_csv_data(os.path.join(GOLDEN, "csv_slice.csv"))[:300]
    assert b.vectorize_and_index(recs) is True
    yield {"ms": b.milvus_service, "es": b.embedding_service}
    b.milvus_service.disconnect()
    mp.undo()


@pytest.fixture(scope="module")
def world(services, oracle):
    """the stored vectors, two texts and their vectors, and the oracle's scores by row on demand: computed once"""
    ms, es = services["ms"], services["es"]
    corpus = np.ascontiguousarray(ms.client.matrix(), np.float32)
    levels = np.asarray(ms.client.levels(), np.int32)
    n = len(corpus)
    assert 100 <= n <= 300
    texts = ["发热伴腹泻三天", "反复咳嗽"]
    assert all(ms._row_of_code(t) is None for t in texts)
    vecs = np.ascontiguousarray(np.asarray(es.encode_query_batch(texts), np.float32).reshape(2, -1))
    keep = {e: np.isin(np.arange(n), ms.filter_rows(e)) for e in FILTERS}
    assert all(0 < keep[e].sum() < n for e in FILTERS)
    cache = {}

    def scores(vector, x):
        key = np.asarray(vector, np.float32).tobytes()
        if key not in cache:
            cache[key] = oracle.scores(np.asarray(vector, np.float32), x)
        return cache[key]
    codes = [ms.client.records[r]["code"] for r in (17, 40, 99)]
    rows = [int(ms._row_of_code(c)) for c in codes]                              # (the first row that carries the code)
    assert len(set(rows)) == 3
    return {"corpus": corpus, "levels": levels, "n": n, "texts": texts, "vecs": vecs, "keep": keep, "scores": scores, "codes": codes, "rows": rows}


def rec_of(services):
    from rag_project_icd10_amd.services.recommend import Recommend
    return Recommend(services["ms"])


def want(w, positive, negative, strategy, k, first=0, masks=None, radius=None):
    return ro.recommend_batch(w["corpus"], w["levels"], positive, negative, strategy, k, first, masks, radius, None, 0, w["scores"])


def test_codes_texts_and_ids_against_the_oracle(services, world):
    rec, w = rec_of(services), world
    # the same three requests as the service takes them and as the oracle does: a code is its row, a text its vector
    positive = [[w["codes"][0], w["texts"][0], 5], [w["codes"][1]], [w["texts"][1], w["vecs"][0]]]
    negative = [[w["codes"][2], w["texts"][1]], [], [7, w["codes"][0]]]
    r0, r1, r2 = w["rows"]
    o_pos = [[r0, w["vecs"][0], 5], [r1], [w["vecs"][1], w["vecs"][0]]]
    o_neg = [[r2, w["vecs"][1]], [], [7, r0]]
    for strategy in ro.STRATEGIES:
        for filters in (None, FILTERS[0], [FILTERS[1], None, FILTERS[0]]):
            per = [filters] * 3 if not isinstance(filters, list) else filters
            masks = None if filters is None else [None if e is None else w["keep"][e] for e in per]
            x = want(w, o_pos, o_neg, strategy, 1000, 0, masks)
            got, totals = rec.recommend_batch(positive, negative, strategy, 1000, filter=filters, as_dicts=False, with_totals=True)
            for g, y in zip(got, x[1]):
                assert g.dtype == y.dtype and g.tobytes() == y.tobytes(), (strategy, filters)
            assert totals.tobytes() == x[3].tobytes()
            lists = rec.recommend_batch(positive, negative, strategy, 1000, filter=filters)
            assert [len(h) for h in lists] == x[2].tolist()
            for hits, ids, pos, neg in zip(lists, x[1][2], o_pos, o_neg):            # `search`-shaped; a stored example is never a hit
                assert [h["code"] for h in hits[:5]] == [services["ms"].client.records[i]["code"] for i in ids[:5]]
                assert not {i for i in pos + neg if isinstance(i, int)} & set(ids[ids >= 0].tolist())


def test_offset_and_radius_against_the_oracle(services, world):
    rec, w = rec_of(services), world
    pos, neg = [w["codes"][0], w["codes"][1]], [w["texts"][0]]
    o_pos, o_neg = [[w["rows"][0], w["rows"][1]]], [[w["vecs"][0]]]
    for offset, top_k in ((0, 10), (7, 20), (150, 100), (290, 50)):
        x = want(w, o_pos, o_neg, "sum_scores", top_k, offset)
        got = rec.recommend_batch([pos], [neg], "sum_scores", top_k, offset=offset, as_dicts=False)
        for g, y in zip(got, x[1]):
            assert g.tobytes() == y.tobytes(), (offset, top_k)
        hits = rec.recommend(pos, neg, "sum_scores", top_k, offset=offset)
        assert len(hits) == int(x[2][0]) and [h["original_score"] for h in hits] == [float(v) for v in x[1][1][0][:len(hits)]]
    lo = float(want(w, o_pos, o_neg, "best_score", 200)[0][0][0][100])
    x = want(w, o_pos, o_neg, "best_score", 100, 0, [w["keep"][FILTERS[1]]], lo)
    hits = rec.recommend(pos, neg, "best_score", 100, filter=FILTERS[1], radius=lo)
    assert len(hits) == int(x[2][0]) and 0 < len(hits) < 101 and [h["original_score"] for h in hits] == [float(v) for v in x[1][1][0][:len(hits)]]


def test_endpoint(services, world):
    # (last of the module: the app's lifespan disconnects the installed services when the client closes)
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    ms, es = services["ms"], services["es"]
    rec, w = rec_of(services), world
    appmod.install_services(es, ms, MultiDiagnosisService(es, ms))
    try:
        with TestClient(appmod.app) as client:
            for body in ({"positive": [w["codes"][0], w["texts"][0]], "negative": [w["codes"][2]], "strategy": "best_score", "top_k": 1000},
                         {"positive": [17, w["vecs"][1].tolist()], "negative": [], "strategy": "average_vector", "top_k": 50, "filter": FILTERS[1], "offset": 3},
                         {"positive": [w["codes"][1]], "negative": [w["texts"][1]], "strategy": "sum_scores", "top_k": 20, "radius": 0.0}):
                r = client.post("/recommend", json=body)
                assert r.status_code == 200, r.text
                kw = {key: body[key] for key in ("filter", "offset", "radius") if key in body}
                lists, totals = rec.recommend_batch([body["positive"]], [body["negative"]], body["strategy"], body["top_k"], with_totals=True, **kw)
                assert r.json() == {"candidates": lists[0], "total": int(totals[0])} and len(lists[0]) > 0
            assert client.post("/recommend", json={"positive": [w["codes"][0]], "top_k": 16385}).status_code == 400
            assert client.post("/recommend", json={"positive": [w["codes"][0]], "filter": "level =="}).status_code == 400
            assert client.post("/recommend", json={"negative": [w["codes"][0]]}).status_code == 400
            assert client.post("/recommend", json={"positive": [10 ** 6]}).status_code == 404
    finally:
        appmod.install_services(None, None, None)
