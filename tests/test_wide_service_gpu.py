"""services/wide_search.py: WideSearch.search_wide / search_wide_batch over a MilvusService on the golden CSV
slice's store, with the test encoder weights the neighbouring service tests use: against `search` at top_k = 10, against
tests/wide_oracle.py over the CPU oracle's full ranking at top_k = 1 000 with and without a filter, against the existing paged
`search(offset=..)`, the totals against `count`, and the API route. Exact: every comparison is of equal values, no tolerance."""
import os

import numpy as np
import pytest

import wide_oracle as wo

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILTERS = ['level >= 2 and code like "A0%"', 'parent_code != "" and (level in [2] or secondary_code like "G%")',
           'level >= 2 and TEXT_MATCH(preferred_zh, "伤寒")']
NQ = 6


@pytest.fixture(scope="module")
def services(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("MILVUS_DB_PATH", str(tmp_path_factory.mktemp("db")))
    mp.setenv("MILVUS_COLLECTION_NAME", "icd10_wide")
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
    """the stored vectors, a fixed query batch and the oracle's full ranking of it: computed once"""
    ms = services["ms"]
    corpus = np.ascontiguousarray(ms.client.matrix(), np.float32)
    levels = np.asarray(ms.client.levels(), np.int32)
    n = len(corpus)
    assert 100 <= n <= 300
    rng = np.random.default_rng(12)
    queries = np.ascontiguousarray(corpus[rng.integers(0, n, NQ)] + 0.05 * rng.standard_normal((NQ, corpus.shape[1])).astype(np.float32))
    fs, fi = oracle.flat_ip_topk(corpus, queries, n)
    keep = {e: np.isin(np.arange(n), ms.filter_rows(e)) for e in FILTERS}
    assert all(0 < keep[e].sum() < n for e in FILTERS)
    return {"levels": levels, "n": n, "queries": queries, "fs": fs, "fi": fi, "keep": keep}


def wide_of(services):
    from rag_project_icd10_amd.services.wide_search import WideSearch
    return WideSearch(services["ms"])


def test_top_k_10_equals_search(services, world):
    ms, wide = services["ms"], wide_of(services)
    for q in world["queries"]:
        assert wide.search_wide(q, 10) == ms.search(q, top_k=10)
        for e in FILTERS:
            got = wide.search_wide(q, 10, filter=e)
            assert got == ms.search(q, top_k=10, filter=e, filter_mode="mask") and len(got) > 0


def test_top_k_1000_against_the_oracle(services, world):
    wide = wide_of(services)
    w = world
    for filters in (None, FILTERS[0], [FILTERS[1], None, FILTERS[2], FILTERS[0], None, FILTERS[1]]):
        per = [filters] * NQ if not isinstance(filters, list) else filters
        masks = None if filters is None else [None if e is None else w["keep"][e] for e in per]
        want = wo.wide_batch(w["fs"], w["fi"], w["levels"], 1000, 0, masks)
        got, totals = wide.search_wide_batch(w["queries"], 1000, filter=filters, with_totals=True)
        for g, x in zip(got, want[1]):
            assert g.dtype == x.dtype and g.tobytes() == x.tobytes(), filters
        assert totals.tobytes() == want[3].tobytes()
        lists = wide.search_wide_batch(w["queries"], 1000, filter=filters, as_dicts=True)
        assert [len(x) for x in lists] == want[2].tolist() and all(len(x) == t for x, t in zip(lists, totals))


def test_offsets_equal_the_paged_search(services, world):
    ms, wide = services["ms"], wide_of(services)
    q = world["queries"][0]
    for offset, top_k in ((900, 100), (100, 100), (150, 100), (0, 100)):          # the existing route is the yardstick (its lists end at the store's max_k = 100)
        for e in (None, FILTERS[1]):
            kw = {} if e is None else {"filter": e, "filter_mode": "mask"}
            assert wide.search_wide(q, top_k, filter=e, offset=offset) == ms.search(q, top_k=top_k, offset=offset, **kw), (offset, top_k, e)
    assert wide.search_wide(q, 100, offset=900) == [] and len(wide.search_wide(q, 100, offset=100)) == 100
    lo = float(world["fs"][0][60])
    assert wide.search_wide(q, 100, radius=lo) == ms.search(q, top_k=100, radius=lo) and 0 < len(wide.search_wide(q, 100, radius=lo)) < 61


def test_totals_equal_count(services, world):
    ms, wide = services["ms"], wide_of(services)
    _out, totals = wide.search_wide_batch(world["queries"][:4], 500, filter=FILTERS + [None], with_totals=True)
    assert totals.tolist() == [ms.count(e) for e in FILTERS] + [world["n"]]


def test_endpoint(services, world):
    # (last of the module: the app's lifespan disconnects the installed services when the client closes)
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    ms, es = services["ms"], services["es"]
    wide = wide_of(services)
    appmod.install_services(es, ms, MultiDiagnosisService(es, ms))
    try:
        with TestClient(appmod.app) as client:
            text = ms.client.records[17]["preferred_zh"]
            vec = np.asarray(es.encode_query(text), np.float32)
            for body, kw in (({"text": text, "top_k": 1000}, {}), ({"text": text, "top_k": 200, "filter": FILTERS[2], "offset": 3}, {"filter": FILTERS[2], "offset": 3})):
                r = client.post("/wide_query", json=body)
                assert r.status_code == 200, r.text
                lists, totals = wide.search_wide_batch(vec.reshape(1, -1), body["top_k"], as_dicts=True, with_totals=True, **kw)
                assert r.json() == {"candidates": lists[0], "total": int(totals[0])} and len(lists[0]) > 0
            assert client.post("/wide_query", json={"text": text, "top_k": 16385}).status_code == 400
            assert client.post("/wide_query", json={"text": text, "filter": "level =="}).status_code == 400
    finally:
        appmod.install_services(None, None, None)
