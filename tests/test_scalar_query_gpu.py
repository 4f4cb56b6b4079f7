"""MilvusService's scalar queries (query, count(*), get, query_batch, query_iterator) on the golden CSV slice's
store, against the host route's row lists (MilvusService.filter_rows): the ids of every window, the totals, the fields of every
row, with the filters' masks made on the device and on the host, and the two routes of the API. Integer output: no tolerance."""
import os

import numpy as np
import pytest

from rag_project_icd10_amd.services import filter_expr as fe

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (test_filter_device_gpu.py's expressions: or / not nesting, like, in, TEXT_MATCH under every shape, one a program refuses)
SCALAR = [
    'code like "A0%"', 'level >= 2 and code like "A01%"', 'code like "A00%" or code like "A02%"', 'not code like "A0%"',
    "code like '%.9' and level == 2", 'preferred_zh like "%伤寒%" or level == 1', 'code in ["A00", "A01.0", "nope"] or level < 2',
    'code not in ["A00"] and has_complication == false', 'not (level == 1 or (code like "A01%" and not has_complication == true))',
    'parent_code != "" and (level in [2] or secondary_code like "G%")', "level > -1", "level in []", 'main_code == "A01.0" or code like "A00"',
]
TEXTUAL = [
    'level == 1 or TEXT_MATCH(preferred_zh, "伤寒")', 'not TEXT_MATCH(preferred_zh, "霍乱")',
    'TEXT_MATCH(preferred_zh, "伤寒") and not TEXT_MATCH(preferred_zh, "副伤寒", minimum_should_match=3)',
    'TEXT_MATCH(preferred_zh, "霍乱") or TEXT_MATCH(preferred_zh, "结核")', 'code like "A0%" and (level >= 3 or TEXT_MATCH(preferred_zh, "zzzz 感染"))',
    'TEXT_MATCH(preferred_zh, "结核")', 'level >= 2 and TEXT_MATCH(preferred_zh, "伤寒")',
]
HOST_ONLY = [" or ".join(f"level == {i}" for i in range(17))]   # (17 leaves: device_program refuses it)
EXPRESSIONS = SCALAR + TEXTUAL + HOST_ONLY
FIELDS = ("code", "preferred_zh", "has_complication", "main_code", "secondary_code", "level", "parent_code", "category_path", "semantic_text")


@pytest.fixture(scope="module")
def services(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("MILVUS_DB_PATH", str(tmp_path_factory.mktemp("db")))
    mp.setenv("MILVUS_COLLECTION_NAME", "icd10_scalar_query")
    mp.setenv("EMBEDDING_MODEL_NAME", "shibing624/text2vec-base-chinese")
    mp.setenv("ICD_EMBEDDING_ALLOW_SYNTHETIC", "1")
    from rag_project_icd10_amd.tools.build_database import DatabaseBuilder
    b = DatabaseBuilder()
    b.initialize_services()
    recs = b.load_csv_data(os.path.join(GOLDEN, "csv_slice.csv"))
    assert b.vectorize_and_index(recs) is True
    yield {"ms": b.milvus_service, "es": b.embedding_service}
    b.milvus_service.disconnect()
    mp.undo()


@pytest.fixture(scope="module")
def want(services):
    """expression -> the host route's rows, computed once"""
    ms = services["ms"]
    rows = {e: ms.filter_rows(e) for e in EXPRESSIONS}
    n = ms.client.count
    sizes = [len(r) for r in rows.values()]
    assert len(EXPRESSIONS) >= 20 and 0 in sizes and n in sizes and any(0 < s < n for s in sizes)
    return rows


def ids_of(rows):
    return [r["id"] for r in rows]


def check_routes(ms, want):
    n = ms.client.count
    recs = ms.client.records
    for e in EXPRESSIONS:
        rows = want[e]
        for limit, offset in ((5, 0), (3, 2), (1, max(len(rows) - 1, 0)), (1000, len(rows)), (16384, 0), (7, 16377)):
            got = ms.query(e, limit=limit, offset=offset)
            assert ids_of(got) == rows[offset:offset + limit].tolist(), (e, limit, offset)
            for r in got:   # the fields of every returned row
                assert set(r) == set(FIELDS) | {"id"} and all(r[f] == recs[r["id"]].get(f) for f in FIELDS), (e, r)
        assert ms.count(e) == len(rows) and ms.query(e, output_fields=["count(*)"]) == [{"count(*)": len(rows)}], e
        assert ids_of(ms.query(e)) == rows.tolist(), e                                   # limit=None: all of it
    assert ms.count() == n and ids_of(ms.query("", limit=4, offset=n - 2)) == [n - 2, n - 1]
    v = ms.query(EXPRESSIONS[0], limit=2, output_fields=["vector", "code"])
    assert [r["vector"] for r in v] == [ms.client.matrix()[i].tolist() for i in want[EXPRESSIONS[0]][:2]]


def test_query_count_and_windows_equal_the_host_rows(services, want):
    ms = services["ms"]
    assert ms.FILTER_ON_DEVICE and ms.TEXT_MATCH_ON_DEVICE
    ms._clear_views()
    check_routes(ms, want)
    assert ms.get([3, 10 ** 9, 0, -1]) == ms.query(ids=[3, 0]) and ids_of(ms.get([3, 10 ** 9, 0, -1])) == [3, 0]


def test_the_same_with_the_masks_made_on_the_host(services, want):
    ms = services["ms"]
    ms._clear_views()
    ms.FILTER_ON_DEVICE = ms.TEXT_MATCH_ON_DEVICE = False
    try:
        check_routes(ms, want)
    finally:
        del ms.FILTER_ON_DEVICE, ms.TEXT_MATCH_ON_DEVICE
        ms._clear_views()
    assert ms.FILTER_ON_DEVICE and ms.TEXT_MATCH_ON_DEVICE


def test_a_batch_is_one_masks_call_and_one_select(services, want):
    ms = services["ms"]
    index = ms._ready_index()
    ms._clear_views()
    filters = EXPRESSIONS + ["", None, EXPRESSIONS[0], EXPRESSIONS[14]]
    offsets = [(3 * i) % 7 for i in range(len(filters))]
    calls = {"filter_masks": [], "select_rows": [], "count_rows": []}
    real_filter, real_select, real_count = index.filter_masks, index.select_rows, index.count_rows
    index.filter_masks = lambda *a, **k: (calls["filter_masks"].append(len(a[2]) - 1), real_filter(*a, **k))[1]
    index.select_rows = lambda *a, **k: (calls["select_rows"].append(len(a[0])), real_select(*a, **k))[1]
    index.count_rows = lambda *a, **k: (calls["count_rows"].append(len(a[0])), real_count(*a, **k))[1]
    try:
        lists, totals = ms.query_batch(filters, 6, offsets, with_totals=True)
        # ONE filter_masks launch for every device program of the batch (the refused expression went to the host), ONE select
        assert calls == {"filter_masks": [len(SCALAR) + len(TEXTUAL)], "select_rows": [len(filters)], "count_rows": []}
        counted = ms.count_batch(filters)
        assert calls["select_rows"] == [len(filters)] and calls["count_rows"] == [len(filters)]
    finally:
        del index.filter_masks, index.select_rows, index.count_rows
    n = ms.client.count
    rows = [want[f] if f else np.arange(n) for f in filters]
    assert [ids_of(l) for l in lists] == [r[o:o + 6].tolist() for r, o in zip(rows, offsets)]
    assert totals == counted == [len(r) for r in rows]
    assert lists == [ms.query(f or "", limit=6, offset=o) for f, o in zip(filters, offsets)]   # ... equals one query per expression
    assert ms.query_batch(filters[:3], 2, 1) == [ms.query(f, limit=2, offset=1) for f in filters[:3]]
    # the search's own masks (a TEXT_MATCH made on the device) were closed behind the select; the scalar ones are cached
    cached = {f["expression"] for f in ms.filter_masks()}
    assert not any("TEXT_MATCH" in k for k in cached) and fe.compile(SCALAR[0]) in cached


def test_iterator_pages_concatenate_and_it_raises_after_an_insert(services, want):
    ms, es = services["ms"], services["es"]
    for e in (SCALAR[0], SCALAR[3], TEXTUAL[1], TEXTUAL[5], HOST_ONLY[0], "level in []", ""):
        rows = want[e].tolist() if e else list(range(ms.client.count))
        for batch in (1, 7, 16384):
            if batch == 1 and len(rows) > 60:
                continue
            it = ms.query_iterator(batch_size=batch, filter=e, output_fields=["code"])
            got = []
            while True:
                page = it.next()
                if not page:
                    break
                assert len(page) <= batch
                got += ids_of(page)
            it.close()
            assert got == rows, (e, batch)
        it = ms.query_iterator(batch_size=4, limit=6, filter=e)
        assert ids_of(it.next() + it.next() + it.next()) == rows[:6], e
        it.close()
    live = [ms.query_iterator(batch_size=2, filter=e) for e in (SCALAR[0], TEXTUAL[5], "")]
    firsts = [ids_of(it.next()) for it in live]
    assert firsts == [want[SCALAR[0]][:2].tolist(), want[TEXTUAL[5]][:2].tolist(), [0, 1]]
    rec = dict(ms.client.records[0], code="Z99.9")
    assert ms.insert_records([rec], [np.asarray(es.encode_query("新增记录"), np.float32)]) is True
    for it in live:
        with pytest.raises(RuntimeError):
            it.next()
        it.close()
    # the store moved on: the new row is found by a fresh query
    assert ids_of(ms.query('code == "Z99.9"', limit=3)) == [ms.client.count - 1] and ms.count() == ms.client.count


def test_endpoints(services):
    # (last of the module: the app's lifespan disconnects the installed services when the client closes)
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    ms, es = services["ms"], services["es"]
    recs = ms.client.records
    appmod.install_services(es, ms, MultiDiagnosisService(es, ms))
    try:
        with TestClient(appmod.app) as client:
            for e in (SCALAR[1], TEXTUAL[0], HOST_ONLY[0], "level in []", ""):
                rows = ms.filter_rows(e).tolist() if e else list(range(ms.client.count))
                r = client.post("/codes/query", json={"filter": e, "limit": 4, "offset": 1})
                assert r.status_code == 200, r.text
                body = r.json()
                assert body["total"] == len(rows) and [x["id"] for x in body["rows"]] == rows[1:5], e
                assert all(x["code"] == recs[x["id"]]["code"] and x["preferred_zh"] == recs[x["id"]]["preferred_zh"] for x in body["rows"])
                c = client.post("/codes/query", json={"filter": e, "count": True}).json()
                assert c == {"total": len(rows), "rows": []}, e
            d = client.post("/codes/query", json={"filter": SCALAR[0]}).json()               # the defaults: 100 rows from 0
            assert [x["id"] for x in d["rows"]] == ms.filter_rows(SCALAR[0])[:100].tolist()
            f = client.post("/codes/query", json={"filter": SCALAR[0], "limit": 2, "output_fields": ["code"]}).json()
            assert all(set(x) == {"code", "id"} for x in f["rows"]) and len(f["rows"]) == 2
            for bad in ({"filter": "level =="}, {"limit": 0}, {"limit": 1001}, {"offset": -1}, {"limit": 1000, "offset": 16000}, {"output_fields": ["nope"]}):
                assert client.post("/codes/query", json=bad).status_code == 400, bad
            code = recs[5]["code"]
            g = client.get(f"/codes/{code}")
            assert g.status_code == 200 and g.json()["code"] == code and g.json()["id"] == ms.filter_rows(f'code == "{code}"')[0]
            assert g.json()["preferred_zh"] == recs[g.json()["id"]]["preferred_zh"]
            assert client.get("/codes/NOPE.0").status_code == 404 and client.get('/codes/A"0').status_code == 400
    finally:
        appmod.install_services(None, None, None)
