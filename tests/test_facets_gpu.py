"""MilvusService.facet / facet_batch on the golden CSV slice's store: every facet list against the rows
MilvusService.query returns for the same filter, counted in Python; the filters' masks made on the device and on the host; a batch as
one masks call and one count; the API route. Integer output: no tolerance."""
import os
from collections import Counter

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("level", "has_complication", "category", "parent_code", "code")
# (no filter, three of test_filter_device_gpu.py's expressions, one TEXT_MATCH)
FILTERS = ["", 'level >= 2 and code like "A01%"', 'not (level == 1 or (code like "A01%" and not has_complication == true))',
           'parent_code != "" and (level in [2] or secondary_code like "G%")', 'level >= 2 and TEXT_MATCH(preferred_zh, "伤寒")']


@pytest.fixture(scope="module")
def services(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("MILVUS_DB_PATH", str(tmp_path_factory.mktemp("db")))
    mp.setenv("MILVUS_COLLECTION_NAME", "icd10_facets")
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


def value_of(rec, field):
    if field == "category":
        return (rec.get("category_path") or "").split(">")[0].strip() or rec["code"]
    return rec[field]


def by_query(ms, field, expr, limit=None, min_count=1):
    """the facet list from MilvusService.query's rows: a Counter over the field's values, count descending then value ascending"""
    counted = Counter(value_of(r, field) for r in ms.query(expr))
    out = [{"value": v, "count": c} for v, c in sorted(counted.items(), key=lambda vc: (-vc[1], vc[0])) if c >= min_count]
    return out if limit is None else out[:limit]


@pytest.fixture(scope="module")
def want(services):
    """(field, filter) -> the list counted from query's rows, computed once"""
    ms = services["ms"]
    lists = {(f, e): by_query(ms, f, e) for f in FIELDS for e in FILTERS}
    sizes = [sum(x["count"] for x in lists[("level", e)]) for e in FILTERS]
    assert sizes[0] == ms.client.count and all(0 < s < sizes[0] for s in sizes[1:])   # every filter selects some rows, none all
    return lists


def check_routes(ms, want):
    for (field, expr), lst in want.items():
        assert ms.facet(field, expr) == lst, (field, expr)
        assert ms.facet(field, expr, limit=3) == lst[:3] and ms.facet(field, expr, min_count=2) == [x for x in lst if x["count"] >= 2]
        assert sum(x["count"] for x in lst) == ms.count(expr)
    zeros = ms.facet("parent_code", FILTERS[1], min_count=0)
    assert zeros[:len(want[("parent_code", FILTERS[1])])] == want[("parent_code", FILTERS[1])] and zeros[-1]["count"] == 0
    assert [z["value"] for z in zeros if z["count"] == 0] == sorted(z["value"] for z in zeros if z["count"] == 0)
    assert ms.facet("level", "level in []") == []


def test_facets_equal_the_counted_query_rows(services, want):
    ms = services["ms"]
    assert ms.FILTER_ON_DEVICE and ms.TEXT_MATCH_ON_DEVICE
    ms._clear_views()
    check_routes(ms, want)


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


def test_a_batch_of_twenty_is_one_masks_call_and_one_count(services, want):
    ms = services["ms"]
    index = ms._ready_index()
    ms._clear_views()
    filters = (FILTERS * 4)[:18] + [None, 'code like "A0%"']
    assert len(filters) == 20
    calls = {"_masks_for": [], "group_counts": []}
    real_masks, real_counts = ms._masks_for, index.group_counts
    ms._masks_for = lambda idx, exprs, nq: (calls["_masks_for"].append(nq), real_masks(idx, exprs, nq))[1]
    index.group_counts = lambda *a, **k: (calls["group_counts"].append(len(a[0])), real_counts(*a, **k))[1]
    try:
        lists, totals = ms.facet_batch("parent_code", filters, with_totals=True)
        assert calls == {"_masks_for": [20], "group_counts": [20]}
    finally:
        del ms._masks_for, index.group_counts
    assert lists[:18] == [want[("parent_code", e)] for e in filters[:18]] and lists[18] == want[("parent_code", "")]
    assert lists[19] == by_query(ms, "parent_code", filters[19])
    assert totals == [ms.count(e or "") for e in filters]
    assert ms.facet_batch("category", filters[:5], limit=2, min_count=2) == [[x for x in want[("category", e)] if x["count"] >= 2][:2] for e in filters[:5]]
    # the search's own masks (a TEXT_MATCH made on the device) were closed behind the count; the scalar ones are cached
    assert not any("TEXT_MATCH" in f["expression"] for f in ms.filter_masks())
    assert len([g for g in ms.groupings() if g["field"] == "parent_code" and g["filter"] is None]) == 1


def test_endpoint(services, want):
    # (last of the module: the app's lifespan disconnects the installed services when the client closes)
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    ms, es = services["ms"], services["es"]
    appmod.install_services(es, ms, MultiDiagnosisService(es, ms))
    try:
        with TestClient(appmod.app) as client:
            r = client.post("/codes/facets", json={"field": "parent_code", "filter": FILTERS[3], "limit": 4, "min_count": 1})
            assert r.status_code == 200, r.text
            lst = want[("parent_code", FILTERS[3])]
            assert r.json() == {"field": "parent_code", "total": sum(x["count"] for x in lst), "facets": lst[:4]}
    finally:
        appmod.install_services(None, None, None)
