"""Embedding-list search through the service and the API (run with -m gpu on an MI355X):
MilvusService.search_embedding_list / search_embedding_lists_batch on the golden CSV slice against tests/maxsim_oracle.py through
the service's field groupings, every row its own group, and a filter's view; POST /segments_query with the synthetic encoder."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from grouped_oracle import Ranking
from maxsim_oracle import expected

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 2, 5, 1, 4]
FILTER = "level >= 2"


@pytest.fixture(scope="module")
def services(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("MILVUS_DB_PATH", str(tmp_path_factory.mktemp("db")))
    mp.setenv("MILVUS_COLLECTION_NAME", "icd10_maxsim")
    mp.setenv("EMBEDDING_MODEL_NAME", "shibing624/text2vec-base-chinese")
    mp.setenv("ICD_EMBEDDING_ALLOW_SYNTHETIC", "1")
    from rag_project_icd10_amd.tools.build_database import DatabaseBuilder
    b = DatabaseBuilder()
    b.initialize_services()
    recs = b.load_csv_data(os.path.join(GOLDEN, "csv_slice.csv"))
    assert b.vectorize_and_index(recs) is True
    strings = [l.rstrip("\n") for l in open(os.path.join(GOLDEN, "diagnosis_strings.txt"), encoding="utf-8")][:sum(SIZES)]
    yield {"b": b, "recs": recs, "ms": b.milvus_service, "es": b.embedding_service, "strings": strings}
    b.milvus_service.disconnect()
    mp.undo()


def _field_values(recs, field):
    if field is None:
        return [r["code"] for r in recs]
    if field == "category":
        return [(r.get("category_path") or "").split(">")[0].strip() or r["code"] for r in recs]
    return ["" if r.get(field) is None else str(r.get(field)) for r in recs]


def _check(ms, recs, got, want, off, vals, labels):
    """the service's dicts of every list against the oracle's arrays"""
    gsc, gid, msc, mid, mlv = want
    assert len(got) == len(off) - 1
    for li, groups in enumerate(got):
        m = int((gid[li] >= 0).sum())
        assert [g["group"] for g in groups] == [labels[int(g)] for g in gid[li, :m]], li
        assert [g["score"] for g in groups] == [float(x) for x in gsc[li, :m]]
        for j, g in enumerate(groups):
            ts = range(int(off[li]), int(off[li + 1]))
            assert len(g["matches"]) == len(ts)
            for seg, (t, hit) in enumerate(zip(ts, g["matches"])):
                if mid[t, j] < 0:
                    assert hit is None
                    continue
                row = int(mid[t, j])
                assert hit["code"] == recs[row]["code"] and hit["segment"] == seg and vals[row] == g["group"]
                assert hit["original_score"] == float(msc[t, j]) and hit["metadata"]["level"] == int(mlv[t, j])
                assert hit["score"] == float(np.float64(msc[t, j]) * ms._calculate_level_weight(int(mlv[t, j])))


@pytest.mark.parametrize("field", [None, "category", "parent_code"])
def test_search_embedding_lists(services, oracle, field):
    ms, es, recs = services["ms"], services["es"], services["recs"]
    corpus, levels = ms.client.matrix(), ms.client.levels()
    vals = _field_values(recs, field)
    if field is None:
        group_of, labels = np.arange(len(recs)), vals
    else:
        labels = sorted(set(vals))
        rank = {v: i for i, v in enumerate(labels)}
        group_of = np.array([rank[v] for v in vals], np.int64)
    vecs = np.stack([es.encode_query(s) for s in services["strings"]]).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(SIZES)])
    lists = [vecs[off[i]:off[i + 1]] for i in range(len(SIZES))]
    s_all, i_all = oracle.flat_ip_topk(corpus, vecs, len(recs))
    rk = Ranking(s_all, i_all, group_of)
    rows = ms.filter_rows(FILTER)
    assert 0 < len(rows) < len(recs)
    vs, vi = oracle.flat_ip_topk(corpus[rows], vecs, len(rows))
    rk_f = Ranking(vs, vi, group_of[rows])
    for k, scorer in ((5, "sum"), (3, "mean")):
        batch = ms.search_embedding_lists_batch(lists, k, group_by_field=field, scorer=scorer)
        _check(ms, recs, batch, expected(rk, off, levels, k, scorer), off, vals, labels)
        for li in (0, 3):
            assert ms.search_embedding_list(lists[li], k, group_by_field=field, scorer=scorer) == batch[li]
        filtered = ms.search_embedding_lists_batch(lists, k, group_by_field=field, filter=FILTER, scorer=scorer)
        _check(ms, recs, filtered, expected(rk_f, off, levels, k, scorer, row_map=rows), off, vals, labels)
        for groups in filtered:
            assert all(h is None or h["metadata"]["level"] >= 2 for g in groups for h in g["matches"])
    cached = [(g["field"], g["filter"] is None) for g in ms.groupings()]      # the groupings are cached where the others are
    assert (field, True) in cached and (field, False) in cached
    assert ms.search_embedding_lists_batch(lists, 3, group_by_field=field, filter="level > 99") == [[] for _ in lists]


def test_segments_query_endpoint(services):
    # (last of the module: the app's lifespan disconnects the installed services when the client closes)
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    ms, es = services["ms"], services["es"]
    appmod.install_services(es, ms, object())
    try:
        with TestClient(appmod.app) as client:
            segments = services["strings"][:4]
            vecs = np.asarray(es.encode_query_batch(segments), dtype=np.float32)
            mean = {"group_by_field": "category", "scorer": "mean", "top_k": 3}
            for kw in ({}, mean, {"filter": FILTER, "top_k": 4}):
                r = client.post("/segments_query", json=dict(kw, segments=segments))
                assert r.status_code == 200, r.text
                want = ms.search_embedding_list(vecs, **kw)
                got = r.json()
                assert got["segments"] == 4 and len(got["groups"]) == len(want) > 0
                assert [g["group"] for g in got["groups"]] == [g["group"] for g in want]
                assert [g["score"] for g in got["groups"]] == [g["score"] for g in want]
                pairs = lambda groups: [[None if h is None else (h["code"], h["segment"]) for h in g["matches"]] for g in groups]   # noqa: E731
                assert pairs(got["groups"]) == pairs(want)
            assert client.post("/segments_query", json={"segments": segments, "scorer": "max"}).status_code == 400
            assert client.post("/segments_query", json={"segments": segments, "group_by_field": "colour"}).status_code == 400
            assert client.post("/segments_query", json={"segments": segments, "filter": "level =="}).status_code == 400
            assert client.post("/segments_query", json={"segments": []}).status_code == 400
    finally:
        appmod.install_services(None, None, None)
