"""Milvus-style filter expressions (services/filter_expr.py) over the records of the full ICD-10 CSV, and their way through
MilvusService and /query with stub services. No GPU."""
import lzma
import os

import numpy as np
import pytest

from conftest import GOLDEN

from rag_project_icd10_amd.services import filter_expr as fe


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    from rag_project_icd10_amd.tools.build_database import DatabaseBuilder
    path = tmp_path_factory.mktemp("csv") / "ICD_10v601.csv"
    path.write_bytes(lzma.open(os.path.join(GOLDEN, "ICD_10v601.csv.xz")).read())
    recs = DatabaseBuilder.__new__(DatabaseBuilder).load_csv_data(str(path))   # (the CSV parser needs no services)
    assert len(recs) == 40474
    return recs


@pytest.fixture(scope="module")
def columns(records):
    return fe.Columns.from_records(records)


# (expression, the same predicate written out in Python over one record)
CASES = [
    ('code like "C%"', lambda r: r["code"].startswith("C")),
    ('code like "E11%"', lambda r: r["code"].startswith("E11")),
    ("code like '%.9'", lambda r: r["code"].endswith(".9")),
    ('preferred_zh like "%糖尿病%"', lambda r: "糖尿病" in r["preferred_zh"]),
    ('code like "I10"', lambda r: r["code"] == "I10"),
    ("has_complication == true", lambda r: r["has_complication"]),
    ("has_complication == False", lambda r: not r["has_complication"]),
    ("has_complication != TRUE", lambda r: not r["has_complication"]),
    ("level == 1", lambda r: r["level"] == 1),
    ("level != 3", lambda r: r["level"] != 3),
    ("level < 2", lambda r: r["level"] < 2),
    ("level <= 2", lambda r: r["level"] <= 2),
    ("level > 2", lambda r: r["level"] > 2),
    ("level >= 2", lambda r: r["level"] >= 2),
    ("level > -1", lambda r: True),
    ("level in [1, 3]", lambda r: r["level"] in (1, 3)),
    ("level not in [1,3]", lambda r: r["level"] not in (1, 3)),
    ('code in ["A00", "E11.9", \'I10\', "nope"]', lambda r: r["code"] in ("A00", "E11.9", "I10", "nope")),
    ('code not in ["A00"]', lambda r: r["code"] != "A00"),
    ("code in []", lambda r: False),
    ('parent_code == "E11"', lambda r: r["parent_code"] == "E11"),
    ('parent_code != ""', lambda r: r["parent_code"] != ""),
    ('main_code == "A01.0"', lambda r: r["main_code"] == "A01.0"),
    ('secondary_code like "K%"', lambda r: r["secondary_code"].startswith("K")),
    ('category_path like "E11 >%"', lambda r: r["category_path"].startswith("E11 >")),
    ('level >= 2 and code like "E11%"', lambda r: r["level"] >= 2 and r["code"].startswith("E11")),
    ('level >= 2 && code like "E11%"', lambda r: r["level"] >= 2 and r["code"].startswith("E11")),
    ('code like "A%" or code like "B%"', lambda r: r["code"][:1] in ("A", "B")),
    ('code like "A%" || code like "B%"', lambda r: r["code"][:1] in ("A", "B")),
    ('not code like "C%"', lambda r: not r["code"].startswith("C")),
    ('!(code like "C%")', lambda r: not r["code"].startswith("C")),
    # precedence: not > and > or
    ('code like "A%" or code like "B%" and level == 1', lambda r: r["code"].startswith("A") or (r["code"].startswith("B") and r["level"] == 1)),
    ('(code like "A%" or code like "B%") and level == 1', lambda r: r["code"][:1] in ("A", "B") and r["level"] == 1),
    ('not level == 1 and code like "E%"', lambda r: r["level"] != 1 and r["code"].startswith("E")),
    ('not (level == 1 and code like "E%")', lambda r: not (r["level"] == 1 and r["code"].startswith("E"))),
    ('NOT has_complication == true OR level IN [1] AND code LIKE "Z%"',
     lambda r: (not r["has_complication"]) or (r["level"] == 1 and r["code"].startswith("Z"))),
    ('((((level == 2))))', lambda r: r["level"] == 2),
    ('code == "it\\"s"', lambda r: r["code"] == 'it"s'),
    ('has_complication == true and secondary_code != ""', lambda r: r["has_complication"] and r["secondary_code"] != ""),
]


@pytest.mark.parametrize("expr,pred", CASES, ids=[c[0] for c in CASES])
def test_selection_equals_the_python_predicate(records, columns, expr, pred):
    want = np.array([i for i, r in enumerate(records) if pred(r)], dtype=np.int64)
    got = fe.select(expr, columns)
    assert got.dtype == np.int64 and np.array_equal(got, want), (expr, len(got), len(want))
    assert np.all(np.diff(got) > 0)
    # the plain-dict form of the columns gives the same rows (evaluated every time, nothing cached)
    assert np.array_equal(fe.select(expr, dict(columns.arrays)), want)


def test_issue_counts(columns):
    assert len(fe.select('code like "C%"', columns)) == 1850
    assert len(fe.select('code like "E11%"', columns)) == 154
    assert len(fe.select("has_complication == true", columns)) == 1000
    # a chapter letter covers 22 to 4 017 rows; level >= 2 is 88 % of the corpus
    sizes = [len(fe.select(f'code like "{c}%"', columns)) for c in "ABCDEFGHIJKLMNOPQRSTUVWXYZ"]
    assert min(s for s in sizes if s) == 22 and max(sizes) == 4017
    assert round(len(fe.select("level >= 2", columns)) / columns.n, 2) == 0.88


def test_normalised_key_ignores_spelling():
    same = ['level >= 2 and code like "E11%"', "(level>=2) && (code LIKE 'E11%')", '((level >= 2)) AND code like "E11%"']
    assert len({fe.compile(e) for e in same}) == 1
    assert fe.compile("level in [3, 1, 1]") == fe.compile("level IN [1,3]")
    assert fe.compile("has_complication == True") == fe.compile("has_complication == true")
    assert fe.compile('code == "A"') != fe.compile('code != "A"')
    # the key parses back to itself
    for e in ('not (level == 1 or code like "%.9") and has_complication != false', 'code in ["a\\"b", "c"]'):
        k = fe.compile(e)
        assert fe.compile(k) == k


def test_columns_cache_selections(columns):
    a = columns.select('code like "E11%"')
    b = columns.select("(code LIKE 'E11%')")
    assert a is b and not a.flags.writeable


@pytest.mark.parametrize("expr,where,what", [
    ("", 0, "empty"),
    ("level >", 7, "literal"),
    ("level == 1 and", 14, "field name"),
    ("(level == 1", 11, "')'"),
    ("level == 1)", 10, "unexpected"),
    ("level = 1", 6, "unexpected character"),
    ('code == "abc', 8, "unterminated"),
    ("code like E11", 10, "quoted pattern"),
    ('code like "A%B"', 10, "leading and / or trailing"),
    ('code like "%A%B%"', 10, "leading and / or trailing"),
    ("level in [1, 2", 14, "',' or ']'"),
    ("level in 1", 9, "'['"),
    ("level not 1", 10, "'in'"),
    ("level", 5, "comparison"),
    ("foo == 1", 0, "unknown field 'foo'"),
    ("semantic_text == 'x'", 0, "unknown field"),
    ("1 == level", 0, "field name"),
    ('level == "2"', 9, "type mismatch"),
    ("level == true", 9, "type mismatch"),
    ("code == 5", 8, "type mismatch"),
    ("has_complication == 1", 20, "type mismatch"),
    ('code in ["A", 1]', 14, "type mismatch"),
    ('code < "B"', 5, "type mismatch"),
    ("has_complication >= true", 17, "type mismatch"),
    ("level like '1%'", 6, "type mismatch"),
    ("has_complication like 'x'", 17, "type mismatch"),
    ("__import__('os')", 0, "unknown field"),
])
def test_bad_expressions_raise_value_error_with_position(expr, where, what):
    with pytest.raises(ValueError) as e:
        fe.compile(expr)
    msg = str(e.value)
    assert f"position {where}:" in msg and what in msg, msg


def test_not_a_string():
    with pytest.raises(ValueError):
        fe.compile(None)


# ---- MilvusService without a GPU: the filter's host side --------------------------------------------------------------------
def test_service_filter_rows_follow_the_store_generation(tmp_path, monkeypatch):
    """filter_rows answers from columns of the CURRENT store: a rebuild with the same row count selects the new rows (the view
    cache is keyed on the store's generation counter, not on the row count); a bad expression raises there, search logs and
    returns []"""
    monkeypatch.setenv("MILVUS_DB_PATH", str(tmp_path / "db"))
    from rag_project_icd10_amd.services import milvus_service as msmod

    class NoGpu(msmod.MilvusService):   # (the host side only: nothing is uploaded)
        def _load_collection_to_memory(self):
            self._loaded = True

    class Emb:
        def encode_query(self, text):
            return np.zeros(4, np.float32)

    svc = NoGpu(Emb())
    rows = lambda codes: [{"code": c, "preferred_zh": c, "level": 2 if "." in c else 1} for c in codes]
    vecs = lambda n: [np.ones(4, np.float32)] * n
    assert svc.insert_records(rows(["A00", "A00.1", "B01", "B01.2"]), vecs(4))
    g0 = svc.client.generation
    assert svc.filter_rows('code like "A%"').tolist() == [0, 1]
    assert svc.filter_rows("level == 2").tolist() == [1, 3]
    assert svc.clear_collection()
    assert svc.insert_records(rows(["C00", "C00.1", "A02", "D01"]), vecs(4))
    assert svc.client.count == 4 and svc.client.generation != g0
    assert svc.filter_rows('code like "A%"').tolist() == [2]
    assert svc.filter_rows("level == 2").tolist() == [1]
    with pytest.raises(ValueError):
        svc.filter_rows("level == 'x'")
    assert svc.search(np.zeros(4, np.float32), 3, filter="nope == 1") == []
    with pytest.raises(ValueError):
        svc.search_batch(np.zeros((2, 4), np.float32), 3, filter="level >")
    # an empty selection answers without a device call: [] / -1-padded arrays
    assert svc.search(np.zeros(4, np.float32), 3, filter='code == "none"') == []
    svc._ready_index = lambda: type("Idx", (), {"n": 4})()
    adj, raw, ids, lv = svc.search_batch(np.zeros((2, 4), np.float32), 3, filter='code == "none"')
    assert ids.shape == (2, 3) and (ids == -1).all() and np.isneginf(adj).all() and np.isneginf(raw).all() and (lv == 0).all()
    assert adj.dtype == np.float64 and raw.dtype == np.float32 and ids.dtype == np.int64 and lv.dtype == np.int32
    assert svc.search_batch(np.zeros((2, 4), np.float32), 3, as_dicts=True, filter='code == "none"') == [[], []]


def test_store_generation_bumps_on_every_mutation(tmp_path):
    from rag_project_icd10_amd.corpus_store import CorpusStore
    st = CorpusStore.open(str(tmp_path), "c", 4)
    seen = [st.generation]
    st.create()
    seen.append(st.generation)
    st.append([{"code": "A"}], np.ones((1, 4), np.float32))
    seen.append(st.generation)
    st.drop()
    seen.append(st.generation)
    st.create()
    st.append([{"code": "B"}], np.ones((1, 4), np.float32))
    seen.append(st.generation)
    assert all(b > a for a, b in zip(seen, seen[1:])), seen


# ---- /query with stub services ----------------------------------------------------------------------------------------------
def _stub_app():
    from rag_project_icd10_amd.api import app as appmod

    class Emb:
        def encode_batch(self, texts, show_progress=True):
            return [[0.0, 1.0]] * len(texts)

        def encode_query_batch(self, qs, **kw):
            return np.zeros((len(qs), 2), np.float32)

        def get_model_info(self):
            return {"loaded": True, "model_name": "stub"}

    class Mil:
        calls = []

        def search_batch(self, v, k, as_dicts=False, **kw):
            Mil.calls.append(kw.get("filter"))
            hit = lambda c, s, lv: {"code": c, "title": "t" + c, "score": s, "original_score": s, "metadata": {"level": lv}}
            hits = [hit("I21.9", 0.9, 2), hit("I21", 0.5, 1), hit("K29.7", -0.1, 2)]
            if kw.get("filter") is not None:
                rows = fe.select(kw["filter"], {"code": np.array([h["code"] for h in hits]),
                                                "level": np.array([h["metadata"]["level"] for h in hits])})
                hits = [hits[i] for i in rows]
            return [hits[:k] for _ in range(len(v))]

        def test_connection(self):
            return {"connected": True}

        def get_collection_stats(self):
            return {"num_entities": 3}

        def filter_views(self):
            return [{"expression": "level == 1", "rows": 1, "generation": 1, "bytes": 4096}]

        def disconnect(self):
            return {}

    return appmod, Emb, Mil


def test_query_filter_reaches_the_service_and_bad_filters_are_400():
    from fastapi.testclient import TestClient
    appmod, Emb, Mil = _stub_app()
    appmod.install_services(Emb(), Mil())
    try:
        with TestClient(appmod.app) as client:
            plain = client.post("/query", json={"text": "高血压，糖尿病", "top_k": 2})
            assert plain.status_code == 200 and Mil.calls == [None]
            # a request without filter gives the same response as an explicit null
            assert client.post("/query", json={"text": "高血压，糖尿病", "top_k": 2, "filter": None}).json() == plain.json()
            r = client.post("/query", json={"text": "高血压，糖尿病", "top_k": 2, "filter": "level == 1"})
            assert r.status_code == 200 and Mil.calls[-1] == "level == 1"
            codes = {c["code"] for m in r.json()["diagnosis_matches"] for c in m["candidates"]}
            assert codes == {"I21"}, codes
            assert {c["code"] for m in plain.json()["diagnosis_matches"] for c in m["candidates"]} == {"I21.9", "I21"}
            n = len(Mil.calls)
            for bad, where in (("level == 'x'", "position 9"), ("foo == 1", "unknown field"), ("level >", "position 7")):
                r = client.post("/query", json={"text": "高血压", "filter": bad})
                assert r.status_code == 400 and where in r.json()["detail"], r.json()
            assert len(Mil.calls) == n   # (rejected before any search)
            assert client.get("/stats").json()["filter_views"] == [{"expression": "level == 1", "rows": 1, "generation": 1, "bytes": 4096}]
            # every other failure keeps the 500
            appmod.install_services(None, None, None)
            r = client.post("/query", json={"text": "x", "filter": "level == 1"})
            assert r.status_code == 500
    finally:
        appmod.install_services(None, None, None)
