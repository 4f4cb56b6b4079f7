"""Wide search off the device: wide_select_plan.hpp under the host sanitizers, the symbols, tests/wide_oracle.py
(the ranking walk against a brute force that builds no ranking and against a model of the device's three stages; its vectorised
reweight against range_oracle.reweight), services/wide_search.py's argument rules and results over a stub index, and the shape of
POST /wide_query over stub services."""
import os
import subprocess

import numpy as np
import pytest

import range_oracle
import wide_oracle as wo
from conftest import ROOT
from rag_project_icd10_amd import _native

CSRC = os.path.join(ROOT, "rag_project_icd10_amd", "csrc")


def test_plan_header_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "wide_select_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "wide_select_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "wide select plan ok" in out.stdout


def test_symbols_and_abi():
    lib = _native.load_library()
    for name in ("icd_wide_create", "icd_wide_destroy", "icd_wide_stats", "icd_index_search_wide"):
        assert hasattr(lib, name) and name in _native.EXPORTED_SYMBOLS
    assert lib.icd_abi_version() == _native.ABI_VERSION == 6
    header = open(os.path.join(ROOT, "include", "icd_search.h"), encoding="utf-8").read()
    assert "#define ICD_ABI_VERSION 6" in header and "#define ICD_WIDE_MAX_K 16384" in header
    assert _native.WIDE_MAX_K == wo.MAX_K == 16384
    plan = open(os.path.join(CSRC, "wide_select_plan.hpp"), encoding="utf-8").read()
    assert "hip/" not in plan and "__global__" not in plan                         # host only: no HIP header, no kernel
    kernel = open(os.path.join(CSRC, "wide_select_kernel.hpp"), encoding="utf-8").read()
    body = kernel.split("#pragma once")[1]
    assert '#include "wide_select_plan.hpp"' in kernel and "order_f32(" in body and "level_weight(" in body and "rk_valid_bits(" in body
    assert "printf(" not in body and " assert(" not in body and "atomicAdd(float" not in body
    # the checks that need no device: a destroyed / missing handle is ICD_ERR_STATE
    assert lib.icd_wide_destroy(None) == -5 and lib.icd_wide_stats(None, None, None, None) == -5
    assert lib.icd_index_search_wide(None, None, None, None, 0, 1, 0, 0, None, None, 0, 1, None, None, None, None, None, None, 0, None) == -5


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def ranking_of(row_scores, id_base=0):
    """the full ranking oracle.flat_ip_topk returns for these row scores: (score desc, id asc), NaN rows left out, padding behind"""
    sc = np.asarray(row_scores, np.float32)
    o = wo.order_u32(sc).astype(np.int64)
    rows = np.array([r for r in np.lexsort((np.arange(len(sc)), -o)) if not np.isnan(sc[r])], np.int64)
    s = np.full(len(sc), -np.inf, np.float32)
    i = np.full(len(sc), -1, np.int64)
    s[:len(rows)], i[:len(rows)] = sc[rows], rows + id_base
    return s, i


def test_oracle_against_brute_force_and_the_stage_model():
    rng = np.random.default_rng(5)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, np.nan], np.float32)
    for case in range(300):
        n = int(rng.integers(1, 60))
        sc = (rng.integers(-6, 7, n) / 8.0).astype(np.float32)            # runs of ties
        if case % 3 == 0:
            at = rng.integers(0, n, 4)
            sc[at] = specials[rng.integers(0, len(specials), 4)]
        if case % 7 == 0:
            sc = (np.float32(1.0) + rng.integers(0, 5, n).astype(np.float32) * np.float32(2.0 ** -23)).astype(np.float32)   # the lowest digit only
        levels = rng.choice(np.array([0, 1, 2, 3, 7], np.int32), n)
        mask = None if case % 2 == 0 else rng.random(n) < 0.6
        lo = None if case % 4 < 2 else float(np.sort(sc[~np.isnan(sc)])[len(sc[~np.isnan(sc)]) // 4]) if (~np.isnan(sc)).any() else None
        hi = None if case % 5 < 3 else 0.5
        if lo is not None and hi is not None and not lo < hi:
            hi = None
        id_base = int(rng.integers(0, 2)) * 900
        k, first = int(rng.integers(1, 70)), int(rng.integers(0, 30))
        s, i = ranking_of(sc, id_base)
        (raw, ids, lv), adj, count, selected = wo.wide_query(s, i, levels, k, first, mask, lo, hi, id_base)
        b_raw, b_ids, b_count, b_sel = wo.brute_force(sc, k, first, mask, lo, hi, id_base)
        assert raw.tobytes() == b_raw.tobytes() and ids.tobytes() == b_ids.tobytes() and count == b_count and selected == b_sel, case
        s_raw, s_ids, s_count, s_sel, rec = wo.staged(sc, k, first, mask, lo, hi, id_base)
        assert raw.tobytes() == s_raw.tobytes() and ids.tobytes() == s_ids.tobytes() and count == s_count and selected == s_sel, case
        assert rec[1] + rec[2] == min(first + k, selected) and rec[3] == selected
        assert (lv[:count] == levels[ids[:count] - id_base]).all() and (lv[count:] == 0).all()
        for got, want in zip(adj, range_oracle.reweight(raw, ids, lv)):       # the vectorised reweight is range_oracle's, byte for byte
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), case


def test_oracle_on_hand_made_rankings():
    levels = np.array([1, 2, 3, 1, 2, 3, 1, 2], np.int32)
    sc = np.full(8, 0.25, np.float32)                                       # all tied: the rows in order
    (raw, ids, lv), adj, count, selected = wo.wide_query(*ranking_of(sc), levels, 3, first=2)
    assert ids.tolist() == [2, 3, 4] and count == 3 and selected == 8 and adj[2].tolist() == [3, 4, 2]   # level 1 first, level 3 last
    (raw, ids, lv), adj, count, selected = wo.wide_query(*ranking_of(sc), levels, 4, first=6, mask=np.array([1, 1, 1, 1, 1, 1, 1, 0], bool))
    assert ids.tolist() == [6, -1, -1, -1] and count == 1 and selected == 7 and np.isneginf(raw[1:]).all() and np.isneginf(adj[0][1:]).all()
    sc = np.array([0.5, np.nan, 0.5, 0.1, np.nan, 0.9, -0.2, 0.5], np.float32)
    (raw, ids, lv), adj, count, selected = wo.wide_query(*ranking_of(sc), levels, 8, radius=0.1, range_filter=0.5)
    assert ids.tolist() == [0, 2, 7, -1, -1, -1, -1, -1] and selected == 3                     # radius is strict, range_filter inclusive
    (raw, ids, lv), adj, count, selected = wo.wide_query(*ranking_of(sc), levels, 2, first=9)
    assert count == 0 and selected == 6 and (ids == -1).all()
    assert wo.staged(np.array([np.nan, np.nan], np.float32), 5)[4] == (0xFFFFFFFF, 0, 0, 0)


# ---- the service on its host side ---------------------------------------------------------------------------------------------
class StubMask:
    def __init__(self, rows):
        self.rows, self.closed, self.transient = len(rows), False, False

    def stats(self):
        return {"rows": self.rows, "bytes": 0}

    def close(self):
        self.closed = True


class StubWorkspace:
    """IcdWide as search_wide_batch sees it: every call is noted on its index; query q's hits are rows 0, 1, .. of the index in
    order, from `first` on"""

    def __init__(self, index, max_nq):
        self.index, self.max_nq, self.closed = index, max_nq, False

    def search_wide(self, queries, k, *, masks=None, radius=None, range_filter=None, first=0, reweighted=True):
        q = np.asarray(queries)
        assert q.ndim == 2 and q.dtype == np.float32 and not self.closed and reweighted
        self.index.calls.append(dict(nq=len(q), k=k, first=first, masks=masks, radius=radius, range_filter=range_filter))
        n, nq = self.index.n, len(q)
        ids = np.full((nq, k), -1, np.int64)
        m = max(0, min(k, n - first))
        ids[:, :m] = np.arange(first, first + m)
        raw = np.where(ids >= 0, 0.9 - 0.01 * ids, -np.inf).astype(np.float32)
        return raw.astype(np.float64), raw, ids, np.where(ids >= 0, 2, 0).astype(np.int32), np.full(nq, m, np.int32), np.full(nq, n, np.int64)


class StubIndex:
    def __init__(self, n, dim, max_nq=8):
        self.n, self.dim, self.max_nq, self.max_k, self.device, self.closed = n, dim, max_nq, 64, 0, False
        self.calls, self.made, self.handles = [], [], []

    def rowmask(self, rows):
        self.made.append(len(rows))
        return StubMask(rows)

    def make_workspace(self, max_nq):
        self.handles.append(StubWorkspace(self, max_nq))
        return self.handles[-1]


RECORDS = [{"code": c, "preferred_zh": t, "level": lv, "parent_code": p, "has_complication": False, "main_code": None, "secondary_code": None,
            "category_path": ""}
           for c, t, lv, p in [("A00", "霍乱", 1, ""), ("A00.0", "霍乱，由于O1群霍乱弧菌", 2, "A00"), ("A00.1", "埃尔托霍乱", 2, "A00"),
                               ("A01", "伤寒和副伤寒", 1, ""), ("A01.0", "伤寒", 2, "A01"), ("A01.1", "副伤寒甲", 2, "A01")]]
DIM = 64


@pytest.fixture()
def svc(tmp_path, monkeypatch):
    monkeypatch.setenv("MILVUS_DB_PATH", str(tmp_path / "db"))
    monkeypatch.setenv("MILVUS_COLLECTION_NAME", "wide")
    from rag_project_icd10_amd.services.milvus_service import MilvusService

    class Emb:                      # (the store takes its dimension from the encoder)
        def encode_query(self, t):
            return np.ones(DIM, np.float32) / 8

        def encode_query_batch(self, texts):
            return np.stack([np.full(DIM, len(t) / 64, np.float32) for t in texts])

    class Small(MilvusService):
        FILTER_ON_DEVICE = False    # the host route: filter_rows -> index.rowmask
        TEXT_MATCH_ON_DEVICE = False
        _WORKSPACE_FACTORIES = {"wide": (lambda index, size: index.make_workspace(size), "max_nq")}   # (the stub's, in place of _native.IcdWide)

    from rag_project_icd10_amd.services.wide_search import WideSearch
    s = WideSearch(Small(Emb()))
    yield s
    s.ms.disconnect()


def load(svc, **kw):
    rng = np.random.default_rng(0)
    ms = svc.ms
    assert ms.insert_records(RECORDS, [rng.standard_normal(DIM).astype(np.float32) for _ in RECORDS]) is True
    ms._index = StubIndex(len(RECORDS), DIM, **kw)
    ms._index_rows, ms._index_gen = ms.client.count, ms.client.generation
    return ms._index


Q = np.ones(DIM, np.float32)


def test_the_factory_is_registered():
    from rag_project_icd10_amd.services import wide_search
    from rag_project_icd10_amd.services.milvus_service import MilvusService
    assert MilvusService._WORKSPACE_FACTORIES["wide"] == (wide_search.make_workspace, "max_nq") and wide_search.MAX_TOP_K == 16384


def test_empty_collection_and_argument_checks(svc):
    assert svc.search_wide(Q, 1000) == []
    out, totals = svc.search_wide_batch(np.stack([Q, Q]), 200, with_totals=True)
    assert out[2].shape == (2, 200) and (out[2] == -1).all() and totals.tolist() == [0, 0]
    index = load(svc)
    bad = [
        lambda: svc.search_wide(Q, 0), lambda: svc.search_wide(Q, 16385), lambda: svc.search_wide(Q, 10.5), lambda: svc.search_wide(Q, True),
        lambda: svc.search_wide(Q, 10, offset=-1), lambda: svc.search_wide(Q, 385, offset=16000), lambda: svc.search_wide(Q, 10, offset=1.5),
        lambda: svc.search_wide(Q, 10, radius=0.5, range_filter=0.5), lambda: svc.search_wide(Q, 10, radius=float("nan")),
        lambda: svc.search_wide(Q, 10, radius=0.1, search_params={"params": {"radius": 0.2}}),
        lambda: svc.search_wide(Q, 10, filter="level =="), lambda: svc.search_wide(Q, 10, filter="nope == 1"), lambda: svc.search_wide(Q, 10, filter=["level == 2"]),
        lambda: svc.search_wide(np.stack([Q, Q]), 10), lambda: svc.search_wide(np.ones(DIM + 1, np.float32), 10),
        lambda: svc.search_wide_batch(Q, 10), lambda: svc.search_wide_batch(np.stack([Q, Q]), 10, filter=["level == 2"]),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} did not raise")
    assert index.calls == [] and index.made == [] and index.handles == []      # every check came before the index was asked


def test_results_and_one_call_per_batch(svc):
    index = load(svc)
    hits = svc.search_wide(Q, 1000, offset=2, radius=0.5, search_params={"params": {"range_filter": 0.75}})
    assert index.calls == [dict(nq=1, k=1000, first=2, masks=None, radius=0.5, range_filter=0.75)] and len(index.handles) == 1
    assert [h["code"] for h in hits] == ["A00.1", "A01", "A01.0", "A01.1"]      # `search`-shaped, padding dropped
    assert set(hits[0]) == {"code", "title", "score", "original_score", "metadata"} and hits[0]["original_score"] == float(np.float32(0.9 - 0.02))
    (adj, raw, ids, lv), totals = svc.search_wide_batch(np.stack([Q, Q, Q]), 200, filter=["level == 2", None, "level == 2"], with_totals=True)
    masks = index.calls[-1]["masks"]
    assert masks[1] is None and masks[0] is masks[2] and index.made == [4] and len(index.handles) == 1
    assert ids.shape == (3, 200) and adj.dtype == np.float64 and totals.tolist() == [6, 6, 6] and totals.dtype == np.int64
    lists = svc.search_wide_batch(np.stack([Q, Q]), 3, as_dicts=True)
    assert [len(x) for x in lists] == [3, 3] and lists[0][0]["code"] == "A00"


def test_endpoint_over_the_stub(svc):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as api
    index = load(svc)
    saved = (api.embedding_service, api.milvus_service, api.multi_diagnosis_service)
    api.install_services(svc.ms.embedding_service, svc.ms, multi=object())
    try:
        client = TestClient(api.app)
        r = client.post("/wide_query", json={"text": "霍乱", "top_k": 2000, "offset": 1})
        assert r.status_code == 200, r.text
        body = r.json()
        assert set(body) == {"candidates", "total"} and body["total"] == 6 and [c["code"] for c in body["candidates"]] == [r_["code"] for r_ in RECORDS[1:]]
        assert body["candidates"] == svc.search_wide(np.ones(DIM, np.float32) / 8, 2000, offset=1)
        assert index.calls[-1]["k"] == 2000 and index.calls[-1]["first"] == 1
        for bad in ({"text": "霍乱", "top_k": 16385}, {"text": "霍乱", "top_k": 0}, {"text": "", "top_k": 5}, {"text": "霍乱", "top_k": 10, "offset": 16380},
                    {"text": "霍乱", "filter": "level =="}, {"text": "霍乱", "radius": 0.5, "range_filter": 0.1}):
            assert client.post("/wide_query", json=bad).status_code == 400, bad
        r = client.post("/wide_query", json={"text": "霍乱", "top_k": 500, "filter": "level == 2", "radius": 0.0})
        assert r.status_code == 200 and index.calls[-1]["masks"][0] is not None and index.calls[-1]["radius"] == 0.0
    finally:
        api.embedding_service, api.milvus_service, api.multi_diagnosis_service = saved
