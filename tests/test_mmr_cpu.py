"""MMR search without a GPU: the host-visible arithmetic (csrc/mmr_plan.hpp) in a program of its own under
the host sanitizers, the exported symbols and the ABI version, the numpy oracle against a brute-force Python loop,
MilvusService.search_mmr / search_mmr_batch on their host side over a stub index, and the /diverse_query route over a stub service."""
import os
import subprocess

import numpy as np
import pytest

import mmr_oracle as mo
from conftest import ROOT
from rag_project_icd10_amd import _native

CSRC = os.path.join(ROOT, "rag_project_icd10_amd", "csrc")


def test_plan_header_under_the_host_sanitizers(tmp_path):
    """tests/mmr_plan_check.cpp: ties to the lower index, NaN never wins, the all-NaN fallback, lambda 0 and 1, random arrays
    against a plain loop - with ASan and UBSan"""
    exe = str(tmp_path / "mmr_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "mmr_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mmr plan ok" in out.stdout


def test_symbols_and_abi():
    lib = _native.load_library()
    for name in ("icd_mmr_create", "icd_mmr_destroy", "icd_mmr_stats", "icd_index_search_mmr"):
        assert hasattr(lib, name) and name in _native.EXPORTED_SYMBOLS
    assert lib.icd_abi_version() == _native.ABI_VERSION == 6
    header = open(os.path.join(ROOT, "include", "icd_search.h"), encoding="utf-8").read()
    assert "#define ICD_ABI_VERSION 6" in header
    assert "int icd_index_search_mmr(icd_index *idx, icd_mmr *mmr, icd_rowmask *const *masks, const float *queries, int64_t nq, int32_t k," in header
    plan = open(os.path.join(CSRC, "mmr_plan.hpp"), encoding="utf-8").read()
    assert "hip/" not in plan and "__global__" not in plan                         # host only: no HIP header, no kernel
    kernel = open(os.path.join(CSRC, "mmr_select_kernel.hpp"), encoding="utf-8").read()
    assert '#include "mmr_plan.hpp"' in kernel and "mmr_value(" in kernel and "mmr_pen_update(" in kernel and "mmr_fold(" in kernel
    assert "atomic" not in kernel.split("#pragma once")[1]                         # nothing is summed or ordered by arrival
    # the checks that need no device: a destroyed / missing handle is ICD_ERR_STATE
    assert lib.icd_mmr_destroy(None) == -5 and lib.icd_mmr_stats(None, None, None) == -5
    assert lib.icd_index_search_mmr(None, None, None, None, 0, 1, 1, 0.5, 0, None, None, 0, 0, None, None, None, None, None, 0, None) == -5


class FakeOracle:
    """oracle.scores / reweight / level_weight for rows of small dyadic values, where every fmaf step is exact: plain numpy"""

    @staticmethod
    def scores(query, corpus):
        return (np.asarray(corpus, np.float64) @ np.asarray(query, np.float64)).astype(np.float32)

    @staticmethod
    def level_weight(level):
        return {1: 1.2, 3: 0.8}.get(int(level), 1.0)


def test_oracle_against_a_brute_force_loop(oracle):
    """30 random small cases: rows of multiples of 1/8 (every chain step exact, many ties), random masks, every lambda"""
    rng = np.random.default_rng(11)
    for case in range(30):
        n, dim = int(rng.integers(1, 24)), 8
        corpus = (rng.integers(-8, 9, (n, dim)) / 8.0).astype(np.float32)
        if case % 3 == 0:      # families of copies
            corpus = corpus[rng.integers(0, max(1, n // 3), n)]
        levels = rng.integers(1, 4, n).astype(np.int32)
        queries = (rng.integers(-8, 9, (2, dim)) / 8.0).astype(np.float32)
        id_base = int(rng.integers(0, 3)) * 1000
        fetch_k = int(rng.integers(1, 12))
        k = int(rng.integers(1, fetch_k + 1))
        lam = (0.0, 0.3, 0.5, 1.0)[case % 4]
        keep = [None, rng.random(n) < 0.6]
        fs, fi = oracle.flat_ip_topk(corpus, queries, n, id_base=id_base)
        assert np.array_equal(oracle.scores(queries[0], corpus), FakeOracle.scores(queries[0], corpus))   # (exact data: the chain IS the sum)
        pick, rew = mo.mmr_batch(oracle, corpus, levels, fs, fi, k, fetch_k, lam, masks=keep, id_base=id_base)
        for q in range(2):
            ids, values = mo.brute_force(corpus, levels, queries[q], k, fetch_k, lam, keep[q], id_base)
            t = len(ids)
            assert pick[1][q][:t].tolist() == ids and (pick[1][q][t:] == -1).all(), (case, q)
            assert pick[3][q][:t].tolist() == values and np.isneginf(pick[3][q][t:]).all()
            assert np.array_equal(pick[2][q][:t], levels[np.asarray(ids, np.int64) - id_base])
            # the reweighted form: the same hits, adjusted scores descending, the mmr value with its hit
            assert sorted(rew[2][q][:t].tolist()) == sorted(ids) and (np.diff(rew[0][q][:t]) <= 0).all()
            by_id = dict(zip(ids, values))
            assert [by_id[i] for i in rew[2][q][:t].tolist()] == rew[4][q][:t].tolist()
        if lam == 1.0:         # plain relevance: the candidate list's head
            assert np.array_equal(pick[1], mo.masked_batch([fs[q][fi[q] >= 0] for q in range(2)], [fi[q][fi[q] >= 0] for q in range(2)],
                                                           levels, keep, k, id_base=id_base)[0][1])


def test_greedy_rules_by_hand():
    rel = np.array([0.9, 0.9, 0.8, 0.8, 0.5, 0.1], np.float32)
    sim = np.array([[1, 1, .2, .2, .1, 0], [1, 1, .2, .2, .1, 0], [.2, .2, 1, 1, .3, 0], [.2, .2, 1, 1, .3, 0], [.1, .1, .3, .3, 1, 0],
                    [0, 0, 0, 0, 0, 1]], np.float32)
    picks, values = mo.greedy(rel, lambda i: sim[i], 6, 0.5)
    assert picks == [0, 2, 4, 5, 1, 3]                                              # the tie 2 / 3 goes to 2; the copies come last
    assert values[0] == 0.5 * float(rel[0]) and values[1] == 0.5 * float(rel[2]) - 0.5 * float(sim[2][0])
    assert mo.greedy(rel, lambda i: sim[i], 3, 1.0)[0] == [0, 1, 2] and mo.greedy(rel, lambda i: sim[i], 9, 1.0)[0] == [0, 1, 2, 3, 4, 5]
    assert mo.greedy(rel[:0], lambda i: sim[i], 3, 0.5) == ([], [])
    nan = np.full((3, 3), np.nan, np.float32)                                       # no comparable value: the lowest unpicked index
    picks, values = mo.greedy(rel[:3], lambda i: nan[i], 3, 0.5)
    assert picks == [0, 1, 2] and all(np.isnan(v) for v in values[1:])


# ---- the service on its host side -------------------------------------------------------------------------------------------------
class StubMask:
    def __init__(self, rows, transient=False):
        self.rows, self.closed, self.transient = len(rows), False, transient

    def stats(self):
        return {"rows": self.rows, "bytes": 0}

    def close(self):
        self.closed = True


class StubMmr:
    def __init__(self, max_nq):
        self.max_nq, self.closed = max_nq, False

    def stats(self):
        return {"max_nq": self.max_nq, "bytes": 0}

    def close(self):
        self.closed = True


class StubIndex:
    """IcdIndex as search_mmr_batch sees it: every call is noted; the hits are rows 0 .. k - 1"""

    def __init__(self, n, dim, max_nq=8, max_k=64):
        self.n, self.dim, self.max_nq, self.max_k, self.device, self.closed = n, dim, max_nq, max_k, 0, False
        self.calls, self.made, self.handles, self.fail = [], [], [], None

    def rowmask(self, rows):
        self.made.append(len(rows))
        return StubMask(rows)

    def mmr(self, max_nq=None):
        self.handles.append(StubMmr(max_nq))
        return self.handles[-1]

    def search_mmr(self, queries, k, fetch_k, lam, *, mmr, masks=None, radius=None, range_filter=None, reweighted=True, on_device=False):
        q = np.asarray(queries)
        assert q.ndim == 2 and q.shape[1] == self.dim and not mmr.closed and mmr.max_nq >= len(q) and reweighted
        assert masks is None or (len(masks) == len(q) and all(m is None or not m.closed for m in masks))
        self.calls.append(dict(nq=len(q), k=k, fetch_k=fetch_k, lam=lam, masks=masks, radius=radius, range_filter=range_filter))
        if self.fail is not None:
            raise self.fail
        nq = len(q)
        ids = np.tile(np.arange(k, dtype=np.int64), (nq, 1))
        ids[:, min(self.n, k):] = -1
        raw = np.where(ids >= 0, 0.5 - 0.01 * ids, -np.inf).astype(np.float32)
        return raw.astype(np.float64), raw, ids, np.where(ids >= 0, 2, 0).astype(np.int32), np.where(ids >= 0, 0.25 - 0.01 * ids, -np.inf)

    def close(self):
        self.closed = True


RECORDS = [{"code": c, "preferred_zh": t, "level": lv, "parent_code": p, "has_complication": False, "main_code": None, "secondary_code": None,
            "category_path": ""}
           for c, t, lv, p in [("A00", "霍乱", 1, ""), ("A00.0", "霍乱，由于O1群霍乱弧菌", 2, "A00"), ("A00.1", "埃尔托霍乱", 2, "A00"),
                               ("A01", "伤寒和副伤寒", 1, ""), ("A01.0", "伤寒", 2, "A01"), ("A01.1", "副伤寒甲", 2, "A01")]]
DIM = 64


@pytest.fixture()
def svc(tmp_path, monkeypatch):
    monkeypatch.setenv("MILVUS_DB_PATH", str(tmp_path / "db"))
    monkeypatch.setenv("MILVUS_COLLECTION_NAME", "mmr")
    from rag_project_icd10_amd.services.milvus_service import MilvusService

    class Emb:
        def encode_query(self, t):
            return np.ones(DIM, np.float32) / 8

    class Small(MilvusService):
        FILTER_ON_DEVICE = False    # the host route: filter_rows -> index.rowmask
        TEXT_MATCH_ON_DEVICE = False

    s = Small(Emb())
    yield s
    s.disconnect()


def load(svc, **kw):
    rng = np.random.default_rng(0)
    assert svc.insert_records(RECORDS, [rng.standard_normal(DIM).astype(np.float32) for _ in RECORDS]) is True
    svc._index = StubIndex(len(RECORDS), DIM, **kw)
    svc._index_rows, svc._index_gen = svc.client.count, svc.client.generation
    return svc._index


VEC = np.ones(DIM, np.float32) / 8


def test_empty_collection(svc):
    assert svc.search_mmr(VEC) == [] and svc.search_mmr(VEC, 3, 10, 0.2, filter="level == 2") == []
    assert svc.search_mmr_batch(np.stack([VEC, VEC]), 3) == [[], []]
    for bad in (lambda: svc.search_mmr(VEC, 0), lambda: svc.search_mmr(VEC, 3, 2), lambda: svc.search_mmr(VEC, lambda_mult=2.0),
                lambda: svc.search_mmr(VEC, filter="level ==")):
        with pytest.raises(ValueError):      # a bad argument raises on an empty collection too
            bad()


def test_argument_checks(svc):
    index = load(svc)
    two = np.stack([VEC, VEC])
    bad = [
        lambda: svc.search_mmr(VEC, 0), lambda: svc.search_mmr(VEC, -1), lambda: svc.search_mmr(VEC, 129), lambda: svc.search_mmr(VEC, 2.5),
        lambda: svc.search_mmr(VEC, True), lambda: svc.search_mmr(VEC, "3"),
        lambda: svc.search_mmr(VEC, 5, 4), lambda: svc.search_mmr(VEC, 5, 129), lambda: svc.search_mmr(VEC, 5, 0), lambda: svc.search_mmr(VEC, 5, 7.5),
        lambda: svc.search_mmr(VEC, 5, 65),                                          # above the store's max k (64)
        lambda: svc.search_mmr(VEC, lambda_mult=-0.1), lambda: svc.search_mmr(VEC, lambda_mult=1.1), lambda: svc.search_mmr(VEC, lambda_mult=float("nan")),
        lambda: svc.search_mmr(VEC, lambda_mult=None), lambda: svc.search_mmr(VEC, lambda_mult="0.5"), lambda: svc.search_mmr(VEC, lambda_mult=True),
        lambda: svc.search_mmr(VEC, filter="level =="), lambda: svc.search_mmr(VEC, filter="nope == 1"), lambda: svc.search_mmr(VEC, filter=["level == 2"]),
        lambda: svc.search_mmr(VEC, radius=0.5, range_filter=0.1), lambda: svc.search_mmr(VEC, radius=float("nan")), lambda: svc.search_mmr(VEC, radius="x"),
        lambda: svc.search_mmr(VEC, radius=0.1, search_params={"params": {"radius": 0.2}}),
        lambda: svc.search_mmr(two), lambda: svc.search_mmr(np.ones(DIM + 1, np.float32)),
        lambda: svc.search_mmr_batch(two, 3, filter=["level == 2"]), lambda: svc.search_mmr_batch(two, 3, filter=["level == 2", "level =="]),
        lambda: svc.search_mmr_batch(np.ones((2, 2, DIM), np.float32), 3),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} did not raise")
    assert index.calls == [] and index.made == [] and index.handles == []      # every check came before the index was asked


def test_fetch_k_default_and_the_hits(svc):
    index = load(svc)
    for top_k, want in ((1, 20), (5, 20), (6, 24), (10, 40), (16, 64), (20, 64), (64, 64)):   # min(128, the store's max k = 64, max(20, 4 top_k))
        svc.search_mmr(VEC, top_k)
        assert index.calls[-1]["fetch_k"] == want and index.calls[-1]["k"] == top_k
    svc._index = StubIndex(len(RECORDS), DIM, max_k=128)
    for top_k, want in ((10, 40), (32, 128), (50, 128), (128, 128)):
        svc.search_mmr(VEC, top_k)
        assert svc._index.calls[-1]["fetch_k"] == want
    svc._index = index
    hits = svc.search_mmr(VEC, 4, 10, 0.25, radius=0.1, search_params={"params": {"range_filter": 0.9}})
    call = index.calls[-1]
    assert (call["k"], call["fetch_k"], call["lam"], call["masks"]) == (4, 10, 0.25, None)
    assert call["radius"] == float(np.float32(0.1)) and call["range_filter"] == float(np.float32(0.9))
    assert [h["code"] for h in hits] == ["A00", "A00.0", "A00.1", "A01"]
    assert [h["mmr_score"] for h in hits] == [0.25, 0.24, 0.23, 0.22] and all(type(h["mmr_score"]) is float for h in hits)
    plain = svc._hits_to_dicts(np.float64(np.float32(0.5)) - 0 * np.arange(1), np.float32([0.5]), np.int64([0]))[0]
    assert {k: v for k, v in hits[0].items() if k != "mmr_score"} == plain          # `search`'s dict with one key added
    assert len(svc.search_mmr(VEC, 10, 20)) == len(RECORDS)                         # padding is dropped
    adj, raw, ids, levels, mmr = svc.search_mmr_batch(np.stack([VEC, VEC, VEC]), 2, 5, 1.0)
    assert adj.shape == raw.shape == ids.shape == levels.shape == mmr.shape == (3, 2) and mmr.dtype == np.float64


def test_one_masks_call_and_one_search_per_batch(svc):
    index = load(svc)
    vecs = np.stack([VEC] * 5)
    seen = []
    real = svc._masks_for
    svc._masks_for = lambda idx, flt, nq: (seen.append((flt, nq)), real(idx, flt, nq))[1]
    try:
        filters = ["level == 2", None, 'code like "A01%"', "level == 2", "level > 5"]
        lists = svc.search_mmr_batch(vecs, 3, 6, 0.5, filter=filters, as_dicts=True)
        assert len(seen) == 1 and seen[0] == (filters, 5) and len(index.calls) == 1 and index.calls[0]["nq"] == 5
        masks = index.calls[0]["masks"]
        assert masks[1] is None and masks[0] is masks[3] and index.made == [4, 3, 0]      # equal expressions share a mask, no filter is a NULL entry
        assert len(lists) == 5 and all(len(hits) == 3 for hits in lists)
        svc.search_mmr_batch(vecs, 3, 6, 0.5, filter="level == 1")                        # one expression serves the whole batch
        assert len(seen) == 2 and seen[1] == ("level == 1", 5) and len(index.calls) == 2
        assert len(set(map(id, index.calls[1]["masks"]))) == 1 and index.calls[1]["masks"][0] is not None
        svc.search_mmr_batch(vecs, 3, 6, 0.5)                                             # no filter: no masks at all
        assert len(seen) == 2 and index.calls[2]["masks"] is None
    finally:
        del svc._masks_for
    # the handle is cached per index and dropped with the views on a store change
    assert len(index.handles) == 1 and index.handles[0].max_nq >= 5
    svc._clear_views()
    svc.search_mmr(VEC, 2)
    assert len(index.handles) == 2


def test_masks_are_released_when_the_search_raises(svc):
    index = load(svc)
    own = [StubMask([1, 2], transient=True), None, StubMask([3])]   # a search's own mask, no filter, a cached one
    svc._masks_for = lambda idx, flt, nq: own
    index.fail = RuntimeError("the device said no")
    with pytest.raises(RuntimeError, match="the device said no"):
        svc.search_mmr_batch(np.stack([VEC] * 3), 2, 4, 0.5, filter=["level == 2", None, "level == 1"])
    assert own[0].closed and not own[2].closed and len(index.calls) == 1
    index.fail = None
    own[0] = StubMask([1, 2], transient=True)
    assert len(svc.search_mmr_batch(np.stack([VEC] * 3), 2, 4, 0.5, filter=["level == 2", None, "level == 1"], as_dicts=True)) == 3 and own[0].closed


def test_diverse_query_endpoint():
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod

    class Mil:
        def __init__(self):
            self.seen = []

        def search_mmr(self, vec, top_k=10, fetch_k=None, lambda_mult=0.5, filter=None, radius=None, range_filter=None, search_params=None):   # noqa: A002
            self.seen.append((np.asarray(vec).shape, top_k, fetch_k, lambda_mult, filter, radius, range_filter))
            if filter == "level == 9":
                raise ValueError("fetch_k=99 exceeds the store's max k")
            if filter == "level == 8":
                raise RuntimeError("boom")
            return [{"code": "I21.9", "title": "急性心肌梗死", "score": np.float64(0.96), "original_score": np.float32(0.8), "mmr_score": np.float64(0.4),
                     "metadata": {"level": 1, "parent_code": "I21"}},
                    {"code": "I25.2", "title": None, "score": -0.1, "original_score": -0.1, "mmr_score": -0.3, "metadata": {"level": 2, "parent_code": "I25"}}][:top_k]

        def get_collection_stats(self):
            return {"num_entities": 3}

        def test_connection(self):
            return {"connected": True}

        def disconnect(self):
            return {}

    class Emb:
        def encode_query(self, text):
            return np.ones(DIM, np.float32)

        def get_model_info(self):
            return {"loaded": True, "model_name": "stub"}

    mil = Mil()
    appmod.install_services(Emb(), mil, object())
    try:
        with TestClient(appmod.app) as client:
            r = client.post("/diverse_query", json={"text": "心肌梗死", "top_k": 2, "fetch_k": 30, "lambda_mult": 0.3, "filter": "level >= 1", "radius": 0.1})
            assert r.status_code == 200, r.text
            body = r.json()
            assert mil.seen == [((DIM,), 2, 30, 0.3, "level >= 1", 0.1, None)]
            assert [c["code"] for c in body["candidates"]] == ["I21.9", "I25.2"] and body["extracted_diagnoses"] == ["心肌梗死"]
            first, second = body["candidates"]
            assert first["score"] == 0.96 and first["original_score"] == pytest.approx(0.8) and first["similarity_factors"] == {"mmr_score": 0.4}
            assert first["parent_code"] == "I21" and first["level"] == 1 and second["title"] == ""
            assert second["score"] == 0.0 and second["enhanced_score"] == -0.1              # /hybrid_query's shape: score is non-negative
            assert client.post("/diverse_query", json={"text": "x"}).status_code == 200 and mil.seen[-1][1:4] == (5, None, 0.5)
            n = len(mil.seen)
            for bad in ({"text": ""}, {"text": "  "}, {"text": "x", "top_k": 0}, {"text": "x", "top_k": 51}, {"text": "x", "fetch_k": 4},
                        {"text": "x", "fetch_k": 129}, {"text": "x", "lambda_mult": -0.5}, {"text": "x", "lambda_mult": 1.5},
                        {"text": "x", "filter": "level =="}, {"text": "x", "radius": 0.5, "range_filter": 0.2}):
                assert client.post("/diverse_query", json=bad).status_code == 400, bad
            assert len(mil.seen) == n                                                        # refused before the service was asked
            assert client.post("/diverse_query", json={"text": "x", "filter": "level == 9"}).status_code == 400   # ... and what only the store can judge
            assert client.post("/diverse_query", json={"text": "x", "filter": "level == 8"}).status_code == 500
            assert client.post("/diverse_query", json={}).status_code == 422               # no text at all: the model's own answer
    finally:
        appmod.install_services(None, None, None)
