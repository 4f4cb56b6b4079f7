"""Boosted search without a GPU: the numpy oracle against the masked search's oracle and on constructed
values, the exported symbols and the host-side refusals of the C entry points, BoostRanker's argument checks,
MilvusService.search_boosted / search_boosted_batch / search_boosted_iterator on their host side over a stub index, and the
/boosted_query route over a stub service."""
import ctypes

import numpy as np
import pytest

import boost_oracle as bo
from mask_oracle import masked_batch
from rag_project_icd10_amd import _native
from rag_project_icd10_amd.services import boost_ranker
from rag_project_icd10_amd.services.boost_ranker import BoostRanker


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
def _world(n=300, nq=7, seed=3):
    rng = np.random.default_rng(seed)
    by_row = rng.uniform(-1, 1, (nq, n)).astype(np.float32)
    by_row[:, 10] = by_row[:, 11]                                  # an exact tie: id order decides
    levels = rng.integers(1, 4, n).astype(np.int32)
    order = np.stack([np.lexsort((np.arange(n), -by_row[q].astype(np.float64))) for q in range(nq)])
    s_all, i_all = np.take_along_axis(by_row, order, 1), order.astype(np.int64)
    return by_row, levels, s_all, i_all


def test_no_boost_and_weight_one_are_the_masked_search():
    by_row, levels, s_all, i_all = _world()
    n, nq = by_row.shape[1], len(by_row)
    assert _bits(bo.by_row(s_all, i_all, n)) == _bits(by_row)
    rng = np.random.default_rng(5)
    masks = [None if q % 3 == 0 else rng.random(n) < 0.4 for q in range(nq)]
    some = rng.random(n) < 0.5
    bounds = dict(radius=s_all[:, 200].copy(), range_filter=s_all[:, 20].copy(), after=(s_all[:, 40].copy(), i_all[:, 40].copy()))
    for k in (1, 10, 128):
        for kw in ({}, bounds):
            want = masked_batch(s_all, i_all, levels, masks, k, **kw)
            for boosts in ([None] * nq, [[]] * nq, [[None, None, None, None]] * nq, [[(some, 1.0)]] * nq,
                           [[None, (some, np.float32(1.0)), None, (~some, 1.0)]] * nq):
                got = bo.boosted_batch(by_row, levels, boosts, k, masks=masks, **kw)
                assert all(_bits(g) == _bits(w) for g, w in zip(got[0] + got[1], want[0] + want[1]))


def test_slot_order_is_part_of_the_contract():
    x = np.float32(0.3)
    a, b = (x * bo.W1) * bo.W2, (x * bo.W2) * bo.W1
    assert a.dtype == b.dtype == np.float32 and _bits(a) != _bits(b)            # the constructed pair: the two orders differ in the last bit
    every = np.ones(1, bool)
    assert _bits(bo.boost_scores([x], [(every, bo.W1), (every, bo.W2)])) == _bits(a)
    assert _bits(bo.boost_scores([x], [(every, bo.W2), None, (every, bo.W1)])) == _bits(b)      # a hole keeps the order of the rest
    # on a corpus: many rows differ, and some pair of rows swaps its order
    by_row = _world(4000, 1, 9)[0]
    all_rows = np.ones(by_row.shape[1], bool)
    s12 = bo.boost_scores(by_row[0], [(all_rows, bo.W1), (all_rows, bo.W2)])
    s21 = bo.boost_scores(by_row[0], [(all_rows, bo.W2), (all_rows, bo.W1)])
    assert (s12.view(np.uint32) != s21.view(np.uint32)).mean() > 0.1


def test_edge_values_of_the_ranking():
    sub = np.float32(1e-38) * np.float32(0.01)
    assert sub != 0 and sub < np.finfo(np.float32).tiny                          # numpy keeps subnormal products, as the contract asks
    big = np.float32(3e38)
    scores = np.array([0.5, np.nan, -np.inf, big, -big, 1e-38, -1e-38, 0.25, np.inf], np.float32)
    m = np.ones(len(scores), bool)
    s, i = bo.ranking(bo.boost_scores(scores, [(m, 2.0)]))
    assert i.tolist() == [3, 8, 0, 7, 5, 6] and np.isposinf(s[:2]).all()        # +inf ranks first (ties by id); NaN, -inf and the overflow to -inf are no hits
    s, i = bo.ranking(bo.boost_scores(scores, [(m, 0.01)]))
    assert i.tolist() == [8, 3, 0, 7, 5, 6, 4] and s[4] == sub and s[5] == -sub  # subnormal products stay apart from zero and keep their sign
    tied = np.full(6, 0.5, np.float32)
    s, i = bo.ranking(bo.boost_scores(tied, [([1, 4], 2.0), ([4], 0.5)]))        # a boost breaks a tie, a second one restores it
    assert i.tolist() == [1, 0, 2, 3, 4, 5] and s.tolist() == [1.0, 0.5, 0.5, 0.5, 0.5, 0.5]
    assert bo.boosted_pages(tied, [([5], 1.5)], 4) == [[5, 0, 1, 2], [3, 4]]
    with pytest.raises(AssertionError):
        bo.boost_scores(tied, [None] * 5)


# ---- the C ABI on the host --------------------------------------------------------------------------------------------------------
def test_symbols_and_refusals_that_need_no_device():
    lib = _native.load_library()
    for name in ("icd_boost_create", "icd_boost_destroy", "icd_boost_stats", "icd_index_search_boosted"):
        assert name in _native.EXPORTED_SYMBOLS and getattr(lib, name)
    assert _native.MAX_BOOSTS == bo.MAX_BOOSTS == boost_ranker.MAX_BOOSTS == 4 and lib.icd_abi_version() == 6
    out = ctypes.c_void_p(7)
    assert lib.icd_boost_create(None, 4, None) == -1 and b"out is NULL" in lib.icd_last_error()
    assert lib.icd_boost_create(None, 4, ctypes.byref(out)) == -5 and out.value is None             # an invalid index: STATE, the out handle cleared
    assert lib.icd_boost_destroy(None) == -5 and b"boost" in lib.icd_last_error()
    assert lib.icd_boost_stats(None, None, None) == -5
    q = np.zeros((1, 32), np.float32)
    raw, ids = np.full((1, 4), 7.0, np.float32), np.full((1, 4), 7, np.int64)
    tab, w = np.zeros((1, 4), np.uint64), np.ones((1, 4), np.float32)
    rc = lib.icd_index_search_boosted(None, None, None, tab.ctypes.data, w.ctypes.data, q.ctypes.data, 1, 4, 0, None, None, None, None, 0, 0,
                                      None, raw.ctypes.data, ids.ctypes.data, None, 0, None)
    assert rc == -5 and b"invalid handle" in lib.icd_last_error()
    assert (raw == 7.0).all() and (ids == 7).all()                                                    # a refused call writes nothing


# ---- BoostRanker ------------------------------------------------------------------------------------------------------------------
def test_boost_ranker_argument_checks():
    r = BoostRanker('code like "I%"', 1.5)
    assert (r.filter, r.weight) == ('code like "I%"', 1.5) and "1.5" in repr(r)
    assert BoostRanker("level == 3", 0.1).weight == float(np.float32(0.1))       # the weight is the fp32 value the device multiplies by
    assert BoostRanker("level == 3", np.float32(2)).weight == 2.0 and BoostRanker("level == 3", 3).weight == 3.0
    assert BoostRanker.from_dict({"reranker": "boost", "filter": "level == 1", "weight": 2}).weight == 2.0
    for flt, w in (("level ==", 1.5), ("nope == 1", 1.5), ("", 1.5), ("  ", 1.5), (None, 1.5), (5, 1.5),
                   ("level == 1", 0), ("level == 1", -1.0), ("level == 1", float("nan")), ("level == 1", float("inf")),
                   ("level == 1", 1e-40), ("level == 1", 1e39), ("level == 1", "2"), ("level == 1", None), ("level == 1", True)):
        with pytest.raises(ValueError):
            BoostRanker(flt, w)
    for d in ({"filter": "level == 1"}, {"weight": 2.0}, {"reranker": "decay", "filter": "level == 1", "weight": 2.0}, "level == 1"):
        with pytest.raises(ValueError):
            BoostRanker.from_dict(d)
    a, b = BoostRanker("level == 1", 2.0), BoostRanker("level == 3", 0.5)
    per = boost_ranker.rankers_per_query([a, b], 3)
    assert len(per) == 3 and all(p == [a, b] for p in per)
    per = boost_ranker.rankers_per_query([[a], None, [b, {"filter": "level == 2", "weight": 4}]], 3)
    assert per[0] == [a] and per[1] == [] and per[2][0] is b and per[2][1].weight == 4.0
    assert boost_ranker.rankers_per_query(None, 2) == [[], []] and boost_ranker.rankers_per_query(a, 2) == [[a], [a]]
    for bad in ([[a], [b]], [a] * 5, [[a] * 5, None, None], "level == 1", [a, 3], [[a], None, "x"]):
        with pytest.raises(ValueError):
            boost_ranker.rankers_per_query(bad, 3)


# ---- the service on its host side -------------------------------------------------------------------------------------------------
class StubMask:
    def __init__(self, rows, transient=False):
        self.rows, self.closed, self.transient = len(rows), False, transient

    def stats(self):
        return {"rows": self.rows, "bytes": 0}

    def close(self):
        self.closed = True


class StubWorkspace:
    def __init__(self, max_nq):
        self.max_nq, self.closed = max_nq, False


class StubIndex:
    """IcdIndex as the boosted search sees it: every call is noted; the hits are rows 0 .. k - 1 behind the cursor"""

    def __init__(self, n, dim, max_nq=8, max_k=64):
        self.n, self.dim, self.max_nq, self.max_k, self.device, self.closed = n, dim, max_nq, max_k, 0, False
        self.calls, self.made, self.handles, self.fail = [], [], [], None

    def rowmask(self, rows):
        self.made.append(len(rows))
        return StubMask(rows)

    def boost_workspace(self, max_nq=None):
        self.handles.append(StubWorkspace(max_nq))
        return self.handles[-1]

    def search_boosted(self, queries, k, boosts, masks=None, *, workspace, reweighted=True, radius=None, range_filter=None, after=None):
        q = np.asarray(queries)
        assert q.ndim == 2 and q.shape[1] == self.dim and not workspace.closed and workspace.max_nq >= len(q) and len(boosts) == len(q)
        assert masks is None or len(masks) == len(q)
        self.calls.append(dict(nq=len(q), k=k, boosts=boosts, masks=masks, radius=radius, range_filter=range_filter, after=after, reweighted=reweighted))
        if self.fail is not None:
            raise self.fail
        first = 0 if after is None else int(np.asarray(after[1]).reshape(-1)[0]) + 1
        ids = np.tile(np.arange(first, first + k, dtype=np.int64), (len(q), 1))
        ids[ids >= self.n] = -1
        raw = np.where(ids >= 0, 0.5 - 0.01 * ids, -np.inf).astype(np.float32)
        lv = np.where(ids >= 0, 2, 0).astype(np.int32)
        return (raw.astype(np.float64), raw, ids, lv) if reweighted else (raw, ids, lv)

    def close(self):
        self.closed = True


RECORDS = [{"code": c, "preferred_zh": t, "level": lv, "parent_code": p, "has_complication": False, "main_code": None, "secondary_code": None,
            "category_path": ""}
           for c, t, lv, p in [("A00", "霍乱", 1, ""), ("A00.0", "霍乱，由于O1群霍乱弧菌", 2, "A00"), ("A00.1", "埃尔托霍乱", 2, "A00"),
                               ("A01", "伤寒和副伤寒", 1, ""), ("A01.0", "伤寒", 2, "A01"), ("A01.1", "副伤寒甲", 2, "A01")]]
DIM = 64
VEC = np.ones(DIM, np.float32) / 8


@pytest.fixture()
def svc(tmp_path, monkeypatch):
    monkeypatch.setenv("MILVUS_DB_PATH", str(tmp_path / "db"))
    monkeypatch.setenv("MILVUS_COLLECTION_NAME", "boost")
    from rag_project_icd10_amd.services.milvus_service import MilvusService

    class Emb:
        def encode_query(self, t):
            return VEC

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


def test_service_argument_checks(svc):
    a = BoostRanker("level == 2", 2.0)
    assert svc.search_boosted(VEC, 3, [a]) == [] and svc.search_boosted_batch(np.stack([VEC, VEC]), 3, [a]) == [[], []]   # an empty collection
    assert svc.search_boosted_iterator(VEC, [a]).next() == []
    index = load(svc)
    two = np.stack([VEC, VEC])
    bad = [
        lambda: svc.search_boosted(VEC, 0, [a]), lambda: svc.search_boosted(VEC, 129, [a]), lambda: svc.search_boosted(VEC, 2.5, [a]),
        lambda: svc.search_boosted(VEC, True, [a]), lambda: svc.search_boosted(VEC, 3, [a] * 5), lambda: svc.search_boosted(VEC, 3, [[a]]),
        lambda: svc.search_boosted(VEC, 3, "level == 2"), lambda: svc.search_boosted(VEC, 3, [{"filter": "level ==", "weight": 2}]),
        lambda: svc.search_boosted(VEC, 3, [{"filter": "level == 2", "weight": -2}]),
        lambda: svc.search_boosted(VEC, 3, [a], filter="level =="), lambda: svc.search_boosted(VEC, 3, [a], filter=["level == 2"]),
        lambda: svc.search_boosted(VEC, 3, [a], radius=0.5, range_filter=0.1), lambda: svc.search_boosted(VEC, 3, [a], radius=float("nan")),
        lambda: svc.search_boosted(VEC, 3, [a], offset=-1), lambda: svc.search_boosted(VEC, 3, [a], offset=16384),
        lambda: svc.search_boosted(two, 3, [a]), lambda: svc.search_boosted(np.ones(DIM + 1, np.float32), 3, [a]),
        lambda: svc.search_boosted_batch(two, 3, [[a]]), lambda: svc.search_boosted_batch(two, 3, [a], filter=["level == 2"]),
        lambda: svc.search_boosted_batch(np.ones((2, 2, DIM), np.float32), 3, [a]),
        lambda: svc.search_boosted_iterator(VEC, [a], batch_size=0), lambda: svc.search_boosted_iterator(VEC, [a], batch_size=65),
        lambda: svc.search_boosted_iterator(VEC, [a] * 5), lambda: svc.search_boosted_iterator(VEC, [a], filter=["level == 2"]),
        lambda: svc.search_boosted_iterator(VEC, [a], radius=0.5, range_filter=0.1),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} did not raise")
    assert index.calls == [] and index.made == [] and index.handles == []      # every check came before the index was asked


def test_one_masks_call_and_one_search_per_batch(svc):
    index = load(svc)
    vecs = np.stack([VEC] * 3)
    seen = []
    real = svc._masks_for
    svc._masks_for = lambda idx, flt, nq: (seen.append((list(flt), nq)), real(idx, flt, nq))[1]
    a, b, c = BoostRanker("level == 2", 2.0), BoostRanker('code like "A01%"', 0.5), BoostRanker("level >= 1", 3.0)
    try:
        lists = svc.search_boosted_batch(vecs, 3, [[a, b], None, [b, c]], as_dicts=True, filter=["level == 2", None, "level == 1"])
        assert seen == [(["level == 2", 'code like "A01%"', 'code like "A01%"', "level >= 1", "level == 2", None, "level == 1"], 7)]
        assert len(index.calls) == 1 and len(lists) == 3 and all(len(hits) == 3 for hits in lists)
        call = index.calls[0]
        pairs, masks = call["boosts"], call["masks"]
        assert [len(p) for p in pairs] == [2, 0, 2] and [w for p in pairs for _, w in p] == [2.0, 0.5, 0.5, 3.0]
        assert pairs[0][1][0] is pairs[2][0][0] and masks[0] is pairs[0][0][0] and masks[1] is None          # equal expressions share a mask
        assert pairs[2][1][0].rows == len(RECORDS) and pairs[2][1][0].transient and pairs[2][1][0].closed    # "every row" still gets a mask: the search's own
        assert lists[0][0]["code"] == "A00" and lists[0][0]["original_score"] == pytest.approx(0.5) and lists[0][0]["score"] == pytest.approx(0.5)
        svc.search_boosted_batch(vecs, 2, [a])                                                                # one list serves every query
        assert index.calls[1]["masks"] is None and [len(p) for p in index.calls[1]["boosts"]] == [1, 1, 1]
        adj, raw, ids, lv = svc.search_boosted_batch(vecs, 2, None)
        assert adj.shape == raw.shape == ids.shape == lv.shape == (3, 2) and adj.dtype == np.float64
        hits = svc.search_boosted(VEC, 2, [a], filter="level == 2", radius=0.1, offset=3, search_params={"params": {"range_filter": 0.9}})
        call = index.calls[-1]
        assert call["k"] == 5 and call["radius"] == float(np.float32(0.1)) and call["range_filter"] == float(np.float32(0.9))
        assert [h["code"] for h in hits] == ["A01", "A01.0"]                                                  # ranks 3 and 4 of the boosted ranking
    finally:
        del svc._masks_for
    assert len(index.handles) == 1 and index.handles[0].max_nq >= 3                # the workspace is cached per index ...
    svc._clear_views()
    svc.search_boosted(VEC, 2, [a])
    assert len(index.handles) == 2                                                 # ... and dropped with the views on a store change


def test_iterator_pages_and_released_masks(svc):
    index = load(svc)
    it = svc.search_boosted_iterator(VEC, [BoostRanker("level == 2", 2.0)], batch_size=4, filter="level >= 1")
    pages = [[h["code"] for h in it.next()] for _ in range(3)]
    assert pages == [["A00", "A00.0", "A00.1", "A01"], ["A01.0", "A01.1"], []]
    assert [c["after"] is None for c in index.calls] == [True, False] and int(index.calls[1]["after"][1]) == 3
    assert all(not c["reweighted"] and len(c["boosts"]) == 1 for c in index.calls)
    own = [StubMask([1, 2], transient=True), StubMask([3])]
    svc._masks_for = lambda idx, flt, nq: list(own)
    index.fail = RuntimeError("the device said no")
    with pytest.raises(RuntimeError, match="the device said no"):
        svc.search_boosted_batch(VEC.reshape(1, -1), 2, [BoostRanker("level == 2", 2.0)], filter="level == 1")
    assert own[0].closed and not own[1].closed


def test_boosted_query_endpoint():
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod

    class Mil:
        def __init__(self):
            self.seen = []

        def search_boosted_batch(self, vecs, top_k=10, boosts=None, as_dicts=False, filter=None, **kw):   # noqa: A002
            self.seen.append((np.asarray(vecs).shape, top_k, [(b.filter, b.weight) for b in boosts], as_dicts, filter))
            if filter == "level == 9":
                raise ValueError("query dim 64 != index dim 768")
            if filter == "level == 8":
                raise RuntimeError("boom")
            hit = lambda code, s, raw: {"code": code, "title": None if code == "I25.2" else "t", "score": s, "original_score": raw,   # noqa: E731
                                        "metadata": {"level": 1, "parent_code": code[:3]}}
            return [[hit("I21.9", 0.96, 0.8), hit("I25.2", -0.1, -0.1)][:top_k] for _ in range(len(vecs))]

    class Emb:
        def encode_query(self, t):
            return VEC

    mil = Mil()
    appmod.install_services(Emb(), mil, object())
    try:
        with TestClient(appmod.app) as client:
            r = client.post("/boosted_query", json={"texts": ["心肌梗死", "胸痛"], "top_k": 2, "filter": "level >= 1",
                                                    "boosts": [{"filter": 'code like "I%"', "weight": 1.5}, {"filter": "level == 3", "weight": 0.5}]})
            assert r.status_code == 200, r.text
            body = r.json()
            assert mil.seen == [((2, DIM), 2, [('code like "I%"', 1.5), ("level == 3", 0.5)], True, "level >= 1")]
            assert [c["code"] for c in body["candidates"]] == ["I21.9", "I25.2"] and body["extracted_diagnoses"] == ["心肌梗死", "胸痛"]
            assert body["is_multi_diagnosis"] is True and [m["diagnosis_text"] for m in body["diagnosis_matches"]] == ["心肌梗死", "胸痛"]
            first, second = body["candidates"]
            assert first["score"] == 0.96 and first["original_score"] == pytest.approx(0.8) and first["parent_code"] == "I21" and second["title"] == ""
            assert second["score"] == 0.0 and second["enhanced_score"] == -0.1               # /diverse_query's shape: score is non-negative
            assert client.post("/boosted_query", json={"texts": ["x"]}).status_code == 200 and mil.seen[-1][1:3] == (5, [])
            n = len(mil.seen)
            ok = {"filter": "level == 1", "weight": 2.0}
            for bad in ({"texts": []}, {"texts": [""]}, {"texts": ["x"] * 17}, {"texts": ["x"], "top_k": 0}, {"texts": ["x"], "top_k": 51},
                        {"texts": ["x"], "boosts": [ok] * 5}, {"texts": ["x"], "boosts": [{"filter": "level ==", "weight": 2.0}]},
                        {"texts": ["x"], "boosts": [{"filter": "level == 1", "weight": 0.0}]}, {"texts": ["x"], "boosts": [{"filter": "level == 1", "weight": -1}]},
                        {"texts": ["x"], "filter": "level =="}):
                assert client.post("/boosted_query", json=bad).status_code == 400, bad
            assert len(mil.seen) == n                                                         # refused before the service was asked
            assert client.post("/boosted_query", json={"texts": ["x"], "filter": "level == 9"}).status_code == 400   # ... and what only the store can judge
            assert client.post("/boosted_query", json={"texts": ["x"], "filter": "level == 8"}).status_code == 500
            assert client.post("/boosted_query", json={}).status_code == 422                # no texts at all: the model's own answer
            assert client.post("/boosted_query", json={"texts": ["x"], "boosts": [{"filter": "level == 1"}]}).status_code == 422
    finally:
        appmod.install_services(None, None, None)
