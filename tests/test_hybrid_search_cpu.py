"""Hybrid search, the parts that need no GPU: the oracle (tests/hybrid_oracle.py) against a dictionary-based brute force, rule 7's
identities on the oracle, the request and ranker classes' ValueErrors, the argument checks of MilvusService and /hybrid_query,
the exported symbols and the library's checks that come before any device call."""
import ctypes
import math

import numpy as np
import pytest

from hybrid_oracle import brute_force, fuse_query, hybrid_batch, sub_list

from rag_project_icd10_amd import _native
from rag_project_icd10_amd.services.hybrid_search import (AnnSearchRequest, RRFRanker, WeightedRanker, check_requests,
                                                          ranker_from_dict, stack_requests)


def _tiny(n=200, dim=16, nv=24, seed=11):
    """200 x 16 random rows (well separated: a float64 dot product rounded to fp32 ranks them as any summation order does) and a
    pool of vectors: noisy copies of rows, so that requests built from neighbouring pool entries overlap partially"""
    rng = np.random.default_rng(seed)
    corpus = rng.standard_normal((n, dim)).astype(np.float32)
    base = corpus[rng.integers(0, n, nv // 4)]
    pool = (np.repeat(base, 4, axis=0) + 0.3 * rng.standard_normal((nv, dim))).astype(np.float32)
    levels = rng.integers(1, 4, n).astype(np.int32)
    sc = (corpus.astype(np.float64) @ pool.astype(np.float64).T).T.astype(np.float32)
    order = np.stack([np.lexsort((np.arange(n), -sc[i])) for i in range(nv)])
    return corpus, pool, levels, np.take_along_axis(sc, order, 1), order.astype(np.int64)


@pytest.mark.parametrize("ranker,kw", [("rrf", {}), ("rrf", {"c": 0.5}), ("weighted", {"weights": [1.0, 0.5, 0.25, 0.0], "norm": "none"}),
                                       ("weighted", {"weights": [0.9, 0.8, 0.7, 0.6], "norm": "cosine"}),
                                       ("weighted", {"weights": [0.3, 1.0, 0.2, 0.1], "norm": "atan"})])
def test_oracle_against_a_dictionary_brute_force(ranker, kw):
    corpus, pool, levels, s_all, i_all = _tiny()
    n = len(corpus)
    rows = np.arange(n)
    for R, limits, k in ((1, [10], 5), (2, [10, 3], 10), (3, [7, 64, 1], 128), (4, [128, 128, 128, 128], 30)):
        kwr = dict(kw)
        if "weights" in kwr:
            kwr["weights"] = kwr["weights"][:R]
        sel = np.array([[(4 * q + r) % len(pool) for r in range(R)] for q in range(6)])
        masks = [[None if (q + r) % 3 else rows % 5 == r for r in range(R)] for q in range(6)]
        (f, ids, lv, bits), (adj, f2, ids2, lv2, bits2) = hybrid_batch(s_all, i_all, levels, sel, limits, k, ranker, masks=masks, **kwr)
        for q in range(6):
            want = brute_force(corpus, pool[sel[q]], limits, k, ranker, rows=[None if m is None else np.nonzero(m)[0] for m in masks[q]], **kwr)
            m = len(want)
            assert ids[q, :m].tolist() == [i for i, _ in want] and (ids[q, m:] == -1).all()
            assert np.isneginf(f[q, m:]).all() and (lv[q, m:] == 0).all() and (bits[q, m:] == 0).all()
            if ranker == "rrf":
                assert f[q, :m].tolist() == [v for _, v in want]          # ranks only: bit for bit
            else:
                assert np.allclose(f[q, :m], [v for _, v in want], rtol=0, atol=1e-6)
            assert np.array_equal(lv[q, :m], levels[ids[q, :m]])
            # reweighted: the same hits with their tags, adjusted scores descending, stable
            assert sorted(zip(ids2[q, :m].tolist(), bits2[q, :m].tolist())) == sorted(zip(ids[q, :m].tolist(), bits[q, :m].tolist()))
            assert (np.diff(adj[q, :m]) <= 0).all() and np.isneginf(adj[q, m:]).all()
            w = np.array([{1: 1.2, 3: 0.8}.get(int(x), 1.0) for x in lv2[q, :m]])
            assert np.array_equal(adj[q, :m], f2[q, :m] * w)


def test_rule_7_identities_on_the_oracle():
    corpus, pool, levels, s_all, i_all = _tiny()
    for p in range(4):
        s, i = sub_list(s_all[p], i_all[p], 20)
        (f, ids, _lv, bits), _ = fuse_query([(s, i)], levels, 20, "rrf", c=60)
        assert np.array_equal(ids, i) and f.tolist() == [1.0 / (60 + j + 1) for j in range(20)] and (bits == 1).all()
        (f, ids, _lv, _b), _ = fuse_query([(s, i)], levels, 20, "weighted", weights=[1.0], norm="none")
        assert np.array_equal(ids, i) and np.array_equal(f, s.astype(np.float64))
        for R in (2, 3, 8):
            (f, ids, _lv, bits), _ = fuse_query([(s, i)] * R, levels, 20, "rrf", c=60)
            want = []
            for j in range(20):
                acc = 0.0
                for _ in range(R):
                    acc = acc + 1.0 / (60 + j + 1)
                want.append(acc)
            assert np.array_equal(ids, i) and f.tolist() == want and (bits == (1 << R) - 1).all()
    # disjoint lists: every rank ties R ways and the id decides
    a, b = (s_all[0][:5], np.array([9, 7, 5, 3, 1])), (s_all[1][:5], np.array([0, 2, 4, 6, 8]))
    (f, ids, _lv, bits), _ = fuse_query([a, b], levels, 10, "rrf")
    assert ids.tolist() == [0, 9, 2, 7, 4, 5, 3, 6, 1, 8] and bits.tolist() == [2, 1] * 2 + [2, 1, 1, 2, 1, 2]
    # k above the distinct ids: padding
    (f, ids, lv, bits), (adj, *_rest) = fuse_query([a, a], levels, 8, "rrf")
    assert (ids[5:] == -1).all() and np.isneginf(f[5:]).all() and np.isneginf(adj[5:]).all() and (lv[5:] == 0).all() and (bits[5:] == 0).all()
    # a band and a mask shorten a sub-list; an empty one contributes nothing
    s, i = sub_list(s_all[0], i_all[0], 10, mask=np.arange(len(corpus)) < 3)
    assert len(i) == 3 and set(i.tolist()) == {0, 1, 2}
    s, i = sub_list(s_all[0], i_all[0], 10, radius=float(s_all[0][4]))
    assert len(i) == 4
    assert len(sub_list(s_all[0], i_all[0], 10, mask=np.zeros(len(corpus), bool))[1]) == 0


def test_request_and_ranker_classes_raise_value_errors():
    v = np.zeros(8, np.float32)
    for bad in (0, -1, 129, 1.5, "10", None, True):
        with pytest.raises(ValueError):
            AnnSearchRequest(v, bad)
    with pytest.raises(ValueError):
        AnnSearchRequest(v, 10, expr="level >")
    with pytest.raises(ValueError):
        AnnSearchRequest(v, 10, expr=5)
    with pytest.raises(ValueError):
        AnnSearchRequest(v, 10, param="radius")
    with pytest.raises(ValueError):
        AnnSearchRequest(v, 10, param={"params": {"radius": 0.9, "range_filter": 0.1}})
    r = AnnSearchRequest(v, 128, expr="level >= 2", param={"metric_type": "IP", "params": {"radius": 0.25}})
    assert (r.limit, r.expr, r.radius, r.range_filter) == (128, "level >= 2", 0.25, None)
    for bad in (0, -1, 16384, float("nan"), "60", None, True):
        with pytest.raises(ValueError):
            RRFRanker(bad)
    assert RRFRanker().k == 60.0 and RRFRanker(0.5).k == 0.5
    for bad in ((), (1.5,), (-0.1, 0.5), (float("nan"),), ("a",), (True,)):
        with pytest.raises(ValueError):
            WeightedRanker(*bad)
    with pytest.raises(ValueError):
        WeightedRanker(0.5, norm_score="l2")
    w = WeightedRanker(0.25, 1, 0)
    assert w.weights == [0.25, 1.0, 0.0] and w.norm_score == "atan"
    assert WeightedRanker(1, norm_score=False).norm_score == "none" and WeightedRanker(1, norm_score=True).norm_score == "atan"
    assert ranker_from_dict({"strategy": "rrf", "params": {"k": 10}}).k == 10.0
    assert ranker_from_dict(w.dict()).weights == w.weights
    for bad in (None, {}, {"strategy": "max"}, {"strategy": "weighted"}, {"strategy": "rrf", "params": {"k": 0}}):
        with pytest.raises(ValueError):
            ranker_from_dict(bad)
    reqs = [AnnSearchRequest(v, 10), AnnSearchRequest(v, 5)]
    assert check_requests(reqs, RRFRanker(), 10) == 10
    for args in (([], RRFRanker(), 10), (reqs * 5, RRFRanker(), 10), (reqs, WeightedRanker(0.5), 10), (reqs, "rrf", 10),
                 (reqs, RRFRanker(), 0), (reqs, RRFRanker(), 129), ([v, v], RRFRanker(), 10), (reqs[0], RRFRanker(), 10)):
        with pytest.raises(ValueError):
            check_requests(*args)
    assert stack_requests(reqs).shape == (1, 2, 8)
    with pytest.raises(ValueError):
        stack_requests([AnnSearchRequest(v, 10), AnnSearchRequest(np.zeros((2, 8), np.float32), 5)])


def test_library_exports_the_fusion_symbols_and_checks_before_any_device_call():
    lib = _native.load_library()
    for name in ("icd_fusion_create", "icd_fusion_destroy", "icd_fusion_stats", "icd_index_search_hybrid"):
        assert hasattr(lib, name) and name in _native.EXPORTED_SYMBOLS, name
    assert lib.icd_abi_version() == 6 == _native.ABI_VERSION
    assert hasattr(_native.IcdIndex, "fusion") and hasattr(_native.IcdIndex, "search_hybrid") and hasattr(_native, "IcdFusion")
    out = ctypes.c_void_p()
    assert lib.icd_fusion_create(None, 16, ctypes.byref(out)) == -5 and not out.value      # ICD_ERR_STATE: no index
    assert lib.icd_fusion_destroy(None) == -5 and lib.icd_fusion_stats(None, None, None) == -5
    q = np.zeros((1, 2, 64), np.float32)
    lim = np.array([5, 5], np.int32)
    assert lib.icd_index_search_hybrid(None, None, q.ctypes.data, 1, 2, 0, lim.ctypes.data, None, None, None, 0, 0, 0, 60.0, None, 0,
                                       5, 0, None, None, None, None, None, 0, None) == -5


def test_milvus_service_hybrid_argument_checks_need_no_device(tmp_path, monkeypatch):
    monkeypatch.setenv("MILVUS_DB_PATH", str(tmp_path / "db"))
    monkeypatch.setenv("MILVUS_COLLECTION_NAME", "h")
    from rag_project_icd10_amd.services.milvus_service import MilvusService

    class Emb:
        def encode_query(self, t):
            return np.ones(64, np.float32) / 8

    svc = MilvusService(Emb())
    recs = [{"code": c, "preferred_zh": c, "level": lv, "main_code": None, "secondary_code": None} for c, lv in (("A00", 1), ("A00.1", 2), ("B01", 2))]
    assert svc.insert_records(recs, [np.ones(64, np.float32) * (i + 1) for i in range(3)]) is True

    def no_device(*a, **k):
        raise AssertionError("an argument error must be raised before the index is loaded")
    monkeypatch.setattr(svc, "_ready_index", no_device)
    v = np.ones(64, np.float32)
    reqs = [AnnSearchRequest(v, 2), AnnSearchRequest(v, 2, expr="level >= 2")]
    bad = [([], RRFRanker(), 2), (reqs * 5, RRFRanker(), 2), (reqs, WeightedRanker(1.0), 2), (reqs, None, 2), (reqs, RRFRanker(), 0),
           (reqs, RRFRanker(), 200), ([v], RRFRanker(), 2),
           ([AnnSearchRequest(v, 2), AnnSearchRequest(np.ones((2, 64), np.float32), 2)], RRFRanker(), 2)]
    for args in bad:
        with pytest.raises(ValueError):
            svc.hybrid_search(*args)
        with pytest.raises(ValueError):
            svc.hybrid_search_batch(*args)
    with pytest.raises(ValueError):
        svc.hybrid_search([AnnSearchRequest(np.ones((2, 64), np.float32), 2)], RRFRanker(), 2)   # a batch needs hybrid_search_batch
    with pytest.raises(AssertionError, match="before the index is loaded"):
        svc.hybrid_search(reqs, RRFRanker(), 2)                                                  # good arguments get as far as the index
    assert svc.fusions() == []


def test_hybrid_query_endpoint_argument_checks():
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod

    class Emb:
        def __init__(self):
            self.calls = []

        def encode_query_batch(self, qs, **kw):
            self.calls.append(list(qs))
            return np.zeros((len(qs), 2), np.float32)

        def get_model_info(self):
            return {"loaded": True, "model_name": "stub"}

    class Mil:
        def __init__(self):
            self.seen = []

        def hybrid_search(self, reqs, ranker, limit):
            self.seen.append((reqs, ranker, limit))
            return [{"code": "I21.9", "title": "t", "score": 0.03, "fused_score": 0.03, "matched_requests": [0, 1],
                     "metadata": {"level": 2, "parent_code": "I21"}}][:limit]

        def fusions(self):
            return [{"max_total": 64, "generation": 1, "bytes": 4096}]

        def get_collection_stats(self):
            return {"num_entities": 3}

        def test_connection(self):
            return {"connected": True}

        def disconnect(self):
            return {}

    emb, mil = Emb(), Mil()
    appmod.install_services(emb, mil)
    try:
        with TestClient(appmod.app) as client:
            good = {"texts": ["心肌梗死", "myocardial infarction"], "top_k": 1}
            for patch in ({"texts": []}, {"texts": ["a"] * 9}, {"texts": ["a", " "]}, {"ranker": {"strategy": "max"}},
                          {"ranker": {"strategy": "rrf", "params": {"k": 0}}}, {"ranker": {"strategy": "weighted", "params": {"weights": [0.5]}}},
                          {"ranker": {"strategy": "weighted", "params": {"weights": [0.5, 1.5]}}}, {"req_limit": 0}, {"req_limit": 129},
                          {"top_k": 0}, {"top_k": 51},
                          {"filter": "level >"}):
                r = client.post("/hybrid_query", json={**good, **patch})
                assert r.status_code == 400, (patch, r.status_code, r.text)
            assert mil.seen == [] and emb.calls == []
            r = client.post("/hybrid_query", json={**good, "ranker": {"strategy": "weighted", "params": {"weights": [0.7, 0.3], "norm_score": "none"}},
                                                   "req_limit": 7, "filter": "level >= 2"})
            assert r.status_code == 200, r.text
            assert emb.calls == [good["texts"]]                                       # ONE encode call for all phrasings
            reqs, ranker, limit = mil.seen[-1]
            assert [x.limit for x in reqs] == [7, 7] and [x.expr for x in reqs] == ["level >= 2"] * 2 and limit == 1
            assert ranker.weights == [0.7, 0.3] and ranker.norm_score == "none"
            body = r.json()
            assert body["candidates"][0]["code"] == "I21.9" and body["candidates"][0]["original_score"] == 0.03
            assert body["candidates"][0]["enhanced_score"] == 0.03 and body["candidates"][0]["similarity_factors"] == {"matched_requests": [0, 1]}
            assert body["extracted_diagnoses"] == [good["texts"][0]] and body["diagnosis_matches"] == [] and body["is_multi_diagnosis"] is False
            # a ValueError only the store can raise (a limit above its max_k) is a 400 too; a negative weighted score is not hidden
            mil.hybrid_search = lambda reqs, ranker, limit: (_ for _ in ()).throw(ValueError("a request's limit exceeds the index's max_k"))
            r = client.post("/hybrid_query", json=good)
            assert r.status_code == 400 and "max_k" in r.json()["detail"]
            mil.hybrid_search = lambda reqs, ranker, limit: [{"code": "A00", "title": "t", "score": -0.25, "fused_score": -0.3125,
                                                              "matched_requests": [1], "metadata": {"level": 3}}]
            c = client.post("/hybrid_query", json=good).json()["candidates"][0]
            assert (c["score"], c["enhanced_score"], c["original_score"]) == (0.0, -0.25, -0.3125)
            del mil.hybrid_search
            assert client.post("/hybrid_query", json=good).status_code == 200         # the default ranker: RRF, k = 60
            assert mil.seen[-1][1].k == 60.0
            assert client.get("/stats").json()["fusions"] == mil.fusions()
    finally:
        appmod.install_services(None, None, None)
    assert math.isclose(1.0 / 61, 1.0 / (60.0 + 0 + 1))


@pytest.mark.parametrize("id_base", [1000, 2**32 + 12345])
@pytest.mark.parametrize("ranker,kw", [("rrf", {}), ("weighted", {"weights": [1.0, 0.5, 0.25], "norm": "none"}),
                                       ("weighted", {"weights": [0.9, 0.8, 0.7], "norm": "cosine"})])
def test_a_ranking_shifted_by_id_base_gives_the_same_outputs_with_the_ids_shifted(ranker, kw, id_base):
    corpus, pool, levels, s_all, i_all = _tiny()
    n = len(corpus)
    rows = np.arange(n)
    R, limits = 3, [7, 64, 1]
    sel = np.array([[(4 * q + r) % len(pool) for r in range(R)] for q in range(6)])
    masks = [[None if (q + r) % 3 else rows % 5 == r for r in range(R)] for q in range(6)]   # masks stay over ROWS
    lo = np.full((6, R), -np.inf, np.float32)
    lo[:, 1] = s_all[sel[:, 1], 30]
    shift = lambda a: np.where(a >= 0, a + id_base, a)
    for k in (5, 128):
        for extra in (dict(), dict(masks=masks), dict(masks=masks, radius=lo)):
            want = hybrid_batch(s_all, i_all, levels, sel, limits, k, ranker, **kw, **extra)
            got = hybrid_batch(s_all, i_all + id_base, levels, sel, limits, k, ranker, id_base=id_base, **kw, **extra)
            for j, (g, w) in enumerate(zip(got[0] + got[1], want[0] + want[1])):
                assert g.dtype == w.dtype and g.tobytes() == (shift(w) if w.dtype == np.int64 else w).tobytes(), (k, sorted(extra), j)
    lists = [sub_list(s_all[p], i_all[p], 10) for p in (0, 1)]
    moved = [(s, i + id_base) for s, i in lists]
    kw2 = {**kw, "weights": kw["weights"][:2]} if kw else {}
    want = fuse_query(lists, levels, 10, ranker, **kw2)
    got = fuse_query(moved, levels, 10, ranker, id_base=id_base, **kw2)
    for g, w in zip(got[0] + got[1], want[0] + want[1]):
        assert g.tobytes() == (shift(w) if w.dtype == np.int64 else w).tobytes()


def test_fuse_params_normalises_limits_ranker_norm_and_weights_without_a_library():
    """_native._fuse_params, what search_hybrid and fuse_lists share in front of the C call: search_hybrid's messages, no library"""
    lim, wts, fuse = _native._fuse_params(7, 3, "rrf", 60, [0.5, "not read"], "atan")   # (weights is ignored for "rrf")
    assert lim.dtype == np.int32 and lim.flags.c_contiguous and lim.tolist() == [7, 7, 7] and wts is None
    assert fuse == (_native.RANKER_RRF, 60.0, None, _native.NORMS["atan"]) and isinstance(fuse[1], float)
    lim, wts, fuse = _native._fuse_params([3, 1], 2, "weighted", 60.0, (0.25, 1), "cosine")
    assert lim.tolist() == [3, 1] and wts.dtype == np.float64 and wts.flags.c_contiguous and wts.tolist() == [0.25, 1.0]
    assert fuse == (_native.RANKER_WEIGHTED, 60.0, wts.ctypes.data, _native.NORMS["cosine"])
    for args, text in ((([3, 1], 3, "rrf", 60.0, None, "none"), "limits holds 2 entries for 3 requests"),
                       ((4, 2, "max", 60.0, None, "none"), "ranker='max': 'rrf' or 'weighted'"),
                       ((4, 2, "rrf", 60.0, None, "l2"), f"norm='l2': one of {sorted(_native.NORMS)}"),
                       ((4, 2, "weighted", 60.0, [0.5], "none"), "weights holds 1 entries for 2 requests"),
                       (([3, 1], 3, "max", 60.0, None, "l2"), "limits holds 2 entries for 3 requests")):   # (limits first, then the ranker)
        with pytest.raises(ValueError) as err:
            _native._fuse_params(*args)
        assert str(err.value) == text
