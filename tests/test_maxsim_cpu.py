"""Embedding-list search without a GPU: tests/maxsim_oracle.py against a brute force over all rows and on
the identities of the contract's rule 6, the plan of the passes under the host sanitizers, the ABI's symbols and header, and the
argument refusals of IcdIndex.search_lists and the service that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, unit_rows
from group_scorer_oracle import ScoredRanking
from grouped_oracle import Ranking
from maxsim_oracle import ListRanking, brute_force, expected, order_sensitive_share

from rag_project_icd10_amd import _native

CSRC = os.path.join(ROOT, "rag_project_icd10_amd", "csrc")


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _case(oracle, n=90, nv=23, groups=11, seed=3):
    corpus, q = unit_rows(n, 32, seed), unit_rows(nv, 32, seed + 1)
    corpus[5] = corpus[40]                                     # duplicated rows: tied scores, the row decides
    corpus[7, 0] = np.nan                                      # a row that is no hit for any vector
    group_of = (np.arange(n) * 7 + 3) % groups * 5 + 2
    group_of[7] = 999                                          # ... alone in its group
    s_all, i_all = oracle.flat_ip_topk(corpus, q, n)
    with np.errstate(invalid="ignore"):
        S = np.stack([[np.float32(np.nan) if r == 7 else s_all[t][list(i_all[t]).index(r)] for r in range(n)] for t in range(nv)])
    return corpus, q, group_of, s_all, i_all, S.astype(np.float32)


def test_oracle_against_a_brute_force_over_all_rows(oracle):
    corpus, q, group_of, s_all, i_all, S = _case(oracle)
    list_off = np.array([0, 1, 3, 6, 11, 23])
    rk = Ranking(s_all, i_all, group_of)
    for scorer in ("sum", "mean"):
        for k in (1, 4, 12, 20):
            got = ListRanking(rk, list_off, scorer).outputs(k)
            want = brute_force(S, group_of, list_off, k, scorer)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and _bits(g) == _bits(w), (scorer, k)
    gid = ListRanking(rk, list_off).outputs(20)[1]
    assert len(np.unique(group_of)) == 12                                                     # 11 groups with hits, and group 999
    assert (gid != 999).all() and (gid[:, 11:] == -1).all() and (gid[:, :11] >= 0).all()      # ... whose only row is no hit


def test_rule_6_identities(oracle):
    corpus, q, group_of, s_all, i_all, _S = _case(oracle)
    nv = len(q)
    rk = Ranking(s_all, i_all, group_of)
    levels = (np.arange(len(corpus)) % 3 + 1).astype(np.int32)
    for k in (1, 5, 20):
        # lists of one vector each: the grouped search under scorer MAX at group_size 1
        gsc, gid, msc, mid, mlv = expected(rk, np.arange(nv + 1), levels, k)
        sc, ids, grp, wsc, wid = ScoredRanking(rk, 1, "max").raw(k)
        assert _bits(gsc) == _bits(wsc) and _bits(gid) == _bits(wid) and _bits(msc) == _bits(sc) and _bits(mid) == _bits(ids)
        assert _bits(mlv) == _bits(np.where(ids >= 0, levels[np.clip(ids, 0, None)], 0).astype(np.int32))
        # MEAN at T = 1 is SUM
        for a, b in zip(expected(rk, np.arange(nv + 1), levels, k, "mean"), (gsc, gid, msc, mid, mlv)):
            assert _bits(a) == _bits(b)
        # [v, v]: the groups of [v], aggregates x + x, both vectors' matches those of [v]
        twice = Ranking(np.repeat(s_all, 2, axis=0), np.repeat(i_all, 2, axis=0), group_of)
        dsc, did, dms, dmi, _lv = expected(twice, np.arange(0, 2 * nv + 1, 2), levels, k)
        assert _bits(did) == _bits(gid) and _bits(dsc) == _bits((gsc + gsc).astype(np.float32))
        assert _bits(dms) == _bits(np.repeat(msc, 2, axis=0)) and _bits(dmi) == _bits(np.repeat(mid, 2, axis=0))
        # the mean of [v, v] is x again
        assert _bits(expected(twice, np.arange(0, 2 * nv + 1, 2), levels, k, "mean")[0]) == _bits(gsc)
    # a view with an id_base: the parent's ids and levels
    rows = np.arange(0, len(corpus), 2)
    vs, vi = oracle.flat_ip_topk(corpus[rows], q, len(rows))
    out = expected(Ranking(vs, vi, group_of[rows]), [0, 3, nv], np.arange(len(corpus)), 4, row_map=rows, id_base=2**32 + 77)
    hit = out[3] >= 0
    assert ((out[3][hit] - (2**32 + 77)) % 2 == 0).all() and (out[4][hit] == out[3][hit] - (2**32 + 77)).all() and (out[4][~hit] == 0).all()


def test_the_order_of_the_chain_matters(oracle):
    corpus, q = unit_rows(400, 32, 11), unit_rows(3 + 5 + 64, 32, 12)
    s_all, i_all = oracle.flat_ip_topk(corpus, q, 400)
    rk = Ranking(s_all, i_all, np.arange(400) % 60)
    share, total = order_sensitive_share(rk, [0, 3, 8, 72], 10)
    assert total == 30 and share >= 0.10, share
    assert order_sensitive_share(rk, [0, 3, 8, 72], 10, min_t=6)[1] == 10


def test_abi_symbols_argtypes_and_header():
    lib = _native.load_library()
    for name in ("icd_grouping_prepare_maxsim", "icd_index_search_maxsim"):
        assert hasattr(lib, name) and name in _native.EXPORTED_SYMBOLS
    assert lib.icd_abi_version() == _native.ABI_VERSION == 6
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert lib.icd_grouping_prepare_maxsim.argtypes == [vp, vp, i64, i64]
    assert list(lib.icd_index_search_maxsim.argtypes) == [vp, vp, vp, vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp]
    assert _native.MAXSIM_SCORERS == {"sum": 1, "mean": 2} and _native.MAXSIM_MAX_T == 64
    header = open(os.path.join(ROOT, "include", "icd_search.h"), encoding="utf-8").read()
    for line in ("#define ICD_ABI_VERSION 6", "#define ICD_MAXSIM_SUM 1", "#define ICD_MAXSIM_MEAN 2", "#define ICD_MAXSIM_MAX_T 64",
                 "int icd_grouping_prepare_maxsim(icd_index *idx, icd_grouping *grouping, int64_t max_lists, int64_t max_vectors);",
                 "int icd_index_search_maxsim(icd_index *idx, icd_grouping *grouping, const float *queries, const int64_t *list_off, int64_t nl, int32_t k,"):
        assert line in header, line
    plan = open(os.path.join(CSRC, "maxsim_plan.hpp"), encoding="utf-8").read()
    assert "MAXSIM_MAX_T = 64" in plan and "MAXSIM_SUM = 1, MAXSIM_MEAN = 2" in plan


def test_maxsim_plan_under_the_sanitizers(tmp_path):
    """tests/maxsim_plan_check.cpp: every vector and list in exactly one pass, no pass above the block or across a list, lists that
    end at B, B - 1 and B + 1, a list of 64 that does not fit, one list, empty input refused - with ASan and UBSan"""
    exe = str(tmp_path / "maxsim_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "maxsim_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "maxsim plan ok" in out.stdout


class _NoGrouping:
    closed, maxsim, max_nq = False, None, 8

    def prepare_maxsim(self, *a):
        raise AssertionError("a refused call must not prepare the grouping")


def test_search_lists_refuses_bad_arguments_before_any_device_call():
    index = _native.IcdIndex.__new__(_native.IcdIndex)      # a handle that counts as open and no library: a call that reaches it fails
    index._h, index._lib, index.dim, index.device = C.c_void_p(1), None, 8, 0
    q = np.zeros((5, 8), np.float32)
    g = _NoGrouping()
    for bad_off in ([0, 2, 2, 5], [0, 6], [1, 5], [0, 3], [0, 5, 3, 5], [[0, 5]], [], [0.0, 5.0], list(range(0, 5)) + [70]):
        with pytest.raises(ValueError, match="list_off"):
            index.search_lists(q, bad_off, 3, g)
    with pytest.raises(ValueError, match="list_off"):
        index.search_lists(np.zeros((65, 8), np.float32), [0, 65], 3, g)             # a list of 65
    for k in (0, -1, 129):
        with pytest.raises(ValueError, match="k="):
            index.search_lists(q, [0, 2, 5], k, g)
    for scorer in ("max", "avg", "SUM", None, 1):
        with pytest.raises(ValueError, match="scorer"):
            index.search_lists(q, [0, 2, 5], 3, g, scorer=scorer)
    with pytest.raises(ValueError, match="need"):
        index.search_lists(np.zeros((5, 9), np.float32), [0, 2, 5], 3, g)            # another dim
    closed = _NoGrouping()
    closed.closed = True
    with pytest.raises(_native.IcdError):
        index.search_lists(q, [0, 2, 5], 3, closed)
    assert _native.check_list_offsets(np.array([0, 64, 65], np.int32), 65).dtype == np.int64
    with pytest.raises(ValueError, match="max_lists"):
        _native.IcdGrouping.prepare_maxsim(g, index, 0, 64)
    with pytest.raises(ValueError, match="max_vectors"):
        _native.IcdGrouping.prepare_maxsim(g, index, 4, 63)
    index._h = C.c_void_p()      # (closed again: nothing is destroyed when the object goes)


def test_the_service_checks_its_arguments_before_anything_runs():
    from rag_project_icd10_amd.services.milvus_service import MilvusService
    ms = MilvusService.__new__(MilvusService)      # (nothing of it may be touched: the checks come first)
    v = np.zeros((3, 8), np.float32)
    for kw in ({"top_k": 0}, {"top_k": 129}, {"top_k": True}, {"group_by_field": "colour"}, {"scorer": "max"}, {"scorer": None},
               {"filter": "level =="}, {"filter": ["level == 1"]}):
        with pytest.raises(ValueError):
            ms.search_embedding_list(v, **kw)
    for bad in (np.zeros(8, np.float32), np.zeros((0, 8), np.float32), np.zeros((65, 8), np.float32)):
        with pytest.raises(ValueError, match="list 0"):
            ms.search_embedding_list(bad)
    with pytest.raises(ValueError, match="list 1"):
        ms.search_embedding_lists_batch([v, np.zeros((2, 9), np.float32)])
    assert ms.search_embedding_lists_batch([]) == []


class _StubEmbedding:
    def encode_query_batch(self, texts):
        return np.ones((len(texts), 8), np.float32)


class _StubLists:
    LIST_MAX_VECTORS = 64

    def __init__(self):
        self.calls = []

    def search_embedding_list(self, vectors, top_k, group_by_field, filter, scorer):   # noqa: A002
        if scorer not in ("sum", "mean"):
            raise ValueError(f"scorer={scorer!r}")
        self.calls.append((vectors.shape, top_k, group_by_field, filter, scorer))
        hit = {"code": "A00", "title": "t", "score": np.float64(0.6), "original_score": np.float32(0.5), "metadata": {"level": 1}, "segment": 0}
        return [{"group": "A00-A09", "score": 1.25, "matches": [hit] + [None] * (len(vectors) - 1)}]

    def disconnect(self):
        pass


def test_segments_query_endpoint():
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    from rag_project_icd10_amd.api.icd_models import SegmentsQueryRequest
    r = SegmentsQueryRequest(segments=["a"])
    assert (r.top_k, r.group_by_field, r.filter, r.scorer) == (10, None, None, "sum")
    lists = _StubLists()
    appmod.install_services(_StubEmbedding(), lists, object())
    try:
        with TestClient(appmod.app) as client:
            r = client.post("/segments_query", json={"segments": ["a", "b", "c"], "top_k": 4, "group_by_field": "category", "scorer": "mean"})
            assert r.status_code == 200 and lists.calls[-1] == ((3, 8), 4, "category", None, "mean")
            body = r.json()
            assert body["segments"] == 3 and body["groups"][0]["group"] == "A00-A09" and body["groups"][0]["score"] == 1.25
            assert body["groups"][0]["matches"][0]["segment"] == 0 and body["groups"][0]["matches"][1:] == [None, None]
            assert client.post("/segments_query", json={"segments": ["a"]}).status_code == 200 and lists.calls[-1] == ((1, 8), 10, None, None, "sum")
            n = len(lists.calls)
            assert client.post("/segments_query", json={"segments": []}).status_code == 400
            assert client.post("/segments_query", json={"segments": ["x"] * 65}).status_code == 400
            assert client.post("/segments_query", json={"segments": ["x"], "scorer": "max"}).status_code == 400
            assert client.post("/segments_query", json={"top_k": 3}).status_code == 422
            assert len(lists.calls) == n
    finally:
        appmod.install_services(None, None, None)
