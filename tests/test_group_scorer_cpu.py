"""Group scorers of the grouping search, the parts that need no GPU: the oracle of
tests/group_scorer_oracle.py against a brute force over all rows, MAX against grouped_oracle.expected, the ABI, the host plan
under the sanitizers, and the service / /query plumbing over stubs."""
import os
import subprocess

import numpy as np
import pytest

import grouped_oracle
from conftest import ROOT
from group_scorer_oracle import SCORERS, ScoredRanking, chain_sum, expected, order_sensitive_share, order_u32
from grouped_oracle import Ranking

from rag_project_icd10_amd import _native
from rag_project_icd10_amd.services import filter_expr

CSRC = os.path.join(ROOT, "rag_project_icd10_amd", "csrc")


def _ranking(scores):
    """ids and scores of every query in (score desc, id asc) order, NaN rows dropped (-1 / -inf at the end) as the oracle's
    flat_ip_topk at k = n leaves them"""
    nq, n = scores.shape
    ids = np.full((nq, n), -1, np.int64)
    ranked = np.full((nq, n), -np.inf, np.float32)
    for q in range(nq):
        live = [i for i in range(n) if not np.isnan(scores[q, i])]
        live.sort(key=lambda i: (-int(order_u32(scores[q, i])), i))
        ids[q, :len(live)] = live
        ranked[q, :len(live)] = scores[q, live]
    return ranked, ids


def _brute(scores, group_of, k, s, scorer):
    """the contract by the book, one query, over all rows: -> (rows, [(aggregate, group)])"""
    members = {}
    for i in sorted((i for i in range(len(scores)) if not np.isnan(scores[i])), key=lambda i: (-int(order_u32(scores[i])), i)):
        members.setdefault(int(group_of[i]), []).append(i)
    ranked = []
    for g, rows in members.items():
        xs = [scores[i] for i in rows[:s]]
        a = xs[0] if scorer == "max" else chain_sum(xs)
        if scorer == "avg":
            with np.errstate(all="ignore"):
                a = np.float32(a / np.float32(len(xs)))
        if not np.isnan(a):
            ranked.append((-int(order_u32(a)), rows[0], np.float32(a), g))
    ranked.sort(key=lambda t: t[:2])
    return [i for t in ranked[:k] for i in members[t[3]][:s]], [(t[2], t[3]) for t in ranked[:k]]


def _edge_scores():
    n = 48
    rng = np.random.default_rng(5)
    scores = rng.standard_normal((9, n)).astype(np.float32)
    scores[1] = rng.integers(0, 6, n).astype(np.float32) / 4     # many exact ties inside and across groups
    scores[2, :] = 0.25                                          # everything ties: groups by their best member's row id
    scores[3, :] = np.float32(3e38)                              # sums overflow to +inf: those groups tie at +inf
    scores[3, ::7] = 1.0
    scores[4, 5], scores[4, [4, 6, 7]] = np.inf, -np.inf         # rows 4 .. 7 as one group: +inf + -inf, a NaN aggregate from s = 2 on
    scores[5, ::3] = np.nan                                      # NaN rows; in the //4 grouping below rows 0 ... are mixed
    scores[6, 8:16] = np.nan                                     # groups whose only rows are NaN
    scores[7] = (rng.standard_normal(n) * 1e-38).astype(np.float32)   # sums of tiny normals go subnormal
    scores[8, :] = -np.inf                                       # every aggregate -inf: still hits
    return scores


def test_oracle_against_a_brute_force_over_all_rows(oracle):
    scores = _edge_scores()
    n = scores.shape[1]
    levels = np.random.default_rng(2).integers(1, 4, n).astype(np.int32)
    ranked, ids = _ranking(scores)
    for group_of in (np.arange(n) // 4, np.arange(n) // 8, np.arange(n), np.zeros(n, int), (np.arange(n) // 2) * 7 % 5 + 3):
        rk = Ranking(ranked, ids, group_of)
        for scorer in SCORERS:
            for k, s in ((1, 1), (3, 1), (3, 2), (10, 3), (2, 40), (48, 1), (8, 5), (6, 8)):
                (raw, rid, lv, grp), adjusted, (gsc, gid) = expected(oracle, rk, levels, k, s, scorer)
                assert raw.shape == (9, k * s) and gsc.shape == gid.shape == (9, k)
                for q in range(9):
                    want, groups = _brute(scores[q], group_of, k, s, scorer)
                    m, ng = len(want), len(groups)
                    assert rid[q, :m].tolist() == want and (rid[q, m:] == -1).all(), (scorer, k, s, q)
                    assert raw[q, :m].tobytes() == scores[q, want].tobytes() and np.isneginf(raw[q, m:]).all()
                    assert grp[q, :m].tolist() == [group_of[i] for i in want] and (grp[q, m:] == -1).all()
                    assert gsc[q, :ng].tobytes() == np.array([a for a, _ in groups], np.float32).tobytes(), (scorer, k, s, q)
                    assert gid[q, :ng].tolist() == [g for _, g in groups] and (gid[q, ng:] == -1).all() and np.isneginf(gsc[q, ng:]).all()
                    assert sorted(adjusted[2][q].tolist()) == sorted(rid[q].tolist())
    # the NaN aggregate really drops a group, and a group of NaN rows is none
    rk = Ranking(ranked, ids, np.arange(n) // 4)
    _sc, _ids, _grp, gsc, gid = ScoredRanking(rk, 2, "sum").raw(12)
    assert 1 not in gid[4].tolist() and 1 in ScoredRanking(rk, 1, "sum").raw(12)[4][4].tolist()
    assert not {2, 3} & set(gid[6].tolist()) and (gid[6] >= 0).sum() == 10
    assert np.isposinf(gsc[3, 0]) and np.isneginf(gsc[8, :12]).all() and (gid[8] >= 0).all()


def test_max_is_the_grouped_oracle_and_s1_is_max(oracle):
    scores = _edge_scores()
    n = scores.shape[1]
    levels = np.random.default_rng(3).integers(1, 4, n).astype(np.int32)
    ranked, ids = _ranking(scores)
    for group_of in (np.arange(n) // 4, (np.arange(n) * 7) % 3, np.arange(n), np.zeros(n, int)):
        rk = Ranking(ranked, ids, group_of)
        for k, s in ((1, 1), (3, 2), (10, 3), (2, 40), (48, 1)):
            want = grouped_oracle.expected(oracle, rk, levels, k, s)
            got = expected(oracle, rk, levels, k, s, "max")
            for g, w in zip(got[0] + got[1], want[0] + want[1]):
                assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (k, s)
            if s == 1:
                assert got[2][0].tobytes() == got[0][0].tobytes()      # a group's MAX score is its best row's
        for k in (1, 5, 48):
            base = expected(oracle, rk, levels, k, 1, "max")
            for scorer in ("sum", "avg"):
                other = expected(oracle, rk, levels, k, 1, scorer)
                for g, w in zip(other[0] + other[1] + other[2], base[0] + base[1] + base[2]):
                    assert g.tobytes() == w.tobytes(), (scorer, k)


def test_the_order_of_the_sum_matters_on_random_scores():
    rng = np.random.default_rng(9)
    x = rng.standard_normal((40, 256)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    scores = x @ x[:24].T
    ranked, ids = _ranking(np.ascontiguousarray(scores.T, np.float32))
    share, total = order_sensitive_share(Ranking(ranked, ids, np.arange(40) // 5), 5)
    assert total == 24 * 8 and share >= 0.25, share


def test_abi_symbols_argtypes_and_header():
    import ctypes as C
    lib = _native.load_library()
    for name in ("icd_grouping_prepare_scorers", "icd_index_search_grouped_scored"):
        assert hasattr(lib, name) and name in _native.EXPORTED_SYMBOLS
    assert lib.icd_abi_version() == _native.ABI_VERSION == 6
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert lib.icd_grouping_prepare_scorers.argtypes == [vp, vp]
    plain = list(lib.icd_index_search_grouped.argtypes)
    assert list(lib.icd_index_search_grouped_scored.argtypes) == plain[:8] + [i32] + plain[8:13] + [vp, vp] + plain[13:]
    assert _native.GROUP_SCORERS == {"max": 0, "sum": 1, "avg": 2}
    header = open(os.path.join(ROOT, "include", "icd_search.h"), encoding="utf-8").read()
    assert "#define ICD_ABI_VERSION 6" in header
    for line in ("#define ICD_GROUP_SCORER_MAX 0", "#define ICD_GROUP_SCORER_SUM 1", "#define ICD_GROUP_SCORER_AVG 2",
                 "int icd_grouping_prepare_scorers(icd_index *idx, icd_grouping *grouping);",
                 "int32_t queries_on_device, int32_t reweighted, int32_t scorer, double *out_adj, float *out_raw,"):
        assert line in header, line
    # the unknown scorer and the other argument checks of the wrapper come before any handle is touched
    import inspect
    sig = inspect.signature(_native.IcdIndex.search_grouped)
    assert sig.parameters["scorer"].default == "max" and sig.parameters["group_scores"].default is False


def test_group_aggregate_plan_under_the_sanitizers(tmp_path):
    """tests/group_aggregate_plan_check.cpp: every position in exactly one pack or long item, no pack above 64 positions or across a
    group, long items = the runs above 64, the edge shapes - with ASan and UBSan"""
    exe = str(tmp_path / "group_aggregate_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "group_aggregate_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "group aggregate plan ok" in out.stdout


# ---- the service over a stub index, /query over a stub service -----------------------------------------------------------------
class _StubIndex:
    """search_grouped of an index of 6 rows in 3 groups: fixed answers, the call recorded"""
    max_nq, n, closed = 8, 6, False

    def __init__(self):
        self.calls = []

    def search_grouped(self, q, k, s, grouping, reweighted=True, **kw):
        self.calls.append((k, s, dict(kw)))
        nq = len(q)
        ids = np.tile(np.array([4, 5, 0, 1][:k * s] + [-1] * max(0, k * s - 4), np.int64), (nq, 1))
        raw = np.where(ids >= 0, np.float32(0.5), -np.inf).astype(np.float32)
        out = (raw.astype(np.float64), raw, ids, np.ones_like(ids, dtype=np.int32), np.where(ids >= 0, ids // 2, -1).astype(np.int32))
        if kw.get("group_scores"):
            gsc = np.tile(np.array([1.0, 0.75][:k] + [-np.inf] * max(0, k - 2), np.float32), (nq, 1))
            gid = np.tile(np.array([2, 0][:k] + [-1] * max(0, k - 2), np.int32), (nq, 1))
            out += (gsc, gid)
        return out


class _StubClient:
    generation, count = 1, 6
    records = [{"code": f"C{i}", "preferred_zh": f"t{i}", "level": 1, "parent_code": f"P{i // 2}"} for i in range(6)]

    def exists(self):
        return True


def _stub_service():
    from rag_project_icd10_amd.services.milvus_service import MilvusService
    ms = MilvusService.__new__(MilvusService)
    ms.client, ms.collection_name = _StubClient(), "stub"
    index = _StubIndex()
    ms._index = index
    ms._ready_index = lambda: index
    ms._grouping = lambda field, idx, rows, key: (object(), np.array(["P0", "P1", "P2"]))
    return ms, index


def test_milvus_service_passes_the_scorer_and_tags_the_hits():
    ms, index = _stub_service()
    q = np.zeros(8, np.float32)
    plain = ms.search(q, 2, group_by_field="parent_code", group_size=2)
    assert index.calls[-1] == (2, 2, {}) and [h["code"] for h in plain] == ["C4", "C5", "C0", "C1"]
    assert all("group_score" not in h["metadata"] and "group_score" not in h for h in plain)     # no new key without the argument
    for scorer in ("max", "sum", "avg"):
        hits = ms.search(q, 2, group_by_field="parent_code", group_size=2, group_scorer=scorer)
        assert index.calls[-1] == (2, 2, {"scorer": scorer, "group_scores": True})
        assert [h["metadata"]["parent_code"] for h in hits] == ["P2", "P2", "P0", "P0"]
        assert [h["metadata"]["group_score"] for h in hits] == [1.0, 1.0, 0.75, 0.75]
        strip = [dict(h, metadata={k: v for k, v in h["metadata"].items() if k != "group_score"}) for h in hits]
        assert strip == plain
        arrays = ms.search_batch(np.zeros((3, 8), np.float32), 2, group_by_field="parent_code", group_size=2, group_scorer=scorer)
        assert len(arrays) == 7 and arrays[5].shape == arrays[6].shape == (3, 2) and arrays[6].dtype == np.int32
        dicts = ms.search_batch(np.zeros((3, 8), np.float32), 2, as_dicts=True, group_by_field="parent_code", group_size=2, group_scorer=scorer)
        assert dicts == [hits] * 3
    assert len(ms.search_batch(np.zeros((3, 8), np.float32), 2, group_by_field="parent_code", group_size=2)) == 5
    calls = len(index.calls)
    for bad in ({"group_scorer": "median", "group_by_field": "parent_code"}, {"group_scorer": "sum"}, {"group_scorer": 1, "group_by_field": "level"},
                {"group_scorer": "SUM", "group_by_field": "level"}):
        with pytest.raises(ValueError, match="group_scorer"):
            ms.search(q, 2, **bad)
        with pytest.raises(ValueError, match="group_scorer"):
            ms.search_batch(q[None], 2, **bad)
    assert len(index.calls) == calls
    filter_expr.check_group_scorer(None, None)
    filter_expr.check_group_scorer("level", "avg")


def test_multi_diagnosis_service_checks_the_scorer_before_anything_runs():
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService, _search_options
    md = MultiDiagnosisService.__new__(MultiDiagnosisService)   # (nothing of it may be touched: the check comes first)
    for bad in ({"group_scorer": "best", "group_by_field": "category"}, {"group_scorer": "sum"}):
        with pytest.raises(ValueError, match="group_scorer"):
            md.match_multiple_diagnoses("x", **bad)
        with pytest.raises(ValueError, match="group_scorer"):
            md.match_diagnoses_batch(["x"], **bad)
    assert _search_options(None, "category", 2) == {"group_by_field": "category", "group_size": 2}
    assert _search_options(None, "category", 2, group_scorer="avg") == {"group_by_field": "category", "group_size": 2, "group_scorer": "avg"}


class _StubMulti:
    def __init__(self):
        self.calls = []

    def match_multiple_diagnoses(self, **kw):
        self.calls.append(kw)
        return {"matches": [], "extracted_diagnoses": ["x"]}


class _StubMilvus:
    def disconnect(self):
        pass


def test_query_endpoint_takes_a_group_scorer():
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    from rag_project_icd10_amd.api.icd_models import QueryRequest
    assert QueryRequest(text="x").group_scorer is None and QueryRequest(text="x", group_scorer="sum").group_scorer == "sum"
    multi = _StubMulti()
    appmod.install_services(object(), _StubMilvus(), multi)
    try:
        with TestClient(appmod.app) as client:
            plain = client.post("/query", json={"text": "x", "top_k": 3, "group_by_field": "category", "group_size": 2})
            assert plain.status_code == 200 and "group_scorer" not in multi.calls[-1]
            for scorer in ("max", "sum", "avg"):
                r = client.post("/query", json={"text": "x", "top_k": 3, "group_by_field": "category", "group_size": 2, "group_scorer": scorer})
                assert r.status_code == 200 and r.json() == plain.json()
                assert multi.calls[-1]["group_scorer"] == scorer and multi.calls[-1]["group_by_field"] == "category"
            n = len(multi.calls)
            assert client.post("/query", json={"text": "x", "group_by_field": "category", "group_scorer": "median"}).status_code == 400
            assert client.post("/query", json={"text": "x", "group_scorer": "sum"}).status_code == 400
            assert client.post("/query", json={"text": "x", "group_by_field": "category", "group_scorer": 3}).status_code == 422
            assert len(multi.calls) == n
            assert client.post("/query", json={"text": "x", "top_k": 3}).status_code == 200 and set(multi.calls[-1]) == {"text", "top_k"}
    finally:
        appmod.install_services(None, None, None)
