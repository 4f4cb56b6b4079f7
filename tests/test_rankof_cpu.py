"""Rank-of search off the device: tests/rankof_oracle.py against the definition by brute force on tiny
hand-made corpora (all tied, copies of the target row, NaN rows, a masked-out target), rankof_plan.hpp under the host sanitizers,
the symbols, evaluate's arithmetic on fixed rank arrays, and services/rank_of.py's RankOf.rank_of / rank_of_batch / evaluate on
their host side (argument checks, the unknown-code error, one library call per batch) over a stub index."""
import os
import subprocess

import numpy as np
import pytest

import rankof_oracle as ro
from conftest import ROOT
from rag_project_icd10_amd import _native

CSRC = os.path.join(ROOT, "rag_project_icd10_amd", "csrc")


def test_plan_header_under_the_host_sanitizers(tmp_path):
    """tests/rankof_plan_check.cpp: the tile split, the output offsets, the limits, a mask word's valid bits and the sweep's
    bookkeeping against a plain count - with ASan and UBSan"""
    exe = str(tmp_path / "rankof_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "rankof_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rankof plan ok" in out.stdout


def test_symbols_and_abi():
    lib = _native.load_library()
    for name in ("icd_rankof_create", "icd_rankof_destroy", "icd_rankof_stats", "icd_index_rank_of"):
        assert hasattr(lib, name) and name in _native.EXPORTED_SYMBOLS
    assert lib.icd_abi_version() == _native.ABI_VERSION == 6
    header = open(os.path.join(ROOT, "include", "icd_search.h"), encoding="utf-8").read()
    assert "#define ICD_ABI_VERSION 6" in header and "#define ICD_RANKOF_MAX_TARGETS 16" in header
    assert _native.RANKOF_MAX_TARGETS == 16
    plan = open(os.path.join(CSRC, "rankof_plan.hpp"), encoding="utf-8").read()
    assert "hip/" not in plan and "__global__" not in plan                         # host only: no HIP header, no kernel
    kernel = open(os.path.join(CSRC, "rankof_kernel.hpp"), encoding="utf-8").read()
    body = kernel.split("#pragma once")[1]
    assert '#include "rankof_plan.hpp"' in kernel and "mmr_quad_chain(" in body and "make_key(" in body and "br_row_of(" in body
    assert "rk_valid_bits(" in body and "rk_slot(" in body
    assert "printf(" not in body and " assert(" not in body and "fmaf(" not in body   # the chain is the shared one, not a copy
    # the checks that need no device: a destroyed / missing handle is ICD_ERR_STATE
    assert lib.icd_rankof_destroy(None) == -5 and lib.icd_rankof_stats(None, None, None) == -5
    assert lib.icd_index_rank_of(None, None, None, 0, 0, None, 1, None, None, None, None, None, None, None) == -5


# ---- the oracle against the definition ----------------------------------------------------------------------------------------
def ranking_of(row_scores, id_base=0):
    """the full ranking oracle.flat_ip_topk returns for these row scores: (score desc, id asc), NaN rows left out, padding behind"""
    sc = np.asarray(row_scores, np.float32)
    rows = np.array([r for r in np.lexsort((np.arange(len(sc)), -sc)) if not np.isnan(sc[r])], np.int64)
    s = np.full(len(sc), -np.inf, np.float32)
    i = np.full(len(sc), -1, np.int64)
    s[:len(rows)], i[:len(rows)] = sc[rows], rows + id_base
    return s, i


def check_against_brute_force(row_scores, levels, mask, id_base=0):
    n = len(row_scores)
    s, i = ranking_of(row_scores, id_base)
    admitted = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    targets = np.concatenate([np.arange(n) + id_base, [-1, id_base + n, id_base - 1 if id_base else -5]])
    rank, adj, raw, lv, sel = ro.rank_of_query(s, i, levels, targets, mask, n, id_base)
    assert sel == admitted.sum()
    for r in range(n):
        want = ro.brute_force(row_scores, r, admitted)
        assert rank[r] == want, (r, rank[r], want)
        if want >= 0:
            assert raw[r].tobytes() == np.float32(row_scores[r]).tobytes() and lv[r] == levels[r]
            assert adj[r] == float(np.float64(np.float32(row_scores[r])) * ro.W.get(int(levels[r]), 1.0))
        else:
            assert np.isnan(raw[r]) and np.isnan(adj[r]) and lv[r] == (levels[r] if admitted[r] else 0)
    assert (rank[n:] == -1).all() and np.isnan(raw[n:]).all() and np.isnan(adj[n:]).all() and (lv[n:] == 0).all()
    return rank


def test_oracle_on_hand_made_corpora():
    levels = np.array([1, 2, 3, 1, 2, 3, 1, 2], np.int32)
    # all tied: the rank is the number of admitted smaller ids
    rank = check_against_brute_force(np.full(8, 0.25, np.float32), levels, None)
    assert rank[:8].tolist() == list(range(8))
    mask = np.array([1, 0, 1, 1, 0, 1, 0, 1], bool)
    rank = check_against_brute_force(np.full(8, 0.25, np.float32), levels, mask, id_base=1000)
    assert rank[:8].tolist() == [0, -1, 1, 2, -1, 3, -1, 4]
    # copies of the target row in front of it and behind it
    sc = np.array([0.5, 0.9, 0.5, 0.1, 0.5, 0.9, -0.2, 0.5], np.float32)
    rank = check_against_brute_force(sc, levels, None)
    assert rank[:8].tolist() == [2, 0, 3, 6, 4, 1, 7, 5]
    # NaN rows are in no ranking and ahead of nothing
    sc = np.array([0.5, np.nan, 0.5, 0.1, np.nan, 0.9, -0.2, 0.5], np.float32)
    rank = check_against_brute_force(sc, levels, None)
    assert rank[:8].tolist() == [1, -1, 2, 4, -1, 0, 5, 3]
    # a masked-out target, masked-out rows ahead of a target, the empty mask
    rank = check_against_brute_force(sc, levels, np.array([1, 1, 0, 1, 1, 0, 1, 1], bool), id_base=7)
    assert rank[:8].tolist() == [0, -1, -1, 2, -1, -1, 3, 1]
    rank = check_against_brute_force(sc, levels, np.zeros(8, bool))
    assert (rank == -1).all()
    # subnormal and signed-zero scores compare as floats
    check_against_brute_force(np.array([1e-45, 0.0, -0.0, -1e-45, 1e-45], np.float32), levels[:5], None)
    # random rankings with runs of ties
    rng = np.random.default_rng(3)
    for case in range(200):
        n = int(rng.integers(1, 40))
        sc = (rng.integers(-4, 5, n) / 8.0).astype(np.float32)
        if case % 5 == 0:
            sc[rng.integers(0, n)] = np.nan
        check_against_brute_force(sc, rng.integers(1, 4, n).astype(np.int32), None if case % 3 == 0 else rng.random(n) < 0.6, id_base=int(rng.integers(0, 2)) * 500)


def test_oracle_batch_and_duplicates():
    levels = np.array([1, 2, 3, 1], np.int32)
    s0, i0 = ranking_of(np.array([0.1, 0.4, 0.4, 0.2], np.float32))
    s1, i1 = ranking_of(np.array([0.9, 0.4, 0.5, 0.2], np.float32))
    rank, adj, raw, lv, sel = ro.rank_of_batch([s0, s1], [i0, i1], levels, np.array([[2, 2, -1, 0], [3, 9, 3, 1]]), [None, np.array([1, 0, 1, 1], bool)], 4)
    assert rank.tolist() == [[1, 1, -1, 3], [2, -1, 2, -1]] and sel.tolist() == [4, 3]
    assert lv.tolist() == [[3, 3, 0, 1], [1, 0, 1, 0]] and raw.dtype == np.float32 and adj.dtype == np.float64 and rank.dtype == np.int64


# ---- evaluate's arithmetic ------------------------------------------------------------------------------------------------------
def test_rank_metrics_on_fixed_ranks():
    from rag_project_icd10_amd.services.rank_of import RankOf
    m = RankOf.rank_metrics([0, 4, 9, 10, None, -1, 2, 299], ks=(1, 5, 10))
    assert m["n"] == 8 and m["recall@1"] == 1 / 8 and m["recall@5"] == 3 / 8 and m["recall@10"] == 4 / 8
    assert m["mrr"] == pytest.approx((1 + 1 / 5 + 1 / 10 + 1 / 11 + 1 / 3 + 1 / 300) / 8, rel=1e-15)
    assert m["mean_rank"] == pytest.approx((0 + 4 + 9 + 10 + 2 + 299) / 6, rel=1e-15)
    assert m["ranks"] == [0, 4, 9, 10, None, None, 2, 299]
    want = ro.metrics([0, 4, 9, 10, None, -1, 2, 299])
    assert all(m[k] == pytest.approx(want[k], rel=1e-15) for k in want)
    empty = RankOf.rank_metrics([], ks=(3,))
    assert empty == {"n": 0, "recall@3": 0.0, "mrr": 0.0, "mean_rank": None, "ranks": []}
    none = RankOf.rank_metrics([None, None])
    assert none["recall@10"] == 0.0 and none["mrr"] == 0.0 and none["mean_rank"] is None


# ---- the service on its host side ---------------------------------------------------------------------------------------------
class StubMask:
    def __init__(self, rows):
        self.rows, self.closed, self.transient = len(rows), False, False

    def stats(self):
        return {"rows": self.rows, "bytes": 0}

    def close(self):
        self.closed = True


class StubWorkspace:
    """IcdRankOf as rank_of_batch sees it: every call is noted on its index; target row r of query q has rank (q + r) % 7, and no
    rank when r = 5"""

    def __init__(self, index, max_nq):
        self.index, self.max_nq, self.closed = index, max_nq, False

    def rank_of(self, queries, targets, masks=None):
        q, t = np.asarray(queries), np.asarray(targets, np.int64)
        assert q.ndim == 2 and q.dtype == np.float32 and t.shape[0] == q.shape[0] and not self.closed
        self.index.calls.append(dict(nq=len(q), targets=t.tolist(), masks=masks))
        rank = np.where((t < 0) | (t == 5), -1, (np.arange(len(q))[:, None] + t) % 7).astype(np.int64)
        raw = np.where(rank >= 0, 0.5 - 0.01 * rank, np.nan).astype(np.float32)
        return rank, raw.astype(np.float64) * 1.2, raw, np.where(rank >= 0, 1, 0).astype(np.int32), np.full(len(q), self.index.n, np.int64)


class StubIndex:
    """IcdIndex as rank_of_batch sees it: the masks and the workspaces it makes are noted, and the calls of the latter"""

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
    monkeypatch.setenv("MILVUS_COLLECTION_NAME", "rankof")
    from rag_project_icd10_amd.services.milvus_service import MilvusService

    class Emb:                      # (the store takes its dimension from the encoder)
        def encode_query(self, t):
            return np.ones(DIM, np.float32) / 8

        def encode_query_batch(self, texts):
            return np.stack([np.full(DIM, len(t) / 64, np.float32) for t in texts])

    class Small(MilvusService):
        FILTER_ON_DEVICE = False    # the host route: filter_rows -> index.rowmask
        TEXT_MATCH_ON_DEVICE = False
        _WORKSPACE_FACTORIES = {"rankof": (lambda index, size: index.make_workspace(size), "max_nq")}   # (the stub's, in place of _native.IcdRankOf)

    from rag_project_icd10_amd.services.rank_of import RankOf
    s = RankOf(Small(Emb()))
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


def test_empty_collection(svc):
    assert svc.rank_of(Q, ["A00"]) == [] and svc.rank_of_batch([Q, Q], [["A00"], "A01"]) == [[], []]
    for bad in (lambda: svc.rank_of(Q, []), lambda: svc.rank_of(Q, ["A00"], filter="level =="), lambda: svc.evaluate([(Q, "A00")], ks=(0,))):
        with pytest.raises(ValueError):          # a bad argument raises on an empty collection too
            bad()


def test_argument_checks(svc):
    index = load(svc)
    bad = [
        lambda: svc.rank_of(Q, []), lambda: svc.rank_of(Q, ["A00"] * 17), lambda: svc.rank_of(Q, [7]), lambda: svc.rank_of(Q, [""]), lambda: svc.rank_of(Q, None),
        lambda: svc.rank_of(np.ones((2, DIM), np.float32), ["A00"]), lambda: svc.rank_of(["a", "b"], ["A00"]),
        lambda: svc.rank_of(np.ones(DIM + 1, np.float32), ["A00"]),                                  # not the index's dim
        lambda: svc.rank_of(Q, ["A00"], filter="level =="), lambda: svc.rank_of(Q, ["A00"], filter="nope == 1"), lambda: svc.rank_of(Q, ["A00"], filter=["level == 2"]),
        lambda: svc.rank_of_batch([Q, Q], [["A00"]]), lambda: svc.rank_of_batch([Q, Q], "A00"), lambda: svc.rank_of_batch([Q, "text"], [["A00"], ["A00"]]),
        lambda: svc.rank_of_batch([Q, Q], [["A00"], ["A01"]], filter=["level == 2"]), lambda: svc.rank_of_batch(np.ones((2, 2, DIM), np.float32), [["A00"], ["A00"]]),
        lambda: svc.evaluate([(Q, "A00", 1)]), lambda: svc.evaluate([Q]), lambda: svc.evaluate([(Q, "A00")], ks=()), lambda: svc.evaluate([(Q, "A00")], ks=(0,)),
        lambda: svc.evaluate([(Q, "A00")], ks=(1.5,)), lambda: svc.evaluate([(Q, "A00"), ("text", "A00")]), lambda: svc.evaluate([(Q, [])]),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} did not raise")
    assert index.calls == [] and index.made == [] and index.handles == []      # every check came before the index was asked
    for code in ("Z99", "a00"):                   # an unknown code is a KeyError, not a missing rank
        with pytest.raises(KeyError):
            svc.rank_of(Q, ["A00", code])
    assert index.calls == []


def test_results_and_one_call_per_batch(svc):
    index = load(svc)
    hits = svc.rank_of(Q, ["A00", "A01.1", "A00.1"])
    assert index.calls == [dict(nq=1, targets=[[0, 5, 2]], masks=None)] and len(index.handles) == 1
    assert hits[0] == {"code": "A00", "rank": 0, "score": float(np.float64(np.float32(0.5)) * 1.2), "raw_score": float(np.float32(0.5)), "level": 1, "selected": 6}
    assert hits[1] == {"code": "A01.1", "rank": None, "score": None, "raw_score": None, "level": 0, "selected": 6}
    assert hits[2]["rank"] == 2
    # a batch: ragged code lists are padded with -1, a bare string is a list of one; texts go through the encoder
    out = svc.rank_of_batch(["霍乱", "伤寒吧"], [["A00", "A01"], "A00.0"])
    assert index.calls[-1]["targets"] == [[0, 3], [1, -1]] and [len(o) for o in out] == [2, 1] and len(index.handles) == 1
    assert out[1][0]["rank"] == 2
    # per-query filters: one masks call, equal expressions share a mask, no filter is a NULL entry
    svc.rank_of_batch([Q, Q, Q], [["A00"]] * 3, filter=["level == 2", None, "level == 2"])
    masks = index.calls[-1]["masks"]
    assert masks[1] is None and masks[0] is masks[2] and index.made == [4]
    # evaluate: the best rank among a query's acceptable codes
    before = len(index.calls)
    m = svc.evaluate([(Q, "A00"), (Q, ["A01", "A00.0"]), (Q, "A01.1")], ks=(1, 3))
    assert len(index.calls) == before + 1 and index.calls[-1]["targets"] == [[0, -1], [3, 1], [5, -1]]
    assert m["ranks"] == [0, 2, None] and m["n"] == 3 and m["recall@1"] == 1 / 3 and m["recall@3"] == 2 / 3
    assert m["mrr"] == pytest.approx((1 + 1 / 3) / 3) and m["mean_rank"] == 1.0
    assert svc.evaluate([], ks=(1,))["n"] == 0


def test_endpoint_over_the_stub(svc):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as api
    index = load(svc)
    saved = (api.embedding_service, api.milvus_service, api.multi_diagnosis_service)
    api.install_services(svc.ms.embedding_service, svc.ms, multi=object())
    try:
        client = TestClient(api.app)
        r = client.post("/codes/rank", json={"text": "霍乱", "codes": ["A00", "A01.1"]})
        assert r.status_code == 200, r.text
        body = r.json()
        want = svc.rank_of("霍乱", ["A00", "A01.1"])
        assert body == want and body[1]["rank"] is None
        assert client.post("/codes/rank", json={"text": "霍乱", "codes": ["Z99"]}).status_code == 404
        assert client.post("/codes/rank", json={"text": "霍乱", "codes": []}).status_code in (400, 422)
        assert client.post("/codes/rank", json={"text": "霍乱", "codes": ["A00"], "filter": "level =="}).status_code == 400
        r = client.post("/codes/rank", json={"text": "霍乱", "codes": ["A00"], "filter": "level == 2"})
        assert r.status_code == 200 and index.calls[-1]["masks"][0] is not None
    finally:
        api.embedding_service, api.milvus_service, api.multi_diagnosis_service = saved
