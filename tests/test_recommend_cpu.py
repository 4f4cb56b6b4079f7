"""Recommend search off the device: recommend_plan.hpp under the host sanitizers, the symbols,
tests/recommend_oracle.py (its fmaf chain against exact rational arithmetic, its vectorised fold and window against a brute force
that folds row by row and builds no ranking, hand-made cases of every branch), services/recommend.py's argument rules and results
over a stub index, and the shape of POST /recommend over stub services."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import recommend_oracle as ro
from conftest import ROOT
from rag_project_icd10_amd import _native

CSRC = os.path.join(ROOT, "rag_project_icd10_amd", "csrc")
F = np.float32


def test_plan_header_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "recommend_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "recommend_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "recommend plan ok" in out.stdout


def test_symbols_and_abi():
    lib = _native.load_library()
    for name in ("icd_recommend_create", "icd_recommend_destroy", "icd_recommend_stats", "icd_recommend_read_vectors", "icd_index_recommend"):
        assert hasattr(lib, name) and name in _native.EXPORTED_SYMBOLS
    assert lib.icd_abi_version() == _native.ABI_VERSION == 6
    header = open(os.path.join(ROOT, "include", "icd_search.h"), encoding="utf-8").read()
    assert "#define ICD_ABI_VERSION 6" in header and "#define ICD_RECOMMEND_MAX_EXAMPLES 16" in header
    for name, code in _native.RECOMMEND_STRATEGIES.items():
        assert f"#define ICD_RECOMMEND_{name.upper()} {code}" in header
    assert _native.RECOMMEND_MAX_EXAMPLES == ro.MAX_EXAMPLES == 16 and tuple(_native.RECOMMEND_STRATEGIES) == ro.STRATEGIES
    plan = open(os.path.join(CSRC, "recommend_plan.hpp"), encoding="utf-8").read()
    assert "hip/" not in plan and "__global__" not in plan                         # host only: no HIP header, no kernel
    kernel = open(os.path.join(CSRC, "recommend_kernel.hpp"), encoding="utf-8").read()
    body = kernel.split("#pragma once")[1]
    assert '#include "recommend_plan.hpp"' in kernel and "order_f32(" in body and "unorder_f32(" in body and "__fdiv_rn(" in body
    assert "printf(" not in body and " assert(" not in body and "atomic" not in body and "__shared__" not in body
    wide = open(os.path.join(CSRC, "icd_recommend.hpp"), encoding="utf-8").read()
    for launched in ("recommend_examples_kernel", "wide_scores_kernel", "recommend_combine_kernel", "wide_threshold_kernel", "wide_collect_kernel", "launch_wide_sort_emit"):
        assert launched in wide
    # the checks that need no device: a destroyed / missing handle is ICD_ERR_STATE
    assert lib.icd_recommend_destroy(None) == -5 and lib.icd_recommend_stats(None, None, None, None, None) == -5
    assert lib.icd_recommend_read_vectors(None, 0, None) == -5
    assert lib.icd_index_recommend(None, None, None, None, None, None, None, 0, 1, 1, 0, None, None, 0, 1, None, None, None, None, None, None, 0, 0, None) == -5


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def round_once_f32(fr):
    """a Fraction rounded ONCE to float32, ties to even - by bisection over the float32 neighbours of its double value"""
    d = F(float(fr))
    lo, hi = (np.nextafter(d, F(-np.inf)), d) if Fraction(float(d)) > fr else (d, np.nextafter(d, F(np.inf)))
    if Fraction(float(lo)) == fr:
        return lo
    if Fraction(float(hi)) == fr:
        return hi
    dl, dh = fr - Fraction(float(lo)), Fraction(float(hi)) - fr
    if dl != dh:
        return lo if dl < dh else hi
    return lo if (lo.view(np.uint32) & 1) == 0 else hi


def test_the_chain_is_fmaf():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((40, 24)).astype(F)
    v = rng.standard_normal(24).astype(F)
    # a row where rounding twice goes wrong: acc = 2^24 + 2, product = (1 + 2^-23)(1 - 2^-23) = 1 - 2^-46. The exact sum lies just
    # below the float32 tie 2^24 + 3 and rounds to 2^24 + 2; a double holds the tie itself, which would go to the even 2^24 + 4
    v[:2] = (1.0, F(1.0) - F(2.0 ** -23))
    x[0, :2], x[0, 2:] = (F(2.0 ** 24 + 2), F(1.0) + F(2.0 ** -23)), 0.0
    x[1, :2], x[1, 2:] = (F(1.0), F(2.0 ** -24)), 0.0                               # a true tie: 1 + 2^-24 (1 - 2^-23) is below it, stays 1
    assert F(np.float64(x[0, 0]) + np.float64(x[0, 1]) * np.float64(v[1])) == F(2.0 ** 24 + 4)
    want = []
    for row in x:
        acc = F(0.0)
        for a, b in zip(row, v):
            acc = round_once_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(acc)))
        want.append(acc)
    got = ro.chain_scores(v, x)
    assert got.dtype == F and got.tobytes() == np.array(want, F).tobytes()
    sp = np.array([[np.inf, 1.0], [np.nan, 1.0], [-np.inf, 0.0], [3e38, 3e38]], F)       # inf, NaN, inf x 0 and an overflow
    got = ro.chain_scores(np.array([1.0, 1.0], F), sp)
    assert np.isposinf(got[0]) and np.isnan(got[1]) and np.isneginf(got[2]) and np.isposinf(got[3])
    assert np.isnan(ro.chain_scores(np.array([0.0, 1.0], F), sp)[0])


def test_oracle_against_brute_force():
    rng = np.random.default_rng(5)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, np.nan], F)
    for case in range(300):
        n = int(rng.integers(1, 50))
        P, N = int(rng.integers(0, 5)), int(rng.integers(0, 5))
        if P + N == 0:
            P = 1
        strategy = ("best_score", "sum_scores")[case % 2]
        scores = [(rng.integers(-6, 7, n) / 8.0).astype(F) for _ in range(P + N)]       # runs of ties, bp == bn among them
        if case % 3 == 0:
            for s in scores:
                at = rng.integers(0, n, 3)
                s[at] = specials[rng.integers(0, len(specials), 3)]
        sp, sn = scores[:P], scores[P:]
        excluded = sorted(set(rng.integers(0, n, int(rng.integers(0, 4))).tolist()))
        mask = None if case % 2 == 0 else rng.random(n) < 0.6
        lo = None if case % 4 < 2 else -0.25
        hi = None if case % 5 < 3 else 0.5
        id_base = int(rng.integers(0, 2)) * 900
        k, first = int(rng.integers(1, 60)), int(rng.integers(0, 20))
        levels = rng.choice(np.array([0, 1, 2, 3, 7], np.int32), n)
        c, clean = ro.fold(strategy, sp, sn, n)
        ok = ro.ranks_mask(c, clean, excluded, mask, lo, hi)
        (raw, ids, lv), adj, count, selected = ro.window(c, ok, levels, k, first, id_base)
        b_raw, b_ids, b_count, b_sel = ro.brute_force(sp, sn, strategy, excluded, k, first, mask, lo, hi, id_base)
        assert raw.tobytes() == b_raw.tobytes() and ids.tobytes() == b_ids.tobytes() and count == b_count and selected == b_sel, case
        assert (lv[:count] == levels[ids[:count] - id_base]).all() and (lv[count:] == 0).all()
        assert adj[0].dtype == np.float64 and sorted(adj[2][:count].tolist()) == sorted(ids[:count].tolist())


def test_oracle_on_hand_made_cases():
    a = lambda *v: np.array(v, F)   # noqa: E731
    # best_score: bp > bn takes bp; bp == bn takes the negative branch; no positives: -(bn * bn); -0.0 from -(0 * 0)
    c, clean = ro.fold("best_score", [a(0.5, 0.25, 0.25, 0.0)], [a(0.25, 0.25, 0.5, 0.0)], 4)
    assert c.tobytes() == a(0.5, -0.0625, -0.25, -0.0).tobytes() and clean.all() and np.signbit(c[3])
    c, _ = ro.fold("best_score", [], [a(0.0, -0.5, np.inf)], 3)
    assert c.tobytes() == a(-0.0, -0.25, -np.inf).tobytes()
    c, _ = ro.fold("best_score", [a(-np.inf, 0.5)], [], 2)                        # bp = -inf is not above bn = -inf: -(inf * inf)
    assert c.tobytes() == a(-np.inf, 0.5).tobytes()
    c, _ = ro.fold("best_score", [a(-0.0), a(0.0)], [], 1)                        # +0.0 is not above -0.0: the first stays
    assert np.signbit(c[0])
    # sum_scores: list order matters in float32
    big, one = F(2.0 ** 24), F(1.0)
    c1, _ = ro.fold("sum_scores", [a(big), a(one), a(one)], [a(big)], 1)
    c2, _ = ro.fold("sum_scores", [a(one), a(one), a(big)], [a(big)], 1)
    assert c1[0] == 0.0 and c2[0] == 2.0
    c, clean = ro.fold("sum_scores", [a(np.inf, np.nan, 1.0)], [a(np.inf, 1.0, 1.0)], 3)
    assert np.isnan(c[0]) and clean.tolist() == [True, False, True] and c[2] == 0.0 and not np.signbit(c[2])
    ok = ro.ranks_mask(c, clean, [], None, None, None)
    assert ok.tolist() == [False, False, True]                                    # inf - inf: c is NaN; a NaN example score
    # the target: sums in list order, one divide, t = mp + (mp - mn)
    corpus = np.array([[1.0, 2.0 ** 24], [3.0, 1.0], [2.0, 1.0], [0.5, 0.0]], F)
    t = ro.target_vector([0, 1, 2], [], corpus)
    assert t.tobytes() == a(2.0, F(F(2.0 ** 24) / F(3.0))).tobytes()              # 2^24 + 1 + 1 stays 2^24 in float32
    t = ro.target_vector([1, a(0.0, 3.0)], [3], corpus)
    assert t.tobytes() == a(1.5 + (1.5 - 0.5), 2.0 + (2.0 - 0.0)).tobytes()
    # exclusion: a stored example never ranks, its bit-identical duplicate does; a vector example excludes nothing
    corpus = np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0]], F)
    levels = np.ones(3, np.int32)
    (raw, ids, lv), _adj, count, selected = ro.recommend_query(corpus, levels, [0], [], "best_score", 3)
    assert ids.tolist() == [1, 2, -1] and count == 2 and selected == 2 and raw[0] == 1.0
    (raw, ids, lv), _adj, count, selected = ro.recommend_query(corpus, levels, [corpus[0]], [], "average_vector", 3, id_base=10)
    assert ids.tolist() == [10, 11, 12] and selected == 3
    (raw, ids, lv), _adj, count, selected = ro.recommend_query(corpus, levels, [0], [0], "sum_scores", 2, first=1)    # positive and negative at once
    assert ids.tolist() == [2, -1] and raw[0] == 0.0 and selected == 2


# ---- the service on its host side ---------------------------------------------------------------------------------------------
class StubMask:
    def __init__(self, rows):
        self.rows, self.closed, self.transient = len(rows), False, False

    def stats(self):
        return {"rows": self.rows, "bytes": 0}

    def close(self):
        self.closed = True


class StubWorkspace:
    """IcdRecommend as recommend_batch sees it: every call is noted on its index; request r's hits are rows 0, 1, .. of the index in
    order, from `first` on"""

    def __init__(self, index, max_requests):
        self.index, self.max_requests, self.closed = index, max_requests, False

    def recommend(self, positive, negative, strategy, k, *, masks=None, radius=None, range_filter=None, first=0, reweighted=True):
        assert len(positive) == len(negative) and not self.closed and reweighted
        self.index.calls.append(dict(positive=positive, negative=negative, strategy=strategy, k=k, first=first, masks=masks, radius=radius,
                                     range_filter=range_filter))
        n, nr = self.index.n, len(positive)
        ids = np.full((nr, k), -1, np.int64)
        m = max(0, min(k, n - first))
        ids[:, :m] = np.arange(first, first + m)
        raw = np.where(ids >= 0, 0.9 - 0.01 * ids, -np.inf).astype(np.float32)
        return raw.astype(np.float64), raw, ids, np.where(ids >= 0, 2, 0).astype(np.int32), np.full(nr, m, np.int32), np.full(nr, n, np.int64)


class StubIndex:
    def __init__(self, n, dim, max_nq=8):
        self.n, self.dim, self.max_nq, self.max_k, self.device, self.closed = n, dim, max_nq, 64, 0, False
        self.calls, self.made, self.handles = [], [], []

    def rowmask(self, rows):
        self.made.append(len(rows))
        return StubMask(rows)

    def make_workspace(self, size):
        self.handles.append(StubWorkspace(self, size))
        return self.handles[-1]


RECORDS = [{"code": c, "preferred_zh": t, "level": lv, "parent_code": p, "has_complication": False, "main_code": None, "secondary_code": None,
            "category_path": ""}
           for c, t, lv, p in [("A00", "霍乱", 1, ""), ("A00.0", "霍乱，由于O1群霍乱弧菌", 2, "A00"), ("A00.1", "埃尔托霍乱", 2, "A00"),
                               ("A01", "伤寒和副伤寒", 1, ""), ("A01.0", "伤寒", 2, "A01"), ("A01.1", "副伤寒甲", 2, "A01")]]
DIM = 64


class Emb:                      # (the store takes its dimension from the encoder)
    def __init__(self):
        self.batches = []

    def encode_query(self, t):
        return np.ones(DIM, np.float32) / 8

    def encode_query_batch(self, texts):
        self.batches.append(list(texts))
        return np.stack([np.full(DIM, len(t) / 64, np.float32) for t in texts])


@pytest.fixture()
def svc(tmp_path, monkeypatch):
    monkeypatch.setenv("MILVUS_DB_PATH", str(tmp_path / "db"))
    monkeypatch.setenv("MILVUS_COLLECTION_NAME", "recommend")
    from rag_project_icd10_amd.services.milvus_service import MilvusService

    class Small(MilvusService):
        FILTER_ON_DEVICE = False    # the host route: filter_rows -> index.rowmask
        TEXT_MATCH_ON_DEVICE = False
        _WORKSPACE_FACTORIES = {"recommend": (lambda index, size: index.make_workspace(size), "max_requests")}   # (the stub's, in place of _native.IcdRecommend)

    from rag_project_icd10_amd.services.recommend import Recommend
    s = Recommend(Small(Emb()))
    yield s
    s.ms.disconnect()


def load(svc, **kw):
    rng = np.random.default_rng(0)
    ms = svc.ms
    assert ms.insert_records(RECORDS, [rng.standard_normal(DIM).astype(np.float32) for _ in RECORDS]) is True
    ms._index = StubIndex(len(RECORDS), DIM, **kw)
    ms._index_rows, ms._index_gen = ms.client.count, ms.client.generation
    return ms._index


V = np.ones(DIM, np.float32)


def test_the_factory_is_registered():
    from rag_project_icd10_amd.services import recommend
    from rag_project_icd10_amd.services.milvus_service import MilvusService
    assert MilvusService._WORKSPACE_FACTORIES["recommend"] == (recommend.make_workspace, "max_requests")
    assert recommend.MAX_TOP_K == 16384 and recommend.MAX_EXAMPLES == 16 and recommend.STRATEGIES == ro.STRATEGIES


def test_empty_collection_and_argument_checks(svc):
    assert svc.recommend(["A00"], top_k=5) == []
    out, totals = svc.recommend_batch([[1], [2]], None, "best_score", 20, as_dicts=False, with_totals=True)
    assert out[2].shape == (2, 20) and (out[2] == -1).all() and totals.tolist() == [0, 0]
    index = load(svc)
    bad = [
        lambda: svc.recommend([], []), lambda: svc.recommend(["A00"] * 17), lambda: svc.recommend(["A00"] * 9, ["A01"] * 8),
        lambda: svc.recommend([], ["A00"]),                                        # average_vector needs a positive
        lambda: svc.recommend(["A00"], strategy="nearest"), lambda: svc.recommend("A00"), lambda: svc.recommend(["A00"], "A01"),
        lambda: svc.recommend([""]), lambda: svc.recommend([-1]), lambda: svc.recommend([True]), lambda: svc.recommend([1.5]),
        lambda: svc.recommend([np.ones((2, DIM), np.float32)]), lambda: svc.recommend([None]),
        lambda: svc.recommend(["A00"], top_k=0), lambda: svc.recommend(["A00"], top_k=16385), lambda: svc.recommend(["A00"], top_k=10.5),
        lambda: svc.recommend(["A00"], top_k=10, offset=-1), lambda: svc.recommend(["A00"], top_k=385, offset=16000),
        lambda: svc.recommend(["A00"], radius=0.5, range_filter=0.5), lambda: svc.recommend(["A00"], radius=float("nan")),
        lambda: svc.recommend(["A00"], filter="level =="), lambda: svc.recommend(["A00"], filter="nope == 1"), lambda: svc.recommend(["A00"], filter=["level == 2"]),
        lambda: svc.recommend_batch([["A00"], ["A01"]], [["A00"]]), lambda: svc.recommend_batch(["A00"], None),
        lambda: svc.recommend_batch([["A00"], ["A01"]], None, filter=["level == 2"]),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} did not raise")
    assert index.calls == [] and index.made == [] and index.handles == [] and svc.ms.embedding_service.batches == []   # every check came before the index was asked
    with pytest.raises(ValueError):
        svc.recommend([np.ones(DIM + 1, np.float32)])
    with pytest.raises(KeyError):
        svc.recommend([6])
    assert index.calls == []


def test_examples_results_and_one_call_per_batch(svc):
    index = load(svc)
    hits = svc.recommend(["A00.1", "发热伴腹泻", 4], ["A01", V], "best_score", 3, offset=1, radius=0.5, range_filter=0.75)
    call = index.calls[-1]
    assert len(index.calls) == 1 and len(index.handles) == 1 and svc.ms.embedding_service.batches == [["发热伴腹泻"]]
    pos, neg = call["positive"][0], call["negative"][0]
    assert pos[0] == 2 and pos[2] == 4 and neg[0] == 3                           # a stored code is its row, an id is itself
    assert pos[1].dtype == np.float32 and pos[1].tobytes() == np.full(DIM, 5 / 64, np.float32).tobytes() and neg[1].tobytes() == V.tobytes()
    assert (call["strategy"], call["k"], call["first"], call["masks"], call["radius"], call["range_filter"]) == ("best_score", 3, 1, None, 0.5, 0.75)
    assert [h["code"] for h in hits] == ["A00.0", "A00.1", "A01"]              # `search`-shaped, from `first` on
    assert set(hits[0]) == {"code", "title", "score", "original_score", "metadata"} and hits[0]["original_score"] == float(np.float32(0.9 - 0.01))
    # a batch: one device call, one encode for all texts, a filter per request through the mask route
    lists, totals = svc.recommend_batch([["甲"], ["A00", "乙丙"], [V]], [[], ["丁"], [0]], "sum_scores", 200, filter=["level == 2", None, "level == 2"],
                                        with_totals=True)
    call = index.calls[-1]
    assert len(index.calls) == 2 and svc.ms.embedding_service.batches[-1] == ["甲", "乙丙", "丁"] and len(index.handles) == 1
    assert call["masks"][1] is None and call["masks"][0] is call["masks"][2] and index.made == [4]
    assert [len(x) for x in lists] == [6, 6, 6] and totals.tolist() == [6, 6, 6] and totals.dtype == np.int64
    adj, raw, ids, lv = svc.recommend_batch([[0]], None, "average_vector", 8, as_dicts=False)
    assert ids.shape == (1, 8) and adj.dtype == np.float64 and ids[0, 6] == -1


def test_endpoint_over_the_stub(svc):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as api
    index = load(svc)
    saved = (api.embedding_service, api.milvus_service, api.multi_diagnosis_service)
    api.install_services(svc.ms.embedding_service, svc.ms, multi=object())
    try:
        client = TestClient(api.app)
        r = client.post("/recommend", json={"positive": ["A00.1", 4, "发热"], "negative": ["A01", [0.5] * DIM], "strategy": "best_score", "top_k": 2000, "offset": 1})
        assert r.status_code == 200, r.text
        body = r.json()
        assert set(body) == {"candidates", "total"} and body["total"] == 6 and [c["code"] for c in body["candidates"]] == [r_["code"] for r_ in RECORDS[1:]]
        call = index.calls[-1]
        assert call["k"] == 2000 and call["first"] == 1 and call["strategy"] == "best_score" and call["positive"][0][:2] == [2, 4]
        assert call["negative"][0][0] == 3 and call["negative"][0][1].tobytes() == np.full(DIM, 0.5, np.float32).tobytes()
        assert body["candidates"] == svc.recommend(["A00.1", 4, "发热"], ["A01", [0.5] * DIM], "best_score", 2000, offset=1)
        for bad in ({"positive": [], "negative": []}, {"positive": ["A00"], "top_k": 16385}, {"positive": ["A00"], "top_k": 0},
                    {"positive": ["A00"], "top_k": 10, "offset": 16380}, {"positive": ["A00"], "strategy": "closest"}, {"negative": ["A00"]},
                    {"positive": ["A00"] * 17}, {"positive": ["A00"], "filter": "level =="}, {"positive": ["A00"], "radius": 0.5, "range_filter": 0.1},
                    {"positive": [[0.5] * (DIM + 1)]}):
            assert client.post("/recommend", json=bad).status_code == 400, bad
        assert client.post("/recommend", json={"positive": [99]}).status_code == 404
        r = client.post("/recommend", json={"positive": ["A00"], "negative": ["A01.0"], "strategy": "sum_scores", "top_k": 500, "filter": "level == 2", "radius": 0.0})
        assert r.status_code == 200 and index.calls[-1]["masks"][0] is not None and index.calls[-1]["radius"] == 0.0
    finally:
        api.embedding_service, api.milvus_service, api.multi_diagnosis_service = saved
