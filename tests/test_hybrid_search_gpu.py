"""Hybrid search (run with -m gpu on an MI355X): IcdIndex.search_hybrid - R dense requests per query fused on the device by RRF or a
weighted sum - against tests/hybrid_oracle.py's walk over the oracle's FULL ranking of every request's vector, bit for bit (ids,
levels, request bits, fused and adjusted doubles); rule 7's identities against the index's own searches; views, device tensors,
graph capture; MilvusService.hybrid_search and /hybrid_query. DESIGN.md section 13."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from hybrid_oracle import fuse_query, hybrid_batch
from test_grouped_search_gpu import N, NQ, _corpus  # noqa: F401  (the 12 000 x 768 corpora; _corpus through the cached parent below)
from test_range_search_gpu import _parent

pytestmark = pytest.mark.gpu

from rag_project_icd10_amd import _native  # noqa: E402
from rag_project_icd10_amd._native import MODE_AUTO, MODE_EXACT, IcdIndex  # noqa: E402

MAX_TOTAL = 1024   # >= 300 * 3
COPIES = 8         # noisy copies per base row of the extra pool
BASES = 20
_CACHE = {}
ROWS = np.arange(N, dtype=np.int64)


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes()


def _setup(kind, oracle):
    """corpus, levels, the POOL of request vectors with its full rankings, an index for 1 024 sub-lists and its fusion. Pool entries
    0 .. 299 are the corpus's own queries (0 .. 39 the duplicated rows 5000 + 2j themselves; ranked once for all the exact-search
    tests), 300 .. 459 eight noisy copies each of twenty rows (ranked here, once)."""
    if kind not in _CACHE:
        corpus, levels, q, _index, s, i = _parent(kind, oracle)
        rng = np.random.default_rng(99)
        base = corpus[rng.integers(0, N, BASES)]
        extra = np.repeat(base, COPIES, axis=0) + 0.04 * rng.standard_normal((BASES * COPIES, corpus.shape[1])).astype(np.float32)
        extra = np.ascontiguousarray(extra, dtype=np.float32)
        es, ei = oracle.flat_ip_topk(corpus, extra, N)
        pool = np.ascontiguousarray(np.concatenate([q, extra]))
        index = IcdIndex(corpus, levels, max_nq=MAX_TOTAL, max_k=128)
        _CACHE[kind] = (corpus, levels, pool, np.concatenate([s, es]), np.concatenate([i, ei]), index, index.fusion(MAX_TOTAL))
    return _CACHE[kind]


def _sel(name, nq, R):
    q, r = np.meshgrid(np.arange(nq), np.arange(R), indexing="ij")
    if name == "same":          # the same vector R times: full overlap
        return q % NQ + 0 * r
    if name == "noisy":         # noisy copies of one row: partial overlap
        return NQ + (q % BASES) * COPIES + r % COPIES
    if name == "unrelated":     # unrelated rows: no overlap, every fused score of rank j ties R ways
        return (40 + q + 41 * r) % NQ
    assert name == "dups"       # the duplicated rows 5000 + 2j / 5001 + 2j: equal sub-scores
    return (q + r) % 40


RANKERS = [("rrf", {"c": 60.0}), ("weighted", {"weights": [1.0, 0.5, 0.25, 0.75, 0.125, 0.875, 0.375, 0.0], "norm": "none"}),
           ("weighted", {"weights": [0.3, 1.0, 0.7, 0.9, 0.2, 0.6, 0.1, 0.8], "norm": "cosine"})]


def _kw(ranker, kw, R):
    out = {"ranker": ranker}
    if ranker == "rrf":
        out["rrf_c"] = kw["c"]
    else:
        out["weights"], out["norm"] = kw["weights"][:R], kw["norm"]
    return out


def _okw(ranker, kw, R):
    return {"c": kw["c"]} if ranker == "rrf" else {"weights": kw["weights"][:R], "norm": kw["norm"]}


def _compare(got_raw, got_adj, want, nq, what):
    for label, got, exp in (("raw", got_raw, want[0]), ("reweighted", got_adj, want[1])):
        assert len(got) == len(exp)
        for j, (g, w) in enumerate(zip(got, exp)):
            g = g.cpu().numpy() if hasattr(g, "cpu") else g
            w = w[:nq]
            if g.dtype == np.int32 and w.dtype == np.uint32:
                g = g.view(np.uint32)
            assert g.dtype == w.dtype and g.shape == w.shape, (what, label, j, g.dtype, w.dtype, g.shape, w.shape)
            assert _bits(g) == _bits(w), (what, label, j, nq, np.nonzero((g != w).any(1))[0][:5])


def _check(index, fusion, pool, sel, limits, k, want, nq, what, ranker, kw, mode=MODE_AUTO, **extra):
    R = sel.shape[1]
    qv = np.ascontiguousarray(pool[sel[:nq]])
    cut = {name: (None if v is None else v[:nq]) for name, v in extra.items()}
    got_raw = index.search_hybrid(qv, limits, k, fusion, reweighted=False, mode=mode, **_kw(ranker, kw, R), **cut)
    got_adj = index.search_hybrid(qv, limits, k, fusion, reweighted=True, mode=mode, **_kw(ranker, kw, R), **cut)
    _compare(got_raw, got_adj, want, nq, what)


CASES = [   # request set, R, limits, k, batch sizes
    ("same", 1, [10], 10, (1, 4, 17, 300)),
    ("same", 3, [10, 10, 10], 10, (1, 17)),
    ("noisy", 2, [63, 65], 10, (1, 4, 17, 300)),
    ("noisy", 3, [1, 64, 128], 128, (4, 300)),
    ("noisy", 8, [128] * 8, 128, (1, 17)),          # all 1 024 slots
    ("noisy", 8, [10] * 8, 1, (17,)),
    ("unrelated", 3, [10, 10, 10], 128, (1, 17, 300)),   # k above the distinct ids: padding
    ("unrelated", 8, [1] * 8, 10, (4,)),
    ("dups", 2, [10, 65], 10, (4, 17)),
    ("dups", 3, [128, 128, 128], 128, (17,)),
]


@pytest.mark.parametrize("kind", ["gauss", "family"])
def test_hybrid_search_equals_the_oracle_bit_for_bit(oracle, kind):
    corpus, levels, pool, s_all, i_all, index, fusion = _setup(kind, oracle)
    for name, R, limits, k, batches in CASES:
        sel = _sel(name, max(batches), R)
        for ranker, kw in RANKERS:
            want = hybrid_batch(s_all, i_all, levels, sel, limits, k, ranker, **_okw(ranker, kw, R))
            if name == "unrelated" and R == 3:
                assert (want[0][1][:, -1] == -1).all()       # at most 30 distinct ids: padded
                if ranker == "rrf":                          # ranks tie R ways: the id decides the order
                    tie = want[0][0][:, 0] == want[0][0][:, 2]
                    assert tie.mean() > 0.5 and (np.diff(want[0][1][tie, :3], axis=1) > 0).all()
            for nq in batches:
                _check(index, fusion, pool, sel, limits, k, want, nq, (kind, name, R, k, ranker, kw.get("norm")), ranker, kw)
    # the caller's mode: the exact kernels give the same sub-lists
    sel = _sel("noisy", 17, 3)
    want = hybrid_batch(s_all, i_all, levels, sel, [10, 64, 20], 10, "rrf", c=60.0)
    _check(index, fusion, pool, sel, [10, 64, 20], 10, want, 17, (kind, "exact mode"), "rrf", {"c": 60.0}, mode=MODE_EXACT)


def test_masks_and_bands_per_query_and_request(oracle):
    corpus, levels, pool, s_all, i_all, index, fusion = _setup("gauss", oracle)
    nq, R, limits = 17, 3, [10, 65, 128]
    sel = _sel("noisy", nq, R)
    few = np.zeros(N, bool)
    few[[3, 5000, 5001, 9000, 11999]] = True                 # fewer rows than any limit but 1
    empty = np.zeros(N, bool)
    sels = [[None if (q + r) % 4 == 0 else ROWS % 7 == (q + 2 * r) % 7 for r in range(R)] for q in range(nq)]
    sels[1] = [few, None, few]
    sels[2] = [None, empty, ROWS % 2 == 0]                   # an empty mask on one request
    sels[3] = [empty, empty, empty]                          # ... on all of them: all padding
    made = {}

    def dev(m):
        if m is None:
            return None
        if m.tobytes() not in made:
            made[m.tobytes()] = index.rowmask(np.nonzero(m)[0])
        return made[m.tobytes()]
    try:
        dmasks = [[dev(m) for m in row] for row in sels]
        # bands on request 1 only: a floor at its rank-20 score, a ceiling at its rank-2 score
        lo = np.full((nq, R), -np.inf, np.float32)
        hi = np.full((nq, R), np.inf, np.float32)
        lo[:, 1] = s_all[sel[:, 1], 20]
        hi[:, 1] = s_all[sel[:, 1], 2]
        for k in (10, 128):
            for ranker, kw in RANKERS:
                okw = _okw(ranker, kw, R)
                want = hybrid_batch(s_all, i_all, levels, sel, limits, k, ranker, masks=sels, **okw)
                assert (want[0][1][3] == -1).all() and (want[0][1][1] >= 0).sum() <= 5 + 65
                _check(index, fusion, pool, sel, limits, k, want, nq, ("masks", k, ranker), ranker, kw, masks=dmasks)
                want = hybrid_batch(s_all, i_all, levels, sel, limits, k, ranker, radius=lo, range_filter=hi, **okw)
                _check(index, fusion, pool, sel, limits, k, want, nq, ("bands", k, ranker), ranker, kw, radius=lo, range_filter=hi)
                want = hybrid_batch(s_all, i_all, levels, sel, limits, k, ranker, masks=sels, radius=lo, **okw)
                _check(index, fusion, pool, sel, limits, k, want, nq, ("masks + floor", k, ranker), ranker, kw, masks=dmasks, radius=lo)
        # a mask of another index, a closed mask
        other = IcdIndex(corpus[:256], levels[:256], max_nq=8, max_k=16)
        om = other.rowmask(np.arange(5))
        with pytest.raises(_native.IcdError) as e:
            index.search_hybrid(pool[sel[:1]], limits, 10, fusion, masks=[[om, None, None]])
        assert e.value.code == -1
        om.close()
        with pytest.raises(_native.IcdError) as e:
            index.search_hybrid(pool[sel[:1]], limits, 10, fusion, masks=[[om, None, None]])
        assert e.value.code == -5
        other.close()
    finally:
        for m in made.values():
            m.close()


def test_weighted_atan_within_1e_12_of_the_oracle(oracle):
    """the device's atan need not round as the host's does: fused scores within 1e-12 absolute (at most 8 terms with weights <= 1,
    each a few ulp of a value below 1); ids wherever the oracle's neighbouring fused scores differ by more than 1e-9 - which, with
    distinct weights and noisy copies, is at least 95 % of the ranks (measured on the oracle on the CPU: 96.3 % on these inputs)"""
    corpus, levels, pool, s_all, i_all, index, fusion = _setup("gauss", oracle)
    weights = [0.3, 1.0, 0.7, 0.9, 0.2, 0.6, 0.1, 0.8]
    compared = total = 0
    for R, limits, k, nq in ((3, [10, 65, 128], 128, 17), (8, [64] * 8, 10, 17), (2, [10, 10], 10, 300)):
        sel = _sel("noisy", nq, R)
        (wf, wi, wl, wb), _ = hybrid_batch(s_all, i_all, levels, sel, limits, k, "weighted", weights=weights[:R], norm="atan")
        fused, ids, lv, bits = index.search_hybrid(pool[sel], limits, k, fusion, ranker="weighted", weights=weights[:R], norm="atan",
                                                   reweighted=False)
        valid = wi >= 0
        assert np.array_equal(ids >= 0, valid)
        err = np.abs(fused[valid] - wf[valid]).max()
        print(f"atan R={R}: max |fused - oracle| = {err:.3e}")
        assert err <= 1e-12
        gap_prev = np.concatenate([np.full((nq, 1), np.inf), np.abs(np.diff(wf, axis=1))], axis=1)
        gap_next = np.concatenate([np.abs(np.diff(wf, axis=1)), np.full((nq, 1), np.inf)], axis=1)
        clear = valid & (np.nan_to_num(gap_prev, nan=np.inf) > 1e-9) & (np.nan_to_num(gap_next, nan=np.inf) > 1e-9)
        assert np.array_equal(ids[clear], wi[clear]) and np.array_equal(lv[clear], wl[clear]) and np.array_equal(bits[clear], wb[clear])
        compared += int(clear.sum())
        total += int(valid.sum())
    print(f"atan: {compared} of {total} ranks compared by id")
    assert compared >= 0.95 * total


def test_rule_7_identities_against_the_index_itself(oracle):
    corpus, levels, pool, s_all, i_all, index, fusion = _setup("family", oracle)
    q = np.ascontiguousarray(pool[:40])
    for k in (1, 10, 128):
        raw, ids = index.search(q, k, MODE_EXACT)
        fused, hid, _lv, bits = index.search_hybrid(q[:, None, :], [k], k, fusion, ranker="rrf", rrf_c=60.0, reweighted=False)
        assert _bits(hid) == _bits(ids) and (bits == 1).all()
        assert _bits(fused) == _bits(np.tile(np.array([1.0 / (60.0 + j + 1) for j in range(k)]), (40, 1)))
        fused, hid, _lv, _b = index.search_hybrid(q[:, None, :], [k], k, fusion, ranker="weighted", weights=[1.0], norm="none", reweighted=False)
        assert _bits(hid) == _bits(ids) and _bits(fused) == _bits(raw.astype(np.float64))
        adj, _f, hid, hlv, _b = index.search_hybrid(q[:, None, :], [k], k, fusion, ranker="weighted", weights=[1.0], norm="none")
        w_adj, _w_raw, w_ids, w_lv = index.search_reweighted(q, k, MODE_EXACT)
        assert _bits(adj) == _bits(w_adj) and _bits(hid) == _bits(w_ids) and _bits(hlv) == _bits(w_lv)
        for R in (2, 8):
            fused, hid, _lv, bits = index.search_hybrid(np.repeat(q[:, None, :], R, axis=1), [k] * R, k, fusion, ranker="rrf", reweighted=False)
            want = np.zeros(k)
            for _ in range(R):
                want = want + np.array([1.0 / (60.0 + j + 1) for j in range(k)])
            assert _bits(hid) == _bits(ids) and _bits(fused) == _bits(np.tile(want, (40, 1))) and (bits == (1 << R) - 1).all()
    mask = index.rowmask(np.nonzero(ROWS % 3 == 1)[0])
    try:
        raw, ids, _lv = index.search_masked(q, 10, mask, reweighted=False)
        fused, hid, _l, _b = index.search_hybrid(q[:, None, :], [10], 10, fusion, ranker="weighted", weights=[1.0], masks=[mask] * 40, reweighted=False)
        assert _bits(hid) == _bits(ids) and _bits(fused) == _bits(raw.astype(np.float64))
    finally:
        mask.close()


def test_hybrid_search_on_a_view(oracle):
    corpus, levels, pool, s_all, i_all, index, fusion = _setup("gauss", oracle)
    rows = np.sort(np.random.default_rng(5).choice(N, N // 3, replace=False)).astype(np.int64)
    view = index.view(rows, max_nq=64)
    vf = view.fusion(64)
    try:
        nq, R, limits = 4, 2, [10, 65]
        sel = _sel("noisy", nq, R)
        used = np.unique(sel)
        vs, vi = oracle.flat_ip_topk(corpus[rows], pool[used], len(rows))
        s_v = {int(p): vs[j] for j, p in enumerate(used)}
        i_v = {int(p): rows[vi[j]] for j, p in enumerate(used)}          # the view's hits carry the parent's ids
        lo = np.full((nq, R), -np.inf, np.float32)
        lo[:, 0] = [s_v[int(p)][5] for p in sel[:, 0]]
        for ranker, kw in RANKERS:
            for b in ({}, {"radius": lo}):
                want = hybrid_batch(s_v, i_v, levels, sel, limits, 10, ranker, **_okw(ranker, kw, R), **b)
                _check(view, vf, pool, sel, limits, 10, want, nq, ("view", ranker, bool(b)), ranker, kw, **b)
        mask = index.rowmask(np.arange(100))
        try:
            with pytest.raises(_native.IcdError) as e:
                view.search_hybrid(pool[sel], limits, 10, vf, masks=[[mask, None]] * nq)
            assert e.value.code == -4
        finally:
            mask.close()
        # the parent's fusion does not serve the view
        with pytest.raises(_native.IcdError) as e:
            view.search_hybrid(pool[sel], limits, 10, fusion)
        assert e.value.code == -1
    finally:
        vf.close()
        view.close()


def test_device_tensors_graph_capture_and_argument_errors(oracle):
    import torch
    corpus, levels, pool, s_all, i_all, index, fusion = _setup("gauss", oracle)
    R, limits, k = 3, [10, 65, 128], 10
    for nq in (1, 17, 300):
        sel = _sel("noisy", nq, R)
        dq = torch.from_numpy(np.ascontiguousarray(pool[sel])).cuda()
        lo = np.full((nq, R), -np.inf, np.float32)
        lo[:, 2] = s_all[sel[:, 2], 30]
        dlo = torch.from_numpy(lo).cuda()
        for ranker, kw in RANKERS[:2]:
            want = hybrid_batch(s_all, i_all, levels, sel, limits, k, ranker, radius=lo, **_okw(ranker, kw, R))
            got = index.search_hybrid(dq, limits, k, fusion, radius=dlo, **_kw(ranker, kw, R))
            assert all(t.is_cuda for t in got)
            torch.cuda.synchronize()
            _compare(index.search_hybrid(dq, limits, k, fusion, radius=dlo, reweighted=False, **_kw(ranker, kw, R)), got, want, nq, ("device", nq, ranker))
        # one device-in / device-out call inside a graph replays to the same bits (single-branch graph, no runtime setting touched)
        glimits = [10, 7, 10]
        want = hybrid_batch(s_all, i_all, levels, sel, glimits, k, "rrf", c=60.0)
        mask = index.rowmask(np.arange(100))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            index.search_hybrid(dq, glimits, k, fusion)   # warm-up on the capture stream
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cap = index.search_hybrid(dq, glimits, k, fusion)
            with pytest.raises(_native.IcdError) as e:   # a masked call fills its table on the host: refused while capturing
                index.search_hybrid(dq, glimits, k, fusion, masks=[[mask, None, None]] * nq)
        assert e.value.code == -1
        for _ in range(2):
            for t in cap:
                t.zero_()
            graph.replay()
            torch.cuda.synchronize()
            for g, w in zip(cap, want[1]):
                g = g.cpu().numpy()
                assert _bits(g.view(np.uint32) if w.dtype == np.uint32 else g) == _bits(w[:nq]), nq
        del graph
        mask.close()
    # argument errors: ICD_ERR_INVALID before any device call
    q3 = np.ascontiguousarray(pool[_sel("noisy", 2, 3)])
    bad = [dict(limits=[10, 0, 10]), dict(limits=[10, 129, 10]), dict(k=0), dict(k=129), dict(rrf_c=0.0), dict(rrf_c=16384.0), dict(rrf_c=float("nan")),
           dict(ranker="weighted", weights=[0.5, 1.5, 0.1]), dict(ranker="weighted", weights=[0.5, -0.1, 0.1]),
           dict(ranker="weighted", weights=[0.5, float("nan"), 0.1]), dict(radius=np.float32(0.5), range_filter=np.float32(0.5)),
           dict(radius=np.float32("nan"))]
    for b in bad:
        args = {"limits": limits, "k": 10, **b}
        with pytest.raises(_native.IcdError) as e:
            index.search_hybrid(q3, args.pop("limits"), args.pop("k"), fusion, **args)
        assert e.value.code == -1, b
    with pytest.raises(_native.IcdError) as e:
        index.search_hybrid(np.zeros((2, 9, corpus.shape[1]), np.float32), [10] * 9, 10, fusion)      # R = 9
    assert e.value.code == -1
    with pytest.raises(_native.IcdError) as e:
        index.search_hybrid(np.zeros((400, 3, corpus.shape[1]), np.float32), limits, 10, fusion)       # nq * R above the capacity
    assert e.value.code == -1
    small = index.fusion(4)
    assert small.stats()["max_total"] == 4 and small.stats()["bytes"] > 0
    with pytest.raises(_native.IcdError) as e:
        index.search_hybrid(q3, limits, 10, small)                                                      # 6 sub-lists, room for 4
    assert e.value.code == -1
    other = IcdIndex(corpus[:256], levels[:256], max_nq=8, max_k=16)
    of = other.fusion(8)
    with pytest.raises(_native.IcdError) as e:
        index.search_hybrid(q3, limits, 10, of)                                                         # a fusion of another index
    assert e.value.code == -1
    with pytest.raises(_native.IcdError) as e:
        other.search_hybrid(q3[:1], [10, 17, 10], 10, of)                                               # a limit above that index's max_k
    assert e.value.code == -1
    of.close()
    other.close()
    small.close()
    with pytest.raises(_native.IcdError) as e:
        index.search_hybrid(q3, limits, 10, small)                                                      # a destroyed fusion
    assert e.value.code == -5


# ---- services ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def services(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("MILVUS_DB_PATH", str(tmp_path_factory.mktemp("db")))
    mp.setenv("MILVUS_COLLECTION_NAME", "icd10_hybrid")
    mp.setenv("EMBEDDING_MODEL_NAME", "shibing624/text2vec-base-chinese")
    mp.setenv("ICD_EMBEDDING_ALLOW_SYNTHETIC", "1")
    from rag_project_icd10_amd.tools.build_database import DatabaseBuilder
    b = DatabaseBuilder()
    b.initialize_services()
    recs = b.load_csv_data(os.path.join(GOLDEN, "csv_slice.csv"))
    assert b.vectorize_and_index(recs) is True
    strings = [l.rstrip("\n") for l in open(os.path.join(GOLDEN, "diagnosis_strings.txt"), encoding="utf-8")][:12]
    yield {"b": b, "recs": recs, "ms": b.milvus_service, "es": b.embedding_service, "strings": strings}
    b.milvus_service.disconnect()
    mp.undo()


def _sub_list_through_search_batch(ms, vec, limit, expr, band):
    """one request sent through MilvusService.search_batch, back in RAW order (score desc, id asc), padding dropped"""
    kw = {} if expr is None else {"filter": expr, "filter_mode": "mask"}
    _adj, raw, ids, _lv = ms.search_batch(vec[None, :], limit, **kw, **band)
    keep = ids[0] >= 0
    raw, ids = raw[0][keep], ids[0][keep]
    order = np.lexsort((ids, -raw.astype(np.float64)))
    return raw[order], ids[order]


def test_milvus_service_hybrid_search_and_the_endpoint(services):
    # (last of the module: the app's lifespan disconnects the installed services when the client closes)
    from fastapi.testclient import TestClient
    from rag_project_icd10_amd.api import app as appmod
    from rag_project_icd10_amd.services.hybrid_search import AnnSearchRequest, RRFRanker, WeightedRanker
    ms, es, recs, strings = services["ms"], services["es"], services["recs"], services["strings"]
    levels = ms.client.levels()
    vecs = np.stack([es.encode_query(s) for s in strings]).astype(np.float32)
    plain = ms.search_batch(vecs[:1], 20)[1][0]
    setups = [([None, None, None], [{}, {}, {}]), ([None, "level >= 2", "level == 3"], [{}, {}, {}]),
              (["level >= 2", None, "level >= 1"], [{"radius": float(plain[15])}, {}, {"range_filter": float(plain[1])}])]
    for exprs, bands in setups:
        for ranker, okw in ((RRFRanker(60), dict(ranker="rrf", c=60.0)), (RRFRanker(0.5), dict(ranker="rrf", c=0.5)),
                            (WeightedRanker(0.6, 0.3, 1.0, norm_score="none"), dict(ranker="weighted", weights=[0.6, 0.3, 1.0], norm="none")),
                            (WeightedRanker(0.6, 0.3, 1.0, norm_score="cosine"), dict(ranker="weighted", weights=[0.6, 0.3, 1.0], norm="cosine"))):
            limits = [20, 7, 64]
            for qi in (0, 4):
                three = [vecs[qi], vecs[qi + 1], vecs[qi + 2]]
                reqs = [AnnSearchRequest(v, lim, expr=e, param=({"params": b} if b else None)) for v, lim, e, b in zip(three, limits, exprs, bands)]
                lists = [_sub_list_through_search_batch(ms, v, lim, e, b) for v, lim, e, b in zip(three, limits, exprs, bands)]
                _raw, (adj, fused, ids, _lv, bits) = fuse_query(lists, levels, 10, **okw)
                hits = ms.hybrid_search(reqs, ranker, 10)
                m = int((ids >= 0).sum())
                assert len(hits) == m and [h["code"] for h in hits] == [recs[i]["code"] for i in ids[:m]], (exprs, okw, qi)
                assert [h["score"] for h in hits] == [float(a) for a in adj[:m]]
                assert [h["fused_score"] for h in hits] == [float(f) for f in fused[:m]]
                assert [h["matched_requests"] for h in hits] == [[r for r in range(3) if (int(b) >> r) & 1] for b in bits[:m]]
                assert all("original_score" not in h for h in hits)
    # the array form: [nq, dim] per request
    reqs = [AnnSearchRequest(vecs[0:6], 20), AnnSearchRequest(vecs[3:9], 7, expr="level >= 2")]
    adj, fused, ids, lv, bits = ms.hybrid_search_batch(reqs, RRFRanker(), 10)
    for qi in range(6):
        lists = [_sub_list_through_search_batch(ms, vecs[qi], 20, None, {}), _sub_list_through_search_batch(ms, vecs[3 + qi], 7, "level >= 2", {})]
        _raw, want = fuse_query(lists, levels, 10, "rrf", c=60.0)
        assert [_bits(a[qi]) for a in (adj, fused, ids, lv, bits)] == [_bits(w) for w in want], qi
    assert len(ms.fusions()) == 1 and ms.fusions()[0]["bytes"] > 0
    appmod.install_services(es, ms)
    try:
        with TestClient(appmod.app) as client:
            texts = strings[:3]
            r = client.post("/hybrid_query", json={"texts": texts, "top_k": 5, "req_limit": 20})
            assert r.status_code == 200, r.text
            tv = np.asarray(es.encode_query_batch(list(texts)), dtype=np.float32)
            lists = [_sub_list_through_search_batch(ms, tv[i], 20, None, {}) for i in range(3)]
            _raw, (adj, fused, ids, _lv, _b) = fuse_query(lists, levels, 5, "rrf", c=60.0)
            cands = r.json()["candidates"]
            assert [c["code"] for c in cands] == [recs[i]["code"] for i in ids if i >= 0]
            assert [c["score"] for c in cands] == [float(a) for a in adj[ids >= 0]]
            assert [c["original_score"] for c in cands] == [float(f) for f in fused[ids >= 0]]
            r = client.post("/hybrid_query", json={"texts": texts, "top_k": 5, "req_limit": 20, "filter": "level >= 2",
                                                   "ranker": {"strategy": "weighted", "params": {"weights": [1.0, 0.5, 0.25], "norm_score": "none"}}})
            assert r.status_code == 200, r.text
            lists = [_sub_list_through_search_batch(ms, tv[i], 20, "level >= 2", {}) for i in range(3)]
            _raw, (adj, fused, ids, _lv, _b) = fuse_query(lists, levels, 5, "weighted", weights=[1.0, 0.5, 0.25], norm="none")
            assert [c["code"] for c in r.json()["candidates"]] == [recs[i]["code"] for i in ids if i >= 0]
            assert client.post("/hybrid_query", json={"texts": texts, "ranker": {"strategy": "weighted", "params": {"weights": [1.0]}}}).status_code == 400
            assert client.post("/hybrid_query", json={"texts": texts, "filter": "level >"}).status_code == 400
            assert "fusions" in client.get("/stats").json()
    finally:
        appmod.install_services(None, None, None)
