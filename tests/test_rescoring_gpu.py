"""The kernels after the search, at the sizes the service runs them (run with -m gpu on an MI355X): the device-side
hierarchical rescoring (icd_hier_rescore) and the packing of its winners (icd_pack_winners) at k = 1 ... 128, the row-sharded
merge (icd_merge_topk) at G * k up to 1 024, and match_diagnoses_batch end to end at top_k up to 50 (a search of k = 100).

A live /query without NER searches 2 * top_k = 100 hits (api/icd_models.py: top_k <= 50), so the rescoring runs both of a
lane's slots (j = lane and j = lane + 64) and ranks across them; the merge of 8 shards at k = 128 fills all 16 slots of a
lane. Every kernel is held bit for bit against a plain reference that is already pinned: the host method
HierarchicalSimilarityService.batch_calculate_similarities (tests/golden/hier_cases.json), the CPU oracle (flat_ip_topk /
reweight / merge), torch gathers, and the confidence service's per-call numpy methods."""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN, icd_levels, unit_rows

pytestmark = pytest.mark.gpu

from rag_project_icd10_amd import _native  # noqa: E402
from rag_project_icd10_amd._native import IcdError, IcdIndex  # noqa: E402

EDGE = ["待查", "？", " 疑似 ", "肺炎待查", "高血压 糖尿病 肿瘤 感染"]   # empty clean query (exact-match rule), markers, chapter keywords
NROWS = 6000
BIG_BASE = 1 << 40


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


@functools.lru_cache(maxsize=None)
def _strings():
    s = [l.strip() for l in open(os.path.join(GOLDEN, "diagnosis_strings.txt"), encoding="utf-8") if l.strip()]
    assert len(s) == 1000
    return tuple(s)


@functools.lru_cache(maxsize=None)
def _row_codes():
    """NROWS unique codes: every chapter letter of the table and two outside it (Z, Q); one in five matches the uncertainty
    service's \\.9\\d*$, the others carry another digit behind the dot or a letter at the end; every 17th has no dot"""
    letters = "ABCEIJKNSZQ"
    codes = []
    for i in range(NROWS):
        L = letters[i % 11]
        if i % 17 == 0:
            codes.append(f"{L}{i:05d}")
        elif i % 5 == 0:
            codes.append(f"{L}{i % 100:02d}.9{i:05d}" if i % 10 else f"{L}{i % 100:02d}.9")
        else:
            codes.append(f"{L}{i % 100:02d}.{(i // 3) % 9}{i:05d}" + ("x" if i % 13 == 0 else ""))
    seen = set()
    for i, c in enumerate(codes):          # the bare ".9" codes repeat: keep the first of each
        if c in seen:
            codes[i] = f"{c}{i:05d}"
        seen.add(codes[i])
    assert len(set(codes)) == NROWS
    return tuple(codes)


def _outside_code(i):
    """the code of an id outside [id_base, id_base + n_rows): tag 15 on the device, so no chapter letter and no '.9' here"""
    return f"O{i}"


# ---- 1. icd_hier_rescore against the host method ------------------------------------------------------------------------
RULE_VALUES = [1.0000000000000002, 1.0, 0.9999999999999999, 0.97, 0.9500000000000001, 0.95, 0.9499999999999999,
               0.9000000000000001, 0.9, 0.8999999999999999, 0.5, 0.30000000000000004, 0.3, 0.29999999999999993, 0.0, -0.05]


def _hit_lists(k, nq, id_base, seed):
    """live-shaped hit lists (adjusted score descending, -1 / -inf behind the hits) that exercise both slots of a lane:
    hit counts 0, 1, 63, 64, 65, k - 1 and k; exact ties at positions 63 / 64, at j / j + 64 and over the whole list;
    scores on both sides of the 0.9 / 0.95 / 1.0 / 1.8 rules and of the semantic-coherence value, negative scores; ids
    outside the tag table (beyond the rows, and below id_base when it is not 0)"""
    rng = np.random.default_rng(seed)
    counts = [k, 0, 1, 63, 64, 65, k - 1, k, k]
    ids = np.full((nq, k), -1, np.int64)
    adj = np.full((nq, k), -np.inf)
    nhit = np.zeros(nq, np.int64)
    for q in range(nq):
        n = min(max(counts[q % len(counts)], 0), k)
        nhit[q] = n
        if n == 0:
            continue
        rows = rng.choice(NROWS, n, replace=False).astype(np.int64)
        ids[q, :n] = id_base + rows
        if q % 5 == 2:                                        # ids without a row of the tag table
            for j in (0, 3, 63, 64, 65, n - 1):
                if j < n:
                    ids[q, j] = id_base + NROWS + 7 * q + j if (j % 2 == 0 or id_base == 0) else id_base - 1 - 7 * q - j
        mode = q % 4
        if mode == 0:                                         # wide: negatives up to the 1.8 clamp
            v = rng.uniform(-0.3, 1.75, n)
        elif mode == 1:                                       # packed around the rules, with repeats (ties)
            v = np.concatenate([rng.choice(RULE_VALUES, n // 2), rng.uniform(0.88, 1.02, n - n // 2)])
        elif mode == 2:
            v = rng.uniform(0.2, 1.25, n)
        else:                                                 # one value for the whole list
            v = np.full(n, [0.95, 0.6, 1.2, -0.1, 0.3][(q // 4) % 5])
        v = np.sort(v)[::-1].copy()
        if mode == 2 and n >= 65:
            v[64] = v[63]                                     # tie across the slot boundary
            j0 = q % (n - 64)
            v[j0:j0 + 65] = v[j0]                             # lane j0: both of its slots (j0, j0 + 64) tie
        adj[q, :n] = v
    return ids, adj, nhit


def _hier_service(weights):
    from rag_project_icd10_amd.services.hierarchical_similarity_service import HierarchicalSimilarityService
    if weights == "default":
        return HierarchicalSimilarityService()
    # tuned: update_weights (renormalised to sum 1), and an embedding service present (semantic coherence 0.3, not 0.5)
    hs = HierarchicalSimilarityService(embedding_service=object())
    hs.update_weights({"hierarchy_boost": 0.31, "semantic_coherence": 0.17, "context_relevance": 0.07, "vector_similarity": 0.4})
    assert abs(sum(hs.factor_weights.values()) - 1.0) < 1e-12 and hs.device_weights()[5] == 0.3
    return hs


@functools.lru_cache(maxsize=None)
def _rescored(k, weights, id_base, nstr):
    """(strings, ids, adj, raw, nhit, tags, device outputs) of one rescoring case; the device tensors stay on the GPU"""
    import torch
    strings = list(_strings()[:nstr - len(EDGE)]) + EDGE
    ids, adj, nhit = _hit_lists(k, len(strings), id_base, seed=1000 + k + (id_base > 0))
    raw = np.where(ids >= 0, adj / 1.2, -np.inf).astype(np.float32)
    hs = _hier_service(weights)
    tags = torch.from_numpy(np.asarray([hs.row_tag(c) for c in _row_codes()], np.uint8)).cuda()
    d_ids, d_adj, d_raw = (torch.from_numpy(x).cuda() for x in (ids, adj, raw))
    outs = hs.rescore_live_hits_batch(strings, d_adj, d_ids, tags, id_base=id_base)
    torch.cuda.synchronize()
    return strings, hs, ids, adj, raw, nhit, (d_ids, d_adj, d_raw), outs


RESCORE_CASES = [  # k, weights, id_base, strings
    (1, "default", 0, 300), (2, "default", BIG_BASE, 300), (10, "default", 0, 300), (20, "default", 0, 1005),
    (20, "tuned", BIG_BASE, 300), (63, "default", BIG_BASE, 300), (64, "default", 0, 300), (65, "tuned", BIG_BASE, 300),
    (100, "default", 0, 1005), (100, "tuned", BIG_BASE, 1005), (127, "default", 0, 300), (128, "default", BIG_BASE, 300),
    (128, "tuned", 0, 300),
]


@pytest.mark.parametrize("k,weights,id_base,nstr", RESCORE_CASES)
def test_device_rescoring_matches_host_at_every_k(k, weights, id_base, nstr):
    """icd_hier_rescore against batch_calculate_similarities, string by string: final order, enhanced score, the record's
    score after the uncertainty boost, the boost, the six factors (bit for bit), and -1 / -inf behind the hits; the
    confidence statistics over the rescored order (icd_score_stats) against the service's per-call numpy methods"""
    from rag_project_icd10_amd.services.hierarchical_similarity_service import SimilarityFactors
    from rag_project_icd10_amd.services.multidimensional_confidence_service import MultiDimensionalConfidenceService
    strings, hs, ids, adj, raw, nhit, _dev, outs = _rescored(k, weights, id_base, nstr)
    order, enh, score, vs, hb, boost = (t.cpu().numpy() for t in outs)
    assert order.shape == (len(strings), k)
    codes = _row_codes()
    sc = 0.3 if hs.embedding_service else 0.5
    cross_boost = tie_at_64 = outside = 0
    for q, text in enumerate(strings):
        n = int(nhit[q])
        assert (ids[q, :n] >= 0).all() and (ids[q, n:] < 0).all()
        hits = []
        for j in range(n):
            r = int(ids[q, j]) - id_base
            inside = 0 <= r < NROWS
            outside += not inside
            code = codes[r] if inside else _outside_code(int(ids[q, j]))
            hits.append({"code": code, "title": f"合成{r}", "score": float(adj[q, j]), "original_score": float(raw[q, j]),
                         "metadata": {"level": 1 + r % 3, "parent_code": "", "category_path": "", "semantic_text": "",
                                      "has_complication": False, "main_code": "", "secondary_code": ""}})
        pos = {h["code"]: j for j, h in enumerate(hits)}
        assert len(pos) == n
        want = hs.batch_calculate_similarities(text, {}, [dict(h) for h in hits])
        assert len(want) == n, text
        assert (order[q, n:] == -1).all() and (enh[q, n:] == -np.inf).all() and (score[q, n:] == -np.inf).all(), (text, n)
        assert (vs[q, n:] == 0).all() and (hb[q, n:] == 0).all() and (boost[q, n:] == 0).all(), (text, n)
        ctx = hs.query_params(text)[1]
        for j, (rec, s_host, f_host) in enumerate(want):
            assert order[q, j] == pos[rec["code"]], (text, j)                            # final order (stable sorts included)
            assert enh[q, j] == s_host == rec["enhanced_score"], (text, j)               # bit-exact doubles
            assert score[q, j] == rec["score"], (text, j)                                # after the uncertainty boost
            assert boost[q, j] == rec.get("uncertainty_boost", 0.0), (text, j)
            assert SimilarityFactors(vs[q, j], hb[q, j], 0.0, sc, 0.0, ctx) == f_host, (text, j)
            cross_boost += bool(boost[q, j] > 0 and (j < 64) != (order[q, j] < 64))
        tie_at_64 += bool(n >= 65 and enh[q, 63] == enh[q, 64])
    # what the cases were made to reach did happen: hits moved across the slot boundary by the boosted re-sort, ties of the
    # final score that straddle it, and ids outside the tag table
    if k >= 66:
        assert cross_boost > 0 and tie_at_64 > 0, (cross_boost, tie_at_64)
    assert outside > 0
    if k >= 63:
        cs = MultiDimensionalConfidenceService()
        for use in sorted({1, 50, k}):
            st = cs.score_statistics_batch(outs[1], outs[0], top_k=use).cpu().numpy()
            for q in range(len(strings)):
                recs = [{"score": float(x)} for x in enh[q, :min(use, int(nhit[q]))]]
                assert st[q, 4] == cs._assess_model_uncertainty(recs), (k, use, q)
                assert st[q, 5] == cs._calculate_prediction_variance(None, recs), (k, use, q)


def test_device_rescoring_refuses_k_outside_1_to_128():
    import ctypes as C
    import torch
    lib = _native.load_library()
    nq = 4
    adj = torch.zeros((nq, 129), dtype=torch.float64, device="cuda")
    ids = torch.zeros((nq, 129), dtype=torch.int64, device="cuda")
    tags = torch.zeros(16, dtype=torch.uint8, device="cuda")
    qp = torch.zeros((nq, 12), dtype=torch.float64)
    w = [0.2, 0.15, 0.08, 0.04, 0.03, 0.5, 0.045]
    with pytest.raises(IcdError, match="k=129"):
        _native.hier_rescore(adj, ids, tags, qp, w)
    # k = 0 with valid buffers (a [nq, 0] tensor has no storage to point at): the entry point itself refuses it
    order = torch.empty((nq, 1), dtype=torch.int32, device="cuda")
    outs = [torch.empty((nq, 1), dtype=torch.float64, device="cuda") for _ in range(5)]
    qpd = qp.cuda()
    wd = (C.c_double * 7)(*w)
    rc = lib.icd_hier_rescore(0, adj.data_ptr(), ids.data_ptr(), nq, 0, 0, tags.numel(), tags.data_ptr(), qpd.data_ptr(),
                              C.cast(wd, C.c_void_p), order.data_ptr(), *[t.data_ptr() for t in outs], None)
    assert rc != 0 and b"k=0" in lib.icd_last_error()
    torch.cuda.synchronize()


# ---- 2. icd_pack_winners on the rescoring's real outputs ------------------------------------------------------------------
@pytest.mark.parametrize("k,kk", [(100, 1), (100, 50), (100, 100), (128, 128)])
def test_pack_winners_at_the_live_sizes(k, kk):
    """the winners of real rescored lists (short lists included) in one [8, nq, kk] array: every plane equals the torch
    gather / slice it stands for"""
    import torch
    case = (k, "default", 0, 1005) if k == 100 else (k, "default", BIG_BASE, 300)
    _s, _hs, _ids, _adj, _raw, nhit, (ids, adj, raw), (order, enh, _score, vs, hb, boost) = _rescored(*case)
    assert (nhit < k).any() and (nhit == 0).any()
    out = _native.pack_winners(order, ids, raw, adj, enh, vs, hb, boost, kk).cpu()
    assert out.shape == (8, len(nhit), kk)
    o = order[:, :kk].long().clamp(min=0)
    assert torch.equal(out[0].contiguous().view(torch.int64), torch.gather(ids, 1, o).cpu())
    assert torch.equal(out[1], torch.gather(raw, 1, o).double().cpu()) and torch.equal(out[2], torch.gather(adj, 1, o).cpu())
    assert torch.equal(out[3], order[:, :kk].double().cpu())
    for plane, t in zip((4, 5, 6, 7), (enh, vs, hb, boost)):
        assert torch.equal(out[plane], t[:, :kk].cpu())
    with pytest.raises(IcdError):
        _native.pack_winners(order, ids, raw, adj, enh, vs, hb, boost, k + 1)


# ---- 3. icd_merge_topk against the oracle on the undivided corpus -------------------------------------------------------
MERGE_N = 4000


@functools.lru_cache(maxsize=None)
def _merge_data():
    """corpus whose rows 0..299 reappear as rows 3700..3999 (exact fp32 score ties in different shards of every split
    below), queries half near those rows (the ties are among the best hits) and half random"""
    corpus = unit_rows(MERGE_N, 768, 71)
    corpus[MERGE_N - 300:] = corpus[:300]
    levels = icd_levels(MERGE_N, 72)
    rng = np.random.default_rng(73)
    near = corpus[np.arange(0, 288, 9)] + 0.02 * rng.standard_normal((32, 768)).astype(np.float32)
    near /= np.linalg.norm(near, axis=1, keepdims=True)
    queries = np.ascontiguousarray(np.concatenate([near, unit_rows(32, 768, 74)]), dtype=np.float32)
    return corpus, levels, queries


def _bounds(G, k):
    """uneven row splits: a shard with fewer rows than k, and (G = 8, and G = 2 at k = 1) a shard with no rows at all"""
    if G == 1:
        sizes = [MERGE_N]
    elif G == 2:
        sizes = [k - 1, MERGE_N - (k - 1)]
    elif G == 3:
        sizes = [1700, k // 2 + 1, MERGE_N - 1701 - k // 2]
    else:
        sizes = [611, 0, max(k - 1, 1), 977, 250, 1, 1200]
        sizes.append(MERGE_N - sum(sizes))
    assert len(sizes) == G and sum(sizes) == MERGE_N and min(sizes) >= 0
    lo = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return [(int(a), int(a + s)) for a, s in zip(lo, sizes)]


def _gathered(oracle, corpus, levels, queries, G, k):
    sc = np.empty((G, len(queries), k), np.float32)
    ids = np.empty((G, len(queries), k), np.int64)
    for g, (lo, hi) in enumerate(_bounds(G, k)):
        sc[g], ids[g] = oracle.flat_ip_topk(corpus[lo:hi], queries, k, id_base=lo)
    lv = np.where(ids >= 0, levels[np.clip(ids, 0, None)], 0).astype(np.int32)
    return sc, ids, lv


def _merge(sc, ids, lv, k):
    import torch
    out = _native.merge_topk(*(torch.from_numpy(x).cuda() for x in (sc, ids, lv)), k)
    return tuple(t.cpu().numpy() for t in out)


def _assert_equal_outputs(got, want):
    adj, raw, ids, lv = got
    assert np.array_equal(ids, want[2]), f"id mismatch rows {np.nonzero((ids != want[2]).any(1))[0][:5]}"
    assert _bits(adj) == _bits(want[0]) and _bits(raw) == _bits(want[1]) and np.array_equal(lv, want[3])


@pytest.mark.parametrize("k", [1, 10, 64, 65, 100, 128])
@pytest.mark.parametrize("G", [1, 2, 3, 8])
def test_merge_kernel_equals_the_oracle_on_the_whole_corpus(oracle, G, k):
    assert G * k <= 1024
    corpus, levels, queries = _merge_data()
    sc, ids, lv = _gathered(oracle, corpus, levels, queries, G, k)
    if G == 8:
        assert (ids[1] < 0).all() and ((ids[2] >= 0).sum(1).max() < k or k == 1)    # a shard without rows, one with fewer than k
    want = oracle.reweight(*oracle.flat_ip_topk(corpus, queries, k), levels)
    got = _merge(sc, ids, lv, k)
    _assert_equal_outputs(got, want)
    # the near queries' best hit and its copy tie in fp32 and lie in different shards (G > 1): the lower id wins
    raw_s, raw_i = oracle.flat_ip_topk(corpus, queries[:32], 2)
    assert (raw_s[:, 0] == raw_s[:, 1]).all() and (raw_i[:, 1] == raw_i[:, 0] + MERGE_N - 300).all()
    if k == 1:
        assert (got[2][:32, 0] < 300).all()


@pytest.mark.parametrize("G,k", [(8, 128), (3, 65), (2, 100)])
def test_merge_kernel_drops_nan_scores(oracle, G, k):
    """NaN scores with valid ids in the gathered lists are dropped, as the oracle drops them (oracle.merge); queries without
    one are untouched"""
    corpus, levels, queries = _merge_data()
    sc, ids, lv = _gathered(oracle, corpus, levels, queries, G, k)
    full = [g for g in range(G) if (ids[g] >= 0).all()]
    sc[full[0], 0, 0] = np.nan                                # the best hit of a shard
    sc[full[-1], 1, 60:70] = np.nan                           # around a lane's two slots
    sc[full[-1], 2, :] = np.nan                               # a whole list
    sc[full[0], 33, k - 1] = np.nan                           # the last one
    sc[full[0], 34, 64 % k] = np.nan
    got = _merge(sc, ids, lv, k)
    m_s, m_i = oracle.merge(sc, ids, k)
    _assert_equal_outputs(got, oracle.reweight(m_s, m_i, levels))
    nan_ids = {(int(q), int(ids[g, q, j])) for g, q, j in zip(*np.nonzero(np.isnan(sc)))}
    assert len(nan_ids) >= k + 4 and not any((q, int(i)) in nan_ids for q in range(len(queries)) for i in got[2][q])
    clean = np.setdiff1d(np.arange(len(queries)), [0, 1, 2, 33, 34])
    want = oracle.reweight(*oracle.flat_ip_topk(corpus, queries[clean], k), levels)
    _assert_equal_outputs(tuple(x[clean] for x in got), want)


def test_merge_kernel_refuses_more_than_1024_candidates():
    import torch
    for G, k in ((9, 128), (1, 129)):
        sc = torch.zeros((G, 4, k), dtype=torch.float32, device="cuda")
        ids = torch.zeros((G, 4, k), dtype=torch.int64, device="cuda")
        lv = torch.ones((G, 4, k), dtype=torch.int32, device="cuda")
        with pytest.raises(IcdError, match=f"k={k}"):
            _native.merge_topk(sc, ids, lv, k)


def test_merge_of_eight_real_shards_at_k100(oracle):
    """8 IcdIndex shards on one GPU with global id_base (uneven, one of 7 rows), searched on the device at k = 100,
    levels by lookup_levels, merged: the same four outputs as one index over the whole corpus and as the oracle"""
    import torch
    corpus, levels, queries = _merge_data()
    k = 100
    sizes = [611, 37, 99, 977, 250, 7, 1200]
    sizes.append(MERGE_N - sum(sizes))
    dq = torch.from_numpy(queries).cuda()
    parts, lo = [], 0
    for s in sizes:
        sh = IcdIndex(corpus[lo:lo + s], levels[lo:lo + s], max_nq=len(queries), max_k=k, id_base=lo)
        ps, pi = sh.search(dq, k)
        parts.append((ps, pi, sh.lookup_levels(pi)))
        torch.cuda.synchronize()
        sh.close()
        lo += s
    got = _native.merge_topk(*(torch.stack([p[i] for p in parts]) for i in range(3)), k)
    got = tuple(t.cpu().numpy() for t in got)
    want = oracle.reweight(*oracle.flat_ip_topk(corpus, queries, k), levels)
    _assert_equal_outputs(got, want)
    full = IcdIndex(corpus, levels, max_nq=len(queries), max_k=k)
    _assert_equal_outputs(got, tuple(t.cpu().numpy() for t in full.search_reweighted(dq, k)))
    full.close()


# ---- 4. match_diagnoses_batch end to end --------------------------------------------------------------------------------
def _records(n, levels, seed):
    """codes of every chapter letter, letters outside the table, '.9' codes and codes without a dot"""
    letters = "ABCEIJKNSZQXO"
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        L = letters[i % len(letters)]
        tail = ".9" if i % 5 == 0 else f".{rng.integers(0, 9)}"
        code = f"{L}{i % 100:02d}" + ("" if i % 17 == 0 else tail + f"{i:05d}")
        recs.append({"code": code, "preferred_zh": f"合成疾病{seed}-{i}", "level": int(levels[i]), "parent_code": "",
                     "category_path": "", "semantic_text": f"合成疾病{i}"})
    return recs


@pytest.fixture(scope="module")
def services(tmp_path_factory):
    """synthetic-weights EmbeddingService; a ~6 000-row store whose first rows are embeddings of the test strings and of
    perturbed copies (scores near 1.0 and near the 0.95 rule), and a 70-row store (100 hits with 70 valid ones)"""
    import torch
    from rag_project_icd10_amd.services.embedding_service import EmbeddingService
    from rag_project_icd10_amd.services.milvus_service import MilvusService
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    strings = list(_strings()[:300]) + EDGE
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MILVUS_DB_PATH", str(tmp_path_factory.mktemp("db")))
        mp.setenv("EMBEDDING_MODEL_NAME", "shibing624/text2vec-base-chinese")
        mp.setenv("ICD_EMBEDDING_ALLOW_SYNTHETIC", "1")
        for key in ("ICD_GPU_MAX_K", "ICD_GPU_MAX_BATCH"):
            mp.delenv(key, raising=False)
        es = EmbeddingService()
        assert es.batch_arithmetic() == "canonical"
        vecs = np.stack([es.encode_query(s) for s in strings]).astype(np.float32)
        rng = np.random.default_rng(5)
        near = vecs + 0.012 * rng.standard_normal(vecs.shape).astype(np.float32)
        near /= np.linalg.norm(near, axis=1, keepdims=True)
        n = 6000
        corpus = np.concatenate([vecs, near, unit_rows(n - 2 * len(strings), 768, 6)]).astype(np.float32)
        levels = icd_levels(n, 7)
        mp.setenv("MILVUS_COLLECTION_NAME", "icd10_rescoring")
        ms = MilvusService(embedding_service=es)
        recs = _records(n, levels, 1)
        for s0 in range(0, n, 500):
            assert ms.insert_records(recs[s0:s0 + 500], list(corpus[s0:s0 + 500]))
        assert ms.load_collection() and ms.client.count == n and ms.supports_device_rescoring()
        mp.setenv("MILVUS_COLLECTION_NAME", "icd10_short")
        ms70 = MilvusService(embedding_service=es)
        assert ms70.insert_records(_records(70, levels, 2), list(corpus[-70:])) and ms70.load_collection()
        yield {"es": es, "strings": strings, "vecs": vecs, "ms": ms, "md": MultiDiagnosisService(es, ms),
               "ms70": ms70, "md70": MultiDiagnosisService(es, ms70), "corpus": corpus, "levels": levels}
        torch.cuda.synchronize()


def _check_batch_against_one_at_a_time(svc, md, ms, strings, top_k, expect_n):
    batched = md.match_diagnoses_batch(strings, top_k=top_k, confidence_statistics=True)
    assert len(batched) == len(strings)
    assert [len(m.candidates) for m in batched] == [expect_n] * len(strings)     # no match is empty: two empty lists prove nothing
    cs = md.confidence_service
    for i, s in enumerate(strings):                                              # the reference call shape on every string
        hits = ms.search(svc["vecs"][i], top_k=2 * top_k)                         # (vecs[i] is encode_query(strings[i]))
        one = md._match_from_hits(s, hits, top_k)
        got = batched[i]
        assert [c.code for c in got.candidates] == [c.code for c in one.candidates], (s, top_k)
        for a, b in zip(got.candidates, one.candidates):
            assert a.score == b.score and a.enhanced_score == b.enhanced_score and a.original_score == b.original_score, s
            assert a.similarity_factors == b.similarity_factors and a.title == b.title, s
        assert got.match_confidence == one.match_confidence, s
        recs = [{"score": c.score} for c in one.candidates]
        cf = got.confidence_factors
        assert cf["model_uncertainty"] == cs._assess_model_uncertainty(recs), (s, top_k)
        assert cf["prediction_variance"] == cs._calculate_prediction_variance(None, recs), (s, top_k)
        assert abs(cf["semantic_coherence"] - cs.semantic_coherence(s, hits)) <= 1e-14, (s, top_k)
    return batched


@pytest.mark.parametrize("top_k", [1, 5, 32, 33, 50])
def test_match_diagnoses_batch_equals_one_at_a_time(services, top_k):
    """match_diagnoses_batch (encoder batch -> search of 2 top_k -> device rescoring -> winners -> Candidates, confidence
    statistics on) against encode_query + MilvusService.search + _match_from_hits per string, every field bit for bit"""
    batched = _check_batch_against_one_at_a_time(services, services["md"], services["ms"], services["strings"], top_k, top_k)
    # the strings' own rows and their perturbed copies: hits above the 0.95 rule reach the winners
    assert sum(1 for m in batched if m.candidates[0].similarity_factors.vector_similarity > 0.95) >= 50


def test_match_diagnoses_batch_on_a_70_row_store(services):
    """top_k = 50 on 70 rows: 100 hit slots of which 70 are valid (both slots of some lanes, none of others)"""
    _check_batch_against_one_at_a_time(services, services["md70"], services["ms70"], services["strings"], 50, 50)
    _adj, _raw, ids, _lv = services["ms70"].search_batch(services["vecs"][:4], 100)
    assert ((np.asarray(ids) >= 0).sum(1) == 70).all()


def test_match_diagnoses_batch_after_a_rebuild_with_the_same_row_count(services):
    """drop the 70-row collection and rebuild it in the same process with as many rows and other codes: the batched path
    returns the new codes (the code / title columns were once cached by row count alone)"""
    ms, md = services["ms70"], services["md70"]
    strings = services["strings"][:40]
    before = md.match_diagnoses_batch(strings, top_k=5)
    assert all(m.candidates and m.candidates[0].title.startswith("合成疾病2-") for m in before)
    assert ms.clear_collection() and ms.client.count == 0
    recs = _records(70, services["levels"], 3)
    for r in recs:
        r["code"] = "R" + r["code"]
    assert ms.insert_records(recs, list(services["corpus"][-70:])) and ms.load_collection() and ms.client.count == 70
    after = _check_batch_against_one_at_a_time(services, md, ms, strings, 5, 5)
    assert all(c.code.startswith("R") and c.title.startswith("合成疾病3-") for m in after for c in m.candidates)
