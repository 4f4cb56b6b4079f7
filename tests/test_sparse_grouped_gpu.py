"""icd_sparse_search_grouped on the device against tests/grouped_hybrid_oracle.py, bit for bit: ids, raw
scores, levels, groups and adj, raw and reweighted. The arithmetic is fully specified, so there is no tolerance. Shapes sit around
the sparse kernel's tile (T rows, from the build) and the grouping's 512-query block; the full ranking of a corpus and batch is
computed once and shared by every grouping and (k, s) checked on it."""
import ctypes
import functools

import numpy as np
import pytest

import grouped_hybrid_oracle as gho
import sparse_oracle as so
from rag_project_icd10_amd import _native
from rag_project_icd10_amd.services import sparse_text
from test_sparse_search_gpu import build, make_queries, make_rows, tile

pytestmark = pytest.mark.gpu

KS = [(1, 1), (10, 1), (10, 3), (4, 32), (128, 1)]
NAMES5 = ("adj", "raw", "ids", "levels", "groups")


def groupings(n, seed):
    """the four shapes of a grouping: every row its own group (ids in another order than the rows), one group, three unbalanced
    groups, and ~n / 4 families whose rows are interleaved over the whole index, so that a group spans the tiles"""
    rng = np.random.default_rng(seed)
    fam = max(n // 4, 1)
    return {"own": rng.permutation(n).astype(np.int32),
            "one": np.full(n, 7, np.int32),
            "three": np.where(np.arange(n) < 5, 2, np.where(np.arange(n) % 10 == 0, 0, 9)).astype(np.int32),
            "families": ((np.arange(n) * 7 + 3) % fam).astype(np.int32)}


def same(got, want, what):
    names = NAMES5[5 - len(want):]
    assert len(got) == len(want), what
    for g, w, name in zip(got, want, names):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero((g.view(np.uint8).reshape(g.shape[0], -1) != w.view(np.uint8).reshape(w.shape[0], -1)).any(axis=1))
        assert bad.size == 0, f"{what}: {name} differs in queries {bad[:8].tolist()}: {g[bad[0]][:6]} vs {w[bad[0]][:6]}"


def padded(out, q, hits):
    """a raw-form answer of query q ends in padding behind `hits` slots"""
    raw, ids, lv, grp = out
    return (ids[q, :hits] >= 0).all() and (ids[q, hits:] == -1).all() and np.isneginf(raw[q, hits:]).all() and (lv[q, hits:] == 0).all() \
        and (grp[q, hits:] == -1).all()


# ((a, b): n = a * T + b, vocabulary, batch)
CASES = [((1, -1), 1, 17), ((1, 37), 37, 17), ((2, 5), 5000, 17), ((1, 37), 5000, 1), ((1, -1), 37, 600)]


@functools.lru_cache(maxsize=None)
def reference(case):
    """rows, queries and the full ranking of a case (unmasked), computed once"""
    (a, b), vocab, nq = CASES[case]
    n = a * tile() + b
    rows = make_rows(n, vocab, 40 + case)
    q = make_queries(nq, vocab, 90 + case)
    raw, ids = gho.sparse_ranking(*rows, vocab, *q)
    for x in (raw, ids):
        x.setflags(write=False)
    return n, vocab, nq, rows, q, raw, ids


@pytest.mark.parametrize("kind", ["own", "one", "three", "families"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_grouped_sparse_search_equals_the_oracle(case, kind):
    import torch
    n, vocab, nq, rows, q, r_raw, r_ids = reference(case)
    id_base = 1000 if case % 2 else 0
    index, sp, rows_b, levels = build(n, vocab, 40 + case, id_base, max_nq=640)
    assert all(np.array_equal(x, y) for x, y in zip(rows, rows_b))
    group_of = groupings(n, case)[kind]
    grouping = index.grouping(group_of)
    dq = (torch.from_numpy(q[0]).cuda(), torch.from_numpy(q[1].view(np.int32)).cuda(), torch.from_numpy(q[2]).cuda())
    ranking = gho.Ranking(r_raw, r_ids, group_of)
    for k, s in (KS if nq < 600 else [(10, 3), (128, 1)]):
        for rw in (False, True):
            want = gho.grouped_from(ranking, k, s, levels, id_base, rw)
            same(index.search_sparse(sp, *q, k, reweighted=rw, grouping=grouping, group_size=s), want, f"host, k={k} s={s} rw={rw}")
        got = index.search_sparse(sp, *dq, k, reweighted=True, grouping=grouping, group_size=s)
        assert all(g.is_cuda for g in got)
        same(got, want, f"device, k={k} s={s}")
    # what the adversarial queries are there for (query 1 has no term; with a vocabulary: term 3 is in no row, term 1 in one row
    # per tile, [4, 5, 6] sums to 0 and term 2 times 2.0 lies below zero on every row that carries it)
    if nq >= 17:
        out = index.search_sparse(sp, *q, 10, grouping=grouping, group_size=3)
        assert padded(out, 1, 0)
        if vocab >= 37:
            assert padded(out, 5, 0)
            once = np.arange(5, n, tile())
            g_hit = len(np.unique(group_of[once]))
            assert g_hit < 10 and padded(out, 3, sum(min(3, int((group_of[once] == g).sum())) for g in np.unique(group_of[once])))
            assert (out[0][6][out[1][6] >= 0] == 0.0).all() and (out[1][6] >= 0).any()     # sums of zero are hits
            assert (out[0][4][out[1][4] >= 0] < 0).all() and (out[1][4] >= 0).any()        # hits below zero are hits
    for x in (grouping, sp, index):
        x.close()


def test_identities_with_the_ungrouped_search():
    """G3: every row its own group at s = 1 IS icd_sparse_search at k; one group at s = m IS icd_sparse_search at k = m"""
    n, vocab, nq = tile() + 37, 37, 17
    index, sp, rows, levels = build(n, vocab, 61)
    q = make_queries(nq, vocab, 62)
    gs = groupings(n, 5)
    own, one = index.grouping(gs["own"]), index.grouping(gs["one"])
    for rw in (False, True):
        for k in (1, 10, 128):
            plain = index.search_sparse(sp, *q, k, reweighted=rw)
            got = index.search_sparse(sp, *q, k, reweighted=rw, grouping=own, group_size=1)
            same(got[:-1], plain, f"own groups, k={k} rw={rw}")
            ids = got[2] if rw else got[1]
            assert np.array_equal(got[-1], np.where(ids >= 0, gs["own"][np.clip(ids, 0, None)], -1))
        for m in (1, 32, 128):
            plain = index.search_sparse(sp, *q, m, reweighted=rw)
            same(index.search_sparse(sp, *q, 1, reweighted=rw, grouping=one, group_size=m)[:-1], plain, f"one group, s={m} rw={rw}")
    for x in (own, one, sp, index):
        x.close()


def test_ties_in_one_group_and_over_500_groups():
    """rows 100 .. 599 are identical: as ONE group its members come back in id order; spread over 500 groups the groups do"""
    n, vocab = tile() + 700, 37
    index, sp, rows, levels = build(n, vocab, 7)
    q = sparse_text.csr_from_pairs([(np.array([0], np.uint32), np.ones(1, np.float32)), (np.array([4, 5, 6], np.uint32), np.ones(3, np.float32))])
    block = index.rowmask(np.arange(100, 600))
    dense = np.zeros(n, bool)
    dense[100:600] = True
    r_raw, r_ids = gho.sparse_ranking(*rows, vocab, *q, masks=[dense, dense])
    f_raw, f_ids = gho.sparse_ranking(*rows, vocab, *q)
    together = np.where((np.arange(n) >= 100) & (np.arange(n) < 600), 1, 0).astype(np.int32)
    apart = np.arange(n, dtype=np.int32)[::-1].copy()
    for group_of, (k, s), first in ((together, (1, 128), 128), (together, (4, 32), 32), (apart, (128, 1), 128), (apart, (10, 3), 10)):
        grouping = index.grouping(group_of)
        for masks, rr, ri in ((block, r_raw, r_ids), (None, f_raw, f_ids)):
            ranking = gho.Ranking(rr, ri, group_of)
            for rw in (False, True):
                want = gho.grouped_from(ranking, k, s, levels, 0, rw)
                same(index.search_sparse(sp, *q, k, masks=masks, reweighted=rw, grouping=grouping, group_size=s), want, f"k={k} s={s} rw={rw}")
        raw, ids, _, grp = index.search_sparse(sp, *q, k, masks=block, grouping=grouping, group_size=s)
        assert np.array_equal(ids[0, :first], np.arange(100, 100 + first)) and (raw[0, :first] == raw[0, 0]).all()   # ties: id order
        grouping.close()
    for x in (block, sp, index):
        x.close()


def test_masks_with_none_mixed_in_and_a_group_masked_out():
    n, vocab, k, s, nq = 2 * tile() + 5, 37, 10, 3, 17
    index, sp, rows, levels = build(n, vocab, 11)
    q = make_queries(nq, vocab, 12)
    group_of = groupings(n, 3)["families"]
    grouping = index.grouping(group_of)
    free = index.search_sparse(sp, *q, k, grouping=grouping, group_size=s)
    rng = np.random.default_rng(3)
    dense = []
    for i in range(nq):
        if i % 5 == 1:
            dense.append(None)                                            # a NULL among them
        elif i == 4:
            dense.append(np.zeros(n, bool))                               # an empty mask
        elif i % 5 == 0 and free[1][i][0] >= 0:
            dense.append(group_of != free[3][i][0])                       # the unmasked best GROUP, every row of it
        else:
            dense.append(rng.random(n) < (0.5 if i % 2 else 0.01))
    masks = [None if m is None else index.rowmask(np.flatnonzero(m)) for m in dense]
    ranking = gho.Ranking(*gho.sparse_ranking(*rows, vocab, *q, masks=dense), group_of)
    for rw in (False, True):
        want = gho.grouped_from(ranking, k, s, levels, 0, rw)
        same(index.search_sparse(sp, *q, k, masks=masks, reweighted=rw, grouping=grouping, group_size=s), want, f"masked, reweighted={rw}")
    got = index.search_sparse(sp, *q, k, masks=masks, grouping=grouping, group_size=s)
    assert padded(got, 4, 0)
    for i in range(0, nq, 5):
        if free[1][i][0] >= 0:
            assert free[3][i][0] not in got[3][i], "a group whose rows are all masked out is never emitted"
    same(index.search_sparse(sp, *q, k, masks=[None] * nq, grouping=grouping, group_size=s), free, "an all-NULL table")
    for m in masks:
        if m is not None:
            m.close()
    for x in (grouping, sp, index):
        x.close()


def test_pairing_is_explicit_once_and_leaves_an_unpaired_grouping_alone():
    lib = _native.load_library()
    index, sp, rows, levels = build(700, 37, 21, max_nq=8)
    group_of = groupings(700, 1)["families"]
    grouping, never = index.grouping(group_of), index.grouping(group_of)
    before = grouping.stats()
    q = make_queries(4, 37, 22)
    raw, ids, lv, grp = (np.empty((4, 8), np.float32), np.empty((4, 8), np.int64), np.empty((4, 8), np.int32), np.empty((4, 8), np.int32))
    unpaired = lib.icd_sparse_search_grouped(index._h, sp._h, grouping._h, q[0].ctypes.data, q[1].ctypes.data, q[2].ctypes.data, 4, 4, 2, 0, None, 0,
                                             None, raw.ctypes.data, ids.ctypes.data, lv.ctypes.data, grp.ctypes.data, 0, None)
    assert unpaired == -5 and b"paired" in lib.icd_last_error()   # ICD_ERR_STATE
    index.search_sparse(sp, *q, 4, grouping=grouping, group_size=2)
    after = grouping.stats()
    assert after["bytes"] == before["bytes"] + 700 * 4 and after["groups"] == before["groups"]
    assert lib.icd_grouping_pair_sparse(index._h, grouping._h, sp._h) == 0 and grouping.stats() == after   # idempotent
    assert never.stats() == before
    for x in (grouping, never, sp, index):
        x.close()


def test_refusals_of_the_abi_in_one_process():
    lib = _native.load_library()
    index, sp, rows, levels = build(300, 37, 21, max_nq=8)
    other, sp_other, _, _ = build(300, 37, 22, max_nq=8)
    group_of = (np.arange(300) % 11).astype(np.int32)
    grouping, g_other, g_small = index.grouping(group_of), other.grouping(group_of), index.grouping(group_of, max_nq=2)
    pair = lib.icd_grouping_pair_sparse
    assert pair(index._h, grouping._h, sp_other._h) == -1 and b"another index" in lib.icd_last_error()
    assert pair(index._h, g_other._h, sp._h) == -1 and pair(other._h, grouping._h, sp._h) == -1
    assert pair(index._h, grouping._h, sp._h) == 0 and pair(index._h, g_small._h, sp._h) == 0 and pair(other._h, g_other._h, sp_other._h) == 0
    q_off = np.array([0, 2], np.int64)
    q_t = np.array([0, 5], np.uint32)
    q_v = np.array([1.0, 2.0], np.float32)
    raw, ids, lv, grp, adj = (np.empty((8, 128), np.float32), np.empty((8, 128), np.int64), np.empty((8, 128), np.int32), np.empty((8, 128), np.int32),
                              np.empty((8, 128), np.float64))

    def search(idx_h, sp_h, g_h, off=q_off, t=q_t, v=q_v, nq=1, k=4, s=2, masks=None, rw=0, a=adj):
        return lib.icd_sparse_search_grouped(idx_h, sp_h, g_h, off.ctypes.data, t.ctypes.data, v.ctypes.data, nq, k, s, 0, masks, rw,
                                             a.ctypes.data if a is not None else None, raw.ctypes.data, ids.ctypes.data, lv.ctypes.data,
                                             grp.ctypes.data, 0, None)
    assert search(index._h, sp._h, grouping._h) == 0
    for k, s in ((0, 1), (1, 0), (129, 1), (1, 129), (10, 13), (64, 3)):
        assert search(index._h, sp._h, grouping._h, k=k, s=s) == -1 and b"k * group_size" in lib.icd_last_error()
    assert search(index._h, sp._h, grouping._h, k=128, s=1) == 0 and search(index._h, sp._h, grouping._h, k=4, s=32) == 0
    assert search(index._h, sp._h, grouping._h, t=np.array([5, 0], np.uint32)) == -1 and b"strictly increasing" in lib.icd_last_error()
    assert search(index._h, sp._h, grouping._h, t=np.array([0, 37], np.uint32)) == -1 and b"vocabulary" in lib.icd_last_error()
    assert search(index._h, sp._h, grouping._h, v=np.array([1.0, 0.0], np.float32)) == -1
    assert search(index._h, sp._h, grouping._h, off=np.zeros(10, np.int64), nq=9) == -1 and b"max_nq" in lib.icd_last_error()
    assert search(index._h, sp._h, g_small._h, off=np.zeros(4, np.int64), nq=3) == -1 and b"grouping's max_nq" in lib.icd_last_error()
    assert search(index._h, sp._h, grouping._h, rw=1, a=None) == -1
    assert search(index._h, sp_other._h, grouping._h) == -1 and b"another index" in lib.icd_last_error()
    assert search(index._h, sp._h, g_other._h) == -1 and b"another index" in lib.icd_last_error()
    assert search(other._h, sp._h, grouping._h) == -1
    view = index.view(np.arange(0, 300, 2))
    assert search(view._h, sp._h, grouping._h) == -1 and b"another index" in lib.icd_last_error()   # (a view is another index: no sparse handle is a view's)
    view.close()
    foreign = other.rowmask(np.arange(10))
    assert search(index._h, sp._h, grouping._h, masks=(ctypes.c_void_p * 1)(foreign._h.value)) == -1 and b"another index" in lib.icd_last_error()
    mine = index.rowmask(np.arange(10))
    assert search(index._h, sp._h, grouping._h, masks=(ctypes.c_void_p * 1)(mine._h.value)) == 0
    dead_mask = (ctypes.c_void_p * 1)(mine._h.value)
    mine.close()
    assert search(index._h, sp._h, grouping._h, masks=dead_mask) == -5   # ICD_ERR_STATE
    dead_g = ctypes.c_void_p(g_small._h.value)
    g_small.close()
    assert search(index._h, sp._h, dead_g) == -5 and pair(index._h, dead_g, sp._h) == -5
    with pytest.raises(ValueError):
        index.search_sparse(sp, q_off, q_t, q_v, 10, grouping=grouping, group_size=13)
    with pytest.raises(ValueError):
        index.search_sparse(sp, q_off, q_t, q_v, 10, group_size=2)
    with pytest.raises(_native.IcdError):
        index.search_sparse(sp, q_off, q_t, q_v, 4, grouping=g_small)
    for x in (foreign, g_other, sp_other, other, grouping, sp, index):
        x.close()


@pytest.mark.parametrize("first", ["index", "sparse", "grouping"])
def test_any_destruction_order(first):
    index, sp, rows, levels = build(500, 37, 31, max_nq=8)
    grouping = index.grouping((np.arange(500) % 9).astype(np.int32))
    q = make_queries(4, 37, 32)
    index.search_sparse(sp, *q, 3, grouping=grouping, group_size=2)
    handles = {"index": index, "sparse": sp, "grouping": grouping}
    handles[first].close()
    with pytest.raises(_native.IcdError):
        index.search_sparse(sp, *q, 3, grouping=grouping, group_size=2)
    for name in ("grouping", "index", "sparse"):
        handles[name].close()
    assert index.closed and sp.closed and grouping.closed


# ---- the service ------------------------------------------------------------------------------------------------------------------
from test_sparse_hybrid_gpu import services   # noqa: E402,F401  (the golden slice behind MilvusService, built once for this module)


def test_search_text_grouped_on_the_golden_slice(services):   # noqa: F811
    """search_text(..., group_by_field="parent_code") (main_code is unique per row of the slice; parent_code makes 81 families):
    codes, BM25 and reweighted scores, order and group values equal the oracle's
    for every title of the slice; with a filter the mask restricts the hits and the grouping stays the whole store's"""
    ms, recs = services["ms"], services["recs"]
    titles = [r["preferred_zh"] for r in recs]
    levels = np.array([r.get("level", 1) for r in recs], np.int32)
    parent = np.array([str(r.get("parent_code") or "") for r in recs])
    values, group_of = np.unique(parent, return_inverse=True)
    vocab, row_off, terms, vals, idf = so.bm25(titles)
    q = sparse_text.csr_from_pairs([so.bm25_query(t, vocab, idf) for t in titles])
    sel = np.array([r.get("level", 1) >= 2 for r in recs])
    for flt, masks, (k, s) in ((None, None, (5, 2)), ("level >= 2", [sel] * len(titles), (3, 4))):
        ranking = gho.Ranking(*gho.sparse_ranking(row_off, terms, vals, max(len(vocab), 1), *q, masks=masks), group_of)
        adj, raw, ids, _lv, grp = gho.grouped_from(ranking, k, s, levels, 0, True)
        siblings = 0
        for i, t in enumerate(titles):
            hits = ms.search_text(t, k, filter=flt, group_by_field="parent_code", group_size=s)
            m = int((ids[i] >= 0).sum())
            assert [h["code"] for h in hits] == [recs[j]["code"] for j in ids[i][:m]], t
            assert [h["original_score"] for h in hits] == [float(x) for x in raw[i][:m]] and [h["score"] for h in hits] == [float(x) for x in adj[i][:m]]
            assert [h["metadata"]["parent_code"] for h in hits] == [values[g] for g in grp[i][:m]]
            counts = np.unique(grp[i][:m], return_counts=True)[1]
            assert len(counts) <= k and (counts <= s).all()
            siblings += int((counts > 1).sum())
        assert siblings > 0   # (the slice is family-shaped: the group size matters)
    tx = ms.build_sparse_index()[1]
    out = ms.search_sparse_batch(*tx.encode_queries(titles[:5]), 5, group_by_field="parent_code", group_size=2)
    assert len(out) == 5 and out[2].shape == (5, 10)
    assert any(g["field"] == "parent_code" and g["filter"] is None for g in ms.groupings())
    with pytest.raises(ValueError):
        ms.search_text(titles[0], 10, group_by_field="parent_code", group_size=13)


def test_device_calls_with_masks_and_a_captured_graph():
    """device in / device out: with masks the bits are the host call's; without masks and with validate=False the call only
    enqueues, so it can be captured into a graph, and the replay gives the same bits"""
    import torch
    n, vocab, k, s, nq = tile() + 37, 37, 10, 3, 17
    index, sp, rows, levels = build(n, vocab, 51)
    q = make_queries(nq, vocab, 52)
    group_of = groupings(n, 2)["families"]
    grouping = index.grouping(group_of)
    dq = (torch.from_numpy(q[0]).cuda(), torch.from_numpy(q[1].view(np.int32)).cuda(), torch.from_numpy(q[2]).cuda())
    dense = [None if i % 3 == 0 else (np.arange(n) % (i + 2) != 0) for i in range(nq)]
    masks = [None if m is None else index.rowmask(np.flatnonzero(m)) for m in dense]
    ranking = gho.Ranking(*gho.sparse_ranking(*rows, vocab, *q, masks=dense), group_of)
    for rw in (False, True):
        got = index.search_sparse(sp, *dq, k, masks=masks, reweighted=rw, grouping=grouping, group_size=s)
        assert all(g.is_cuda for g in got)
        same(got, gho.grouped_from(ranking, k, s, levels, 0, rw), f"device call with masks, reweighted={rw}")
    want = gho.grouped_from(gho.Ranking(*gho.sparse_ranking(*rows, vocab, *q), group_of), k, s, levels, 0, True)
    same(index.search_sparse(sp, *dq, k, reweighted=True, validate=False, grouping=grouping, group_size=s), want, "validate=False")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        index.search_sparse(sp, *dq, k, reweighted=True, validate=False, grouping=grouping, group_size=s)   # warm-up on the capture stream
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cap = index.search_sparse(sp, *dq, k, reweighted=True, validate=False, grouping=grouping, group_size=s)
    for t in cap:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    same(cap, want, "graph replay")
    del graph
    for m in masks:
        if m is not None:
            m.close()
    for x in (grouping, sp, index):
        x.close()
