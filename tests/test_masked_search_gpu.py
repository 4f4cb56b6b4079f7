"""Masked search (run with -m gpu on an MI355X): IcdIndex.search_masked - a row mask per query, tested inside the exact kernels -
against a walk over the oracle's FULL ranking restricted to the query's mask (tests/mask_oracle.py), bit for bit, through all
three kernel forms (single launch, streaming, fp32 MFMA); against the view of the same rows; MilvusService with a filter per query."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from mask_oracle import as_bool, masked_batch, masked_pages, restrict
from test_grouped_search_gpu import N, NQ
from test_range_search_gpu import _parent

pytestmark = pytest.mark.gpu

from rag_project_icd10_amd import _native  # noqa: E402
from rag_project_icd10_amd._native import MODE_EXACT, IcdIndex  # noqa: E402
from rag_project_icd10_amd.services import range_search  # noqa: E402

BATCHES = (1, 2, 4, 40, NQ)   # single-launch form (1, 2, 4), streaming form (40), fp32-MFMA form (300)
KS = (1, 10, 100, 128)
ROWS = np.arange(N, dtype=np.int64)
HALF = ((ROWS * 2654435761) >> 7) & 1 == 1   # about half the rows, scattered
NOT_TILE0 = ROWS >= 128
LAST_TILE = ROWS >= 11904                    # inside the partial last tile only (96 rows)


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes()


class _Masks:
    """device masks of boolean selections, made once per (index, selection) and closed with the test"""

    def __init__(self, index):
        self.index, self.made = index, {}

    def __call__(self, sel):
        if sel is None:
            return None
        key = sel.tobytes()
        if key not in self.made:
            self.made[key] = self.index.rowmask(np.nonzero(sel)[0])
        return self.made[key]

    def close(self):
        for m in self.made.values():
            m.close()


def _cut(v, nq):
    if v is None:
        return None
    if isinstance(v, tuple):
        return tuple(_cut(x, nq) for x in v)
    return v[:nq] if hasattr(v, "__len__") else v


def _check(index, q, dev_masks, want, k, nq, what, **bounds):
    """search_masked of the first nq queries, raw and reweighted, against the first nq rows of `want` (masked_batch's result)"""
    b = {name: _cut(v, nq) for name, v in bounds.items()}
    got_raw = index.search_masked(q[:nq], k, dev_masks[:nq], reweighted=False, **b)
    got_adj = index.search_masked(q[:nq], k, dev_masks[:nq], reweighted=True, **b)
    for label, got, exp in (("raw", got_raw, want[0]), ("reweighted", got_adj, want[1])):
        assert len(got) == len(exp)
        for j, (g, w) in enumerate(zip(got, exp)):
            w = w[:nq]
            assert g.dtype == w.dtype and g.shape == w.shape, (what, label, j, g.dtype, w.dtype, g.shape, w.shape)
            assert _bits(g) == _bits(w), (what, label, j, nq, k, np.nonzero((g != w).any(1))[0][:5])


@pytest.mark.parametrize("kind", ["gauss", "family"])
def test_sparse_masks_a_post_filter_cannot_answer(oracle, kind):
    corpus, levels, q, index, s_all, i_all = _parent(kind, oracle)
    sels = [ROWS % 199 == (qi % 199) for qi in range(NQ)]
    # "search(k = 128), then filter" must not be able to pass: no query finds 10 selected rows in the plain top 128 ...
    in_top = np.array([int(sels[qi][i_all[qi, :128]].sum()) for qi in range(NQ)])
    print(f"{kind}: selected rows inside the plain top-128: max {in_top.max()}, mean {in_top.mean():.2f}")
    assert (in_top < 10).all()
    assert float((in_top >= 10).mean()) == 0.0
    # ... and at k = 100 / 128 every list is padded (a mask holds ~60 rows)
    assert max(int(s.sum()) for s in sels) < 100
    mk = _Masks(index)
    try:
        dev = [mk(s) for s in sels]
        for k in KS:
            want = masked_batch(s_all, i_all, levels, sels, k)
            if k >= 100:
                assert (want[0][1][:, -1] == -1).all()
            for nq in BATCHES:
                _check(index, q, dev, want, k, nq, (kind, "sparse"))
    finally:
        mk.close()


@pytest.mark.parametrize("kind", ["gauss", "family"])
def test_every_bit_position_of_the_tile(oracle, kind):
    """mask m = rows r % 128 == m: one row per tile, at every (t, h, r) slot of the MFMA tile's row mapping"""
    corpus, levels, q, index, s_all, i_all = _parent(kind, oracle)
    sels = [ROWS % 128 == m for m in range(128)]
    mk = _Masks(index)
    try:
        dev = [mk(s) for s in sels]
        for k in KS:
            want = masked_batch(s_all[:128], i_all[:128], levels, sels, k)
            for nq in (128, 40, 4):
                _check(index, q, dev, want, k, nq, (kind, "bit positions"))
    finally:
        mk.close()


@pytest.mark.parametrize("kind", ["gauss", "family"])
def test_mixed_batch(oracle, kind):
    corpus, levels, q, index, s_all, i_all = _parent(kind, oracle)
    mk = _Masks(index)
    try:
        for k in KS:
            exact = np.zeros(N, bool)
            exact[np.sort(np.random.default_rng(k).choice(N, k - 1, replace=False))] = True   # exactly k - 1 rows
            kinds = [None, "sparse", HALF, NOT_TILE0, LAST_TILE, exact, np.zeros(N, bool)]
            sels = [(ROWS % 199 == (qi % 199)) if isinstance(kinds[qi % 7], str) else kinds[qi % 7] for qi in range(NQ)]
            want = masked_batch(s_all, i_all, levels, sels, k)
            for qi in range(0, 14):
                m = int((want[0][1][qi] >= 0).sum())
                assert m == min(k, int(as_bool(sels[qi], N).sum())), (qi, k)
            dev = [mk(s) for s in sels]
            for nq in BATCHES:
                _check(index, q, dev, want, k, nq, (kind, "mixed"))
            # the unfiltered entries equal search_range without bounds
            plain = index.search_range(q, k, reweighted=False)
            got = index.search_masked(q, k, dev, reweighted=False)
            for a, b in zip(plain, got):
                assert _bits(a[0::7]) == _bits(b[0::7])
        # no mask on any query: search_range, bit for bit
        assert [_bits(a) for a in index.search_masked(q[:40], 10, [None] * 40)] == [_bits(a) for a in index.search_range(q[:40], 10)]
    finally:
        mk.close()


@pytest.mark.parametrize("kind", ["gauss", "family"])
def test_ties_follow_the_mask(oracle, kind):
    """rows 5000 + 2 j and 5001 + 2 j are exact duplicates and queries 0 .. 39 equal them: the masked-out twin never appears, and
    with both kept the order is id ascending"""
    corpus, levels, q, index, s_all, i_all = _parent(kind, oracle)
    twins = (ROWS >= 5000) & (ROWS < 5400)
    only_odd = ~(twins & (ROWS % 2 == 0))
    only_even = ~(twins & (ROWS % 2 == 1))
    both = np.ones(N, bool)
    mk = _Masks(index)
    try:
        for name, sel in (("odd", only_odd), ("even", only_even), ("both", both)):
            sels = [sel] * NQ
            dev = [mk(sel)] * NQ
            assert dev[0] is not None
            for k in KS + (2,):
                want = masked_batch(s_all, i_all, levels, sels, k)
                for nq in BATCHES:
                    _check(index, q, dev, want, k, nq, (kind, "ties", name))
            raw, ids, lv = index.search_masked(q[:40], 2, dev[:40], reweighted=False)
            j = np.arange(40)
            if name == "both":
                assert np.array_equal(ids[:, 0], 5000 + 2 * j) and np.array_equal(ids[:, 1], 5001 + 2 * j)
                assert _bits(raw[:, 0]) == _bits(raw[:, 1])
            else:
                gone = 5000 + 2 * j + (0 if name == "odd" else 1)
                assert np.array_equal(ids[:, 0], 5000 + 2 * j + (1 if name == "odd" else 0))
                wide = index.search_masked(q[:40], 128, dev[:40], reweighted=False)[1]
                assert not (wide == gone[:, None]).any()
    finally:
        mk.close()


@pytest.mark.parametrize("kind", ["gauss", "family"])
def test_mask_and_band_together(oracle, kind):
    corpus, levels, q, index, s_all, i_all = _parent(kind, oracle)
    mk = _Masks(index)
    try:
        sels, dev = [HALF] * NQ, [mk(HALF)] * NQ
        masked = [restrict(s_all[qi], i_all[qi], HALF) for qi in range(NQ)]
        ceil = np.array([m[0][200] for m in masked], np.float32)    # the query's score at rank 200 of the MASKED ranking
        floor = np.array([m[0][260] for m in masked], np.float32)
        on_in = (np.array([m[0][5] for m in masked], np.float32), np.array([m[1][5] for m in masked], np.int64))
        out_pos = [int(np.nonzero(~HALF[i_all[qi]])[0][3]) for qi in range(NQ)]   # a masked-OUT row near the top of the full ranking
        on_out = (np.array([s_all[qi, p] for qi, p in enumerate(out_pos)], np.float32),
                  np.array([i_all[qi, p] for qi, p in enumerate(out_pos)], np.int64))
        for bounds in ({"range_filter": ceil}, {"radius": floor, "range_filter": ceil}, {"after": on_in}, {"after": on_out},
                       {"after": on_in, "radius": floor}):
            for k in KS:
                want = masked_batch(s_all, i_all, levels, sels, k, **bounds)
                for nq in BATCHES:
                    _check(index, q, dev, want, k, nq, (kind, sorted(bounds)), **bounds)
        # the iterator over a mask: the pages of the restricted ranking, until exhausted
        for sel, bs, qi in ((ROWS % 16 == 3, 7, 1), (HALF, 128, 45)):
            want_pages = masked_pages(s_all[qi], i_all[qi], sel, bs)
            assert sum(len(p) for p in want_pages) == int(sel.sum())
            it = range_search.SearchIterator((index, mk(sel)), q[qi], bs, -1, None, None, lambda adj, raw, ids: list(ids), lambda: 0)
            for p, wp in enumerate(want_pages):
                got = it.next()
                assert it.last_raw_ids == wp, (kind, bs, p)
                assert sorted(int(i) for i in got) == sorted(wp)
            assert it.next() == []
            it.close()
    finally:
        mk.close()


@pytest.mark.parametrize("kind", ["gauss", "family"])
def test_masked_search_equals_the_view(oracle, kind):
    corpus, levels, q, index, s_all, i_all = _parent(kind, oracle)
    mk = _Masks(index)
    try:
        for name, sel in (("sparse", ROWS % 199 == 5), ("half", HALF), ("all but one tile", NOT_TILE0)):
            view = index.view(np.nonzero(sel)[0], max_nq=NQ, max_k=128)
            try:
                for k in KS:
                    for nq in BATCHES:
                        vs, vi = view.search(q[:nq], k, MODE_EXACT)
                        va = view.search_reweighted(q[:nq], k, MODE_EXACT)
                        raw, ids, lv = index.search_masked(q[:nq], k, mk(sel), reweighted=False)
                        assert _bits(raw) == _bits(vs) and _bits(ids) == _bits(vi), (kind, name, k, nq)
                        ga = index.search_masked(q[:nq], k, mk(sel))
                        assert [_bits(a) for a in ga] == [_bits(a) for a in va], (kind, name, k, nq)
            finally:
                view.close()
    finally:
        mk.close()


def test_rowmask_arguments_and_lifetime(oracle):
    import torch
    corpus, levels, q, index, s_all, i_all = _parent("gauss", oracle)
    rows = np.nonzero(HALF)[0]
    host, dev = index.rowmask(rows), index.rowmask(torch.from_numpy(rows).cuda())   # host-packed and kernel-packed: the same bits
    empty = index.rowmask(np.zeros(0, np.int64))
    st = host.stats()
    assert st["rows"] == len(rows) and st["bytes"] >= _native.rowmask_words(N) * 4 and dev.stats() == st
    a = index.search_masked(q[:40], 10, host)
    b = index.search_masked(q[:40], 10, dev)
    assert [_bits(x) for x in a] == [_bits(x) for x in b]
    # device tensors in -> device tensors out
    c = index.search_masked(torch.from_numpy(q[:40]).cuda(), 10, host)
    assert all(t.is_cuda for t in c) and [_bits(x) for x in c] == [_bits(x) for x in a]
    for bad in ([5, 5], [7, 3], [-1], [N]):
        with pytest.raises(ValueError):
            index.rowmask(np.array(bad))
        with pytest.raises(ValueError):
            index.rowmask(torch.tensor(bad, dtype=torch.int64).cuda())
    raw, ids, lv = index.search_masked(q[:4], 10, empty, reweighted=False)
    assert (ids == -1).all() and np.isneginf(raw).all() and (lv == 0).all()
    with pytest.raises(ValueError):
        index.search_masked(q[:4], 10, [host] * 3)
    # back-to-back device calls with different tables and no synchronisation in between (the pinned table is guarded by an event)
    import torch
    dq = torch.from_numpy(q[:40]).cuda()
    tables = [[host if (i + t) % 3 else None for i in range(40)] for t in range(3)] + [[empty] * 40, [dev] * 40]
    outs = [index.search_masked(dq, 10, t) for t in tables]
    for t, o in zip(tables, outs):
        assert [_bits(x) for x in o] == [_bits(x) for x in index.search_masked(q[:40], 10, t)]
    # a mask of another index (same rows, same n: the owner check), a mask on a view, a closed mask
    other = IcdIndex(corpus, levels, max_nq=8, max_k=10)
    foreign = other.rowmask(rows)
    with pytest.raises(_native.IcdError) as e:
        index.search_masked(q[:4], 10, foreign)
    assert e.value.code == -1 and "another index" in str(e.value)
    with pytest.raises(_native.IcdError) as e:
        index.search_masked(q[:4], 10, [host, None, foreign, host])
    assert e.value.code == -1
    assert (other.search_masked(q[:4], 10, foreign, reweighted=False)[1] >= 0).all()
    foreign.close()
    other.close()
    view = index.view(rows[:500], max_nq=8, max_k=10)
    with pytest.raises(_native.IcdError) as e:
        view.search_masked(q[:4], 10, host)
    assert e.value.code == -4
    with pytest.raises(_native.IcdError) as e:
        view.rowmask(np.arange(10))
    assert e.value.code == -4
    view.close()
    host.close()
    assert host.closed
    with pytest.raises(_native.IcdError):
        index.search_masked(q[:4], 10, host)
    dev.close()
    empty.close()


# ---- services ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def services(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("MILVUS_DB_PATH", str(tmp_path_factory.mktemp("db")))
    mp.setenv("MILVUS_COLLECTION_NAME", "icd10_mask")
    mp.setenv("EMBEDDING_MODEL_NAME", "shibing624/text2vec-base-chinese")
    mp.setenv("ICD_EMBEDDING_ALLOW_SYNTHETIC", "1")
    mp.setenv("ICD_FILTER_MASKS", "4")
    from rag_project_icd10_amd.tools.build_database import DatabaseBuilder
    b = DatabaseBuilder()
    b.initialize_services()
    recs = b.load_csv_data(os.path.join(GOLDEN, "csv_slice.csv"))
    assert b.vectorize_and_index(recs) is True
    strings = [l.rstrip("\n") for l in open(os.path.join(GOLDEN, "diagnosis_strings.txt"), encoding="utf-8")][:24]
    yield {"b": b, "recs": recs, "ms": b.milvus_service, "es": b.embedding_service, "strings": strings}
    b.milvus_service.disconnect()
    mp.undo()


EXPRS = ['code like "A0%"', None, "level >= 2", 'code like "%.9"', 'level == 1 or code in ["A01.0", "A02.1"]', "level > 0",
         'code == "none"', 'not code like "A%"']


def test_milvus_service_with_a_filter_per_query(services):
    ms, es, recs = services["ms"], services["es"], services["recs"]
    vecs = np.stack([es.encode_query(s) for s in services["strings"]]).astype(np.float32)
    exprs = [EXPRS[i % len(EXPRS)] for i in range(len(vecs))]
    # the yardstick: one view-path call per query
    want_arrays = [ms.search_batch(vecs[i:i + 1], 5, filter=e) for i, e in enumerate(exprs)]
    want_dicts = [ms.search_batch(vecs[i:i + 1], 5, as_dicts=True, filter=e)[0] for i, e in enumerate(exprs)]
    got = ms.search_batch(vecs, 5, filter=exprs)
    for j in range(4):
        assert _bits(got[j]) == _bits(np.concatenate([w[j] for w in want_arrays])), j
    assert ms.search_batch(vecs, 5, as_dicts=True, filter=tuple(exprs)) == want_dicts
    assert want_dicts[6] == [] and (got[2][6] == -1).all()   # ('code == "none"' selects nothing: padding, [])
    # a band next to the list
    floor = float(np.median(got[1][:, 2][np.isfinite(got[1][:, 2])]))
    got_b = ms.search_batch(vecs, 5, filter=exprs, radius=floor)
    want_b = [ms.search_batch(vecs[i:i + 1], 5, filter=e, radius=floor) for i, e in enumerate(exprs)]
    for j in range(4):
        assert _bits(got_b[j]) == _bits(np.concatenate([w[j] for w in want_b])), j
    # a single expression in mask mode: search, search_batch, the iterator - the view path's answers first, then the mask path's
    singles = ('code like "A0%"', "level >= 2", "level > 0", 'code == "none"')

    def answers(**mode):
        out = []
        for e in singles:
            for i in (0, 3):
                out.append(ms.search(vecs[i], 5, filter=e, **mode))
                out.append(ms.search(vecs[i], 5, filter=e, offset=3, **mode))
            out.append([_bits(x) for x in ms.search_batch(vecs, 7, filter=e, **mode)])
            it = ms.search_iterator(vecs[1], batch_size=6, filter=e, **mode)
            for _page in range(4):
                out.append((it.next(), list(it.last_raw_ids)))
            it.close()
        return out
    want_single = answers()
    # mask-mode calls make no view and touch none: the cache is what the view-path calls left
    views_before = ms.filter_views()
    assert answers(filter_mode="mask") == want_single
    assert ms.search_batch(vecs, 5, as_dicts=True, filter=exprs) == want_dicts
    assert ms.filter_views() == views_before
    masks = ms.filter_masks()
    assert 0 < len(masks) <= 4 and all(m["rows"] < len(recs) and m["bytes"] > 0 and isinstance(m["expression"], str) for m in masks)
    for c in "ABCDEFG":
        ms.search(vecs[0], 3, filter=f'code like "{c}%"', filter_mode="mask")
    assert len(ms.filter_masks()) == 4
    # a mutation of the store under a masked iterator
    it = ms.search_iterator(vecs[0], batch_size=5, filter="level >= 2", filter_mode="mask")
    assert len(it.next()) == 5
    mat = ms.client.matrix().copy()
    assert ms.clear_collection() and ms.insert_records(list(recs), [mat[i] for i in range(len(recs))])
    assert ms.filter_masks() == []
    with pytest.raises(RuntimeError):
        it.next()


@pytest.mark.parametrize("with_entities", [False, True])
def test_match_diagnoses_batch_with_a_filter_per_diagnosis(services, with_entities):
    """one search for the whole batch, every diagnosis over its own selection = one call per diagnosis through the view path, on
    the plain device route and on the device-rescoring route with entities"""
    from test_entity_rescoring_cpu import synthetic_entities
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    ms, es = services["ms"], services["es"]
    md = MultiDiagnosisService(es, ms)
    strings = services["strings"][:8]
    exprs = [EXPRS[i % len(EXPRS)] for i in range(len(strings))]
    ents = [synthetic_entities(i, s) for i, s in enumerate(strings)] if with_entities else None
    got = md.match_diagnoses_batch(strings, top_k=3, entities=ents, filter=exprs)
    for i, (s, e) in enumerate(zip(strings, exprs)):
        one = md.match_diagnoses_batch([s], top_k=3, entities=None if ents is None else [ents[i]], filter=e)[0]
        assert got[i].model_dump() == one.model_dump(), (i, e)
    assert got[6].candidates == []   # ('code == "none"')
    with pytest.raises(ValueError):
        md.match_diagnoses_batch(strings, top_k=3, filter=exprs[:3])
