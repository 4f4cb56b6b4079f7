"""Boosted search (run with -m gpu on an MI355X): IcdIndex.search_boosted against tests/boost_oracle.py -
sequential np.float32 multiplies over the oracle's canonical scores, a stable sort, then the masked search's walk - bit for bit,
raw and reweighted. Corpora and parents: those of tests/test_range_search_gpu.py (N = 12 000 with a 96-row last tile, NQ = 300);
batches (1, 2, 4, 40, 300) run the single-launch form, the streaming form and the fp32-MFMA form. Every weight and bound is taken
from the oracle's scores on the CPU, so every case is decided by construction."""
import numpy as np
import pytest

import boost_oracle as bo
from mask_oracle import masked_batch
from test_grouped_search_gpu import N, NQ
from test_range_search_gpu import BATCHES, _parent

pytestmark = pytest.mark.gpu

from rag_project_icd10_amd import _native  # noqa: E402
from rag_project_icd10_amd._native import IcdIndex  # noqa: E402
from rag_project_icd10_amd.services import range_search  # noqa: E402
from rag_project_icd10_amd.services.boost_ranker import BoostedIndex  # noqa: E402

KS = (1, 10, 100, 128)
ROWS = np.arange(N)
_WS = {}


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes()


def _world(kind, oracle):
    corpus, levels, q, index, s_all, i_all = _parent(kind, oracle)
    if kind not in _WS:
        _WS[kind] = (index.boost_workspace(NQ), bo.by_row(s_all, i_all, N))
    return corpus, levels, q, index, s_all, i_all, _WS[kind][0], _WS[kind][1]


class Masks:
    """boolean selections -> IcdRowMask of one index, made once per distinct selection"""

    def __init__(self, index):
        self.index, self.made = index, {}

    def __call__(self, sel):
        if sel is None:
            return None
        sel = np.asarray(sel, bool)
        key = sel.tobytes()
        if key not in self.made:
            self.made[key] = self.index.rowmask(np.nonzero(sel)[0].astype(np.int64))
        return self.made[key]

    def boosts(self, per_query):
        return [None if per is None else [None if b is None else (self(b[0]), b[1]) for b in per] for per in per_query]

    def close(self):
        for m in self.made.values():
            m.close()


def _cut(v, nq):
    if v is None:
        return None
    if isinstance(v, tuple):
        return tuple(_cut(x, nq) for x in v)
    return v[:nq] if hasattr(v, "__len__") else v


def _check(index, ws, q, want, k, nq, what, boosts, masks=None, **bounds):
    """search_boosted of the first nq queries, raw and reweighted, against the first nq rows of `want` (boosted_batch's result)"""
    b = {name: _cut(v, nq) for name, v in bounds.items()}
    m = None if masks is None else masks[:nq]
    got_raw = index.search_boosted(q[:nq], k, boosts[:nq], m, workspace=ws, reweighted=False, **b)
    got_adj = index.search_boosted(q[:nq], k, boosts[:nq], m, workspace=ws, reweighted=True, **b)
    for label, got, exp in (("raw", got_raw, want[0]), ("reweighted", got_adj, want[1])):
        assert len(got) == len(exp)
        for j, (g, w) in enumerate(zip(got, exp)):
            w = w[:nq]
            assert g.dtype == w.dtype and g.shape == w.shape, (what, label, j, g.dtype, w.dtype, g.shape, w.shape)
            assert _bits(g) == _bits(w), (what, label, j, nq, k, np.nonzero((g != w).any(1))[0][:5])


def _run(index, ws, mk, q, by_row, levels, per_query, what, ks=KS, batches=BATCHES, sels=None, **bounds):
    """one boost table (boolean selections and weights per query) at every k and batch; returns the oracle's rankings"""
    rk = bo.boosted_rankings(by_row, per_query)
    handles = mk.boosts(per_query)
    masks = None if sels is None else [mk(s) for s in sels]
    for k in ks:
        want = bo.boosted_batch(by_row, levels, per_query, k, masks=sels, rankings=rk, **bounds)
        for nq in batches:
            _check(index, ws, q, want, k, nq, (what, k), handles, masks, **bounds)
    return rk


@pytest.mark.parametrize("kind", ["gauss", "family"])
def test_a_post_step_cannot_answer(oracle, kind):
    """rows r % 199 == q % 199 boosted so far that the ten best of them outrank every other row: almost none of them is in the plain
    top-128, so no rescaling of an ordinary search's hits finds them"""
    corpus, levels, q, index, s_all, i_all, ws, by_row = _world(kind, oracle)
    mk = Masks(index)
    try:
        sels = [ROWS % 199 == qi % 199 for qi in range(NQ)]
        tenth = np.array([np.sort(by_row[qi][sels[qi]])[-10] for qi in range(NQ)], np.float32)    # the 10th best boosted row's raw score
        rest = np.array([by_row[qi][~sels[qi]].max() for qi in range(NQ)], np.float32)            # the best row outside the mask
        assert (tenth > 0).all()
        w = np.float32(np.max(rest.astype(np.float64) / tenth.astype(np.float64)) * 1.01)         # found on the CPU from the oracle's scores
        inside = np.array([int(sels[qi][i_all[qi, :128]].sum()) for qi in range(NQ)])
        print(f"{kind}: weight {w:.3f}; boosted rows inside the plain top-128: max {inside.max()}, mean {inside.mean():.2f}")
        assert (inside < 10).all()
        per_query = [[(sels[qi], w)] for qi in range(NQ)]
        rk = _run(index, ws, mk, q, by_row, levels, per_query, (kind, "post step"))
        assert all(sels[qi][rk[qi][1][:10]].all() for qi in range(NQ))                           # the boosted top-10 are boosted rows
    finally:
        mk.close()


@pytest.mark.parametrize("kind", ["gauss", "family"])
def test_every_bit_position(oracle, kind):
    corpus, levels, q, index, s_all, i_all, ws, by_row = _world(kind, oracle)
    mk = Masks(index)
    try:
        per_query = [[(ROWS % 128 == qi % 128, np.float32(1.5))] for qi in range(128)]
        _run(index, ws, mk, q[:128], by_row[:128], levels, per_query, (kind, "bit"), ks=(10, 128), batches=(4, 40, 128))
    finally:
        mk.close()


@pytest.mark.parametrize("kind", ["gauss", "family"])
def test_demotion_and_sign(oracle, kind):
    """w < 1, w > 1 over negative scores (a ceiling of 0 leaves only those), and a mask of every row: a pure rescale. A weight is
    positive, so a rescale is monotone: w = 2 is exact and keeps every rank; w = 0.3 rounds, and rows it makes tie fall back to id
    order - whatever the oracle's multiply gives."""
    corpus, levels, q, index, s_all, i_all, ws, by_row = _world(kind, oracle)
    mk = Masks(index)
    try:
        half, every = ROWS % 2 == 0, np.ones(N, bool)
        _run(index, ws, mk, q, by_row, levels, [[(half, np.float32(0.25))]] * NQ, (kind, "demote"), ks=(10, 128))
        _run(index, ws, mk, q, by_row, levels, [[(half, np.float32(3.0))]] * NQ, (kind, "negative"), ks=(10, 128), range_filter=np.float32(0.0))
        rk = _run(index, ws, mk, q, by_row, levels, [[(every, np.float32(2.0))]] * NQ, (kind, "rescale 2"), ks=(10, 128))
        assert all(_bits(rk[qi][1]) == _bits(i_all[qi]) and _bits(rk[qi][0]) == _bits(s_all[qi] * np.float32(2)) for qi in range(0, NQ, 7))
        _run(index, ws, mk, q, by_row, levels, [[(every, np.float32(0.3))]] * NQ, (kind, "rescale 0.3"), ks=(10, 128))
    finally:
        mk.close()


@pytest.mark.parametrize("kind", ["gauss", "family"])
def test_slots(oracle, kind):
    corpus, levels, q, index, s_all, i_all, ws, by_row = _world(kind, oracle)
    mk = Masks(index)
    try:
        a, b, c, d = ROWS % 3 == 0, ROWS % 5 < 2, (ROWS // 128) % 2 == 0, ROWS % 7 == 3       # overlapping selections
        empty, every = np.zeros(N, bool), np.ones(N, bool)
        f = np.float32
        tables = {"one": [(a, f(1.5))], "two": [(a, f(1.5)), (b, f(0.5))], "three": [(a, f(1.5)), (b, f(0.5)), (c, f(1.25))],
                  "four": [(a, f(1.5)), (b, f(0.5)), (c, f(1.25)), (d, f(3.0))], "a hole": [(a, f(1.5)), None, None, (d, f(3.0))],
                  "the first slot unused": [None, (b, f(0.5))], "an empty mask": [(empty, f(9.0)), (a, f(1.5))],
                  "the same mask twice": [(a, f(1.5)), (a, f(1.5))]}
        for name, table in tables.items():
            _run(index, ws, mk, q, by_row, levels, [table] * NQ, (kind, name), ks=(10, 128))
        # the non-commuting pair of tests/test_boost_cpu.py in both orders: the oracle's two rankings differ, and each is matched
        r12 = _run(index, ws, mk, q, by_row, levels, [[(every, bo.W1), (every, bo.W2)]] * NQ, (kind, "W1 W2"), ks=(10, 128))
        r21 = _run(index, ws, mk, q, by_row, levels, [[(every, bo.W2), (every, bo.W1)]] * NQ, (kind, "W2 W1"), ks=(10, 128))
        assert np.mean([_bits(r12[qi][0][:128]) != _bits(r21[qi][0][:128]) for qi in range(NQ)]) > 0.9
    finally:
        mk.close()


@pytest.mark.parametrize("kind", ["gauss", "family"])
def test_mixed_batch(oracle, kind):
    """per query: no boost, one, four; with and without a filter mask, one of them disjoint from the boost"""
    corpus, levels, q, index, s_all, i_all, ws, by_row = _world(kind, oracle)
    mk = Masks(index)
    try:
        a, b, c, d = ROWS % 3 == 0, ROWS % 5 < 2, (ROWS // 128) % 2 == 0, ROWS % 7 == 3
        f = np.float32
        kinds = [None, [(a, f(2.5))], [(a, f(1.5)), (b, f(0.5)), (c, f(1.25)), (d, f(3.0))], []]
        filters = [None, ROWS % 4 != 1, ~a, None, c]                                      # (~a is disjoint from the one-boost query's mask)
        per_query = [kinds[qi % 4] for qi in range(NQ)]
        sels = [filters[qi % 5] for qi in range(NQ)]
        _run(index, ws, mk, q, by_row, levels, per_query, (kind, "mixed"), sels=sels)
        _run(index, ws, mk, q, by_row, levels, per_query, (kind, "mixed, no filter"), ks=(10,))
    finally:
        mk.close()


@pytest.mark.parametrize("kind", ["gauss", "family"])
def test_bands_and_cursor_on_the_boosted_score(oracle, kind):
    corpus, levels, q, index, s_all, i_all, ws, by_row = _world(kind, oracle)
    mk = Masks(index)
    try:
        sel = ROWS % 2 == 0
        # lift: a floor between the raw and the boosted score of the best masked row outside the plain top-20 admits it only
        # because of its boost; demote: a floor under the raw top-20 excludes the masked ones among them only because of theirs
        up, down = np.float32(1.5), np.float32(0.5)
        floor = s_all[:, 20].copy()
        lifted = bo.boosted_rankings(by_row, [[(sel, up)]] * NQ)
        want = bo.boosted_batch(by_row, levels, [[(sel, up)]] * NQ, 128, radius=floor, rankings=lifted)
        only_boost = [(by_row[qi][want[0][1][qi][want[0][1][qi] >= 0]] <= floor[qi]).sum() for qi in range(NQ)]
        assert min(only_boost) >= 1                                                      # hits whose raw score is at or under the floor
        _run(index, ws, mk, q, by_row, levels, [[(sel, up)]] * NQ, (kind, "lift over a floor"), ks=(10, 128), radius=floor)
        want = bo.boosted_batch(by_row, levels, [[(sel, down)]] * NQ, 128, radius=floor)
        gone = [len(set(i_all[qi, :20][sel[i_all[qi, :20]]].tolist()) - set(want[0][1][qi].tolist())) for qi in range(NQ)]
        assert (np.array(gone) >= 1).mean() > 0.9                                         # raw top-20 rows that fell under the floor
        _run(index, ws, mk, q, by_row, levels, [[(sel, down)]] * NQ, (kind, "demote under a floor"), ks=(10, 128), radius=floor)
        # both bounds and a cursor, all taken from the boosted ranking
        lo = np.array([lifted[qi][0][300] for qi in range(NQ)], np.float32)
        hi = np.array([lifted[qi][0][150] for qi in range(NQ)], np.float32)
        after = (np.array([lifted[qi][0][200] for qi in range(NQ)], np.float32), np.array([lifted[qi][1][200] for qi in range(NQ)], np.int64))
        _run(index, ws, mk, q, by_row, levels, [[(sel, up)]] * NQ, (kind, "band"), ks=(10, 100), radius=lo, range_filter=hi)
        _run(index, ws, mk, q, by_row, levels, [[(sel, up)]] * NQ, (kind, "cursor"), ks=(10, 128), after=after, radius=lo)
    finally:
        mk.close()


def test_iterator_walks_a_whole_boosted_ranking(oracle):
    """pages of 7 over a 600-row selection whose boost makes runs of exact ties (duplicate rows boosted alike, and a weight of 0
    mantissa bits): every row once, in oracle order, the cursor landing inside runs of tied boosted scores"""
    corpus, levels, q, index, s_all, i_all, ws, by_row = _world("gauss", oracle)
    mk = Masks(index)
    try:
        keep = (ROWS >= 4900) & (ROWS < 5500)                                             # holds the duplicate pairs 5000 + 2 j / 5001 + 2 j
        sel = ROWS % 3 != 0
        for qi in (0, 41):                                                                # query 0 IS row 5000
            pages = bo.boosted_pages(by_row[qi], [(sel, np.float32(2.0))], 7, mask=keep)
            flat = [i for p in pages for i in p]
            assert len(flat) == 600 and len(set(flat)) == 600
            boosted = bo.boost_scores(by_row[qi], [(sel, np.float32(2.0))])
            ties_at_page_ends = sum(1 for p in pages[:-1] if _bits(boosted[p[-1]]) == _bits(boosted[flat[flat.index(p[-1]) + 1]]))
            assert ties_at_page_ends >= 1
            bi = BoostedIndex(index, ws, [[(mk(sel), np.float32(2.0))]], [mk(keep)])
            it = range_search.SearchIterator(bi, q[qi], 7, -1, None, None, lambda adj, raw, ids: [int(i) for i in ids], lambda: 0)
            got = []
            while True:
                page = it.next()
                if not page:
                    break
                got.append(list(it.last_raw_ids))
            assert got == pages
    finally:
        mk.close()


@pytest.mark.parametrize("kind", ["gauss", "family"])
def test_identity(oracle, kind):
    """all slots unused, and weight 1.0, give search_masked's bytes"""
    corpus, levels, q, index, s_all, i_all, ws, by_row = _world(kind, oracle)
    mk = Masks(index)
    try:
        a = ROWS % 3 == 0
        sels = [None if qi % 3 == 0 else ROWS % 4 != qi % 4 for qi in range(NQ)]
        masks = [mk(s) for s in sels]
        bounds = dict(radius=s_all[:, 400].copy(), after=(s_all[:, 30].copy(), i_all[:, 30].copy()))
        one = np.float32(1.0)
        tables = {"no slot": [None] * NQ, "empty lists": [[] for _ in range(NQ)], "weight one": [[(mk(a), one)]] * NQ,
                  "four times one": [[(mk(a), one), (mk(~a), one), (mk(a), one), (mk(~a), one)]] * NQ}
        for k in (10, 128):
            for nq in BATCHES:
                for kw in ({}, bounds):
                    b = {name: _cut(v, nq) for name, v in kw.items()}
                    for rew in (False, True):
                        base = index.search_masked(q[:nq], k, masks[:nq], reweighted=rew, **b)
                        for name, table in tables.items():
                            got = index.search_boosted(q[:nq], k, table[:nq], masks[:nq], workspace=ws, reweighted=rew, **b)
                            assert [_bits(g) for g in got] == [_bits(w) for w in base], (kind, name, k, nq, rew)
        # a table prepared once is the per-query lists
        lists = [[(mk(a), np.float32(1.5)), None, (mk(~a), np.float32(0.75))] if qi % 2 else None for qi in range(NQ)]
        table = _native.BoostTable(lists, NQ)
        assert [_bits(g) for g in index.search_boosted(q, 10, table, masks, workspace=ws)] == \
            [_bits(g) for g in index.search_boosted(q, 10, lists, masks, workspace=ws)]
        with pytest.raises(ValueError):
            index.search_boosted(q[:5], 10, table, workspace=ws)
        want = masked_batch(s_all, i_all, levels, sels, 10)
        _check(index, ws, q, want, 10, NQ, (kind, "identity against the oracle"), [None] * NQ, masks)
    finally:
        mk.close()


# ---- small shapes and edge values ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 127, 128, 129, 257])
def test_edge_values_on_small_corpora(oracle, n):
    """dim 32, an id_base, a corpus whose scores are exactly its first column: all-tied scores whose boosts create and break ties,
    products that land in the subnormals, products that overflow to +inf and to -inf, NaN rows"""
    dim, id_base, nq_all = 32, 1000, 65
    big, tiny = np.float32(3e38), np.float32(1e-38)
    cycle = np.array([0.5, 0.5, 0.25, big, -big, tiny, -tiny, np.nan, 0.5, 1.0, -0.5, 0.125], np.float32)
    corpus = np.zeros((n, dim), np.float32)
    corpus[:, 0] = cycle[np.arange(n) % len(cycle)]
    levels = (1 + np.arange(n) % 3).astype(np.int32)
    q = np.zeros((nq_all, dim), np.float32)
    q[:, 0] = np.array([1.0, 0.5, 2.0], np.float32)[np.arange(nq_all) % 3]               # (exact scalings: the score is q0 * column 0)
    by_row = np.stack([oracle.scores(q[qi], corpus) for qi in range(nq_all)])
    assert _bits(by_row[0]) == _bits(corpus[:, 0])
    rows = np.arange(n)
    a, b, every = rows % 3 == 0, rows % 2 == 0, np.ones(n, bool)
    f = np.float32
    tables = {"ties made and broken": [(a, f(2.0)), (b, f(0.5))], "subnormal products": [(every, f(0.01))], "overflow": [(every, f(4.0))],
              "overflow of a part": [(a, f(8.0)), (b, f(0.5))], "subnormal, then back": [(every, f(0.001)), (every, f(1000.0))],
              "none": None}
    index = IcdIndex(corpus, levels, max_nq=128, max_k=128, id_base=id_base)
    ws, mk = index.boost_workspace(128), Masks(index)
    try:
        for name, table in tables.items():
            per_query = [table] * nq_all
            rk = bo.boosted_rankings(by_row, per_query, id_base)
            if name == "overflow" and n >= 12:
                assert np.isposinf(rk[0][0][0]) and not np.isneginf(rk[0][0]).any() and len(rk[0][0]) < n - n // 12   # +inf first; -inf and NaN rows are no hits
            if name == "subnormal products" and n >= 12:
                sub = rk[0][0][(rk[0][0] != 0) & (np.abs(rk[0][0]) < np.finfo(np.float32).tiny)]
                assert len(sub) >= 2 and (sub > 0).any() and (sub < 0).any()
            for sels in (None, [rows % 4 != 1] * nq_all):
                for k in (1, 10, 128):
                    want = bo.boosted_batch(by_row, levels, per_query, k, masks=sels, id_base=id_base, rankings=rk)
                    handles = mk.boosts(per_query)
                    masks = None if sels is None else [mk(s) for s in sels]
                    for nq in (1, 4, 9, 65):
                        _check(index, ws, q, want, k, nq, (n, name, k), handles, masks)
            # a cursor inside the run of ties at the top of query 0's boosted ranking
            if len(rk[0][0]) > 3:
                after = (np.full(nq_all, rk[0][0][1], np.float32), np.full(nq_all, rk[0][1][1], np.int64))
                want = bo.boosted_batch(by_row, levels, per_query, 10, after=after, id_base=id_base, rankings=rk)
                for nq in (1, 4, 65):
                    _check(index, ws, q, want, 10, nq, (n, name, "cursor"), mk.boosts(per_query), None, after=after)
    finally:
        mk.close()
        ws.close()
        index.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(oracle):
    import torch
    corpus, levels, q, index, s_all, i_all, ws, by_row = _world("gauss", oracle)
    lib = index._lib
    other = IcdIndex(corpus[:256], levels[:256], max_nq=8, max_k=16)
    view = index.view(np.arange(0, N, 2))
    mask, foreign = index.rowmask(np.arange(0, N, 3)), other.rowmask(np.arange(5))
    ws_other, ws_small = other.boost_workspace(8), index.boost_workspace(2)
    dead_mask, dead_ws = index.rowmask(np.arange(9)), index.boost_workspace(4)
    dead_mask_h, dead_ws_h = dead_mask._h.value, dead_ws._h.value
    dead_mask.close()
    dead_ws.close()
    nq, k = 3, 5
    qs = np.ascontiguousarray(q[:nq])
    raw, ids = np.full((nq, k), 7.0, np.float32), np.full((nq, k), 7, np.int64)
    adj, lv = np.full((nq, k), 7.0, np.float64), np.full((nq, k), 7, np.int32)

    def call(idx=index._h, w=ws._h, tab=None, weights=None, masks=None, n=nq, kk=k, rad=None, rf=None, a_s=None, a_i=None, stream=None,
             on_dev=0, outs=None, queries=None):
        t = np.zeros((max(n, nq), 4), np.uint64)
        t[:, 0] = mask._h.value
        t = t if tab is None else tab
        wt = np.full((max(n, nq), 4), 1.5, np.float32) if weights is None else weights
        o = (adj.ctypes.data, raw.ctypes.data, ids.ctypes.data, lv.ctypes.data) if outs is None else outs
        ptr = lambda v: None if v is None else v.ctypes.data   # noqa: E731
        return lib.icd_index_search_boosted(idx, w, ptr(masks), t.ctypes.data, wt.ctypes.data, qs.ctypes.data if queries is None else queries, n, kk,
                                            on_dev, ptr(rad), ptr(rf), ptr(a_s), ptr(a_i), 0, 1, *o, on_dev, stream)

    def table(slot_value, slot=(1, 2)):
        t = np.zeros((nq, 4), np.uint64)
        t[:, 0] = mask._h.value
        t[slot] = slot_value
        return t

    def weights(v, slot=(1, 0)):
        w = np.full((nq, 4), 1.5, np.float32)
        w[slot] = v
        return w

    f32 = lambda *v: np.array(v, np.float32)   # noqa: E731
    try:
        assert call() == 0 and (ids[:, 0] >= 0).all()                                   # the call itself is fine
        for a in (raw, ids, adj, lv):
            a.fill(7)
        mtab = np.array([mask._h.value, 0, foreign._h.value], np.uint64)
        dtab = np.array([mask._h.value, dead_mask_h, 0], np.uint64)
        cases = [
            (lambda: call(weights=weights(np.nan)), -1), (lambda: call(weights=weights(np.inf)), -1), (lambda: call(weights=weights(0.0)), -1),
            (lambda: call(weights=weights(-1.5)), -1), (lambda: call(weights=weights(1e-40)), -1), (lambda: call(weights=weights(-0.0)), -1),
            (lambda: call(tab=table(foreign._h.value)), -1),                            # a boost mask of another index
            (lambda: call(w=ws_other._h), -1),                                          # a workspace of another index
            (lambda: call(w=ws_small._h), -1),                                          # nq above the workspace's max_nq
            (lambda: call(n=NQ + 1), -1),                                               # ... and above the index's
            (lambda: call(masks=mtab), -1),                                             # a filter mask of another index
            (lambda: call(kk=0), -1), (lambda: call(kk=129), -1), (lambda: call(n=-1), -1),
            (lambda: call(rad=f32(0.5, 0.5, 0.5), rf=f32(0.1, 0.9, 0.9)), -1), (lambda: call(rad=f32(np.nan, 0, 0)), -1),
            (lambda: call(a_s=f32(0.5, 0.5, 0.5)), -1),                                 # a cursor is a score AND an id
            (lambda: call(outs=(adj.ctypes.data, None, ids.ctypes.data, lv.ctypes.data)), -1),
            (lambda: call(outs=(None, raw.ctypes.data, ids.ctypes.data, lv.ctypes.data)), -1),   # reweighted without out_adj
            (lambda: call(tab=table(dead_mask_h)), -5), (lambda: call(masks=dtab), -5), (lambda: call(w=dead_ws_h), -5), (lambda: call(w=None), -5),
            (lambda: call(idx=None), -5),
            (lambda: call(idx=view._h), -4),
        ]
        for i, (fn, rc) in enumerate(cases):
            assert fn() == rc and lib.icd_last_error(), (i, rc)
            assert (raw == 7).all() and (ids == 7).all() and (adj == 7).all() and (lv == 7).all(), i   # no output byte was written
        # the wrappers say the same
        with pytest.raises(_native.IcdError):
            index.search_boosted(qs, k, [[(mask, 0.0)]] * nq, workspace=ws)
        with pytest.raises(_native.IcdError):
            index.search_boosted(qs, k, [[(mask, 2.0)]] * nq, workspace=dead_ws)
        with pytest.raises(ValueError):
            index.search_boosted(qs, k, [[(mask, 2.0)] * 5] * nq, workspace=ws)
        with pytest.raises(ValueError):
            index.search_boosted(qs, k, [[(mask, 2.0)]], workspace=ws)
        # a capturing stream: the table is staged on the host at call time
        dq = torch.from_numpy(qs).cuda()
        d_raw, d_ids = torch.full((nq, k), 7.0, device="cuda"), torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
        d_adj, d_lv = torch.full((nq, k), 7.0, dtype=torch.float64, device="cuda"), torch.full((nq, k), 7, dtype=torch.int32, device="cuda")
        outs = (d_adj.data_ptr(), d_raw.data_ptr(), d_ids.data_ptr(), d_lv.data_ptr())
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            index.search_reweighted(dq, 5)   # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc = call(on_dev=1, outs=outs, queries=dq.data_ptr(), stream=_native._current_stream_ptr(0))
            msg = lib.icd_last_error()
            ok = index.search_reweighted(dq, 5)   # (the capture survives the refusal and ends with a search that may be captured)
        graph.replay()
        torch.cuda.synchronize()
        assert _bits(ok[0]) == _bits(index.search_reweighted(qs, 5)[0])
        assert rc == -1 and b"captured" in msg
        assert (d_raw == 7).all() and (d_ids == 7).all() and (d_adj == 7).all() and (d_lv == 7).all()
        assert call() == 0                                                               # ... and the handles are as they were
        assert ws.stats()["max_nq"] == NQ and ws.stats()["bytes"] > 0
    finally:
        for h in (mask, foreign, ws_other, ws_small, view, other):
            h.close()
