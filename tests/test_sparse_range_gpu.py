"""icd_sparse_search_range on the device against tests/sparse_range_oracle.py, bit for bit, in the raw and the reweighted form
(DESIGN.md section 16). The arithmetic is fully specified, so there is no tolerance. Shapes sit around the kernel's tile (T rows,
from the build): n = T + 37 (two tiles) and n = 2 T + 1 (three). Every case first asserts on the oracle's answer that it hits
what it aims at."""
import csv
import ctypes
import io
import lzma
import os

import numpy as np
import pytest

import sparse_oracle as so
import sparse_range_oracle as sro
from rag_project_icd10_amd import _native
from rag_project_icd10_amd.services import range_search, sparse_text
from test_sparse_search_gpu import DIM, make_queries, make_rows, same, tile   # (the adversarial rows and queries of section 14's tests)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VOCAB, NQ, ID_BASE = 37, 300, 1000
INF = np.float32(np.inf)


def block_rows(rows, lo, hi):
    """rows lo + 1 .. hi - 1 become copies of row lo: hi - lo rows with identical scores under every query"""
    row_off, terms, vals = rows
    t0, v0 = terms[row_off[lo]:row_off[lo + 1]], vals[row_off[lo]:row_off[lo + 1]]
    m = hi - lo
    terms = np.concatenate([terms[:row_off[lo]], np.tile(t0, m), terms[row_off[hi]:]])
    vals = np.concatenate([vals[:row_off[lo]], np.tile(v0, m), vals[row_off[hi]:]])
    lens = np.diff(row_off)
    lens[lo:hi] = len(t0)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), terms, vals


class World:
    """an index of n rows with a sparse index, a batch of NQ queries and the oracle's scores of them, computed once"""

    def __init__(self, n, seed, block=False):
        T = tile()
        rng = np.random.default_rng(seed)
        self.n, self.T = n, T
        self.levels = rng.integers(1, 4, n).astype(np.int32)
        self.rows = make_rows(n, VOCAB, seed)
        if block:   # 500 identical rows across the tile boundary
            self.rows = block_rows(self.rows, T - 250, T + 250)
        self.index = _native.IcdIndex(rng.standard_normal((n, DIM), dtype=np.float32), self.levels, device=0, max_nq=320, max_k=128,
                                      id_base=ID_BASE, probe=False)
        self.sp = self.index.sparse(*self.rows, VOCAB, max_nq=320, max_k=128)
        self.q = make_queries(NQ, VOCAB, seed + 1)
        self.scored = sro.score_queries(*self.rows, VOCAB, *self.q)

    def query(self, *qs):
        """the CSR of some of the batch's queries and their scores"""
        off, t, v = self.q
        return sparse_text.csr_from_pairs([(t[off[i]:off[i + 1]], v[off[i]:off[i + 1]]) for i in qs]), [self.scored[i] for i in qs]

    def check(self, q, scored, k, what, masks=None, dense=None, **band):
        """host call against the oracle in both forms -> the oracle's raw answer"""
        for rw in (False, True):
            want = sro.search(scored, k, levels=self.levels, id_base=ID_BASE, masks=dense, reweighted=rw, **band)
            same(self.index.search_sparse(self.sp, *q, k, masks=masks, reweighted=rw, **band), want, f"{what}, reweighted={rw}")
        return sro.search(scored, k, levels=self.levels, id_base=ID_BASE, masks=dense, **band)

    def close(self):
        self.sp.close()
        self.index.close()


@pytest.fixture(scope="module")
def worlds():
    T = tile()
    w = {2: World(T + 37, 71), 3: World(2 * T + 1, 72, block=True)}
    yield w
    for x in w.values():
        x.close()


def per_query_bounds(w):
    """different bounds per query of the batch, from the oracle's own ranking: floors and ceilings that EQUAL a hit's score, a
    cursor on a hit, combinations, an empty band; -inf / +inf / (+inf, -1) where a query has no such bound"""
    full = sro.rankings(w.scored, ID_BASE)
    rad, rf = np.full(NQ, -np.inf, np.float32), np.full(NQ, np.inf, np.float32)
    a_s, a_i = np.full(NQ, np.inf, np.float32), np.full(NQ, -1, np.int64)
    for q, (s, i) in enumerate(full):
        m, kind = len(s), q % 8
        if m == 0 or kind == 0:
            continue
        at = lambda f: min(m - 1, int(f * m))
        if kind in (1, 4, 6):
            rad[q] = s[at(0.6)]
        if kind in (2, 4, 7):
            rf[q] = s[at(0.2)]
        if kind in (3, 6, 7):
            p = at(0.1) if kind == 3 else at(0.3)
            a_s[q], a_i[q] = s[p], i[p]
        if kind == 5:
            rad[q] = s[0]   # nothing above the best score: an empty band
        if not rad[q] < rf[q]:
            rad[q] = -np.inf
    return rad, rf, (a_s, a_i)


@pytest.mark.parametrize("tiles,k", [(2, 1), (2, 10), (2, 128), (3, 1), (3, 10), (3, 128)])
def test_a_batch_with_different_bounds_per_query(worlds, tiles, k):
    import torch
    w = worlds[tiles]
    rad, rf, after = per_query_bounds(w)
    free = sro.search(w.scored, k, levels=w.levels, id_base=ID_BASE)
    raw = w.check(w.q, w.scored, k, "per-query bounds", radius=rad, range_filter=rf, after=after)
    assert (raw[1] != free[1]).any(axis=1).sum() > NQ // 3   # the bounds bite
    assert ((raw[1] >= 0).sum(axis=1) == 0).sum() >= NQ // 10 and ((raw[1] >= 0).sum(axis=1) == k).sum() >= NQ // 10
    # no bound at all IS search_sparse
    for rw in (False, True):
        same(w.index.search_sparse(w.sp, *w.q, k, reweighted=rw, radius=None, range_filter=None, after=None),
             [np.asarray(x) for x in w.index.search_sparse(w.sp, *w.q, k, reweighted=rw)], "no bound")
    same(w.index.search_sparse(w.sp, *w.q, k), free, "no bound against the oracle")
    # unbounded VALUES (-inf, +inf, a cursor in front of everything) through the banded kernel give the same answer
    same(w.index.search_sparse(w.sp, *w.q, k, radius=-INF, range_filter=INF, after=(INF, -1)), free, "unbounded values")
    # host and device bounds, device queries and outputs
    dq = (torch.from_numpy(w.q[0]).cuda(), torch.from_numpy(w.q[1].view(np.int32)).cuda(), torch.from_numpy(w.q[2]).cuda())
    dev = lambda a: torch.from_numpy(a).cuda()
    for rw in (False, True):
        host = w.index.search_sparse(w.sp, *w.q, k, reweighted=rw, radius=rad, range_filter=rf, after=after)
        got = w.index.search_sparse(w.sp, *dq, k, reweighted=rw, radius=dev(rad), range_filter=dev(rf), after=(dev(after[0]), dev(after[1])))
        assert all(g.is_cuda for g in got)
        same(got, host, f"device bounds, reweighted={rw}")


def test_bounds_equal_to_a_score_and_the_select_branches(worlds):
    w = worlds[2]
    T, k = w.T, 10
    q0, s0 = w.query(0)        # term 0 sits in every row: every row is a hit, scores in {0.5, 1, -2, 3}
    acc = s0[0][0]
    assert s0[0][1].all() and set(np.unique(acc).tolist()) == {0.5, 1.0, -2.0, 3.0}
    # radius exactly equal to a hit's score: those rows are out; range_filter equal to it: they are in, and lead
    raw = w.check(q0, s0, k, "radius = a score", radius=1.0)
    assert (raw[0] == 3.0).all()
    raw = w.check(q0, s0, k, "range_filter = a score", range_filter=1.0)
    assert (raw[0] == 1.0).all() and (acc[:T] == 3.0).sum() > 128
    # more than k hits in the band of each tile: the radix select runs on band candidates
    assert ((acc[:T] <= 1.0) & (acc[:T] > 0.5)).sum() > k and ((acc[T:] <= 1.0) & (acc[T:] > 0.5)).sum() > k
    w.check(q0, s0, k, "select on band candidates", radius=0.5, range_filter=1.0)
    # a term in every row, a ceiling below the best 128: the look under the crowd
    free = sro.search(s0, 128, id_base=ID_BASE)
    assert (free[0] == 3.0).all()
    raw = w.check(q0, s0, 128, "under the crowd", range_filter=0.5)
    assert (raw[0] == 0.5).all()
    # a tile with more than k hits of which at most k lie in the band: no select there, though the tile's hits exceed k
    pick = next(i for i in range(10, NQ) if len(np.unique(w.scored[i][0][w.scored[i][1]])) > 40 and w.scored[i][1][:T].sum() > 3 * k)
    q1, s1 = w.query(pick)
    ranked = sro.rankings(s1, ID_BASE)[0][0]
    floor = float(np.unique(ranked)[-4])   # only the three largest distinct scores pass
    inside = s1[0][1] & (s1[0][0] > np.float32(floor))
    assert 0 < inside[:T].sum() <= k and s1[0][1][:T].sum() > k
    w.check(q1, s1, k, "more than k hits, at most k in the band", radius=floor)
    # a tile with at most k hits in total, some outside the band: tile 1 holds 37 rows, k = 128
    assert 0 < s1[0][1][T:].sum() <= 37
    mid = float(np.median(s1[0][0][T:][s1[0][1][T:]]))
    below = s1[0][1][T:] & (s1[0][0][T:] <= np.float32(mid))
    assert 0 < below.sum() < s1[0][1][T:].sum()
    w.check(q1, s1, 128, "at most k hits, some outside", range_filter=mid)
    # a band that empties every tile
    raw = w.check(q0, s0, k, "an empty band", radius=3.0)
    assert (raw[1] == -1).all() and np.isneginf(raw[0]).all()
    # negative scores with a negative floor
    qn, sn = w.query(2)        # term 0 weighted -1: scores {-0.5, -1, 2, -3}
    raw = w.check(qn, sn, k, "negative floor", radius=-1.0, range_filter=-0.5)
    assert (raw[0] == -0.5).all()
    raw = w.check(qn, sn, k, "negative floor under negative hits", radius=-3.0, range_filter=-1.0)
    assert (raw[0] == -1.0).all()
    # a floor of -inf: rows without a shared term stay out
    q3, s3 = w.query(3)        # term 1: one row per tile
    assert s3[0][1].sum() == 2
    raw = w.check(q3, s3, k, "floor -inf", radius=-np.inf)
    assert (raw[1] >= 0).sum() == 2 and (raw[1][0][2:] == -1).all()


def test_cursors(worlds):
    for tiles in (2, 3):
        w = worlds[tiles]
        T, n, k = w.T, w.n, 10
        q0, s0 = w.query(0)
        acc = s0[0][0]
        if tiles == 2:   # a band that empties one tile and leaves the other untouched: term 2's rows straddle the boundary with one score
            q4, s4 = w.query(4)
            edge = np.flatnonzero(s4[0][1])
            e0, e1 = edge[(edge >= T - 3) & (edge < T)], edge[(edge >= T) & (edge < T + 3)]
            assert len(e0) == 3 and len(e1) == 3 and len(np.unique(s4[0][0][edge])) == 1 and (edge >= T - 3).all()
            raw = w.check(q4, s4, 128, "empties tile 0", after=(s4[0][0][T - 1], ID_BASE + T - 1))
            got = raw[1][0][raw[1][0] >= 0] - ID_BASE
            assert not np.isin(e0, got).any() and np.isin(e1, got).all() and np.array_equal(got, edge[edge >= T])
        # a cursor on the last row of tile 0 and on the first row of tile 1
        for row in (T - 1, T):
            raw = w.check(q0, s0, k, f"cursor on row {row}", after=(acc[row], ID_BASE + row))
            assert ID_BASE + row not in raw[1][0] and (raw[1] >= 0).all()
        # a cursor id below id_base lets every row of its score through; one at or above id_base + n none of them
        raw = w.check(q0, s0, k, "cursor id below id_base", after=(np.float32(1.0), 5))
        assert (raw[0] == 1.0).all() and raw[1][0][0] == ID_BASE + int(np.flatnonzero(acc == 1.0)[0])
        for far in (ID_BASE + n, ID_BASE + n + 7, np.iinfo(np.int64).max):
            raw = w.check(q0, s0, k, "cursor id behind the index", after=(np.float32(1.0), far))
            assert (raw[0] == 0.5).all()
        # a cursor score that no row has
        assert not (acc == 0.75).any()
        raw = w.check(q0, s0, k, "cursor score no row has", after=(np.float32(0.75), ID_BASE + 3))
        assert (raw[0] == 0.5).all()
        # cursors next to a floor and a ceiling
        w.check(q0, s0, 128, "cursor inside a band", radius=-2.0, range_filter=1.0, after=(np.float32(1.0), ID_BASE + T))


def test_a_cursor_on_every_position_of_a_tied_block_across_the_tile_boundary(worlds):
    w = worlds[3]
    T = w.T
    lo, hi = T - 250, T + 250
    pos = sorted(set(np.linspace(lo, hi - 1, 36).astype(int).tolist() + [lo, T - 2, T - 1, T, T + 1, hi - 1]))
    assert len(pos) >= 38
    one, s_one = w.query(0)
    acc = s_one[0][0]
    assert len(np.unique(acc[lo:hi])) == 1
    q = sparse_text.csr_from_pairs([(one[1], one[2])] * len(pos))
    scored = s_one * len(pos)
    after = (np.full(len(pos), acc[lo], np.float32), np.array(pos, np.int64) + ID_BASE)
    # (the mask keeps the block alone, so the page behind a cursor IS the block's rest in id order)
    dense = np.zeros(w.n, bool)
    dense[lo:hi] = True
    mask = w.index.rowmask(np.arange(lo, hi))
    raw = w.check(q, scored, 128, "tied block", masks=mask, dense=[dense] * len(pos), after=after)
    for j, p in enumerate(pos):
        m = min(128, hi - 1 - p)
        assert np.array_equal(raw[1][j][:m], np.arange(p + 1, p + 1 + m) + ID_BASE) and (raw[1][j][m:] == -1).all()
    w.check(q, scored, 10, "tied block, unmasked", after=after)
    mask.close()


def test_masks_with_bands_per_query(worlds):
    w = worlds[3]
    k = 10
    qs = list(range(10, 26))
    q, scored = w.query(*qs)
    full = sro.rankings(scored, ID_BASE)
    assert all(len(i) > 3 * k for _s, i in full)
    nq = len(qs)
    rng = np.random.default_rng(4)
    a_s = np.array([s[k - 1] for s, _ in full], np.float32)
    a_i = np.array([i[k - 1] for _, i in full], np.int64)
    dense = []
    for j in range(nq):
        if j % 4 == 0:
            m = np.ones(w.n, bool); m[a_i[j] - ID_BASE] = False      # removes the cursor's own row
        elif j == 5:
            m = np.zeros(w.n, bool)                                   # an empty mask
        elif j % 4 == 1:
            m = None
        else:
            m = rng.random(w.n) < 0.5
        dense.append(m)
    masks = [None if m is None else w.index.rowmask(np.flatnonzero(m)) for m in dense]
    rad = np.array([s[-1] if j % 2 else -np.inf for j, (s, _) in enumerate(full)], np.float32)
    raw = w.check(q, scored, k, "masks and bands", masks=masks, dense=dense, radius=rad, after=(a_s, a_i))
    assert (raw[1][5] == -1).all() and np.array_equal(raw[1][0], full[0][1][k:2 * k])   # (the cursor's row is out either way)
    for m in masks:
        if m is not None:
            m.close()


def test_device_bounds_under_a_captured_graph(worlds):
    import torch
    w = worlds[2]
    k = 10
    rad, rf, after = per_query_bounds(w)
    want = sro.search(w.scored, k, levels=w.levels, id_base=ID_BASE, radius=rad, range_filter=rf, after=after, reweighted=True)
    dev = lambda a: torch.from_numpy(a).cuda()
    dq = (dev(w.q[0]), dev(w.q[1].view(np.int32)), dev(w.q[2]))
    b = dict(radius=dev(rad), range_filter=dev(rf), after=(dev(after[0]), dev(after[1])))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        w.index.search_sparse(w.sp, *dq, k, reweighted=True, validate=False, **b)   # warm-up on the capture stream
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cap = w.index.search_sparse(w.sp, *dq, k, reweighted=True, validate=False, **b)
    for t in cap:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    same(cap, want, "graph replay")
    del graph


def test_offset(worlds):
    w = worlds[3]
    qs = [0, 4, 12, 13]
    q, scored = w.query(*qs)
    band = range_search.SparseBandIndex(w.index, w.sp, None)
    assert band.max_k == 128
    rf = float(np.float32(1.0))
    assert len(sro.rankings(scored, ID_BASE, range_filter=rf)[0][0]) > 400
    for k, o in ((10, 0), (10, 5), (100, 28), (10, 119), (128, 1), (100, 200), (44, 256)):   # offset + k = 129 and 300 among them
        for kw in ({}, {"range_filter": rf}):
            want = sro.search(scored, k, levels=w.levels, id_base=ID_BASE, reweighted=True, offset=o, **kw)
            same(range_search.search_band(band, q, k, kw.get("radius"), kw.get("range_filter"), o), want, f"offset {o}, k {k}, {kw}")


def test_errors_of_the_abi_in_one_process():
    lib = _native.load_library()
    rng = np.random.default_rng(3)
    n = 300

    def make(seed):
        idx = _native.IcdIndex(rng.standard_normal((n, DIM), dtype=np.float32), None, device=0, max_nq=8, max_k=16, probe=False)
        return idx, idx.sparse(*make_rows(n, VOCAB, seed), VOCAB, max_nq=8, max_k=16)
    index, sp = make(21)
    other, sp_other = make(22)
    view = index.view(np.arange(0, n, 2))
    q_off, q_t, q_v = np.array([0, 2], np.int64), np.array([0, 5], np.uint32), np.array([1.0, 2.0], np.float32)
    raw, ids, lv, adj = np.empty((8, 16), np.float32), np.empty((8, 16), np.int64), np.empty((8, 16), np.int32), np.empty((8, 16), np.float64)
    f32 = lambda *x: np.array(x, np.float32)
    one = f32(0.5)

    def search(idx_h, sp_h, off=q_off, t=q_t, v=q_v, nq=1, k=4, masks=None, rad=one, rf=None, a_s=None, a_i=None, rw=0, a=adj):
        p = lambda x: None if x is None else x.ctypes.data
        return lib.icd_sparse_search_range(idx_h, sp_h, off.ctypes.data, t.ctypes.data, v.ctypes.data, nq, k, 0, masks, p(rad), p(rf), p(a_s), p(a_i), 0,
                                           rw, p(a), raw.ctypes.data, ids.ctypes.data, lv.ctypes.data, 0, None)
    assert search(index._h, sp._h) == 0
    # the band's own refusals: ICD_ERR_INVALID
    assert search(index._h, sp._h, rad=f32(np.nan)) == -1 and b"NaN" in lib.icd_last_error()
    assert search(index._h, sp._h, rad=None, rf=f32(np.nan)) == -1 and b"NaN" in lib.icd_last_error()
    assert search(index._h, sp._h, rad=None, a_s=f32(np.nan), a_i=np.array([3], np.int64)) == -1 and b"NaN" in lib.icd_last_error()
    assert search(index._h, sp._h, rad=f32(1.0), rf=f32(1.0)) == -1 and b"below range_filter" in lib.icd_last_error()
    assert search(index._h, sp._h, rad=f32(2.0), rf=f32(1.0)) == -1
    assert search(index._h, sp._h, a_s=f32(1.0)) == -1 and b"both or neither" in lib.icd_last_error()
    assert search(index._h, sp._h, rad=None, a_i=np.array([3], np.int64)) == -1 and b"both or neither" in lib.icd_last_error()
    # every check of icd_sparse_search, with a bound present
    assert search(index._h, sp._h, t=np.array([5, 0], np.uint32)) == -1 and b"strictly increasing" in lib.icd_last_error()
    assert search(index._h, sp._h, t=np.array([0, 37], np.uint32)) == -1 and b"vocabulary" in lib.icd_last_error()
    assert search(index._h, sp._h, v=np.array([1.0, 0.0], np.float32)) == -1
    assert search(index._h, sp._h, off=np.array([0, 65], np.int64), t=np.arange(65, dtype=np.uint32), v=np.ones(65, np.float32)) == -1
    assert search(index._h, sp._h, k=0) == -1 and search(index._h, sp._h, k=129) == -1
    assert search(index._h, sp._h, k=17) == -1 and b"max_k" in lib.icd_last_error()
    assert search(index._h, sp._h, off=np.zeros(10, np.int64), nq=9, rad=np.full(9, 0.5, np.float32)) == -1 and b"max_nq" in lib.icd_last_error()
    assert search(index._h, sp._h, rw=1, a=None) == -1
    assert search(index._h, sp_other._h) == -1 and b"another index" in lib.icd_last_error()
    assert search(view._h, sp._h) == -1
    foreign = other.rowmask(np.arange(10))
    assert search(index._h, sp._h, masks=(ctypes.c_void_p * 1)(foreign._h.value)) == -1 and b"another index" in lib.icd_last_error()
    mine = index.rowmask(np.arange(10))
    assert search(index._h, sp._h, masks=(ctypes.c_void_p * 1)(mine._h.value)) == 0
    dead_mask = (ctypes.c_void_p * 1)(mine._h.value)
    mine.close()
    assert search(index._h, sp._h, masks=dead_mask) == -5
    sp2 = index.sparse(*make_rows(n, VOCAB, 21), VOCAB, max_nq=8, max_k=16)
    st = sp2.stats()
    dead = ctypes.c_void_p(sp2._h.value)
    sp2.close()
    assert search(index._h, dead) == -5   # ICD_ERR_STATE
    assert st["bytes"] == sp.stats()["bytes"] and st["bytes"] % 8 == 0
    # the Python layer turns ICD_ERR_INVALID into ValueError
    with pytest.raises(ValueError):
        index.search_sparse(sp, q_off, q_t, q_v, 4, radius=float("nan"))
    with pytest.raises(ValueError):
        index.search_sparse(sp, q_off, q_t, q_v, 4, radius=1.0, range_filter=0.5)
    with pytest.raises(ValueError):
        index.search_sparse(sp, q_off, q_t, q_v, 4, radius=np.array([0.1, 0.2]))   # two values for one query
    grouping = index.grouping(np.arange(n, dtype=np.int32) % 7)
    with pytest.raises(ValueError):
        index.search_sparse(sp, q_off, q_t, q_v, 2, grouping=grouping, group_size=2, radius=0.5)
    for x in (grouping, foreign, sp_other, other, view, sp, index):
        x.close()


def test_destruction_order_with_a_banded_search_in_between():
    rng = np.random.default_rng(8)
    n = 500
    rows = make_rows(n, VOCAB, 31)
    q = make_queries(4, VOCAB, 32)
    scored = sro.score_queries(*rows, VOCAB, *q)
    want = sro.search(scored, 5, radius=-1.0)

    def make():
        idx = _native.IcdIndex(rng.standard_normal((n, DIM), dtype=np.float32), None, device=0, max_nq=8, max_k=8, probe=False)
        return idx, idx.sparse(*rows, VOCAB, max_nq=8, max_k=8), idx.rowmask(np.arange(n))
    for order in ((0, 1, 2), (1, 0, 2), (2, 1, 0), (1, 2, 0), (0, 2, 1), (2, 0, 1)):
        handles = make()
        index, sp, mask = handles
        same(index.search_sparse(sp, *q, 5, masks=mask, radius=-1.0), want, f"order {order}")
        handles[order[0]].close()
        if order[0] != 0:   # the index lives: what is left of the triple still serves or refuses cleanly
            if order[0] == 2:
                same(index.search_sparse(sp, *q, 5, radius=-1.0), want, "after the mask")
            else:
                with pytest.raises(_native.IcdError):
                    index.search_sparse(sp, *q, 5, radius=-1.0)
        else:
            with pytest.raises(_native.IcdError):
                index.search_sparse(sp, *q, 5, radius=-1.0)
        handles[order[1]].close()
        handles[order[2]].close()
        assert all(h.closed for h in handles)


def test_golden_titles_iterated_to_exhaustion():
    """the 40 474 titles of the golden CSV, one text with a common term, pages of 128 by cursor until nothing is left: the raw-order
    concatenation is the oracle's full ranking of the text's hits"""
    rd = csv.DictReader(io.StringIO(lzma.open(os.path.join(GOLDEN, "ICD_10v601.csv.xz")).read().decode("utf-8-sig")))
    titles = [r["disease"] for r in rd]
    assert len(titles) == 40474
    tx = sparse_text.SparseTextIndex(titles)
    q = tx.encode_queries(["糖尿病"])
    scored = sro.score_queries(tx.row_off, tx.terms, tx.vals, tx.vocab_size, *q)
    full = sro.rankings(scored)[0]
    assert 1000 < len(full[1]) < 12000   # a common term: far more hits than one call returns
    rng = np.random.default_rng(1)
    levels = rng.integers(1, 4, len(titles)).astype(np.int32)
    index = _native.IcdIndex(rng.standard_normal((len(titles), DIM), dtype=np.float32), levels, device=0, max_nq=8, max_k=128, probe=False)
    sp = index.sparse(tx.row_off, tx.terms, tx.vals, tx.vocab_size, max_nq=8, max_k=128)
    it = range_search.SearchIterator(range_search.SparseBandIndex(index, sp, None), q, 128, -1, None, None, lambda a, r, i: list(zip(r, i)), lambda: 0)
    seen_ids, seen_raw = [], []
    for _ in range(len(full[1]) // 128 + 2):
        page = it.next()
        if not page:
            break
        seen_ids += it.last_raw_ids
        seen_raw += sorted((float(r) for r, _ in page), reverse=True)
    assert it.next() == []
    assert seen_ids == full[1].tolist() and seen_raw == [float(x) for x in full[0]]
    sp.close()
    index.close()


# ---- services ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def services(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("MILVUS_DB_PATH", str(tmp_path_factory.mktemp("db")))
    mp.setenv("MILVUS_COLLECTION_NAME", "icd10_sparse_range")
    mp.setenv("EMBEDDING_MODEL_NAME", "shibing624/text2vec-base-chinese")
    mp.setenv("ICD_EMBEDDING_ALLOW_SYNTHETIC", "1")
    mp.setenv("ICD_GPU_MAX_K", "128")   # (the service's default is 100: a page of 128 needs the index to hold 128 hits per query)
    from rag_project_icd10_amd.tools.build_database import DatabaseBuilder
    b = DatabaseBuilder()
    b.initialize_services()
    recs = b.load_csv_data(os.path.join(GOLDEN, "csv_slice.csv"))
    assert b.vectorize_and_index(recs) is True
    titles = [r["preferred_zh"] for r in recs]
    vocab, row_off, terms, vals, idf = so.bm25(titles)
    yield {"ms": b.milvus_service, "recs": recs, "bm25": (vocab, row_off, terms, vals, idf),
           "levels": np.array([r.get("level", 1) for r in recs], np.int32)}
    b.milvus_service.disconnect()
    mp.undo()


def _common_text(recs):
    """a text whose terms many titles of the slice share"""
    from collections import Counter
    c = Counter(ch for r in recs for ch in set(r["preferred_zh"]) if "一" <= ch <= "鿿")
    return "".join(ch for ch, _ in c.most_common(2))


def _score_texts(sv, texts):
    vocab, row_off, terms, vals, idf = sv["bm25"]
    q = sparse_text.csr_from_pairs([so.bm25_query(t, vocab, idf) for t in texts])
    return sro.score_queries(row_off, terms, vals, max(len(vocab), 1), *q)


def test_search_text_and_batch_with_bounds_and_offset(services):
    ms, recs, levels = services["ms"], services["recs"], services["levels"]
    texts = [_common_text(recs), recs[40]["preferred_zh"], recs[7]["preferred_zh"] + " " + recs[90]["preferred_zh"]]
    scored = _score_texts(services, texts)
    full = sro.rankings(scored)
    assert len(full[0][1]) > 40 and all(len(i) > 12 for _s, i in full)
    codes = lambda ids: [recs[i]["code"] for i in ids if i >= 0]
    sel = np.array([r.get("level", 1) >= 2 for r in recs])
    for qi, text in enumerate(texts):
        s = full[qi][0]
        floor, ceil = float(s[min(len(s) - 1, 12)]), float(s[3])
        for k, o, b, expr in ((5, 0, {"radius": floor}, None), (20, 0, {"radius": floor}, None), (5, 0, {"radius": floor, "range_filter": ceil}, None),
                              (5, 0, {"range_filter": ceil}, None), (5, 4, {}, None), (5, 4, {"radius": floor}, None), (10, 25, {}, None),
                              (5, 2, {"range_filter": ceil}, "level >= 2")):
            if b.get("radius") is not None and b.get("range_filter") is not None and not b["radius"] < b["range_filter"]:
                continue
            adj, raw, ids, _lv = sro.search(scored[qi:qi + 1], k, levels=levels, masks=None if expr is None else [sel], reweighted=True, offset=o, **b)
            hits = ms.search_text(text, k, offset=o, filter=expr, **b)
            m = int((ids[0] >= 0).sum())
            assert [h["code"] for h in hits] == codes(ids[0]) and len(hits) == m, (qi, k, o, b)
            assert [h["score"] for h in hits] == [float(a) for a in adj[0, :m]] and [h["original_score"] for h in hits] == [float(r) for r in raw[0, :m]]
            if "radius" in b:
                assert all(h["original_score"] > np.float32(floor) for h in hits)
        assert ms.search_text(text, 5, search_params={"params": {"radius": floor}}) == ms.search_text(text, 5, radius=floor)
    # the batch form: per-query arrays, and one value for every query
    tx = ms.build_sparse_index()[1]
    q = tx.encode_queries(texts)
    rad = np.array([s[min(len(s) - 1, 9)] for s, _ in full], np.float32)
    for kw in ({"radius": rad}, {"radius": rad, "offset": 3}, {"range_filter": float(np.median(rad))}, {"offset": 130}):
        want = sro.search(scored, 10, levels=levels, reweighted=True, **kw)
        got = ms.search_sparse_batch(*q, 10, **kw)
        same(got, want, f"search_sparse_batch {list(kw)}")
    dicts = ms.search_sparse_batch(*q, 10, as_dicts=True, radius=rad)
    assert [[h["code"] for h in d] for d in dicts] == [codes(r) for r in sro.search(scored, 10, levels=levels, reweighted=True, radius=rad)[2]]
    assert ms.search_text("zzzzqqq", 5, radius=0.0) == [] and ms.search_text("", 5, offset=3) == []
    with pytest.raises(ValueError):
        ms.search_text(texts[0], 5, radius=0.1, group_by_field="level")


def test_search_text_iterator(services):
    ms, recs = services["ms"], services["recs"]
    text = _common_text(recs)
    acc, hit = _score_texts(services, [text])[0]
    full = sro.band_rows(acc, hit).tolist()
    assert len(full) > 130
    sel = np.array([r.get("level", 1) >= 2 for r in recs])
    floor = float(acc[full[len(full) // 2]])
    for bs, lim, b, expr in ((1, 40, {}, None), (16, -1, {}, None), (128, -1, {}, None), (16, 40, {}, None), (16, -1, {"radius": floor}, None),
                             (16, -1, {"range_filter": floor}, "level >= 2")):
        want_pages = sro.pages(acc, hit, bs, mask=None if expr is None else sel, limit=lim, **b)
        it = ms.search_text_iterator(text, batch_size=bs, limit=lim, filter=expr, **b)
        seen = []
        for p, wp in enumerate(want_pages):
            hits = it.next()
            assert it.last_raw_ids == wp, (bs, lim, p)
            assert sorted(h["code"] for h in hits) == sorted(recs[i]["code"] for i in wp)
            assert [h["score"] for h in hits] == sorted((h["score"] for h in hits), reverse=True)
            seen += wp
        assert it.next() == [] and it.next() == []
        if lim == -1 and not b and expr is None:
            assert seen == full   # the raw-order concatenation of the pages is the full hit ranking
        elif lim != -1:
            assert seen == full[:lim]
        it.close()
    assert ms.search_text_iterator("zzzzqqq").next() == []
    assert ms.search_text_iterator(text, filter="level >= 99").next() == []
    # a mutation of the store under an iterator
    it = ms.search_text_iterator(text, batch_size=5)
    assert len(it.next()) == 5
    mat = ms.client.matrix().copy()
    assert ms.clear_collection() and ms.insert_records(list(recs), [mat[i] for i in range(len(recs))])
    with pytest.raises(RuntimeError):
        it.next()
