"""icd_index_rank_of on the device against tests/rankof_oracle.py over the CPU oracle's full ranking, byte
for byte: ranks and `selected` equal, scores bit-equal, no tolerance anywhere. Corpus sizes sit around the lane, half-wave and
tile edges (n = 1, 2, 63, 64, 65, 257 and T - 1, T, T + 1, 2 T + 5 for the sweep's row tile T = 128), dims 32, 768 and 160 (the
mixed-walk dim of the exact family tests), batches of 1, 5 and 300 queries (one lane of a tile, a few, three query tiles), 1 and
16 targets with -1 padding, id_base 0 and not. Corpora hold families of bit-identical rows (copies of a target on both sides of
it), a row of zeros, rows that tie for every query, subnormal and NaN scores."""
import ctypes

import numpy as np
import pytest

import rankof_oracle as ro
from conftest import icd_levels, unit_rows
from rag_project_icd10_amd import _native

pytestmark = pytest.mark.gpu

T = 128   # rankof_plan.hpp RK_TILE
BASE = 5_000_000_000
SIZES = (1, 2, 63, 64, 65, 257, T - 1, T, T + 1, 2 * T + 5)


def same(got, want, what):
    """arrays compared byte for byte (NaN payloads included)"""
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        g = np.asarray(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, j, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, j, g, w)


def family_corpus(n, dim, seed, special=True):
    """families of 1 .. 5 bit-identical rows (their members tie with each other, the smaller id first); with special: row 3 all
    zeros and row 5 holding a NaN, where the corpus has them"""
    rng = np.random.default_rng(seed)
    base = unit_rows(n, dim, seed)
    fam = np.repeat(np.arange(n), rng.integers(1, 6, n))[:n]
    x = np.ascontiguousarray(base[fam])
    if special and n > 3:
        x[3] = 0.0
    if special and n > 5:
        x[5, dim // 2] = np.nan
    return x


def row_mask(n, seed, keep=0.5):
    m = np.random.default_rng(seed).random(n) < keep
    return m


class Case:
    """one corpus on the device, a fixed query batch and the oracle's full ranking of it (computed once, never changed)"""

    def __init__(self, orc, corpus, queries, seed, id_base=0, max_nq=512):
        self.corpus, self.queries, self.id_base = corpus, np.ascontiguousarray(queries, np.float32), id_base
        self.n, self.dim = corpus.shape
        self.levels = icd_levels(self.n, seed + 1)
        self.index = _native.IcdIndex(corpus, self.levels, device=0, max_nq=max_nq, max_k=128, id_base=id_base, probe=False)
        self.ws = _native.IcdRankOf(self.index)
        self.fs, self.fi = orc.flat_ip_topk(corpus, self.queries, self.n, id_base=id_base)
        self.handles = {}

    def handle(self, mask):
        """the IcdRowMask of a boolean row mask (None stays None), made once per mask object"""
        if mask is None:
            return None
        if id(mask) not in self.handles:
            self.handles[id(mask)] = (mask, self.index.rowmask(np.nonzero(mask)[0].astype(np.int64)))
        return self.handles[id(mask)][1]

    def check(self, targets, masks=None, nq=None):
        nq = len(self.queries) if nq is None else nq
        targets = np.asarray(targets, np.int64).reshape(nq, -1)
        want = ro.rank_of_batch(self.fs[:nq], self.fi[:nq], self.levels, targets, masks, self.n, self.id_base)
        got = self.ws.rank_of(self.queries[:nq], targets, None if masks is None else [self.handle(m) for m in masks])
        same(got, want, (self.n, self.dim, nq, targets.shape[1]))
        return want

    def close(self):
        for _m, h in self.handles.values():
            h.close()
        self.ws.close()
        self.index.close()


@pytest.mark.parametrize("nt", [1, 16])
@pytest.mark.parametrize("dim,id_base", [(32, 0), (768, BASE), (160, 7)])
def test_shapes(oracle, dim, id_base, nt):
    for t, n in enumerate(SIZES):
        nq = (1, 5, 300)[(t + nt) % 3]
        case = Case(oracle, family_corpus(n, dim, 1000 + n + dim), unit_rows(nq, dim, 7 * n + dim), n + nt, id_base=id_base)
        try:
            rng = np.random.default_rng(n * 131 + nt)
            targets = rng.integers(0, n, (nq, nt)) + id_base          # (duplicates wherever nt > n)
            if nt > 1:
                targets[rng.random((nq, nt)) < 0.2] = -1               # padding anywhere in a query's list
                targets[0, -1] = id_base + n                           # one past the last row
                targets[-1, 0] = id_base - 3 if id_base else -7        # below the first
            # the first and the last row, and the first and last row of every tile
            edge = [0, n - 1] + [r for r in (T - 1, T, 2 * T - 1, 2 * T) if r < n]
            for j, r in enumerate(edge[:nt]):
                targets[min(j, nq - 1), j] = r + id_base
            rank = case.check(targets)[0]
            assert rank.max() < n
            # a shared mask, one mask per query (some None), the empty mask
            shared, empty = row_mask(n, n + 1), np.zeros(n, bool)
            case.check(targets, [shared] * nq)
            per = [None if q % 3 == 0 else (empty if q % 7 == 1 else row_mask(n, 50 + q % 11)) for q in range(nq)]
            want = case.check(targets, per)
            for q in range(nq):
                if per[q] is empty:
                    assert (want[0][q] == -1).all() and want[4][q] == 0
        finally:
            case.close()


@pytest.mark.parametrize("dim", [32, 768])
def test_all_tied_corpus(oracle, dim):
    """every row the same vector: every score ties and the rank is the number of admitted smaller ids"""
    n, nq = 2 * T + 5, 5
    corpus = np.ascontiguousarray(np.repeat(unit_rows(1, dim, 3), n, axis=0))
    case = Case(oracle, corpus, unit_rows(nq, dim, 4), 9, id_base=BASE)
    try:
        targets = np.stack([np.array([0, 1, 63, 64, T - 1, T, T + 1, 2 * T - 1, 2 * T, n - 1, 5, 5, 77, n - 2, 2, 200]) + BASE] * nq)
        want = case.check(targets)
        assert np.array_equal(want[0], targets - BASE)
        mask = row_mask(n, 21)
        want = case.check(targets, [mask] * nq)
        smaller = np.concatenate([[0], np.cumsum(mask)[:-1]])
        rows = targets[0] - BASE
        assert np.array_equal(want[0][0], np.where(mask[rows], smaller[rows], -1))
        assert (want[4] == mask.sum()).all()
    finally:
        case.close()


@pytest.mark.parametrize("dim", [32, 768])
def test_copies_zero_row_nan_and_subnormal_scores(oracle, dim):
    n = 2 * T + 5
    corpus = unit_rows(n, dim, 77)
    corpus[3] = 0.0
    corpus[5, dim // 2] = np.nan
    # bit-identical copies of row 100 in front of it and behind it, across a tile edge
    for r in (2, 99, 101, T, n - 1):
        corpus[r] = corpus[100]
    corpus[40] = corpus[41] = 2.0 ** -80      # with a query of 2 ** -60 entries: subnormal scores, two rows tied
    corpus[42] = -(2.0 ** -80)
    queries = unit_rows(6, dim, 5)
    queries[1] = 2.0 ** -60                   # every score of this query is subnormal or zero
    queries[2] = 0.0                          # every non-NaN score is +0: ties everywhere
    case = Case(oracle, corpus, queries, 13, id_base=BASE)
    try:
        targets = np.stack([np.array([100, 2, 99, 101, T, n - 1, 3, 5, 40, 41, 42, 100, 100, 0, 6, 7]) + BASE] * 6)
        want = case.check(targets)
        qs = [0, 1, 3, 4, 5]                                                                         # (query 2 ties every row)
        r100 = want[0][qs, 0]
        assert np.array_equal(want[0][qs, 1], r100 - 2) and np.array_equal(want[0][qs, 2], r100 - 1)   # the copies with smaller ids lead
        assert np.array_equal(want[0][qs, 3], r100 + 1) and np.array_equal(want[0][qs, 5], r100 + 3)
        assert want[0][2].tolist()[:6] == [99, 2, 98, 100, T - 1, n - 2]                             # all tied: the smaller ids without the NaN row
        assert (want[0][:, 7] == -1).all() and np.isnan(want[2][:, 7]).all()                         # the NaN row has no rank
        assert 0 < abs(float(want[2][1, 8])) < np.finfo(np.float32).tiny                             # a subnormal score
        assert want[0][1, 9] == want[0][1, 8] + 1
        mask = row_mask(n, 8)
        mask[[100, 2, 5]] = True
        mask[[99, 3]] = False
        want = case.check(targets, [mask, None, mask, None, mask, mask])
        assert want[0][0, 2] == -1 and np.isnan(want[1][0, 2]) and want[3][0, 2] == 0                # outside its mask
        assert want[0][0, 7] == -1 and want[3][0, 7] == case.levels[5]                               # NaN inside the mask: its level
    finally:
        case.close()


@pytest.mark.parametrize("kind", ["gauss", "clustered"])
@pytest.mark.parametrize("k", [16, 65, 128])
def test_consistent_with_search_masked(oracle, kind, k):
    """the defining property: the id search_masked (raw order) returns at position j has rank j, and its scores are the hit's bits -
    with and without a mask, on a Gaussian corpus and on an encoder-like one with near-ties (tests the device against itself)"""
    n, dim, nq = 2 * T + 5 + 300, 768, 40
    corpus = unit_rows(n, dim, 31, kind)
    corpus[200] = corpus[17]                  # one exact tie
    queries = unit_rows(nq, dim, 32, kind)
    levels = icd_levels(n, 33)
    index = _native.IcdIndex(corpus, levels, device=0, max_nq=64, max_k=128, id_base=BASE, probe=False)
    ws = _native.IcdRankOf(index)
    mask = index.rowmask(np.nonzero(row_mask(n, 34, 0.6))[0].astype(np.int64))
    try:
        for masks in (None, mask):
            raw, ids, lv = index.search_masked(queries, k, masks, reweighted=False) if masks is not None else index.search_range(queries, k, reweighted=False)
            adj_w = raw.astype(np.float64) * np.where(lv == 1, 1.2, np.where(lv == 3, 0.8, 1.0))
            for j0 in range(0, k, 16):
                cols = slice(j0, min(k, j0 + 16))
                rank, adj, raw_t, lv_t, _sel = ws.rank_of(queries, ids[:, cols], masks)
                assert np.array_equal(rank, np.broadcast_to(np.arange(j0, min(k, j0 + 16)), rank.shape)), (kind, k, j0)
                assert raw_t.tobytes() == np.ascontiguousarray(raw[:, cols]).tobytes()
                assert adj.tobytes() == np.ascontiguousarray(adj_w[:, cols]).tobytes()
                assert np.array_equal(lv_t, lv[:, cols])
    finally:
        mask.close()
        ws.close()
        index.close()


def test_same_bytes_on_every_run(oracle):
    n, dim, nq = 2 * T + 5, 160, 300
    case = Case(oracle, family_corpus(n, dim, 5), unit_rows(nq, dim, 6), 3)
    try:
        targets = np.random.default_rng(1).integers(0, n, (nq, 16))
        first = case.ws.rank_of(case.queries, targets)
        for _ in range(3):
            same(case.ws.rank_of(case.queries, targets), first, "repeat")
        import torch
        same(case.ws.rank_of(torch.from_numpy(case.queries).cuda(), targets), first, "device queries")
        small = _native.IcdRankOf(case.index, 64)   # a workspace smaller than the batch: chunks
        same(small.rank_of(case.queries, targets), first, "chunked")
        small.close()
    finally:
        case.close()


def test_errors_leave_outputs_untouched(oracle):
    n, dim = 65, 32
    corpus, levels = unit_rows(n, dim, 1), icd_levels(n, 2)
    lib = _native.load_library()
    index = _native.IcdIndex(corpus, levels, device=0, max_nq=64, max_k=16, probe=False)
    other = _native.IcdIndex(corpus, levels, device=0, max_nq=64, max_k=16, probe=False)
    view = index.view(np.arange(0, n, 2, dtype=np.int64))
    ws, ws_other = _native.IcdRankOf(index, 8), _native.IcdRankOf(other, 8)
    mask, mask_other = index.rowmask(np.arange(5, dtype=np.int64)), other.rowmask(np.arange(5, dtype=np.int64))
    q = unit_rows(8, dim, 3)
    tg = np.zeros((8, 16), np.int64)
    outs = [np.full((8, 16), 77, dt) for dt in (np.int64, np.float64, np.float32, np.int32)] + [np.full(8, 77, np.int64)]
    before = [o.tobytes() for o in outs]

    def call(idx_h, ws_h, nq=8, nt=16, masks=None, queries=q, targets=tg):
        table = None if masks is None else np.array([m._h.value if m is not None else 0 for m in masks], np.uint64)
        rc = lib.icd_index_rank_of(idx_h, ws_h, None if queries is None else queries.ctypes.data, nq, 0, None if targets is None else targets.ctypes.data, nt,
                                   None if table is None else table.ctypes.data, *[o.ctypes.data for o in outs], None)
        assert [o.tobytes() for o in outs] == before, "a refused call wrote an output"
        return rc

    try:
        assert call(view._h, ws._h) == -4                                  # a view as idx
        assert call(index._h, ws_other._h) == -1                           # a workspace of another index
        assert call(index._h, ws._h, masks=[mask_other] * 8) == -1         # a mask of another index
        assert call(index._h, ws._h, nt=0) == -1 and call(index._h, ws._h, nt=17) == -1
        assert call(index._h, ws._h, nq=9) == -1                           # above the workspace's max_nq
        assert call(index._h, ws._h, nq=-1) == -1
        assert call(index._h, ws._h, queries=None) == -1 and call(index._h, ws._h, targets=None) == -1
        assert lib.icd_index_rank_of(index._h, ws._h, q.ctypes.data, 8, 0, tg.ctypes.data, 16, None, None, None, None, None, None, None) == -1   # out_rank NULL
        out = ctypes.c_void_p()
        assert lib.icd_rankof_create(view._h, 8, ctypes.byref(out)) == -4 and not out.value
        assert lib.icd_rankof_create(index._h, 0, ctypes.byref(out)) == -1 and not out.value
        assert ws.stats()["max_nq"] == 8 and ws.stats()["bytes"] > 0
        with pytest.raises(ValueError):
            ws.rank_of(q, np.zeros((8, 17), np.int64))
        with pytest.raises(ValueError):
            ws.rank_of(q, np.zeros((7, 2), np.int64))
        # destroyed handles: the mask, the workspace, the index
        dead_mask = index.rowmask(np.arange(3, dtype=np.int64))
        table = np.array([dead_mask._h.value] * 8, np.uint64)
        dead_mask.close()
        assert lib.icd_index_rank_of(index._h, ws._h, q.ctypes.data, 8, 0, tg.ctypes.data, 16, table.ctypes.data, *[o.ctypes.data for o in outs], None) == -5
        dead_ws = _native.IcdRankOf(index, 8)
        h = ctypes.c_void_p(dead_ws._h.value)
        dead_ws.close()
        assert call(index._h, h) == -5
        assert lib.icd_rankof_destroy(h) == -5 and lib.icd_rankof_stats(h, None, None) == -5
        assert [o.tobytes() for o in outs] == before
        rank = ws.rank_of(q, tg[:, :1])[0]                # (a good call on the same handles still works)
        assert rank.min() >= 0
    finally:
        for h_ in (mask, mask_other, ws, ws_other, view, other):
            h_.close()
        index.close()
    assert lib.icd_index_rank_of(None, None, q.ctypes.data, 8, 0, tg.ctypes.data, 16, None, *[o.ctypes.data for o in outs], None) == -5
    assert [o.tobytes() for o in outs] == before


def test_destruction_orders(oracle):
    """workspace, mask and index may go in any order; a call with a closed partner raises"""
    n, dim = 130, 32
    corpus, levels, q = unit_rows(n, dim, 1), icd_levels(n, 2), unit_rows(3, dim, 3)
    tg = np.array([[0], [64], [128]], np.int64)   # (even rows: inside the mask)
    for order in ("wmi", "iwm", "miw", "imw"):
        index = _native.IcdIndex(corpus, levels, device=0, max_nq=64, max_k=16, probe=False)
        ws, mask = _native.IcdRankOf(index, 4), index.rowmask(np.arange(0, n, 2, dtype=np.int64))
        rank, _adj, _raw, _lv, sel = ws.rank_of(q, tg, mask)
        assert (sel == 65).all() and (rank >= 0).all()
        things = {"w": ws, "m": mask, "i": index}
        for c in order:
            things[c].close()
            if c != "m" and not all(t.closed for t in things.values()):
                with pytest.raises(_native.IcdError):
                    ws.rank_of(q, tg, None)
