"""icd_index_search_by_rows on the device against tests/byrows_oracle.py over the CPU oracle's full
ranking, byte for byte: no tolerance anywhere. Corpus sizes sit around k (n = 1, 2, k, k + 1, k + 2: the (k + 1)-wide list is
short, exactly full, one over), k around the lane and half-wave edges of the drop (15 .. 17, 31 .. 33, 64, 127), batches of 1, 4,
5 and 300 ids (one wave, one work-group of four waves, one wave into the next group, many groups, and the three exact kernels
behind them), dims 32, 768, 1024 and 160 (the mixed-walk set of tests/test_mmr_select_gpu.py). Corpora hold families of
bit-identical rows (the self hit is not rank 0), a row of zeros (everything ties) and a row holding NaN (no hit at all)."""
import ctypes

import numpy as np
import pytest

import byrows_oracle as bo
from conftest import icd_levels, unit_rows
from rag_project_icd10_amd import _native

pytestmark = pytest.mark.gpu

KS = (1, 15, 16, 17, 31, 32, 33, 64, 127)
NQS = (1, 4, 5, 300)
BASE = 5_000_000_000


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def same(got, want, what):
    """arrays compared byte for byte (-0.0 and NaN payloads included)"""
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        g = host(g)
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


class Case:
    """one corpus on the device with the oracle's full ranking of every stored row as a query"""

    def __init__(self, orc, corpus, seed, id_base=0, max_nq=512, max_k=128):
        self.orc, self.corpus, self.id_base = orc, corpus, id_base
        self.n, self.dim = corpus.shape
        self.levels = icd_levels(self.n, seed + 1)
        self.index = _native.IcdIndex(corpus, self.levels, device=0, max_nq=max_nq, max_k=max_k, id_base=id_base, probe=False)
        self.ws = self.index.byrows()
        self.fs, self.fi = orc.flat_ip_topk(corpus, corpus, self.n, id_base=id_base)   # computed once, never changed

    def want(self, ids, k, masks=None, include_self=False, statement=bo.without_self, **bounds):
        rows = np.asarray(ids, np.int64) - self.id_base
        return bo.byrows_batch(self.fs[rows], self.fi[rows], self.levels, ids, k, masks=masks, id_base=self.id_base,
                               include_self=include_self, statement=statement, **bounds)

    def check(self, ids, k, masks=None, handles=None, include_self=False, **bounds):
        raw, rew = self.want(ids, k, masks, include_self, **bounds)
        what = (self.n, self.dim, k, len(ids), include_self)
        kw = dict(workspace=self.ws, masks=handles, include_self=include_self, **bounds)
        same(self.index.search_by_rows(ids, k, reweighted=False, **kw), raw, what + ("raw",))
        same(self.index.search_by_rows(ids, k, reweighted=True, **kw), rew, what + ("reweighted",))
        return raw, rew

    def close(self):
        self.ws.close()
        self.index.close()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dim,id_base", [(32, 0), (768, BASE), (1024, 0), (160, 7)])
def test_shapes(oracle, dim, id_base, k):
    for t, n in enumerate(sorted({1, 2, k, k + 1, k + 2, 129, 257})):
        case = Case(oracle, family_corpus(n, dim, 1000 + n + dim), n + k, id_base=id_base)
        try:
            rng = np.random.default_rng(n * 131 + k)
            nq = NQS[(t + k) % len(NQS)]
            ids = rng.integers(0, n, nq) + id_base            # (the same id may repeat: it does wherever nq > n)
            raw, _ = case.check(ids, k)
            assert (raw[1] != ids[:, None]).all()             # no row is its own neighbour
            hits = (raw[1] >= 0).sum(axis=1)
            if n > 5:                                         # row 5 holds a NaN: it has no neighbour and is nobody's
                assert np.array_equal(hits, np.where(ids - id_base == 5, 0, min(k, n - 2)))
            else:
                assert (hits == min(k, n - 1)).all()          # n = 1: all padding
            # the two statements of the contract agree on this very batch
            same(case.want(ids, k, statement=bo.drop_self)[0], raw, "statements, raw")
            if n == 257:
                for nq2 in NQS:                               # every batch size at the full corpus
                    case.check(rng.integers(0, n, nq2) + id_base, k)
                case.check(ids, k, include_self=True)
        finally:
            case.close()


@pytest.mark.parametrize("dim", [32, 768])
def test_ties_zero_rows_nan_rows_and_repeats(oracle, dim):
    n = 257
    case = Case(oracle, family_corpus(n, dim, 77), 5, id_base=BASE)
    try:
        # a family of bit-identical rows with ids on both sides of the query's: its own hit is not rank 0
        fam = None
        for r in range(8, n - 1):
            b = [case.corpus[j].tobytes() for j in (r - 2, r - 1, r, r + 1)]
            if b[0] != b[2] and b[1] == b[2] == b[3]:
                fam = r
                break
        assert fam is not None
        full = case.want([fam + BASE], 10, include_self=True)[0]
        assert full[1][0][0] == fam - 1 + BASE and (full[1][0] == fam + BASE).any()
        ids = np.array([fam, fam, 3, fam, 5, fam, fam, 0, n - 1], np.int64) + BASE   # the same id five times; the zero row; the NaN row
        for k in (1, 10, 16, 127):
            raw, _ = case.check(ids, k)
            assert all(arr[q].tobytes() == arr[0].tobytes() for arr in raw for q in (1, 3, 5, 6))   # the repeats: the same list
            assert raw[1][0][0] == fam - 1 + BASE and (k == 1 or raw[1][0][1] == fam + 1 + BASE)   # self cut out of the middle of its family
            zero = raw[1][2][raw[1][2] >= 0] - BASE
            assert (raw[0][2][: len(zero)] == 0).all() and list(zero) == [r for r in range(n) if r not in (3, 5)][: len(zero)]   # all tied: id order
            assert (raw[1][4] < 0).all()                                                   # a NaN query has no hit
            case.check(ids, k, include_self=True)
        case.check(ids, 128, include_self=True)
    finally:
        case.close()


@pytest.mark.parametrize("nq", [5, 300])
def test_masks_bands_and_the_masked_search(oracle, nq):
    import torch
    n, dim = 257, 768
    case = Case(oracle, family_corpus(n, dim, 31, special=False), 9)
    try:
        index = case.index
        rng = np.random.default_rng(nq)
        ids = rng.integers(0, n, nq).astype(np.int64)
        rows = np.arange(n)
        shapes = [(None, None), (rows % 2 == 1, index.rowmask(rows[rows % 2 == 1])), (rows < 7, index.rowmask(rows[:7])),
                  (np.zeros(n, bool), index.rowmask(np.zeros(0, np.int64))), (rows % 3 != 0, index.rowmask(rows[rows % 3 != 0]))]
        bools = [shapes[q % len(shapes)][0] for q in range(nq)]
        handles = [shapes[q % len(shapes)][1] for q in range(nq)]
        excl = [b is not None and not b[i] for b, i in zip(bools, ids)]
        assert any(excl) and not all(excl)                    # masks that exclude the row itself, and masks that hold it
        vecs = np.ascontiguousarray(case.corpus[ids])         # the host copy of the same rows
        for k in (10, 16, 64, 127):
            raw, rew = case.check(ids, k, masks=bools, handles=handles)
            assert (raw[1][2] >= 0).sum() <= 7 < k            # a mask that leaves fewer than k rows: padding
            case.check(ids, k, masks=bools, handles=handles, include_self=True)
            # include_self = 1 IS icd_index_search_masked at k
            for rw in (False, True):
                same(index.search_by_rows(ids, k, workspace=case.ws, masks=handles, include_self=True, reweighted=rw),
                     [host(x) for x in index.search_masked(vecs, k, handles, reweighted=rw)], ("include_self against search_masked", k, rw))
            # include_self = 0 IS icd_index_search_masked at k + 1 with the row's own hit dropped in numpy
            m_raw = index.search_masked(vecs, k + 1, handles, reweighted=False)
            m_rew = index.search_masked(vecs, k + 1, handles, reweighted=True)
            cut_raw = [bo.drop_from_list(m_raw[0][q], m_raw[1][q], m_raw[2][q], ids[q]) for q in range(nq)]
            cut_rew = [bo.drop_reweighted_list(m_rew[0][q], m_rew[1][q], m_rew[2][q], m_rew[3][q], ids[q]) for q in range(nq)]
            same(raw, [np.stack([c[j] for c in cut_raw]) for j in range(3)], ("masked at k + 1, raw", k))
            same(rew, [np.stack([c[j] for c in cut_rew]) for j in range(4)], ("masked at k + 1, reweighted", k))
        case.check(ids, 10, masks=[shapes[1][0]] * nq, handles=shapes[1][1])   # ONE mask for every id
        # bands: a ceiling below 1 excludes the row itself (unit rows score 1 against themselves); a floor; both
        ceil = np.full(nq, 0.5, np.float32)
        floor = np.array([case.fs[i][min(20 + q % 5, n - 1)] for q, i in enumerate(ids)], np.float32)
        for k in (10, 33):
            raw, _ = case.check(ids, k, range_filter=ceil)
            assert (raw[0][raw[1] >= 0] <= 0.5).all()
            same(raw, [host(x) for x in index.search_masked(vecs, k, [None] * nq, range_filter=ceil, reweighted=False)], "a band without self is search_masked at k")
            case.check(ids, k, radius=floor)
            case.check(ids, k, masks=bools, handles=handles, radius=floor, range_filter=np.full(nq, 0.999, np.float32))
        # device ids: the same bytes as host ids, twice; one id out of range is padding and the others do not change
        dids = torch.from_numpy(ids).cuda()
        for rw in (False, True):
            a = index.search_by_rows(ids, 10, workspace=case.ws, masks=handles, reweighted=rw)
            for _ in range(2):
                b = index.search_by_rows(dids, 10, workspace=case.ws, masks=handles, reweighted=rw)
                torch.cuda.synchronize()
                same(b, list(a), ("device ids against host ids", rw))
            c = index.search_by_rows(ids, 10, workspace=case.ws, masks=handles, reweighted=rw, on_device=True)
            torch.cuda.synchronize()
            same(c, list(a), ("device outputs", rw))
            for bad in (n, -1, -2**62, 2**62):
                wild = ids.copy()
                wild[1] = bad
                d = [host(x) for x in index.search_by_rows(torch.from_numpy(wild).cuda(), 10, workspace=case.ws, masks=handles, reweighted=rw)]
                pad = [np.full(10, v, x.dtype) for v, x in zip(((-np.inf,) if rw else ()) + (-np.inf, -1, 0), d)]
                for x, p, want in zip(d, pad, a):
                    assert x[1].tobytes() == p.tobytes(), (bad, rw)
                    keep = np.arange(nq) != 1
                    assert x[keep].tobytes() == want[keep].tobytes(), (bad, rw)
        # a workspace smaller than the batch: chunks, the same bytes
        small = index.byrows(2)
        try:
            assert small.stats()["max_nq"] == 2 and small.stats()["bytes"] > 0
            same(index.search_by_rows(ids, 10, workspace=small, masks=handles), case.want(ids, 10, bools)[1], "small workspace")
        finally:
            small.close()
        for _, h in shapes:
            if h is not None:
                h.close()
    finally:
        case.close()


def test_refusals_leave_outputs_as_they_were(oracle):
    """every refusal of icd_index_search_by_rows, through the C entry point itself, outputs pre-filled; each followed by a good call"""
    case = Case(oracle, family_corpus(64, 32, 3, special=False), 3, max_nq=8)
    other = Case(oracle, family_corpus(64, 32, 4, special=False), 4, max_nq=8)
    lib = case.index._lib
    INVALID, UNSUPPORTED, STATE = -1, -4, -5
    try:
        index, ws = case.index, case.ws
        narrow = _native.IcdIndex(case.corpus, case.levels, device=0, max_nq=8, max_k=16, probe=False)
        narrow_ws = narrow.byrows()
        tiny = index.byrows(1)
        view = index.view(np.arange(0, 64, 2))
        foreign_mask = other.index.rowmask(np.arange(10))
        dead_mask = index.rowmask(np.arange(10))
        dead_h = dead_mask._h.value
        dead_mask.close()
        dead_ws = index.byrows(4)
        dead_ws_h = dead_ws._h.value
        dead_ws.close()
        good_ids = np.array([5, 9], np.int64)
        nan = np.array([np.nan, 0.0], np.float32)
        lo, hi = np.array([0.5, 0.5], np.float32), np.array([0.5, 0.1], np.float32)

        def call(idx=index._h, handle=ws._h, masks=None, ids=good_ids, nq=2, k=4, include_self=0, radius=None, range_filter=None, null_ids=False):
            outs = (np.full((2, 128), 7.5), np.full((2, 128), 7.5, np.float32), np.full((2, 128), 77, np.int64), np.full((2, 128), 7, np.int32))
            table = None if masks is None else (ctypes.c_void_p * len(masks))(*masks)
            rc = lib.icd_index_search_by_rows(idx, handle, None if table is None else ctypes.cast(table, ctypes.c_void_p),
                                              None if null_ids else ids.ctypes.data, nq, k, 0, include_self,
                                              None if radius is None else radius.ctypes.data, None if range_filter is None else range_filter.ctypes.data,
                                              0, 1, *[o.ctypes.data for o in outs], 0, None)
            untouched = all((o == (77 if o.dtype == np.int64 else 7 if o.dtype == np.int32 else 7.5)).all() for o in outs)
            return rc, untouched

        def good():
            same(index.search_by_rows(good_ids, 4, workspace=ws), case.want(good_ids, 4)[1], "a good call behind a refusal")

        good()
        refusals = [
            (dict(k=0), INVALID), (dict(k=128), INVALID), (dict(k=129, include_self=1), INVALID), (dict(k=-1), INVALID),
            (dict(idx=narrow._h, handle=narrow_ws._h, k=16), INVALID),                           # k + 1 above the index's max_k
            (dict(ids=np.array([5, 64], np.int64)), INVALID), (dict(ids=np.array([-1, 5], np.int64)), INVALID),   # host ids outside the index
            (dict(null_ids=True), INVALID),
            (dict(handle=tiny._h), INVALID),                                                     # nq above the workspace's max_nq
            (dict(nq=9), INVALID), (dict(nq=-1), INVALID),                                       # nq above the index's
            (dict(radius=nan), INVALID), (dict(range_filter=nan), INVALID), (dict(radius=lo, range_filter=hi), INVALID),
            (dict(handle=other.ws._h), INVALID),                                                 # a workspace of another index
            (dict(masks=[None, foreign_mask._h.value]), INVALID),                                # a mask of another index
            (dict(handle=dead_ws_h), STATE), (dict(masks=[dead_h, None]), STATE), (dict(idx=None), STATE), (dict(handle=None), STATE),
            (dict(idx=view._h), UNSUPPORTED),                                                    # a view as idx: mask the parent
        ]
        for kw, code in refusals:
            rc, untouched = call(**kw)
            assert rc == code, (kw, rc, lib.icd_last_error())
            assert untouched, kw
            good()
        rc, untouched = call(nq=0)
        assert rc == 0 and untouched                                                             # nq = 0 returns ICD_OK and writes nothing
        rc, untouched = call(k=128, include_self=1)
        assert rc == 0 and not untouched                                                         # k = ICD_MAX_K is include_self's alone
        rc, untouched = call(idx=narrow._h, handle=narrow_ws._h, k=15)
        assert rc == 0 and not untouched
        out = ctypes.c_void_p()
        assert lib.icd_byrows_create(view._h, 4, ctypes.byref(out)) == UNSUPPORTED and not out.value
        assert lib.icd_byrows_create(index._h, 0, ctypes.byref(out)) == INVALID and lib.icd_byrows_create(None, 4, ctypes.byref(out)) == STATE
        assert lib.icd_byrows_stats(dead_ws_h, None, None) == STATE and lib.icd_byrows_destroy(dead_ws_h) == STATE
        # the wrapper's own checks raise before the library is asked
        for k, inc in ((0, False), (128, False), (129, True)):
            with pytest.raises(ValueError):
                index.search_by_rows(good_ids, k, workspace=ws, include_self=inc)
        with pytest.raises(_native.IcdError):
            index.search_by_rows(good_ids, 4, workspace=dead_ws)
        good()
        for h in (foreign_mask, tiny, narrow_ws, narrow, view):
            h.close()
    finally:
        case.close()
        other.close()


def test_lifetime_either_may_go_first(oracle):
    case = Case(oracle, family_corpus(33, 32, 9, special=False), 9, max_nq=8)
    ids = np.array([0, 32, 7], np.int64)
    want = case.want(ids, 3)[1]
    same(case.index.search_by_rows(ids, 3, workspace=case.ws), want, "before")
    # the workspace before the index
    case.ws.close()
    assert case.ws.closed
    second = case.index.byrows(4)
    same(case.index.search_by_rows(ids, 3, workspace=second), want, "a second workspace")
    # the index before the workspace: the workspace stays a handle (stats, close), a search with it is refused
    case.index.close()
    assert second.stats()["max_nq"] == 4
    with pytest.raises(_native.IcdError):
        case.index.search_by_rows(ids, 3, workspace=second)
    # an index re-created over the same rows is another index: the old workspace is not its own
    again = _native.IcdIndex(case.corpus, case.levels, device=0, max_nq=8, max_k=128, probe=False)
    try:
        with pytest.raises(_native.IcdError) as e:
            again.search_by_rows(ids, 3, workspace=second)
        assert e.value.code == -1
        second.close()
        mine = again.byrows()
        same(again.search_by_rows(ids, 3, workspace=mine), want, "the new index")
        mine.close()
    finally:
        again.close()
