"""icd_index_search_mmr on the device against tests/mmr_oracle.py, byte for byte: no tolerance anywhere.
Corpus sizes sit around the 128 candidates of a list (fewer rows than fetch_k, one row, one more than a list), dims at every gear
of the chain's walk (32 and 64: pairs only; 768, 1024 and 4096: trips of eight blocks only; 160, 224 and 800: trips, then one or
three pairs - the hand-over of b0 from the trip loop to the pair loop), corpora that make values tie (exact duplicates, every row
equal, rows of zeros; duplicates and subnormals at 160 too), subnormal scores and NaN rows; every (k, fetch_k) of the issue's list at every lambda; batches of 1, 3 and
300 queries with per-query masks and bands; device against host outputs; every refusal of the C entry point."""
import ctypes

import numpy as np
import pytest

from conftest import icd_levels, unit_rows
from mmr_oracle import mmr_batch
from rag_project_icd10_amd import _native
from rag_project_icd10_amd.services import filter_expr as fe

pytestmark = pytest.mark.gpu

K_FETCH = ((1, 1), (1, 128), (2, 2), (10, 20), (10, 128), (63, 64), (64, 65), (128, 128))
LAMBDAS = (0.0, 0.3, 0.5, 1.0)
R, NOT = 1, 6   # filter program words (include/icd_search.h ICD_FILTER_RANGE / _NOT)


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def same(got, want, what):
    """arrays compared byte for byte (-0.0 and NaN payloads included)"""
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        g = host(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, j, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, j, g, w)


def corpus_of(kind, n, dim, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return unit_rows(n, dim, seed)
    if kind == "duplicates":   # families of 1 .. 5 identical rows: sim equals rel's own maximum and values tie
        base = unit_rows(n, dim, seed)
        fam = np.repeat(np.arange(n), rng.integers(1, 6, n))[:n]
        return np.ascontiguousarray(base[fam])
    if kind == "equal":
        return np.ascontiguousarray(np.repeat(unit_rows(1, dim, seed), n, axis=0))
    if kind == "zeros":
        return np.zeros((n, dim), np.float32)
    if kind == "subnormal":    # scores and similarities around 1e-42: below the smallest normal float32
        return np.ascontiguousarray(unit_rows(n, dim, seed) * np.float32(1e-21))
    if kind == "nan":          # rows holding NaN are never candidates
        x = unit_rows(n, dim, seed)
        x[rng.random(n) < 0.25, rng.integers(0, dim)] = np.nan
        x[0, 0] = np.nan
        return x
    raise AssertionError(kind)


class Case:
    """one corpus on the device with its oracle ranking"""

    def __init__(self, orc, kind, n, dim, seed, nq=3, id_base=0, max_nq=512, qscale=1.0):
        self.orc, self.n, self.dim, self.id_base = orc, n, dim, id_base
        self.corpus = corpus_of(kind, n, dim, seed)
        self.levels = icd_levels(n, seed + 1)
        self.queries = np.ascontiguousarray(unit_rows(nq, dim, seed + 2) * np.float32(qscale))
        self.index = _native.IcdIndex(self.corpus, self.levels, device=0, max_nq=max_nq, max_k=128, id_base=id_base, probe=False)
        self.mmr = self.index.mmr()
        self.fs, self.fi = orc.flat_ip_topk(self.corpus, self.queries, n, id_base=id_base)

    def want(self, k, fetch_k, lam, masks=None, **bounds):
        return mmr_batch(self.orc, self.corpus, self.levels, self.fs, self.fi, k, fetch_k, lam, masks=masks, id_base=self.id_base, **bounds)

    def check(self, k, fetch_k, lam, masks=None, handles=None, **bounds):
        pick, rew = self.want(k, fetch_k, lam, masks, **bounds)
        what = (self.n, self.dim, k, fetch_k, lam)
        got = self.index.search_mmr(self.queries, k, fetch_k, lam, mmr=self.mmr, masks=handles, reweighted=False, **bounds)
        assert got[0] is None
        same(got[1:], pick, what + ("pick order",))
        same(self.index.search_mmr(self.queries, k, fetch_k, lam, mmr=self.mmr, masks=handles, reweighted=True, **bounds), rew, what + ("reweighted",))
        return pick, rew

    def close(self):
        self.mmr.close()
        self.index.close()


def sweep(case):
    for k, fetch_k in K_FETCH:
        for lam in LAMBDAS:
            pick, rew = case.check(k, fetch_k, lam)
            hits = min(fetch_k, int((case.fi[0] >= 0).sum()))
            assert int((pick[1][0] >= 0).sum()) == min(k, hits)                       # C < fetch_k, C < k: padding behind the picks
            if lam == 1.0:      # plain relevance: search_masked at k, bit for bit, in both forms
                same(pick[:3], case.index.search_masked(case.queries, k, [None] * len(case.queries), reweighted=False), "lambda = 1, raw")
                same(rew[:4], case.index.search_masked(case.queries, k, [None] * len(case.queries), reweighted=True), "lambda = 1, reweighted")
            if k == fetch_k:    # a permutation of the candidate list
                cand = case.index.search_masked(case.queries, fetch_k, [None] * len(case.queries), reweighted=False)
                for q in range(len(case.queries)):
                    assert sorted(pick[1][q].tolist()) == sorted(cand[1][q].tolist())
                    assert sorted(pick[0][q].tolist()) == sorted(cand[0][q].tolist())


@pytest.mark.parametrize("n,dim,id_base", [(1, 32, 0), (2, 32, 0), (9, 32, 0), (127, 32, 0), (128, 32, 0), (129, 32, 5_000_000_000), (257, 32, 0),
                                           (1, 768, 0), (2, 768, 0), (9, 768, 0), (127, 768, 0), (128, 768, 0), (129, 768, 0), (257, 768, 7),
                                           (129, 4096, 0),
                                           # the walk changes gear (16 floats a block, 8 blocks a trip, then pairs): two pairs and no trip;
                                           # one trip + one pair; one trip + three pairs; six trips + one pair; eight trips and no pair
                                           (129, 64, 0), (129, 160, 0), (129, 224, 0), (129, 800, 0), (129, 1024, 0), (257, 160, 7)])
def test_corpus_shapes(oracle, n, dim, id_base):
    case = Case(oracle, "random", n, dim, 100 + n + dim, id_base=id_base)
    try:
        sweep(case)
    finally:
        case.close()


@pytest.mark.parametrize("kind,dim", [pytest.param(kind, 32, id=kind) for kind in ("duplicates", "equal", "zeros", "subnormal", "nan")]
                         + [pytest.param("duplicates", 160, id="duplicates-160"), pytest.param("subnormal", 160, id="subnormal-160")])
def test_corpora_that_tie(oracle, kind, dim):
    case = Case(oracle, kind, 129, dim, 7, qscale=1e-21 if kind == "subnormal" else 1.0)
    try:
        if kind == "subnormal":
            s = case.fs[np.isfinite(case.fs)]
            assert (np.abs(s[s != 0]) < np.finfo(np.float32).tiny).all() and (s != 0).any()
        if kind == "nan":
            assert (case.fi < 0).any()                                              # the NaN rows are no candidates
        sweep(case)
        if kind == "duplicates":   # both tie rules were exercised: a pick that tied on the value, and one whose value was the maximum alone
            pick, _ = case.want(10, 128, 0.5)
            rows = pick[1][0] - case.id_base
            assert len({case.corpus[r].tobytes() for r in rows}) == len(rows)       # at lambda 0.5 no copy of a picked row is picked in the first 10
            cand = case.want(128, 128, 1.0)[0]
            fam = [case.corpus[r].tobytes() for r in cand[1][0][:20]]
            assert len(set(fam)) < len(fam)                                         # the candidate list does hold copies (equal rel: ties)
    finally:
        case.close()


@pytest.mark.parametrize("nq", [1, 3, 300])
def test_batches_masks_and_bands(oracle, nq):
    n = 257
    case = Case(oracle, "duplicates", n, 768, 31, nq=nq, max_nq=512)
    try:
        index = case.index
        rows = np.arange(n)
        cols = index.columns(np.ascontiguousarray(np.stack([rows, rows % 3]).astype(np.int32)))
        off, words = fe.pack_programs([np.asarray([R, 1, 1, 2], np.uint32)])
        produced = index.filter_masks(cols, None, off, words)[0]                    # column 1 in [1, 2): a mask filter_masks made
        shapes = [(np.zeros(n, bool), index.rowmask(np.zeros(0, np.int64))), (None, None), (rows == 5, index.rowmask(np.array([5]))),
                  (rows % 2 == 1, index.rowmask(rows[rows % 2 == 1])), (rows % 3 == 1, produced)]
        bools = [shapes[q % len(shapes)][0] for q in range(nq)]
        handles = [shapes[q % len(shapes)][1] for q in range(nq)]
        for k, fetch_k, lam in ((10, 20, 0.3), (10, 128, 0.5), (128, 128, 0.0)):
            case.check(k, fetch_k, lam, masks=bools, handles=handles)
        case.check(10, 20, 0.5, masks=[shapes[3][0]] * nq, handles=shapes[3][1])          # ONE mask for every query
        # bands: per-query bounds from the ranking itself; one leaves C = 0, one C = 1
        s = case.fs
        radius = np.array([s[q][min(30 + q % 7, n - 1)] for q in range(nq)], np.float32)
        ceil = np.array([s[q][2] for q in range(nq)], np.float32)
        radius[0], ceil[0] = s[0][0], np.inf                                        # nothing lies above the best score: C = 0
        if nq > 1:
            below = int(np.flatnonzero(s[1] < s[1][0])[0])                          # the first rank behind the best row and its copies
            radius[1], ceil[1] = s[1][below], s[1][0]                               # C = the best row (and its copies) alone
        for k, fetch_k, lam in ((10, 20, 0.5), (64, 65, 0.3)):
            pick, _ = case.check(k, fetch_k, lam, radius=radius, range_filter=ceil)
            assert (pick[1][0] < 0).all()
        pick, _ = case.check(5, 40, 0.5, masks=bools, handles=handles, radius=radius)   # masks and a floor together
        if nq > 1:
            assert int((case.want(128, 128, 0.5, radius=radius, range_filter=ceil)[0][1][1] >= 0).sum()) == below
        # device outputs against host outputs; the same call twice gives the same bytes
        import torch
        qd = torch.from_numpy(case.queries).cuda()
        for rw in (False, True):
            a = index.search_mmr(case.queries, 10, 128, 0.5, mmr=case.mmr, masks=handles, reweighted=rw)
            b = index.search_mmr(qd, 10, 128, 0.5, mmr=case.mmr, masks=handles, reweighted=rw)
            c = index.search_mmr(case.queries, 10, 128, 0.5, mmr=case.mmr, masks=handles, reweighted=rw, on_device=True)
            d = index.search_mmr(qd, 10, 128, 0.5, mmr=case.mmr, masks=handles, reweighted=rw)
            torch.cuda.synchronize()
            for other in (b, c, d):
                same([x for x in other if x is not None], [x for x in a if x is not None], ("device against host", rw))
        # a handle smaller than the index's max_nq: the batch runs in chunks, the bytes are the same
        small = index.mmr(2)
        try:
            assert small.stats()["max_nq"] == 2 and small.stats()["bytes"] > 0
            same(index.search_mmr(case.queries, 10, 20, 0.3, mmr=small, masks=handles), case.want(10, 20, 0.3, bools)[1], "small handle")
        finally:
            small.close()
        for _, h in shapes:
            if h is not None:
                h.close()
        cols.close()
    finally:
        case.close()


def test_refusals_leave_everything_as_it_was(oracle):
    """every refusal of icd_index_search_mmr, through the C entry point itself, outputs pre-filled; each followed by a good call"""
    case = Case(oracle, "random", 64, 32, 3, nq=2, max_nq=8)
    other = Case(oracle, "random", 64, 32, 4, nq=2, max_nq=8)
    lib = case.index._lib
    INVALID, UNSUPPORTED, STATE = -1, -4, -5
    try:
        index, mmr = case.index, case.mmr
        assert index.max_k == 128
        narrow = _native.IcdIndex(case.corpus, case.levels, device=0, max_nq=8, max_k=16, probe=False)
        narrow_mmr = narrow.mmr()
        tiny = index.mmr(1)
        view = index.view(np.arange(0, 64, 2))
        foreign_mask = other.index.rowmask(np.arange(10))
        dead_mask = index.rowmask(np.arange(10))
        dead_h = dead_mask._h.value
        dead_mask.close()
        dead_mmr = index.mmr(4)
        dead_mmr_h = dead_mmr._h.value
        dead_mmr.close()
        q = case.queries
        nan = np.array([np.nan, 0.0], np.float32)
        lo, hi = np.array([0.5, 0.5], np.float32), np.array([0.5, 0.1], np.float32)

        def call(idx=index._h, handle=mmr._h, masks=None, nq=2, k=4, fetch_k=8, lam=0.5, radius=None, range_filter=None):
            outs = (np.full((2, 8), 7.5), np.full((2, 8), 7.5, np.float32), np.full((2, 8), 77, np.int64), np.full((2, 8), 7, np.int32), np.full((2, 8), 7.5))
            table = None
            if masks is not None:
                table = (ctypes.c_void_p * len(masks))(*masks)
            rc = lib.icd_index_search_mmr(idx, handle, None if table is None else ctypes.cast(table, ctypes.c_void_p), q.ctypes.data, nq, k, fetch_k,
                                          ctypes.c_double(lam), 0, None if radius is None else radius.ctypes.data,
                                          None if range_filter is None else range_filter.ctypes.data, 0, 1, *[o.ctypes.data for o in outs], 0, None)
            untouched = all((o == (77 if o.dtype == np.int64 else 7 if o.dtype == np.int32 else 7.5)).all() for o in outs)
            return rc, untouched

        def good():
            same(index.search_mmr(q, 4, 8, 0.5, mmr=mmr), case.want(4, 8, 0.5)[1], "a good call behind a refusal")

        good()
        refusals = [
            (dict(k=0), INVALID), (dict(k=129, fetch_k=128), INVALID), (dict(fetch_k=0, k=1), INVALID), (dict(fetch_k=129), INVALID),
            (dict(k=9, fetch_k=8), INVALID),                                                     # k > fetch_k
            (dict(idx=narrow._h, handle=narrow_mmr._h, fetch_k=17), INVALID),                    # fetch_k above the index's max_k
            (dict(handle=tiny._h), INVALID),                                                     # nq above the handle's max_nq
            (dict(nq=9), INVALID),                                                               # nq above the index's (and the handle's)
            (dict(nq=-1), INVALID),
            (dict(lam=-0.01), INVALID), (dict(lam=1.01), INVALID), (dict(lam=float("nan")), INVALID),
            (dict(radius=nan), INVALID), (dict(range_filter=nan), INVALID), (dict(radius=lo, range_filter=hi), INVALID),   # bad host bounds
            (dict(handle=other.mmr._h), INVALID),                                                # a handle of another index
            (dict(masks=[None, foreign_mask._h.value]), INVALID),                                # a mask of another index
            (dict(handle=dead_mmr_h), STATE), (dict(masks=[dead_h, None]), STATE), (dict(idx=None), STATE), (dict(handle=None), STATE),
            (dict(idx=view._h), UNSUPPORTED),                                                    # a view as idx: mask the parent
        ]
        for kw, code in refusals:
            rc, untouched = call(**kw)
            assert rc == code, (kw, rc, lib.icd_last_error())
            assert untouched, kw
            good()
        rc, untouched = call(nq=0)
        assert rc == 0 and untouched                                                             # nq = 0 returns ICD_OK and writes nothing
        out = ctypes.c_void_p()
        assert lib.icd_mmr_create(view._h, 4, ctypes.byref(out)) == UNSUPPORTED and not out.value
        assert lib.icd_mmr_create(index._h, 0, ctypes.byref(out)) == INVALID and lib.icd_mmr_create(None, 4, ctypes.byref(out)) == STATE
        assert lib.icd_mmr_stats(dead_mmr_h, None, None) == STATE and lib.icd_mmr_destroy(dead_mmr_h) == STATE
        # the wrapper's own checks raise before the library is asked
        for kw in (dict(k=0), dict(k=9, fetch_k=8), dict(fetch_k=129), dict(lam=1.5), dict(lam=float("nan"))):
            args = dict(k=4, fetch_k=8, lam=0.5)
            args.update(kw)
            with pytest.raises(ValueError):
                index.search_mmr(q, args["k"], args["fetch_k"], args["lam"], mmr=mmr)
        with pytest.raises(_native.IcdError):
            index.search_mmr(q, 4, 8, 0.5, mmr=dead_mmr)
        good()
        for h in (foreign_mask, tiny, narrow_mmr, narrow, view):
            h.close()
    finally:
        case.close()
        other.close()


def test_lifetime_either_may_go_first(oracle):
    case = Case(oracle, "random", 33, 32, 9, nq=2, max_nq=8)
    want = case.want(3, 9, 0.5)[1]
    same(case.index.search_mmr(case.queries, 3, 9, 0.5, mmr=case.mmr), want, "before")
    # the handle before the index
    case.mmr.close()
    assert case.mmr.closed
    second = case.index.mmr(4)
    same(case.index.search_mmr(case.queries, 3, 9, 0.5, mmr=second), want, "a second handle")
    # the index before the handle: the handle stays a handle (stats, close), a search with it is refused
    case.index.close()
    assert second.stats()["max_nq"] == 4
    with pytest.raises(_native.IcdError):
        case.index.search_mmr(case.queries, 3, 9, 0.5, mmr=second)
    # an index re-created over the same rows is another index: the old handle is not its own
    again = _native.IcdIndex(case.corpus, case.levels, device=0, max_nq=8, max_k=128, probe=False)
    try:
        with pytest.raises(_native.IcdError) as e:
            again.search_mmr(case.queries, 3, 9, 0.5, mmr=second)
        assert e.value.code == -1
        second.close()
        mine = again.mmr()
        same(again.search_mmr(case.queries, 3, 9, 0.5, mmr=mine), want, "the new index")
        mine.close()
    finally:
        again.close()
