"""icd_index_recommend on the device against tests/recommend_oracle.py, byte for byte: raw and reweighted
outputs, count and selected; no tolerance anywhere. The examples' scores by row come from the CPU oracle's canonical chain
(oracle.scores), which recommend_oracle.chain_scores is held against once. Sizes sit at the sweep's 128-row tile (1, 127, 128, 129)
and one past the combine's and the collect's 1 024-row step (1 025); batches at the sweep's 128-query tile (43 requests of 3
examples: 129 vectors)."""
import ctypes

import numpy as np
import pytest

import recommend_oracle as ro
from conftest import icd_levels, unit_rows
from rag_project_icd10_amd import _native

pytestmark = pytest.mark.gpu

BASE = 5_000_000_000
F = np.float32


def same(got, want, what):
    """arrays compared byte for byte"""
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        g = np.asarray(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, j, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, j, g, w)


class Case:
    """one corpus on the device, a recommend workspace, and the oracle with a cache of the canonical scores of every vector asked"""

    def __init__(self, orc, corpus, levels=None, id_base=0, requests=64, examples=None, max_k=2048, max_nq=512):
        self.orc, self.corpus, self.id_base = orc, np.ascontiguousarray(corpus, F), id_base
        self.n, self.dim = corpus.shape
        self.levels = icd_levels(self.n, self.n + 1) if levels is None else np.asarray(levels, np.int32)
        self.index = _native.IcdIndex(self.corpus, self.levels, device=0, max_nq=max_nq, max_k=128, id_base=id_base, probe=False)
        self.ws = _native.IcdRecommend(self.index, requests, examples, max_k)
        self.cache, self.handles = {}, {}

    def scores(self, vector, corpus):
        key = np.asarray(vector, F).tobytes()
        if key not in self.cache:
            self.cache[key] = self.orc.scores(np.asarray(vector, F), corpus)
        return self.cache[key]

    def handle(self, mask):
        if mask is None:
            return None
        if id(mask) not in self.handles:
            self.handles[id(mask)] = (mask, self.index.rowmask(np.nonzero(mask)[0].astype(np.int64)))
        return self.handles[id(mask)][1]

    def want(self, positive, negative, strategy, k, first=0, masks=None, radius=None, range_filter=None):
        return ro.recommend_batch(self.corpus, self.levels, positive, negative, strategy, k, first, masks, radius, range_filter, self.id_base, self.scores)

    def check(self, positive, negative, strategy, k, first=0, masks=None, radius=None, range_filter=None, forms=(False,)):
        """the forms of one call against the oracle; returns the oracle's (raw, adj, count, selected)"""
        want = self.want(positive, negative, strategy, k, first, masks, radius, range_filter)
        hm = None if masks is None else [self.handle(m) for m in masks]
        what = (self.n, self.dim, len(positive), strategy, k, first)
        for rew in forms:
            got = self.ws.recommend(positive, negative, strategy, k, masks=hm, radius=radius, range_filter=range_filter, first=first, reweighted=rew)
            if rew:
                same(got[:4], want[1], what + ("reweighted",))
            else:
                assert got[0] is None
                same(got[1:4], want[0], what + ("raw",))
            same(got[4:], want[2:], what + ("count, selected", rew))
        return want

    def close(self):
        for _m, h in self.handles.values():
            h.close()
        self.ws.close()
        self.index.close()


def family_corpus(n, dim, seed):
    """families of 1 .. 5 bit-identical rows: their members tie, the smaller id first"""
    rng = np.random.default_rng(seed)
    fam = np.repeat(np.arange(n), rng.integers(1, 6, n))[:n]
    return np.ascontiguousarray(unit_rows(n, dim, seed)[fam])


def draw(rng, case, P, N, kind):
    """one request's (positive, negative): stored ids, vectors, or both in turn"""
    out = []
    for j in range(P + N):
        stored = kind == "stored" or (kind == "mixed" and j % 2 == 0)
        out.append(int(rng.integers(0, case.n)) + case.id_base if stored else unit_rows(1, case.dim, int(rng.integers(1 << 30)))[0])
    return out[:P], out[P:]


SHAPES = ((1, 0), (0, 1), (1, 1), (3, 2), (8, 8), (16, 0))


# ---- rows, dims and example shapes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim", [(1, 32), (127, 32), (128, 32), (129, 768), (1025, 32), (1025, 768)])
def test_rows_and_example_shapes(oracle, n, dim):
    case = Case(oracle, family_corpus(n, dim, 100 + n), id_base=BASE if n % 2 else 0)
    rng = np.random.default_rng(n + dim)
    try:
        if n == 129:
            v = unit_rows(1, dim, 1)[0]
            assert ro.chain_scores(v, case.corpus).tobytes() == oracle.scores(v, case.corpus).tobytes()   # the numpy chain is the C oracle's
        for si, strategy in enumerate(ro.STRATEGIES):
            for t, (P, N) in enumerate(SHAPES):
                if P == 0 and strategy == "average_vector":
                    continue
                kind = ("stored", "vector", "mixed")[(t + si) % 3]
                pos, neg = draw(rng, case, P, N, kind)
                k = (1, 10, 128, 300)[t % 4]
                raw, _adj, count, selected = case.check([pos], [neg], strategy, k, forms=(False, True) if t == 3 else (False,))
                assert count[0] == min(k, selected[0]) and (raw[1][0, count[0]:] == -1).all()
                if kind == "vector" and strategy != "sum_scores":
                    assert selected[0] == n                                    # a vector example excludes nothing
    finally:
        case.close()


@pytest.mark.parametrize("nr", [1, 2, 43])
def test_requests_across_the_sweep_tile(oracle, nr):
    """43 requests of 3 examples are 129 vectors: request 42's examples straddle the sweep's 128-query tile"""
    case = Case(oracle, family_corpus(300, 32, 7))
    rng = np.random.default_rng(nr)
    try:
        reqs = [draw(rng, case, 2, 1, "mixed") for _ in range(nr)]
        for strategy in ro.STRATEGIES:
            case.check([r[0] for r in reqs], [r[1] for r in reqs], strategy, 40)
    finally:
        case.close()


def test_more_than_one_block_and_chunks(oracle):
    """one call whose blocks hold fewer requests than the call: 900 requests x (n padded x 4 + 16 384 x 32 bytes) and their example
    runs exceed the 256 MiB budget; and a workspace of 5 requests / 12 examples, which the ctypes layer feeds in chunks"""
    case = Case(oracle, family_corpus(300, 32, 8), requests=900, max_k=16384, max_nq=1024)
    rng = np.random.default_rng(9)
    try:
        st = case.ws.stats()
        assert st["bytes"] < (320 << 20) and st["max_requests"] == 900 and st["max_examples"] == 900 * 16
        reqs = [draw(rng, case, 1 + r % 3, r % 2, "mixed") for r in range(900)]
        m = np.random.default_rng(10).random(300) < 0.5
        masks = [m if r % 3 == 0 else None for r in range(900)]
        lo = np.where(np.arange(900) % 2 == 0, -0.5, -0.1).astype(F)
        for strategy in ("best_score", "average_vector"):
            case.check([r[0] for r in reqs], [r[1] for r in reqs], strategy, 12, first=3, masks=masks, radius=lo)
    finally:
        case.close()
    case = Case(oracle, family_corpus(200, 32, 11), requests=5, examples=12)
    try:
        reqs = [draw(rng, case, 2, 1 + r % 2, "stored") for r in range(13)]
        case.check([r[0] for r in reqs], [r[1] for r in reqs], "sum_scores", 20)
    finally:
        case.close()


# ---- ties and branches -----------------------------------------------------------------------------------------------------------
def axis_corpus(values, dim=32):
    """rows whose score against e0 is exactly values[i] (and against c * e0 exactly c * values[i] for powers of two)"""
    x = np.zeros((len(values), dim), F)
    x[:, 0] = np.asarray(values, F)
    return x


def test_ties_and_branches(oracle):
    e0 = np.zeros(32, F)
    e0[0] = 1.0
    vals = np.array([0.5, 0.25, 0.0, -0.0, -0.5, 0.25, 1.0, 0.0] * 40, F)           # 320 rows, runs of equal scores
    case = Case(oracle, axis_corpus(vals))
    try:
        # bp == bn on every row (the same vector on both sides): the negative branch, -(s * s); -0.0 from -(0 * 0) on the zero rows
        raw = case.check([[e0]], [[e0]], "best_score", 320)[0]
        assert (raw[0][0] <= 0).all() and np.signbit(raw[0][0][raw[0][0] == 0]).all() and (raw[0][0] == 0).sum() == 120
        # a row that is both a positive and a negative example: excluded, and every other row takes the negative branch
        raw, _a, _c, selected = case.check([[6]], [[6]], "best_score", 320)
        assert selected[0] == 319 and 6 not in raw[1][0]
        # duplicates of an example row still rank: rows 14, 22, .. carry row 6's bits
        raw, _a, _c, selected = case.check([[6]], [[]], "best_score", 10)
        assert selected[0] == 319 and raw[1][0][:3].tolist() == [14, 22, 30] and (raw[0][0][:3] == 1.0).all()
        # all scores tied: the rows in order, past the example
        tied = Case(oracle, axis_corpus(np.full(200, 0.25, F)))
        try:
            for strategy in ro.STRATEGIES:
                raw = tied.check([[3]], [[]] if strategy != "sum_scores" else [[e0]], strategy, 150, first=2)[0]
                assert raw[1][0].tolist() == [r for r in range(200) if r != 3][2:152]
        finally:
            tied.close()
        # sum_scores: list order decides in float32 - 2^24 + 1 + 1 - 2^24 = 0, 1 + 1 + 2^24 - 2^24 = 2
        big, one = e0 * F(2.0 ** 24), e0.copy()
        ones = Case(oracle, axis_corpus(np.ones(130, F)))
        try:
            raw = ones.check([[big, one, one], [one, one, big]], [[big], [big]], "sum_scores", 5)[0]
            assert (raw[0][0] == 0.0).all() and (raw[0][1] == 2.0).all()
        finally:
            ones.close()
        # best_score's fold by plain compares: +0.0 does not replace -0.0 (rows 2, 3, 7 against e0 and -e0)
        case.check([[-e0, e0]], [[]], "best_score", 320)
        case.check([[e0, -e0]], [[-e0 * F(0.5)]], "best_score", 320)
    finally:
        case.close()


# ---- exclusion, masks, bands, first, k ---------------------------------------------------------------------------------------------
def test_exclusion_masks_bands_first_and_k(oracle):
    n = 1025
    case = Case(oracle, family_corpus(n, 32, 61), id_base=BASE)
    rng = np.random.default_rng(63)
    try:
        # examples at the edges of a lane's four rows, of a wave, of the 1 024-row segment and of the index
        pos = [BASE + r for r in (0, 3, 4, 255, 256, 1023, 1024)]
        neg = [BASE + r for r in (1, 1022)]
        for strategy in ro.STRATEGIES:
            raw, _a, _c, selected = case.check([pos], [neg], strategy, 300)
            assert selected[0] <= n - 9 and not (set(raw[1][0].tolist()) & set(pos + neg))
        tail = np.zeros(n, bool)
        tail[1024] = True                                                          # only the last row, alone in its tile and segment
        some = rng.random(n) < 0.5
        none = np.zeros(n, bool)
        reqs = [draw(rng, case, 2, 2, "mixed") for _ in range(5)]
        masks = [tail, some, None, none, some]
        P, N = [r[0] for r in reqs], [r[1] for r in reqs]
        _raw, _a, count, selected = case.check(P, N, "best_score", 128, masks=masks, forms=(False, True))
        assert selected[3] == 0 and count[3] == 0 and selected[0] <= 1
        # bands at scores that occur: radius strict, range_filter inclusive; one scalar; with masks and first
        full = case.want(P, N, "sum_scores", 1024)[0][0]
        lo, hi = full[:, 700].copy(), full[:, 20].copy()
        raw = case.check(P, N, "sum_scores", 1024, radius=lo, range_filter=hi)[0]
        for r in range(5):
            real = raw[0][r][raw[1][r] >= 0]
            assert real[0].tobytes() == hi[r].tobytes() and real[-1] > lo[r]
        case.check(P, N, "average_vector", 10, radius=0.0)
        case.check(P, N, "best_score", 60, first=100, masks=masks, radius=lo, range_filter=hi, forms=(False, True))
        # k of 1, 10, 128, 300; k above the rows that rank: padding; first past the last ranking row
        for k in (1, 10, 128, 300):
            case.check(P, N, "best_score", k)
        raw, _a, count, selected = case.check(P, N, "sum_scores", 2048)
        assert (count == selected).all() and (count >= n - 4).all() and (raw[1][:, n:] == -1).all()
        _raw, _a, count, _s = case.check(P, N, "best_score", 5, first=1025)
        assert (count == 0).all()
        whole = case.ws.recommend(P, N, "best_score", 400, reweighted=False)
        part = case.ws.recommend(P, N, "best_score", 100, first=300, reweighted=False)
        same(part[1:4], [np.ascontiguousarray(w[:, 300:]) for w in whole[1:4]], "the slice of first = 0")
    finally:
        case.close()


# ---- special values ----------------------------------------------------------------------------------------------------------------
def test_special_values(oracle):
    n = 300
    x = family_corpus(n, 32, 51)
    x[10:20] = 0.0
    x[20:30, 3] = np.nan                             # NaN rows: in no list, under any example
    x[30:35, 0], x[30:35, 1:] = np.inf, 0.0          # +-inf scores (the sign of the example's first component decides)
    x[35:40, 0], x[35:40, 1:] = -np.inf, 0.0
    x[40:50] = -0.0
    case = Case(oracle, x)
    try:
        a, b, c = unit_rows(3, 32, 52)
        a[0], b[0] = abs(a[0]), -abs(b[0])
        z = c.copy()
        z[0] = 0.0                                   # inf x 0: NaN on rows 30 .. 39 for this example ONLY
        for strategy in ro.STRATEGIES:
            _raw, _a, _c, selected = case.check([[a, 5]], [[b]], strategy, 300)
            assert selected[0] <= n - 11             # (sum_scores: inf - (-inf) ranks, inf - inf does not)
            _raw, _a, _c, sel_z = case.check([[a, z]], [[b]], strategy, 300)
            if strategy != "average_vector":
                assert sel_z[0] <= n - 20            # NaN in one example only takes the row out
        case.check([[a]], [[a]], "sum_scores", 300)                            # inf - inf = NaN on rows 30 .. 39: c is NaN
        case.check([[30, a]], [[35]], "best_score", 300, radius=-np.inf)        # an explicit radius of -inf leaves c = -inf out
        case.check([[a]], [[]], "best_score", 300, forms=(False, True))         # without a radius c = -inf ranks, as in the wide search
    finally:
        case.close()


# ---- the average_vector target ------------------------------------------------------------------------------------------------------
def test_the_target_vector_is_numpys(oracle):
    n, dim = 200, 768
    x = family_corpus(n, dim, 71)
    x[:20] *= F(3.0e5)                               # sums that round, quotients that are not exact
    x[20:30] *= F(1.0e-10)
    case = Case(oracle, x, id_base=BASE)
    rng = np.random.default_rng(72)
    try:
        reqs = [draw(rng, case, P, N, kind) for P, N, kind in ((1, 0, "stored"), (3, 0, "mixed"), (3, 2, "mixed"), (7, 9, "stored"), (16, 0, "vector"), (5, 1, "vector"))]
        reqs.append(([BASE + 3, BASE + 25, BASE + 7], [BASE + 22, BASE + 1]))
        P, N = [r[0] for r in reqs], [r[1] for r in reqs]
        case.check(P, N, "average_vector", 50)
        want = np.stack([ro.target_vector(p, q, x, BASE) for p, q in reqs])
        got = case.ws.last_vectors(len(reqs))
        assert got.dtype == F and got.tobytes() == want.tobytes()
        case.check(P, N, "best_score", 5)            # ... and the example block itself: copies of rows and vectors, in order
        flat = [e for p, q in reqs for e in list(p) + list(q)]
        got = case.ws.last_vectors(len(flat))
        assert got.tobytes() == np.stack([ro.example_vector(e, x, BASE) for e in flat]).tobytes()
    finally:
        case.close()


# ---- equivalences with the wide search -----------------------------------------------------------------------------------------------
def test_equivalences_with_the_wide_search(oracle):
    n = 1025
    case = Case(oracle, family_corpus(n, 32, 81), id_base=7)
    wide = _native.IcdWide(case.index, 8, 2048)
    rng = np.random.default_rng(82)
    try:
        reqs = [draw(rng, case, 3, 2, "mixed") for _ in range(4)]
        targets = np.stack([ro.target_vector(p, q, case.corpus, 7) for p, q in reqs])
        masks = []
        for p, q in reqs:                            # the wide search of the oracle's target, the stored examples masked out
            m = np.ones(n, bool)
            m[ro.example_rows(p + q, 7)] = False
            masks.append(case.handle(m))
        for rew in (False, True):
            got = case.ws.recommend([r[0] for r in reqs], [r[1] for r in reqs], "average_vector", 300, first=5, reweighted=rew)
            same(got[0 if rew else 1:], wide.search_wide(targets, 300, masks=masks, first=5, reweighted=rew)[0 if rew else 1:], ("average_vector", rew))
        rows = [0, 511, 1024, 600]
        masks = []
        for r in rows:
            m = np.ones(n, bool)
            m[r] = False
            masks.append(case.handle(m))
        got = case.ws.recommend([[7 + r] for r in rows], None, "best_score", 1030)
        same(got, wide.search_wide(case.corpus[rows], 1030, masks=masks), "one stored positive under best_score")
    finally:
        wide.close()
        case.close()


# ---- must fail without the feature: no list of an existing search holds the answer -------------------------------------------------
def test_not_reachable_from_lists(oracle):
    """the best_score winner lies behind rank 128 (ICD_MAX_K, the longest list of every other search) of every single example's
    list: no re-ranking of existing lists can find it. Examples a = e0 and b = e1 as positives, g = e0 + e1 as the negative; 200
    rows near a and 200 near b score high on one positive but higher still on g - the negative branch; the winner scores a modest
    0.5 on a, a little on b and NEGATIVE on g... which no row of the plane spanned by a and b can, so it leans on e2 and g on -e2."""
    dim, n = 32, 500
    x = np.zeros((n, dim), F)
    x[:200, 0], x[:200, 1] = np.linspace(0.9, 0.99, 200, dtype=F), F(0.3)                   # near a: s_a ~ 0.9, s_g ~ 1.2
    x[200:400, 1], x[200:400, 0] = np.linspace(0.9, 0.99, 200, dtype=F), F(0.3)             # near b
    x[400:, 0], x[400:, 1], x[400:, 2] = F(-0.5), F(-0.5), np.linspace(0.0, 0.1, 100, dtype=F)   # filler: far from everything
    w = 450
    x[w, :3] = (0.5, 0.125, 0.75)                                                           # the winner
    a, b, g = np.zeros(dim, F), np.zeros(dim, F), np.zeros(dim, F)
    a[0], b[1] = 1.0, 1.0
    g[0], g[1], g[2] = 1.0, 1.0, -1.0
    case = Case(oracle, x)
    try:
        raw, _adj, _count, selected = case.check([[a, b]], [[g]], "best_score", 10)
        assert raw[1][0][0] == w and raw[0][0][0] == 0.5 and selected[0] == n
        assert (raw[0][0][1:] < 0).all()                                                    # the rows near a or b: -(bn * bn); the filler: bp = -0.5
        for v in (a, b, g):                                                             # behind rank 128 of every example's own list
            s = oracle.scores(v, x)
            assert int((s > s[w]).sum()) >= 128, v[:3]
            top = case.index.search_range(v[None, :], 128, reweighted=False)[1][0]
            assert w not in top.tolist()
    finally:
        case.close()


# ---- determinism, device tensors ------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes_and_device_tensors(oracle):
    import torch
    n = 1025
    case = Case(oracle, family_corpus(n, 32, 95))
    rng = np.random.default_rng(96)
    try:
        reqs = [draw(rng, case, 3, 2, "mixed") for _ in range(43)]
        P, N = [r[0] for r in reqs], [r[1] for r in reqs]
        m = np.random.default_rng(97).random(n) < 0.7
        hm = [case.handle(m)] * 43
        for strategy in ro.STRATEGIES:
            first_run = case.ws.recommend(P, N, strategy, 300, masks=hm, radius=-0.2)
            for _ in range(2):
                same(case.ws.recommend(P, N, strategy, 300, masks=hm, radius=-0.2), first_run, "second run")
            dev = lambda side: [[torch.from_numpy(e).cuda() if isinstance(e, np.ndarray) else e for e in ex] for ex in side]   # noqa: E731
            got = case.ws.recommend(dev(P), dev(N), strategy, 300, masks=hm, radius=torch.full((43,), -0.2, device="cuda"))
            assert all(t.is_cuda for t in got)
            same([t.cpu().numpy() for t in got], first_run, "device tensors")
        raw = case.ws.recommend(dev(P), dev(N), "best_score", 40, reweighted=False)
        assert raw[0] is None
        same([t.cpu().numpy() for t in raw[1:4]], case.want(P, N, "best_score", 40)[0], "device raw")
    finally:
        case.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(oracle):
    import torch
    lib = _native.load_library()
    case = Case(oracle, family_corpus(300, 32, 98), requests=4, examples=10, max_k=1000, max_nq=64)
    other = _native.IcdIndex(case.corpus, case.levels, device=0, max_nq=64, max_k=128, probe=False)
    view = case.index.view(np.arange(0, 300, 2, dtype=np.int64))
    try:
        k_out = 1000
        outs = [np.full((4, k_out), 7, dt) for dt in (np.float64, np.float32, np.int64, np.int32)] + [np.full(4, 7, np.int32), np.full(4, 7, np.int64)]
        p = [o.ctypes.data for o in outs]
        vec = unit_rows(10, 32, 99)
        i64 = lambda *v: np.array(v, np.int64)   # noqa: E731
        i32 = lambda *v: np.array(v, np.int32)   # noqa: E731

        def call(index=case.index, ws=case.ws, rows=i64(5, -1, 7), off=i64(0, 2, 3), npos=i32(1, 1), nr=2, vectors=vec, strategy=1, k=10, first=0, rew=1,
                 out=p, lo=None, hi=None, stream=None):
            ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
            return lib.icd_index_recommend(index._h, ws._h, None, ptr(rows), ptr(vectors), ptr(off), ptr(npos), nr, strategy, k, first, ptr(lo), ptr(hi), 0, rew,
                                           *out, 0, 0, stream)

        assert call() == 0
        untouched = [o.copy() for o in outs]
        for kw in (dict(strategy=3), dict(strategy=-1), dict(k=0), dict(k=16385), dict(first=-1), dict(first=16000, k=385), dict(k=1001), dict(first=1, k=1000),
                   dict(nr=-1), dict(nr=5, off=i64(0, 1, 2, 3, 4, 5), npos=i32(1, 1, 1, 1, 1), rows=i64(1, 2, 3, 4, 5)),
                   dict(index=other), dict(out=[None] + p[1:]), dict(out=p[:1] + [None] + p[2:]), dict(out=p[:4] + [None, p[5]]), dict(out=p[:5] + [None]),
                   dict(rows=None), dict(off=None), dict(npos=None), dict(off=i64(1, 2, 3)),
                   dict(off=i64(0, 0, 3)),                                          # a request without examples
                   dict(off=i64(0, 17, 18), rows=i64(*range(18))),                  # 17 examples
                   dict(off=i64(0, 6, 11), rows=i64(*range(11))),                   # 11 examples in a workspace of 10
                   dict(npos=i32(3, 1)), dict(npos=i32(-1, 1)),
                   dict(strategy=0, npos=i32(0, 1)),                                # average_vector without a positive
                   dict(rows=i64(300, -1, 7)), dict(rows=i64(-2, -1, 7)),
                   dict(vectors=None),                                              # a vector example without example_vectors
                   dict(lo=np.array([0.5, np.nan], F)), dict(lo=np.array([0.5, 0.5], F), hi=np.array([0.6, 0.5], F))):
            assert call(**kw) == -1, kw
        assert call(index=view) == -4                                       # a view: ICD_ERR_UNSUPPORTED
        for o, u in zip(outs, untouched):                                   # a refused call writes no output
            assert o.tobytes() == u.tobytes()
        assert call(rew=0, out=[None] + p[1:]) == 0                       # out_adj may be NULL in the raw form
        assert call(rows=i64(5, 6, 7), vectors=None) == 0                 # no vector example: example_vectors may be NULL
        assert call(nr=0, rows=None, off=None, npos=None, vectors=None) == 0
        # while capturing: the request table is staged on the host at call time
        side, buf = torch.cuda.Stream(), torch.zeros(8, device="cuda")
        with torch.cuda.stream(side):
            buf.add_(1)                                                     # warm-up on the capture stream
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            buf.add_(1)
            rc = call(stream=side.cuda_stream)
        assert rc == -1
        del graph
        h = ctypes.c_void_p()
        assert lib.icd_recommend_create(view._h, 4, 16, 100, ctypes.byref(h)) == -4 and not h.value
        for bad in ((0, 16, 100), (4, 3, 100), (4, 65, 100), (4, 16, 0), (4, 16, 16385)):
            assert lib.icd_recommend_create(case.index._h, *bad, ctypes.byref(h)) == -1 and not h.value, bad
        gone = _native.IcdRecommend(case.index, 4, 10, 100)
        stale = ctypes.c_void_p(gone._h.value)
        gone.close()
        assert lib.icd_index_recommend(case.index._h, stale, None, i64(5).ctypes.data, None, i64(0, 1).ctypes.data, i32(1).ctypes.data, 1, 1, 10, 0, None, None, 0, 1,
                                       *p, 0, 0, None) == -5
        assert lib.icd_recommend_destroy(stale) == -5 and lib.icd_recommend_read_vectors(case.ws._h, 99, outs[1].ctypes.data) == -1
        # the ctypes layer's own checks
        v = vec[0]
        for bad in (dict(positive=[[1]], negative=[[]], strategy="nearest", k=5), dict(positive=[[1]], negative=[[]], strategy="best_score", k=0),
                    dict(positive=[[1]], negative=[[]], strategy="best_score", k=385, first=16000), dict(positive=[[]], negative=[[]], strategy="best_score", k=5),
                    dict(positive=[[1] * 17], negative=[[]], strategy="best_score", k=5), dict(positive=[[]], negative=[[1]], strategy="average_vector", k=5),
                    dict(positive=[[300]], negative=[[]], strategy="best_score", k=5), dict(positive=[[-1]], negative=[[]], strategy="best_score", k=5),
                    dict(positive=[[v[:31]]], negative=[[]], strategy="best_score", k=5), dict(positive=[[1], [2]], negative=[[]], strategy="best_score", k=5),
                    dict(positive=[[v, torch.from_numpy(v).cuda()]], negative=[[]], strategy="best_score", k=5)):
            with pytest.raises(ValueError):
                case.ws.recommend(**bad)
        with pytest.raises(_native.IcdError):
            case.ws.recommend([[1]], None, "best_score", 10, radius=0.5, range_filter=0.25)     # an inverted host band
        with pytest.raises(_native.IcdError):
            case.ws.recommend([[1] * 11], None, "best_score", 10)                                # more examples than the workspace takes
        assert case.ws.stats()["max_requests"] == 4 and case.ws.stats()["max_examples"] == 10 and case.ws.stats()["max_k"] == 1000
    finally:
        view.close()
        other.close()
        case.close()
