"""Group scorers of the grouping search (run with -m gpu on an MI355X): IcdIndex.search_grouped with
scorer = sum / avg / max against tests/group_scorer_oracle.py over the oracle's FULL ranking, byte for byte, raw and reweighted,
with every output array - packs and long groups, the edges of a pack, edge scores, the identities of rule 6, the refusals, a
captured graph."""
import ctypes as C

import numpy as np
import pytest

from conftest import icd_levels, unit_rows
from group_scorer_oracle import ScoredRanking, chain_sum, expected, order_sensitive_share
from grouped_oracle import Ranking

pytestmark = pytest.mark.gpu

from rag_project_icd10_amd import _native  # noqa: E402
from rag_project_icd10_amd._native import MODE_EXACT, IcdIndex  # noqa: E402

ID_BASE = 2**32 + 77
ROWS = [1, 63, 64, 65, 127, 128, 129, 257, 1000]
BATCH = {1: 1, 63: 3, 64: 4, 65: 5, 127: 40, 128: 3, 129: 5, 257: 300, 1000: 513}
SIZES = [(10, 3), (128, 1), (64, 2), (25, 5), (8, 16), (7, 17), (2, 64), (1, 128)]


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes()


def _from_runs(runs, n, seed, sorted_labels):
    """group_of for runs of the given lengths in position order: sparse caller ids, the rows of a group scattered over the index;
    sorted_labels keeps the runs in that order in the grouping's (group, row) order, else the ids are unsorted as well"""
    rng = np.random.default_rng(seed)
    labels = rng.choice(20 * len(runs) + 50, len(runs), replace=False)
    if sorted_labels:
        labels = np.sort(labels)
    rows = rng.permutation(n)
    group_of = np.empty(n, np.int64)
    group_of[rows] = np.repeat(labels, runs)
    return group_of


def _random_runs(n, seed, lo=1, hi=70):
    rng = np.random.default_rng(seed)
    runs = []
    while sum(runs) < n:
        runs.append(int(min(rng.integers(lo, hi + 1), n - sum(runs))))
    return runs


def _groupings(n):
    out = {"identity": np.random.default_rng(n).permutation(n) * 3 + 5, "single": np.full(n, 41, np.int64),
           "runs": _from_runs(_random_runs(n, n + 1), n, n + 2, False)}
    if n == 1000:
        out["ends"] = _from_runs([63, 1, 1] + _random_runs(n - 65, 7), n, 8, True)          # runs that end at positions 63, 64 and 65
        out["long"] = _from_runs([1] * 50 + [200] + [1] * 100 + [600] + [1] * 50, n, 9, True)   # wave_select compacts more than once
    return out


_CACHE = {}


def _setup(oracle, n, dim=32):
    key = (n, dim)
    if key not in _CACHE:
        nq = BATCH[n]
        corpus = unit_rows(n, dim, 100 + n)
        q = unit_rows(nq, dim, 200 + n)
        levels = icd_levels(n, 9)
        s_all, i_all = oracle.flat_ip_topk(corpus, q, n, ID_BASE)
        _CACHE[key] = (corpus, levels, q, IcdIndex(corpus, levels, max_nq=nq, max_k=128, id_base=ID_BASE), s_all, i_all)
    return _CACHE[key]


def _check(index, grouping, q, want, k, s, scorer, what):
    want_raw, want_adj, want_grp = want
    nq = len(q)
    got_raw = index.search_grouped(q, k, s, grouping, reweighted=False, scorer=scorer, group_scores=True)
    got_adj = index.search_grouped(q, k, s, grouping, reweighted=True, scorer=scorer, group_scores=True)
    assert len(got_raw) == 6 and len(got_adj) == 7
    for mode, got, exp in (("raw", got_raw, want_raw + want_grp), ("reweighted", got_adj, want_adj + want_grp)):
        for j, (g, w) in enumerate(zip(got, exp)):
            g = g.cpu().numpy() if hasattr(g, "cpu") else g
            w = w[:nq]
            assert g.dtype == w.dtype and g.shape == w.shape, (what, mode, j, g.dtype, w.dtype, g.shape, w.shape)
            assert _bits(g) == _bits(w), (what, mode, j, np.nonzero((g != w).any(1))[0][:5])


@pytest.mark.parametrize("n", ROWS)
def test_sum_and_avg_equal_the_oracle(oracle, n):
    corpus, levels, q, index, s_all, i_all = _setup(oracle, n)
    nq_all = len(q)
    for name, group_of in _groupings(n).items():
        rk = Ranking(s_all, i_all, group_of, id_base=ID_BASE)
        if n == 1000 and name == "runs":
            # the order of the sum is tested: on these scores the worst-first chain differs in bits for a good share of the groups
            share, total = order_sensitive_share(Ranking(s_all[:40], i_all[:40], group_of, id_base=ID_BASE), 5)     # (s = 5 is in SIZES)
            print(f"best-first vs worst-first sums differ for {100 * share:.1f} % of {total} (query, group) pairs with m >= 3 at s = 5")
            assert total > 1000 and share >= 0.25, share
        grouping = index.grouping(group_of)
        before = grouping.stats()["bytes"]
        sizes = SIZES if (n >= 257 and name == "runs") or name == "long" else [(10, 3), (7, 17), (2, 64), (1, 128)]
        if name == "single":
            sizes = [(4, 3), (1, 128), (2, 64)]      # k above the number of groups: padding
        for k, s in sizes:
            for scorer in ("sum", "avg"):
                big = n == 1000 and name == "long" and (k, s) in ((10, 3), (2, 64))     # 513 queries cross the 512-query block
                nq = nq_all if n < 1000 or big else 40
                want = expected(oracle, Ranking(s_all[:nq], i_all[:nq], group_of, id_base=ID_BASE) if nq != nq_all else rk, levels, k, s, scorer,
                                id_base=ID_BASE)
                _check(index, grouping, q[:nq], want, k, s, scorer, (n, name, k, s, scorer))
                if big and (k, s) == (10, 3):
                    for m in (1, 3, 4, 5, 300):
                        _check(index, grouping, q[:m], want, k, s, scorer, (n, name, k, s, scorer, m))
        assert grouping.stats()["bytes"] > before      # the plan and the staging are counted from the first scored call on
        grouping.close()


def test_dim_768_and_device_tensors(oracle):
    import torch
    corpus, levels, q, index, s_all, i_all = _setup(oracle, 257, 768)
    group_of = _groupings(257)["runs"]
    rk = Ranking(s_all[:5], i_all[:5], group_of, id_base=ID_BASE)
    grouping = index.grouping(group_of)
    dq = torch.from_numpy(q[:5]).cuda()
    for k, s in ((10, 3), (5, 17)):
        for scorer in ("sum", "avg"):
            want = expected(oracle, rk, levels, k, s, scorer, id_base=ID_BASE)
            _check(index, grouping, q[:5], want, k, s, scorer, (768, k, s, scorer))
            _check(index, grouping, dq, want, k, s, scorer, (768, "device", k, s, scorer))
    grouping.close()


def test_max_cannot_answer(oracle):
    """130 stray rows, each a group of its own, outscore every row of 20 groups of five whose SUM is far above any stray: the
    sum-ranked best groups have their best rows behind the plain top-128"""
    dim, k, s = 32, 10, 5
    rng = np.random.default_rng(31)
    noise = lambda m: 0.02 * rng.standard_normal((m, dim - 1)).astype(np.float32)   # noqa: E731
    corpus = np.concatenate([np.c_[np.full(130, 0.9, np.float32) + 0.01 * rng.random(130).astype(np.float32), noise(130)],
                             np.c_[np.full(100, 0.5, np.float32) + 0.01 * rng.random(100).astype(np.float32), noise(100)]]).astype(np.float32)
    perm = rng.permutation(230)
    corpus = np.ascontiguousarray(corpus[perm])
    group_of = np.where(perm < 130, 1000 + perm, (perm - 130) // 5)
    q = np.ascontiguousarray(np.c_[np.ones(6, np.float32), 0.1 * rng.standard_normal((6, dim - 1)).astype(np.float32)], dtype=np.float32)
    levels = icd_levels(230, 3)
    s_all, i_all = oracle.flat_ip_topk(corpus, q, 230)
    rk = Ranking(s_all, i_all, group_of)
    sr = ScoredRanking(rk, s, "sum")
    gmax, gsum = ScoredRanking(rk, s, "max").raw(k)[4], sr.raw(k)[4]
    for qi in range(6):     # asserted from the oracle, on the CPU, before any device call
        assert (sr.first[qi][sr.order[qi][:k]] >= 128).any(), qi
        assert gmax[qi].tolist() != gsum[qi].tolist() and (gsum[qi] < 1000).all() and (gmax[qi] >= 1000).all()
    index = IcdIndex(corpus, levels, max_nq=8, max_k=128)
    grouping = index.grouping(group_of)
    for scorer in ("max", "sum", "avg"):
        _check(index, grouping, q, expected(oracle, rk, levels, k, s, scorer), k, s, scorer, ("max cannot answer", scorer))
    grouping.close()
    index.close()


def test_edge_scores(oracle):
    dim = 32
    tiny = np.float32(2.0 ** -126)
    rng = np.random.default_rng(12)
    v = rng.standard_normal(96).astype(np.float32)
    v[0:8] = 3e38                                             # sums overflow to +inf (to -inf under the negated query)
    v[8:16] = [np.inf] + [-np.inf] * 7                        # +inf + -inf: a NaN aggregate drops the group from s = 2 on
    v[16:24] = np.nan                                         # a group whose only rows are NaN
    v[24:32:2] = np.nan                                       # NaN rows among hits
    v[32:40] = [1.5 * tiny, -tiny, -1.25 * tiny, -2 * tiny, -3 * tiny, -4 * tiny, -5 * tiny, -6 * tiny]   # normal scores, subnormal sums
    v[40:48] = -np.inf                                        # an aggregate of -inf is a hit like a best row at -inf
    corpus = np.zeros((96, dim), np.float32)
    corpus[:, 0] = v
    q = np.zeros((3, dim), np.float32)
    q[:, 0] = [1.0, -1.0, 2.0]
    levels = icd_levels(96, 4)
    group_of = np.arange(96) // 8
    s_all, i_all = oracle.flat_ip_topk(corpus, q, 96)
    rk = Ranking(s_all, i_all, group_of)
    sub = ScoredRanking(rk, 2, "sum")
    assert 0 < chain_sum([1.5 * tiny, -tiny]) < tiny and chain_sum([1.5 * tiny, -tiny]) in sub.raw(12)[3][0]     # a subnormal sum is in the test
    assert 1 not in sub.raw(12)[4][0].tolist() and 2 not in sub.raw(12)[4][0].tolist() and np.isposinf(sub.raw(12)[3][0, 0])
    index = IcdIndex(corpus, levels, max_nq=4, max_k=128, probe=False, center=False)
    grouping = index.grouping(group_of)
    for k, s in ((12, 1), (12, 2), (12, 3), (12, 8), (5, 4)):
        for scorer in ("max", "sum", "avg"):
            _check(index, grouping, q, expected(oracle, rk, levels, k, s, scorer), k, s, scorer, ("edge", k, s, scorer))
    grouping.close()
    index.close()
    # all scores tied: groups and members by row id alone
    row = unit_rows(1, dim, 5)
    corpus = np.ascontiguousarray(np.repeat(row, 65, axis=0))
    q = np.ascontiguousarray(np.concatenate([row, unit_rows(2, dim, 6)]))
    group_of = (np.arange(65) * 7) % 13
    s_all, i_all = oracle.flat_ip_topk(corpus, q, 65)
    assert (s_all == s_all[:, :1]).all()
    rk = Ranking(s_all, i_all, group_of)
    index = IcdIndex(corpus, None, max_nq=4, max_k=128)
    grouping = index.grouping(group_of)
    for k, s in ((13, 5), (4, 2), (20, 1)):
        for scorer in ("sum", "avg"):
            _check(index, grouping, q, expected(oracle, rk, np.ones(65, np.int32), k, s, scorer), k, s, scorer, ("tied", k, s, scorer))
    grouping.close()
    index.close()


def test_rule_6_identities_and_a_view(oracle):
    corpus, levels, q, index, s_all, i_all = _setup(oracle, 257)
    q = q[:40]
    groupings = _groupings(257)
    g = index.grouping(groupings["runs"])
    for k, s in ((10, 3), (7, 17), (128, 1)):
        for rw in (False, True):
            plain = index.search_grouped(q, k, s, g, reweighted=rw)
            scored = index.search_grouped(q, k, s, g, reweighted=rw, scorer="max", group_scores=True)
            assert len(scored) == len(plain) + 2
            for a, b in zip(plain, scored):     # MAX through the new entry point is the old one, byte for byte
                assert _bits(a) == _bits(b), (k, s, rw)
            for a, b in zip(plain, index.search_grouped(q, k, s, g, reweighted=rw, scorer="max")):
                assert _bits(a) == _bits(b)
    for k in (1, 10, 128):                      # SUM and AVG at s = 1 are MAX
        base = index.search_grouped(q, k, 1, g, reweighted=True, scorer="max", group_scores=True)
        for scorer in ("sum", "avg"):
            for a, b in zip(base, index.search_grouped(q, k, 1, g, reweighted=True, scorer=scorer, group_scores=True)):
                assert _bits(a) == _bits(b), (k, scorer)
    g.close()
    one = index.grouping(groupings["single"])     # one group of all rows at s = m: search's rows at k = m
    for m in (1, 17, 128):
        ps, pi = index.search(q, m, MODE_EXACT)
        for scorer in ("sum", "avg"):
            raw, ids, _lv, grp = index.search_grouped(q, 1, m, one, reweighted=False, scorer=scorer)
            assert _bits(raw) == _bits(ps) and _bits(ids) == _bits(pi) and (grp == 41).all()
    one.close()
    rows = np.sort(np.random.default_rng(3).choice(257, 130, replace=False)).astype(np.int64)     # a view: the parent's ids and levels
    view = index.view(rows)
    vs, vi = oracle.flat_ip_topk(corpus[rows], q, len(rows))
    group_of = groupings["runs"][rows]
    rk = Ranking(vs, vi, group_of)
    gv = view.grouping(group_of)
    for k, s in ((10, 3), (3, 40)):
        for scorer in ("sum", "avg"):
            _check(view, gv, q, expected(oracle, rk, levels, k, s, scorer, row_map=rows, id_base=ID_BASE), k, s, scorer, ("view", k, s, scorer))
    gv.close()
    view.close()


def test_refusals_leave_the_outputs_untouched(oracle):
    corpus, levels, q, index, _s, _i = _setup(oracle, 257)
    lib = _native.load_library()
    group_of = _groupings(257)["runs"]
    ready, fresh = index.grouping(group_of), index.grouping(group_of)
    ready.prepare_scorers(index)
    ready.prepare_scorers(index)      # idempotent
    assert lib.icd_grouping_prepare_scorers(index._h, ready._h) == 0
    other = IcdIndex(corpus[:64], levels[:64], max_nq=8, max_k=10)
    theirs = other.grouping(np.arange(64) % 5)
    theirs.prepare_scorers(other)
    qq = np.ascontiguousarray(q[:2])

    def call(grouping, k, s, scorer):
        outs = [np.full((2, 128), 7, dt) for dt in (np.float64, np.float32, np.int64, np.int32, np.int32, np.float32, np.int32)]
        rc = lib.icd_index_search_grouped_scored(index._h, grouping._h, qq.ctypes.data, 2, k, s, 0, 1, scorer, *[o.ctypes.data for o in outs], 0, None)
        assert all((o == 7).all() for o in outs), (k, s, scorer)      # no output byte written
        return rc

    for scorer in (3, -1, 1 << 20):
        assert call(ready, 3, 2, scorer) == -1 and b"scorer" in lib.icd_last_error()
    for k, s in ((0, 1), (1, 0), (129, 1), (16, 9), (1, 129)):
        assert call(ready, k, s, 1) == -1
    assert call(theirs, 3, 2, 1) == -1 and b"another index" in lib.icd_last_error()
    state = call(fresh, 3, 2, 1)                                       # never prepared: ICD_ERR_STATE
    assert state not in (0, -1) and b"icd_grouping_prepare_scorers" in lib.icd_last_error()
    assert call(fresh, 3, 2, 2) == state and call(fresh, 3, 2, 0) == state      # (MAX with the group outputs needs the staging too)
    assert lib.icd_grouping_prepare_scorers(other._h, ready._h) == -1
    with pytest.raises(ValueError, match="scorer"):
        index.search_grouped(qq, 3, 2, fresh, scorer="median")
    with pytest.raises(ValueError, match="128"):
        index.search_grouped(qq, 16, 9, fresh, scorer="sum")
    assert call(fresh, 3, 2, 1) == state                               # the refused wrapper calls did not prepare it
    # the unchanged entry point needs no preparation
    assert len(index.search_grouped(qq, 3, 2, fresh)) == 5
    for h in (theirs, other, fresh, ready):
        h.close()
    with pytest.raises(_native.IcdError):
        index.search_grouped(qq, 3, 2, ready, scorer="sum")


def test_graph_capture_of_a_scored_search(oracle):
    import torch
    corpus, levels, q, index, s_all, i_all = _setup(oracle, 1000)
    group_of = _groupings(1000)["long"]
    want = expected(oracle, Ranking(s_all[:40], i_all[:40], group_of, id_base=ID_BASE), levels, 10, 3, "sum", id_base=ID_BASE)
    grouping, late = index.grouping(group_of), index.grouping(group_of)
    dq = torch.from_numpy(q[:40]).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        index.search_grouped(dq, 10, 3, grouping, scorer="sum", group_scores=True)     # warm-up on the capture stream; prepares the grouping
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cap = index.search_grouped(dq, 10, 3, grouping, scorer="sum", group_scores=True)
        with pytest.raises(_native.IcdError) as e:      # prepare allocates: refused while capturing
            late.prepare_scorers(index)
    assert e.value.code == -1
    for _ in range(2):
        for t in cap:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for g, w in zip(cap, want[1] + want[2]):
            assert _bits(g) == _bits(w)
    del graph
    late.close()
    grouping.close()
