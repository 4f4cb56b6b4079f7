"""Embedding-list search on the device (run with -m gpu on an MI355X): IcdIndex.search_lists against
tests/maxsim_oracle.py over the oracle's FULL ranking, byte for byte, with every output array - lists of 1 .. 64 vectors mixed in
one batch, passes that are filled exactly and lists that would straddle a pass, both scorers, host and device pointers, NULL
outputs, a view with an id_base, edge scores, the identities of rule 6, the refusals of rule 7, a captured graph."""
import numpy as np
import pytest

from conftest import icd_levels, unit_rows
from grouped_oracle import Ranking
from maxsim_oracle import ListRanking, expected, order_sensitive_share
from test_group_scorer_gpu import _groupings

pytestmark = pytest.mark.gpu

from rag_project_icd10_amd import _native  # noqa: E402
from rag_project_icd10_amd._native import IcdIndex  # noqa: E402

ID_BASE = 2**32 + 77
ROWS = [1, 63, 64, 65, 129, 257, 1000]
MIXED = [1, 2, 3, 5, 17, 63, 64]                 # 155 vectors: behind 91 of them the list of 64 would straddle a block of 128
# n = 1000 (a block of 512 vectors): a pass filled exactly | the mixed lists and five of 64, 475 | a list of 40 that would straddle
BIG = [64] * 8 + MIXED + [64] * 5 + [40]
KS = (1, 10, 64, 128)


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes()


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


_CACHE = {}


def _setup(oracle, n):
    if n not in _CACHE:
        sizes = BIG if n == 1000 else MIXED
        nv = int(np.sum(sizes))
        corpus, q, levels = unit_rows(n, 32, 300 + n), unit_rows(nv, 32, 400 + n), icd_levels(n, 9)
        q[sum(sizes[:4]) + 3] = q[sum(sizes[:4])]              # a vector repeated within a list
        s_all, i_all = oracle.flat_ip_topk(corpus, q, n, ID_BASE)
        # the index's max_nq sets the grouping's score block: 128 vectors below n = 1000, 512 there
        _CACHE[n] = (corpus, levels, q, _off(sizes), IcdIndex(corpus, levels, max_nq=600 if n == 1000 else 100, max_k=128, id_base=ID_BASE), s_all, i_all)
    return _CACHE[n]


def _compare(got, want, what):
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.dtype == w.dtype and g.shape == w.shape, (what, j, g.dtype, w.dtype, g.shape, w.shape)
        assert _bits(g) == _bits(w), (what, j, np.nonzero((g != w).any(1))[0][:5])


@pytest.mark.parametrize("n", ROWS)
def test_search_lists_equals_the_oracle(oracle, n):
    import torch
    corpus, levels, q, off, index, s_all, i_all = _setup(oracle, n)
    dq = torch.from_numpy(q).cuda()
    for name, group_of in _groupings(n).items():
        rk = Ranking(s_all, i_all, group_of, id_base=ID_BASE)
        if n == 1000 and name == "runs":
            # the order of the chain is tested: on the lists of three vectors and more the last-first chain differs in bits
            share, total = order_sensitive_share(rk, off, 10)
            print(f"list-order vs reverse-order aggregates differ for {100 * share:.1f} % of {total} winning (list, group) cells at T >= 3")
            assert total >= 150 and share >= 0.10, share
        grouping = index.grouping(group_of)
        before = grouping.stats()["bytes"]
        grouping.prepare_maxsim(index, 64, 1100)             # the whole batch in ONE call: its passes are the library's
        assert grouping.stats()["bytes"] > before
        for scorer in ("sum", "mean"):
            for k in KS if (name in ("runs", "long") or n < 1000) else (10, 128):
                want = expected(rk, off, levels, k, scorer, id_base=ID_BASE)
                _compare(index.search_lists(q, off, k, grouping, scorer=scorer), want, (n, name, scorer, k, "host"))
                if k in (10, 128):
                    _compare(index.search_lists(dq, off, k, grouping, scorer=scorer), want, (n, name, scorer, k, "device"))
                    _compare(index.search_lists(q, off, k, grouping, scorer=scorer, matches=False), want[:2], (n, name, scorer, k, "no matches"))
        # one list; the lists of the first pass alone; single vectors
        for lo, hi in ((0, 1), (6, 7), (0, 6), (2, 5)):
            v0, v1 = int(off[lo]), int(off[hi])
            sub = Ranking(s_all[v0:v1], i_all[v0:v1], group_of, id_base=ID_BASE)
            _compare(index.search_lists(q[v0:v1], off[lo:hi + 1] - v0, 10, grouping), expected(sub, off[lo:hi + 1] - v0, levels, 10, id_base=ID_BASE),
                     (n, name, "lists", lo, hi))
        grouping.close()


def test_a_batch_above_the_preparation_is_split_between_lists(oracle):
    corpus, levels, q, off, index, s_all, i_all = _setup(oracle, 257)
    group_of = _groupings(257)["runs"]
    grouping = index.grouping(group_of)                       # prepared by the first call for (100, 100): 155 vectors take two calls
    want = expected(Ranking(s_all, i_all, group_of, id_base=ID_BASE), off, levels, 10, id_base=ID_BASE)
    _compare(index.search_lists(q, off, 10, grouping), want, "split")
    assert grouping.maxsim == (100, 100)
    grouping.close()


def test_every_nullable_output_may_be_null(oracle):
    corpus, levels, q, off, index, s_all, i_all = _setup(oracle, 129)
    lib = _native.load_library()
    group_of = _groupings(129)["runs"]
    grouping = index.grouping(group_of)
    grouping.prepare_maxsim(index, 16, 200)
    want = expected(Ranking(s_all, i_all, group_of, id_base=ID_BASE), off, levels, 10, "sum", id_base=ID_BASE)
    nl, nv = len(off) - 1, len(q)
    for skip in (None, 2, 3, 4):
        outs = [np.full((nl, 10), 7, np.float32), np.full((nl, 10), 7, np.int32), np.full((nv, 10), 7, np.float32), np.full((nv, 10), 7, np.int64),
                np.full((nv, 10), 7, np.int32)]
        ptrs = [None if j == skip else o.ctypes.data for j, o in enumerate(outs)]
        assert lib.icd_index_search_maxsim(index._h, grouping._h, q.ctypes.data, off.ctypes.data, nl, 10, 1, 0, *ptrs, 0, None) == 0
        for j, (o, w) in enumerate(zip(outs, want)):
            assert (o == 7).all() if j == skip else _bits(o) == _bits(w), (skip, j)
    grouping.close()


def test_edge_scores(oracle):
    dim = 32
    v = np.array([1.0, 2.0, np.nan, 0.5,          # group 0: a NaN row among hits
                  np.nan, np.nan,                 # group 1: only NaN rows: no hit for every vector
                  np.inf, np.inf,                 # group 2: +inf under a positive vector, -inf under a negative one: [+, -] cancels to NaN
                  -np.inf, -np.inf,               # group 3: the same, mirrored; under [+, +] an aggregate of -inf is a hit
                  3e38, 1.0,                      # group 4: the sum overflows to +inf
                  0.25, 0.25, 0.25, 0.25],        # groups 5 and 6: duplicated rows, the aggregates tie and the row decides
                 np.float32)
    n = len(v)
    corpus = np.zeros((n, dim), np.float32)
    corpus[:, 0] = v
    group_of = np.array([0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 6, 5, 6, 5]) * 3 + 1
    q = np.zeros((9, dim), np.float32)
    q[:, 0] = [1.0, -1.0, 1.0, 1.0, 2.0, -1.0, -1.0, 0.5, 0.5]
    off = _off([2, 3, 2, 2])                                  # [+, -] | [+, +, ++] | [-, -] | [v, v]
    levels = icd_levels(n, 4)
    s_all, i_all = oracle.flat_ip_topk(corpus, q, n)
    rk = Ranking(s_all, i_all, group_of)
    lr = ListRanking(rk, off)
    gsc, gid, msc, mid = lr.outputs(8)
    # asserted on the oracle, before any device call: the NaN group never shows, the cancelled groups drop out of list 0 only
    assert 4 not in gid and 7 not in gid[0] and 10 not in gid[0] and 7 in gid[1] and 10 in gid[1] and 7 in gid[2]
    assert np.isposinf(gsc[1, :2]).all() and gid[1, :2].tolist() == [7, 13] and np.isneginf(gsc[1][gid[1] == 10]).all()
    assert (gid >= 0).sum(1).tolist() == [4, 6, 6, 6]
    p16, p19 = list(gid[3]).index(16), list(gid[3]).index(19)
    assert gsc[3][p16] == gsc[3][p19] and p19 + 1 == p16             # the aggregates tie: group 19 holds the lower row and goes first
    index = IcdIndex(corpus, levels, max_nq=16, max_k=128, probe=False, center=False)
    grouping = index.grouping(group_of)
    for scorer in ("sum", "mean"):
        for k in (1, 5, 6, 8, 128):
            _compare(index.search_lists(q, off, k, grouping, scorer=scorer), expected(rk, off, levels, k, scorer), ("edge", scorer, k))
    grouping.close()
    index.close()


def test_rule_6_identities_and_a_view(oracle):
    import torch
    corpus, levels, q, off, index, s_all, i_all = _setup(oracle, 257)
    groupings = _groupings(257)
    g = index.grouping(groupings["runs"])
    qs = q[:40]
    singles = np.arange(41, dtype=np.int64)
    for k in (1, 10, 128):
        # lists of one vector each: icd_index_search_grouped_scored(scorer MAX, group_size 1), byte for byte
        raw, ids, lv, _grp, wsc, wid = index.search_grouped(qs, k, 1, g, reweighted=False, scorer="max", group_scores=True)
        gsc, gid, msc, mid, mlv = index.search_lists(qs, singles, k, g)
        assert _bits(gsc) == _bits(wsc) and _bits(gid) == _bits(wid)
        assert _bits(msc) == _bits(raw) and _bits(mid) == _bits(ids) and _bits(mlv) == _bits(lv)
        # MEAN at T = 1 is SUM
        for a, b in zip(index.search_lists(qs, singles, k, g, scorer="mean"), (gsc, gid, msc, mid, mlv)):
            assert _bits(a) == _bits(b)
        # [v, v]: the groups of [v] with aggregates x + x; both vectors' matches are those of [v]
        dsc, did, dms, dmi, dml = index.search_lists(np.repeat(qs, 2, axis=0), singles * 2, k, g)
        assert _bits(did) == _bits(gid) and _bits(dsc) == _bits((gsc + gsc).astype(np.float32))
        assert _bits(dms) == _bits(np.repeat(msc, 2, axis=0)) and _bits(dmi) == _bits(np.repeat(mid, 2, axis=0)) and _bits(dml) == _bits(np.repeat(mlv, 2, axis=0))
    g.close()
    # a view: the parent's ids (id_base = 2^32 + 77) and levels
    rows = np.sort(np.random.default_rng(3).choice(257, 130, replace=False)).astype(np.int64)
    view = index.view(rows)
    vs, vi = oracle.flat_ip_topk(corpus[rows], q, len(rows))
    group_of = groupings["runs"][rows]
    rk = Ranking(vs, vi, group_of)
    gv = view.grouping(group_of)
    for k, scorer in ((10, "sum"), (128, "mean")):
        want = expected(rk, off, levels, k, scorer, row_map=rows, id_base=ID_BASE)
        assert (want[3][want[3] >= 0] >= ID_BASE).all()
        _compare(view.search_lists(q, off, k, gv, scorer=scorer), want, ("view", k, scorer))
        _compare(view.search_lists(torch.from_numpy(q).cuda(), off, k, gv, scorer=scorer), want, ("view", "device", k, scorer))
    gv.close()
    view.close()


def test_refusals_leave_the_outputs_untouched(oracle):
    corpus, levels, q, off, index, _s, _i = _setup(oracle, 257)
    lib = _native.load_library()
    group_of = _groupings(257)["runs"]
    ready, fresh = index.grouping(group_of), index.grouping(group_of)
    ready.prepare_maxsim(index, 4, 70)
    assert lib.icd_grouping_prepare_maxsim(index._h, ready._h, 4, 70) == 0 and lib.icd_grouping_prepare_maxsim(index._h, ready._h, 2, 64) == 0   # idempotent
    bytes_ready = ready.stats()["bytes"]
    assert lib.icd_grouping_prepare_maxsim(index._h, ready._h, 5, 70) == -1 and lib.icd_grouping_prepare_maxsim(index._h, ready._h, 4, 71) == -1
    assert lib.icd_grouping_prepare_maxsim(index._h, fresh._h, 0, 10) == -1 and lib.icd_grouping_prepare_maxsim(index._h, fresh._h, 5, 4) == -1
    assert ready.stats()["bytes"] == bytes_ready
    other = IcdIndex(corpus[:64], levels[:64], max_nq=8, max_k=10)
    theirs = other.grouping(np.arange(64) % 5)
    theirs.prepare_maxsim(other, 8, 64)
    assert lib.icd_grouping_prepare_maxsim(other._h, ready._h, 4, 70) == -1
    qq = np.ascontiguousarray(q[:80])

    def call(grouping, list_off, k, scorer, nl=None, null=()):
        list_off = np.asarray(list_off, np.int64)
        outs = [np.full((8, 128), 7, np.float32), np.full((8, 128), 7, np.int32), np.full((80, 128), 7, np.float32), np.full((80, 128), 7, np.int64),
                np.full((80, 128), 7, np.int32)]
        ptrs = [None if j in null else o.ctypes.data for j, o in enumerate(outs)]
        rc = lib.icd_index_search_maxsim(index._h, grouping._h, qq.ctypes.data, list_off.ctypes.data, len(list_off) - 1 if nl is None else nl, k, scorer,
                                         0, *ptrs, 0, None)
        assert all((o == 7).all() for o in outs), (list_off, k, scorer)      # no output byte written
        return rc

    good = [0, 3, 10]
    for scorer in (0, 3, -1, 1 << 20):
        assert call(ready, good, 3, scorer) == -1 and b"scorer" in lib.icd_last_error()
    for k in (0, -1, 129):
        assert call(ready, good, k, 1) == -1
    assert call(ready, [0, 65], 3, 1) == -1                            # T = 65
    assert call(ready, [0, 3, 3, 5], 3, 1) == -1                       # T = 0
    assert call(ready, [0, 5, 3], 3, 1) == -1                          # decreasing
    assert call(ready, [1, 5], 3, 1) == -1                             # not from 0
    assert call(ready, good, 3, 1, nl=-1) == -1
    assert call(ready, [0, 1, 2, 3, 4, 5], 3, 1) == -1                 # five lists, prepared for four
    assert call(ready, [0, 30, 60, 71], 3, 1) == -1                    # 71 vectors, prepared for 70
    assert call(ready, good, 3, 1, null=(0,)) == -1 and call(ready, good, 3, 1, null=(1,)) == -1
    assert call(theirs, good, 3, 1) == -1 and b"another index" in lib.icd_last_error()
    state = call(fresh, good, 3, 1)                                     # never prepared: ICD_ERR_STATE
    assert state == -5 and b"icd_grouping_prepare_maxsim" in lib.icd_last_error()
    assert call(fresh, good, 3, 2) == state
    assert call(ready, good, 3, 1, nl=0) == 0                          # no list: nothing to do, nothing written
    with pytest.raises(ValueError, match="scorer"):
        index.search_lists(qq[:10], good, 3, fresh, scorer="max")
    with pytest.raises(ValueError, match="list_off"):
        index.search_lists(qq[:10], [0, 3, 9], 3, fresh)
    assert call(fresh, good, 3, 1) == state                            # the refused wrapper calls did not prepare it
    assert len(index.search_lists(qq[:10], good, 3, ready)) == 5
    for h in (theirs, other, fresh, ready):
        h.close()
    with pytest.raises(_native.IcdError):
        index.search_lists(qq[:10], good, 3, ready)


def test_graph_capture_of_a_list_search(oracle):
    import torch
    corpus, levels, q, off, index, s_all, i_all = _setup(oracle, 1000)
    group_of = _groupings(1000)["long"]
    want = expected(Ranking(s_all, i_all, group_of, id_base=ID_BASE), off, levels, 10, "sum", id_base=ID_BASE)
    grouping, late = index.grouping(group_of), index.grouping(group_of)
    grouping.prepare_maxsim(index, 64, 1100)
    dq = torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eager = index.search_lists(dq, off, 10, grouping)               # warm-up on the capture stream
    side.synchronize()
    _compare(eager, want, "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cap = index.search_lists(dq, off, 10, grouping)
        with pytest.raises(_native.IcdError) as e:      # prepare allocates: refused while capturing
            late.prepare_maxsim(index, 64, 1100)
    assert e.value.code == -1
    for _ in range(2):
        for t in cap:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for g, w in zip(cap, eager):
            assert _bits(g) == _bits(w)
    del graph
    late.close()
    grouping.close()
