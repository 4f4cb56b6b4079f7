"""tests/fuse_list_cases.py without a GPU: every case the synthetic-list tests of the fuse kernels use is built, given to the oracles
(hybrid_oracle.fuse_query, grouped_hybrid_oracle.fuse_query_grouped) and its aim asserted on their answers - that the inputs reach
what they are meant to reach: negative, zero (by cancellation AND by a zero weight, tied), huge and infinite fused values, runs
longer than R, one run over every slot, holes that shift no rank, zero heads between queries with heads, heads below k, group runs
that alternate, split and outlast s, fewer groups than k and groups of fewer than s members."""
import numpy as np
import pytest

import fuse_list_cases as fc
import grouped_hybrid_oracle as gho
from conftest import icd_levels
from hybrid_oracle import fuse_query

N = 300
LEVELS = icd_levels(N, 11)
ID_BASE = 2 ** 32 + 12345


def _measures(sc, ids, limits, id_base, **okw):
    R, lmax = ids.shape[1:]
    return [fc.measure(fuse_query(fc.cut(sc, ids, q, limits), LEVELS, R * lmax, id_base=id_base, n=N, **okw)[0], sc, ids, q, limits, N, id_base)
            for q in range(ids.shape[0])]


def test_the_widths_are_every_width_of_the_sort_network():
    assert sorted({fc.sort_width(R, lmax) for R, lmax in fc.WIDTHS}) == [2, 4, 8, 16, 32, 64, 128, 256, 512, 1024]
    assert (3, 43) in fc.WIDTHS and fc.sort_width(3, 43) == 256 and 3 * 43 < 256      # a tail of slots with r >= R inside the 256 lanes
    for R, lmax in fc.WIDTHS:
        for limits in fc.limit_sets(R, lmax):
            assert len(limits) == R and all(1 <= l <= lmax for l in limits)
        if lmax > 1 and R > 1:
            assert 1 in fc.limit_sets(R, lmax)[1] and max(fc.limit_sets(R, lmax)[1]) < lmax


@pytest.mark.parametrize("id_base", [0, ID_BASE])
@pytest.mark.parametrize("kind", fc.LIST_KINDS)
def test_every_list_kind_reaches_its_aim(kind, id_base):
    for R, lmax in fc.WIDTHS:
        sc, ids = fc.build(kind, 3, R, lmax, N, id_base, seed=R * 1000 + lmax)
        if kind == "holes" and lmax >= 3 and R >= 2:
            held = set(ids.reshape(-1).tolist())
            assert set(fc.foreign_ids(N, id_base)) <= held and (ids[:, 0, 0] < id_base).all() and (ids[:, :, -1] == -1).all()
        for limits in fc.limit_sets(R, lmax):
            for ranker, okw in (("rrf", {"ranker": "rrf", "c": 60.0}), ("weighted", {"ranker": "weighted", "weights": fc.W_MIXED[:R], "norm": "none"})):
                ms = _measures(sc, ids, limits, id_base, **okw)
                for k in (1, 10, 128):
                    fc.assert_list_aim(kind, ms, R, lmax, limits, k, ranker)
    # heads above k at the large widths
    if kind == "disjoint":
        sc, ids = fc.build(kind, 3, 8, 128, N, id_base, seed=1)
        assert all(m["heads"] == N > 128 for m in _measures(sc, ids, [128] * 8, id_base))


@pytest.mark.parametrize("score", fc.SCORE_KINDS)
def test_every_score_kind_reaches_its_aim(score):
    for R, lmax in ((3, 43), (8, 128)):
        for kind in ("rotated", "repeats"):
            sc, ids = fc.build(kind, 3, R, lmax, N, 0, seed=R + lmax, scores=score)
            for weights in (fc.W_MIXED, fc.W_ONES):
                for norm in ("none", "cosine"):
                    ms = _measures(sc, ids, [lmax] * R, 0, ranker="weighted", weights=weights[:R], norm=norm)
                    fc.assert_list_aim(kind, ms, R, lmax, [lmax] * R, 128, "weighted")
                    fc.assert_score_aim(score, ms, R, weights, norm, kind)
    # the two zeros of `cancel` under the weights with a 0.0: they tie, and their request bits differ
    sc, ids = fc.build("repeats", 3, 8, 128, N, 0, seed=136, scores="cancel")
    fused, out, _lv, bits = fuse_query(fc.cut(sc, ids, 1, [128] * 8), LEVELS, 128, "weighted", weights=fc.W_MIXED, norm="none", n=N)[0]
    zero = np.flatnonzero((fused == 0.0) & (out >= 0))
    assert len(zero) >= 2 and 1 << 7 in bits[zero].tolist() and len(set(bits[zero].tolist())) >= 2 and (np.diff(out[zero]) > 0).all()


@pytest.mark.parametrize("gname", ["own", "one", "mod7", "fam20"])
def test_every_grouped_kind_reaches_its_aim(gname):
    group_of = fc.groupings(N)[gname]
    few_groups = few_members = False
    for R, lmax in fc.GROUPED_WIDTHS:
        for k, s in fc.KS:
            limits = fc.grouped_limits(R, lmax, s)
            assert all(1 <= l and l * s <= 128 for l in limits) and k * s <= 128
            for kind in fc.GROUPED_KINDS:
                ids = fc.build_grouped_ids(kind, 3, R, lmax, group_of, s, limits, seed=R + lmax + k)
                sc = fc.build_scores("plain", ids, 3)
                cuts = [[gho.run_cut(ids[q, r], group_of, limits[r]) for r in range(R)] for q in range(3)]
                outs = [gho.fuse_query_grouped([(sc[q, r], ids[q, r]) for r in range(R)], group_of, LEVELS, limits, k, s)[0] for q in range(3)]
                for q, raw in enumerate(outs):
                    ng, least = fc.groups_and_members(raw, k, s)
                    few_groups |= 0 < ng < k
                    few_members |= 0 < least < s
                many = len(np.unique(group_of)) > 1
                if kind == "abab" and many:        # slot j lies in run j + 1: the cut by runs is the cut by slots
                    assert cuts == [[min(l, lmax) for l in limits]] * 3
                if kind == "aabb" and many and lmax >= 43 and s <= 3:   # the last run in front of the cut is longer than s
                    assert all(c > limits[r] + s - 1 for row in cuts for r, c in enumerate(row))
                    long_last = 0
                    for q in range(3):
                        for r in range(R):
                            g = group_of[ids[q, r, :cuts[q][r]]]
                            tail = 1
                            while tail < len(g) and g[-1 - tail] == g[-1]:
                                tail += 1
                            long_last += tail > s
                    assert long_last >= 1
                if kind == "split" and lmax >= 9:  # a run of one group counts twice: an id that is no row in front of the cut, or AT it
                    assert any(((ids[q, r, :cuts[q][r] + 1] < 0) | (ids[q, r, :cuts[q][r] + 1] >= N)).any() for q in range(3) for r in range(R))
                if kind == "empty":
                    assert (outs[1][1] == -1).all() and outs[0][1][0] >= 0 and outs[2][1][0] >= 0
                if kind == "repeats":
                    assert (outs[0][1] >= 0).sum() == 1
    if gname != "own":
        assert few_groups                          # some query has fewer groups than k
    if gname not in ("one",):
        assert few_members                         # some group has fewer than s members
