"""The expected result of a grouping search under a group scorer (max / sum / avg), from a full ranking
alone. Built on grouped_oracle.Ranking: sequential np.float32 adds best first, one np.float32 divide, NaN aggregates dropped, ties
by the row id of the group's best member. Shared by tests/test_group_scorer_cpu.py (checked there against a brute force over all
rows) and the GPU tests."""
import numpy as np

from grouped_oracle import Ranking

SCORERS = ("max", "sum", "avg")


def order_u32(x):
    """the device's sortable image of an fp32 (topk_select.hpp order_f32): larger = better; -0.0 sorts below +0.0"""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u >> 31, u ^ 0xFFFFFFFF, u ^ 0x80000000)


def chain_sum(xs, reverse=False):
    """the contract's sum of a best-first list: x_1, then + x_2, + x_3, ... one fp32 add each (reverse: worst first)"""
    xs = [np.float32(x) for x in (xs[::-1] if reverse else xs)]
    acc = xs[0]
    with np.errstate(all="ignore"):
        for x in xs[1:]:
            acc = np.float32(acc + x)
    return acc


class ScoredRanking:
    """Per query of a Ranking and for one (s, scorer): every group that has a hit - its aggregate, its member count m, the
    position (in the ranking) of its best member - and the groups' order under the scorer."""

    def __init__(self, ranking: Ranking, s: int, scorer: str):
        assert scorer in SCORERS and s >= 1
        self.rk, self.s, self.scorer = ranking, int(s), scorer
        nq = ranking.ids.shape[0]
        self.agg, self.first, self.m, self.order = [], [], [], []
        for q in range(nq):
            hits = int((ranking.ids[q] >= 0).sum())
            if hits == 0:
                self.agg.append(np.zeros(0, np.float32)); self.first.append(np.zeros(0, np.int64))
                self.m.append(np.zeros(0, np.int64)); self.order.append(np.zeros(0, np.int64))
                continue
            gr, oc = ranking.grank[q, :hits], ranking.occ[q, :hits]
            ng = int(gr.max()) + 1
            take = np.flatnonzero(oc < self.s)
            x = np.zeros((ng, min(self.s, int(oc.max()) + 1)), np.float32)
            x[gr[take], oc[take]] = ranking.scores[q, take]
            m = np.minimum(np.bincount(gr, minlength=ng), self.s)
            first = np.empty(ng, np.int64)
            first[gr[oc == 0]] = np.flatnonzero(oc == 0)
            acc = x[:, 0].copy()
            if scorer != "max":
                with np.errstate(all="ignore"):
                    for i in range(1, x.shape[1]):
                        live = m > i
                        acc[live] = acc[live] + x[live, i]          # fp32 + fp32, rounded once, in rank order
                    if scorer == "avg":
                        acc = acc / m.astype(np.float32)            # one fp32 divide
            ok = np.flatnonzero(~np.isnan(acc))                     # a NaN aggregate is no hit
            best_id = ranking.ids[q, first[ok]]
            rank = np.lexsort((best_id, -order_u32(acc[ok]).astype(np.int64)))
            self.agg.append(acc); self.first.append(first); self.m.append(m); self.order.append(ok[rank])

    def raw(self, k):
        """(scores f32, ids i64, groups i32) [nq][k * s] group-rank-major as grouped_oracle.Ranking.raw, and (group scores f32,
        group ids i32) [nq][k]"""
        rk, s = self.rk, self.s
        nq = rk.ids.shape[0]
        sc = np.full((nq, k * s), -np.inf, np.float32)
        ids = np.full((nq, k * s), -1, np.int64)
        grp = np.full((nq, k * s), -1, np.int32)
        gsc = np.full((nq, k), -np.inf, np.float32)
        gid = np.full((nq, k), -1, np.int32)
        for q in range(nq):
            win = self.order[q][:k]
            if len(win) == 0:
                continue
            place = np.full(len(self.agg[q]), -1, np.int64)
            place[win] = np.arange(len(win))
            hits = int((rk.ids[q] >= 0).sum())
            gr, oc = rk.grank[q, :hits], rk.occ[q, :hits]
            pos = np.flatnonzero((place[gr] >= 0) & (oc < s))
            pos = pos[np.lexsort((oc[pos], place[gr[pos]]))]
            sc[q, :len(pos)] = rk.scores[q, pos]
            ids[q, :len(pos)] = rk.ids[q, pos]
            grp[q, :len(pos)] = rk.group_of[rk.ids[q, pos] - rk.id_base]
            gsc[q, :len(win)] = self.agg[q][win]
            gid[q, :len(win)] = rk.group_of[rk.ids[q, self.first[q][win]] - rk.id_base]
        return sc, ids, grp, gsc, gid


def expected(oracle, ranking, levels, k, s, scorer, row_map=None, id_base=0):
    """raw = (scores, ids, levels, groups), adjusted = (adj, scores, ids, levels, groups) as grouped_oracle.expected, and
    group = (group scores, group ids) - the same in both output modes"""
    sc, ids, grp, gsc, gid = ScoredRanking(ranking, s, scorer).raw(k)
    rows = np.clip(ids - ranking.id_base, 0, None)
    gids = np.where(ids >= 0, id_base + (rows if row_map is None else np.asarray(row_map)[rows]), -1)
    levels = np.asarray(levels, np.int32)
    lv = np.where(gids >= 0, levels[np.clip(gids - id_base, 0, None)], 0).astype(np.int32)
    adj, araw, aid, alv = oracle.reweight(sc, gids, levels, id_base)
    agrp = np.full(aid.shape, -1, np.int32)
    for q in range(aid.shape[0]):
        back = dict(zip(gids[q].tolist(), grp[q].tolist()))
        agrp[q] = [back[i] if i >= 0 else -1 for i in aid[q].tolist()]
    return (sc, gids, lv, grp), (adj, araw, aid, alv, agrp), (gsc, gid)


def order_sensitive_share(ranking, s, min_m=3):
    """the share of (query, group) pairs with m >= min_m whose best-first chain differs in bits from the worst-first chain"""
    differ = total = 0
    for q in range(ranking.ids.shape[0]):
        hits = int((ranking.ids[q] >= 0).sum())
        gr, oc = ranking.grank[q, :hits], ranking.occ[q, :hits]
        members = {}
        for p in np.flatnonzero(oc < s):
            members.setdefault(int(gr[p]), []).append(ranking.scores[q, p])
        for xs in members.values():
            if len(xs) >= min_m:
                total += 1
                differ += chain_sum(xs).tobytes() != chain_sum(xs, reverse=True).tobytes()
    return differ / max(total, 1), total
