"""The expected result of a grouping search, from a full ranking alone (rules 2-4 of DESIGN.md section 10). Shared by
tests/test_grouped_search_cpu.py (checked there against a brute force) and tests/test_grouped_search_gpu.py."""
import numpy as np


class Ranking:
    """ids [nq][n] of ALL rows in (score desc, id asc) order with their scores (oracle.flat_ip_topk at k = n; -1 = no hit) and a
    group id per row (of the row id - id_base). Per query: the rank of every group (by its best row) and of every row inside its
    group."""

    def __init__(self, scores, ids, group_of, id_base=0):
        self.scores, self.ids = np.asarray(scores, np.float32), np.asarray(ids, np.int64)
        self.group_of, self.id_base = np.asarray(group_of, np.int64), int(id_base)
        nq, n = self.ids.shape
        self.grank = np.full((nq, n), -1, np.int64)   # rank of the group of the hit at this position
        self.occ = np.full((nq, n), -1, np.int64)     # how many better rows of its group precede it
        for q in range(nq):
            m = int((self.ids[q] >= 0).sum())
            assert (self.ids[q, :m] >= 0).all()
            g = self.group_of[self.ids[q, :m] - self.id_base]
            by_group = np.argsort(g, kind="stable")              # positions, group by group, rank order inside
            gs = g[by_group]
            start = np.r_[0, np.flatnonzero(gs[1:] != gs[:-1]) + 1]
            first = by_group[start]                               # position of every group's best row
            run = np.repeat(np.arange(len(start)), np.diff(np.r_[start, m]))
            rank_of_run = np.empty(len(start), np.int64)
            rank_of_run[np.argsort(first)] = np.arange(len(start))
            self.grank[q, by_group] = rank_of_run[run]
            self.occ[q, by_group] = np.arange(m) - start[run]

    def raw(self, k, s):
        """(scores f32, ids i64, groups i32) [nq][k * s]: group-rank-major, a group's rows best first, back to back; padded with
        -inf / -1 / -1 at the end"""
        nq = self.ids.shape[0]
        sc = np.full((nq, k * s), -np.inf, np.float32)
        ids = np.full((nq, k * s), -1, np.int64)
        grp = np.full((nq, k * s), -1, np.int32)
        for q in range(nq):
            pos = np.flatnonzero((self.grank[q] >= 0) & (self.grank[q] < k) & (self.occ[q] < s))
            pos = pos[np.lexsort((self.occ[q, pos], self.grank[q, pos]))]
            sc[q, :len(pos)] = self.scores[q, pos]
            ids[q, :len(pos)] = self.ids[q, pos]
            grp[q, :len(pos)] = self.group_of[self.ids[q, pos] - self.id_base]
        return sc, ids, grp


def expected(oracle, ranking, levels, k, s, row_map=None, id_base=0):
    """raw = (scores, ids, levels, groups), adjusted = (adj, scores, ids, levels, groups); the ranking's rows (its ids less its own
    id_base) mapped through row_map (a view's rows of its parent, `levels` then being the parent's) and moved to id_base + row
    before the reweight, as the device does; levels is indexed by id - id_base"""
    sc, ids, grp = ranking.raw(k, s)
    rows = np.clip(ids - ranking.id_base, 0, None)
    gids = np.where(ids >= 0, id_base + (rows if row_map is None else np.asarray(row_map)[rows]), -1)
    levels = np.asarray(levels, np.int32)
    lv = np.where(gids >= 0, levels[np.clip(gids - id_base, 0, None)], 0).astype(np.int32)
    adj, araw, aid, alv = oracle.reweight(sc, gids, levels, id_base)
    # the group id travels with the hit: recover it from the hit's id
    back = {}
    agrp = np.full(aid.shape, -1, np.int32)
    for q in range(aid.shape[0]):
        back = dict(zip(gids[q].tolist(), grp[q].tolist()))
        agrp[q] = [back[i] if i >= 0 else -1 for i in aid[q].tolist()]
    return (sc, gids, lv, grp), (adj, araw, aid, alv, agrp)
