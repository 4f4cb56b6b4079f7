"""The expected result of an embedding-list search (MAX_SIM over a query's vectors), from a full ranking
alone. Built on grouped_oracle.Ranking, one ranking row per VECTOR: per (vector, group) the group's best row, then per list the
chain of sequential np.float32 adds in list order over the vectors that hit the group, for "mean" one np.float32 divide by their
number, NaN aggregates dropped, ties by the row id of the first hitting vector's best row. Shared by tests/test_maxsim_cpu.py
(checked there against a brute force over all rows) and the GPU tests."""
import numpy as np

from group_scorer_oracle import order_u32
from grouped_oracle import Ranking

SCORERS = ("sum", "mean")
MAX_T = 64


class ListRanking:
    """Per vector of a Ranking the best row of every group (b(t, g) of the contract), and per list of list_off every group's
    aggregate, the id of its tie-break row, and the groups' order."""

    def __init__(self, ranking: Ranking, list_off, scorer: str = "sum", reverse: bool = False):
        assert scorer in SCORERS
        self.rk, self.scorer = ranking, scorer
        self.list_off = np.asarray(list_off, np.int64)
        nv = ranking.ids.shape[0]
        assert self.list_off[0] == 0 and self.list_off[-1] == nv and (np.diff(self.list_off) >= 1).all() and (np.diff(self.list_off) <= MAX_T).all()
        self.labels = np.unique(ranking.group_of)                     # the caller's group ids, ascending: column g of the tables
        G = len(self.labels)
        col_of_row = np.searchsorted(self.labels, ranking.group_of)
        self.has = np.zeros((nv, G), bool)
        self.bscore = np.zeros((nv, G), np.float32)
        self.bid = np.full((nv, G), -1, np.int64)
        for t in range(nv):
            hits = int((ranking.ids[t] >= 0).sum())
            pos = np.flatnonzero(ranking.occ[t, :hits] == 0)          # every group's best row under t
            col = col_of_row[ranking.ids[t, pos] - ranking.id_base]
            self.has[t, col], self.bscore[t, col], self.bid[t, col] = True, ranking.scores[t, pos], ranking.ids[t, pos]
        self.agg, self.first_id, self.order = [], [], []
        for L in range(len(self.list_off) - 1):
            ts = list(range(int(self.list_off[L]), int(self.list_off[L + 1])))
            acc, n_hit, first = np.zeros(G, np.float32), np.zeros(G, np.int64), np.full(G, -1, np.int64)
            with np.errstate(all="ignore"):
                for t in (ts[::-1] if reverse else ts):
                    new, old = self.has[t] & (n_hit == 0), self.has[t] & (n_hit > 0)
                    acc[new], first[new] = self.bscore[t, new], self.bid[t, new]
                    acc[old] = acc[old] + self.bscore[t, old]          # fp32 + fp32, rounded once, in list order
                    n_hit += self.has[t]
                if scorer == "mean":
                    live = n_hit > 0
                    acc[live] = acc[live] / n_hit[live].astype(np.float32)     # one fp32 divide
            ok = np.flatnonzero((n_hit > 0) & ~np.isnan(acc))          # no hitting vector, or a NaN aggregate: no hit
            rank = np.lexsort((first[ok], -order_u32(acc[ok]).astype(np.int64)))
            self.agg.append(acc); self.first_id.append(first); self.order.append(ok[rank])

    def outputs(self, k):
        """(group scores f32 [lists][k], group ids i32 [lists][k], match scores f32 [vectors][k], match ids i64 [vectors][k] in the
        ranking's own numbering)"""
        nl, nv = len(self.order), self.rk.ids.shape[0]
        gsc, gid = np.full((nl, k), -np.inf, np.float32), np.full((nl, k), -1, np.int32)
        msc, mid = np.full((nv, k), -np.inf, np.float32), np.full((nv, k), -1, np.int64)
        for L in range(nl):
            win = self.order[L][:k]
            gsc[L, :len(win)], gid[L, :len(win)] = self.agg[L][win], self.labels[win]
            for t in range(int(self.list_off[L]), int(self.list_off[L + 1])):
                h = self.has[t, win]
                msc[t, :len(win)][h], mid[t, :len(win)][h] = self.bscore[t, win][h], self.bid[t, win][h]
        return gsc, gid, msc, mid


def expected(ranking, list_off, levels, k, scorer="sum", row_map=None, id_base=0):
    """(group scores, group ids, match scores, match ids, match levels) as IcdIndex.search_lists returns them: the ranking's rows
    (its ids less its own id_base) mapped through row_map (a view's rows of its parent, `levels` then being the parent's) and
    moved to id_base + row; levels is indexed by id - id_base"""
    gsc, gid, msc, ids = ListRanking(ranking, list_off, scorer).outputs(k)
    rows = np.clip(ids - ranking.id_base, 0, None)
    gids = np.where(ids >= 0, id_base + (rows if row_map is None else np.asarray(row_map)[rows]), -1)
    levels = np.asarray(levels, np.int32)
    lv = np.where(gids >= 0, levels[np.clip(gids - id_base, 0, None)], 0).astype(np.int32)
    return gsc, gid, msc, gids, lv


def order_sensitive_share(ranking, list_off, k, scorer="sum", min_t=3):
    """(share, total): among the winning (list, group) cells - the k best groups of every list of at least min_t vectors - the share
    whose aggregate changes in bits when the chain runs last vector first"""
    fwd, rev = ListRanking(ranking, list_off, scorer), ListRanking(ranking, list_off, scorer, reverse=True)
    differ = total = 0
    for L in range(len(fwd.order)):
        if fwd.list_off[L + 1] - fwd.list_off[L] < min_t:
            continue
        win = fwd.order[L][:k]
        total += len(win)
        differ += int((fwd.agg[L][win].view(np.uint32) != rev.agg[L][win].view(np.uint32)).sum())
    return differ / max(total, 1), total


def brute_force(corpus_scores, group_of, list_off, k, scorer="sum"):
    """the contract restated from a plain score matrix [vectors][rows] (NaN = no hit), row by row in Python: the check of this
    module's own tables. Returns (group scores, group ids, match scores, match rows)."""
    S = np.asarray(corpus_scores, np.float32)
    group_of = np.asarray(group_of)
    nl = len(list_off) - 1
    gsc, gid = np.full((nl, k), -np.inf, np.float32), np.full((nl, k), -1, np.int32)
    msc, mid = np.full((S.shape[0], k), -np.inf, np.float32), np.full((S.shape[0], k), -1, np.int64)
    for L in range(nl):
        cells = {}
        best = {}
        for t in range(int(list_off[L]), int(list_off[L + 1])):
            for r in range(S.shape[1]):
                x = S[t, r]
                if np.isnan(x):
                    continue
                key = (t, int(group_of[r]))
                if key not in best or order_u32(x) > order_u32(best[key][0]):      # (equal scores: the lower row stays)
                    best[key] = (x, r)
            for (tt, g), (x, r) in best.items():
                if tt != t:
                    continue
                with np.errstate(all="ignore"):
                    cells[g] = (np.float32(cells[g][0] + x), cells[g][1], cells[g][2] + 1) if g in cells else (x, r, 1)
        ranked = []
        for g, (a, r, m) in cells.items():
            with np.errstate(all="ignore"):
                a = np.float32(a / np.float32(m)) if scorer == "mean" else a
            if not np.isnan(a):
                ranked.append((-int(order_u32(a)), r, g, a))
        ranked.sort()
        for j, (_o, _r, g, a) in enumerate(ranked[:k]):
            gsc[L, j], gid[L, j] = a, g
            for t in range(int(list_off[L]), int(list_off[L + 1])):
                if (t, g) in best:
                    msc[t, j], mid[t, j] = best[(t, g)]
    return gsc, gid, msc, mid
