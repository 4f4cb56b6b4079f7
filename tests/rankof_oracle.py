"""What a rank-of search must return, as a walk over the FULL ranking of every query (oracle.flat_ip_topk at k = n: scores and
ids, best first by (score desc, id asc), rows with a NaN score left out): keep the rows of the query's mask (mask_oracle.restrict)
and look the target up. Rules of DESIGN.md section 26.

  rank      the target's position in the restricted ranking = the rows of the mask strictly ahead of it
  raw, adj  its score there and float64(raw) * w[level] (range_oracle.W)
  no rank   -1, NaN scores, level 0: a padding slot (-1), an id outside [id_base, id_base + n), a row outside the mask; a row inside
            the mask whose score is NaN (it is in no ranking) has rank -1 and NaN scores too, and keeps its level
  selected  the rows the mask admits

No device code and nothing of the package under test: numpy only.
"""
import numpy as np

from mask_oracle import as_bool, restrict
from range_oracle import W


def rank_of_query(scores, ids, levels, targets, mask, n, id_base=0):
    """one query: (rank i64 [nt], adj f64 [nt], raw f32 [nt], level i32 [nt], selected)"""
    scores = np.asarray(scores, np.float32)
    ids = np.asarray(ids, np.int64)
    real = ids >= id_base   # (the padding behind a ranking that left NaN rows out)
    admitted = as_bool(mask, n)
    s, i = restrict(scores[real], ids[real], admitted, id_base)
    targets = np.asarray(targets, np.int64).reshape(-1)
    nt = len(targets)
    rank = np.full(nt, -1, np.int64)
    adj = np.full(nt, np.nan, np.float64)
    raw = np.full(nt, np.nan, np.float32)
    lv = np.zeros(nt, np.int32)
    for j, t in enumerate(targets):
        row = int(t) - id_base
        if t == -1 or not 0 <= row < n or not admitted[row]:
            continue
        lv[j] = levels[row]
        pos = np.nonzero(i == t)[0]
        if len(pos) == 0:   # (a NaN score: in no ranking)
            continue
        rank[j] = pos[0]
        raw[j] = s[pos[0]]
        adj[j] = float(np.float64(raw[j]) * W.get(int(lv[j]), 1.0))
    return rank, adj, raw, lv, int(admitted.sum())


def rank_of_batch(scores, ids, levels, targets, masks, n, id_base=0):
    """a batch: targets [nq, nt]; masks None or one entry per query (None, boolean array or row list, over ROWS). Returns
    (rank [nq, nt], adj, raw, levels, selected [nq])."""
    nq = len(scores)
    masks = [None] * nq if masks is None else masks
    assert len(masks) == nq and len(targets) == nq
    per = [rank_of_query(scores[q], ids[q], levels, targets[q], masks[q], n, id_base) for q in range(nq)]
    return tuple(np.stack([p[j] for p in per]) for j in range(4)) + (np.asarray([p[4] for p in per], np.int64),)


def brute_force(row_scores, target_row, admitted):
    """the definition, without a ranking: the admitted rows r with score[r] > score[t], or score[r] == score[t] and r < t (NaN
    scores compare false both ways); -1 for a target that is not admitted or whose score is NaN"""
    sc = np.asarray(row_scores, np.float32)
    if not admitted[target_row] or np.isnan(sc[target_row]):
        return -1
    st = sc[target_row]
    rows = np.arange(len(sc))
    with np.errstate(invalid="ignore"):
        ahead = admitted & ((sc > st) | ((sc == st) & (rows < target_row)))
    return int(ahead.sum())


def metrics(best_ranks, ks=(1, 5, 10)):
    """recall@k, MRR and mean rank from per-query best ranks (-1 / None: not ranked), written out plainly"""
    n = len(best_ranks)
    found = [int(r) for r in best_ranks if r is not None and int(r) >= 0]
    out = {"n": n}
    for k in ks:
        out[f"recall@{k}"] = (sum(1 for r in found if r < k) / n) if n else 0.0
    out["mrr"] = (sum(1.0 / (r + 1) for r in found) / n) if n else 0.0
    out["mean_rank"] = (sum(found) / len(found)) if found else None
    return out
