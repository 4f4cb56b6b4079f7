"""What a wide search must return, as a walk over the FULL ranking of every query (oracle.flat_ip_topk at
k = n: scores and ids, best first by (score desc, id asc)): mask_oracle.restrict, range_oracle.in_band, the slice
[first, first + k) and range_oracle.reweight. Beside it `brute_force`, which never builds a ranking (per row: count the rows
ahead), and `staged`, a model of the device's three stages (threshold by radix digits, ties kept by smallest id, sort) on the
ordered scores, so that the stage logic can be checked against the ranking without a device.

No device code and nothing of the package under test: numpy only.
"""
import numpy as np

from mask_oracle import restrict
from range_oracle import W, in_band

MAX_K = 16384
DIGITS = ((21, 11), (10, 11), (0, 10))   # (shift, bits) of the radix select, most significant first


def order_u32(scores):
    """topk_select.hpp order_f32: a uint32 whose unsigned order is the float order (-0.0 below +0.0)"""
    u = np.asarray(scores, np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def reweight(raw, ids, levels_of_hits):
    """range_oracle.reweight's bytes without its Python loops (a slice holds up to 16 384 hits): adj = float64(raw) * w[level],
    ONE stable descending sort of the valid hits, padding (-inf, -inf, -1, 0) behind. tests/test_wide_cpu.py holds the two
    against each other."""
    k = len(raw)
    m = int((ids >= 0).sum())
    lv = np.asarray(levels_of_hits[:m])
    w = np.where(lv == 1, W[1], np.where(lv == 3, W[3], 1.0))
    adj = np.asarray(raw[:m], np.float32).astype(np.float64) * w
    order = np.argsort(-adj, kind="stable")
    o_adj, o_raw = np.full(k, -np.inf, np.float64), np.full(k, -np.inf, np.float32)
    o_ids, o_lv = np.full(k, -1, np.int64), np.zeros(k, np.int32)
    o_adj[:m], o_raw[:m], o_ids[:m], o_lv[:m] = adj[order], raw[:m][order], ids[:m][order], lv[order]
    return o_adj, o_raw, o_ids, o_lv


def ranking(scores, ids, mask=None, radius=None, range_filter=None, id_base=0):
    """one query's full ranking restricted to what ranks: inside the mask, not NaN, inside the band; order unchanged"""
    scores, ids = np.asarray(scores, np.float32), np.asarray(ids, np.int64)
    real = ids >= 0
    s, i = (scores[real], ids[real]) if mask is None else restrict(scores[real], ids[real], np.asarray(mask, bool), id_base)
    keep = in_band(s, i, radius, range_filter)
    return s[keep], i[keep]


def wide_query(scores, ids, levels, k, first=0, mask=None, radius=None, range_filter=None, id_base=0):
    """one query: ((raw, ids, levels) in raw order, (adj, raw, ids, levels) reweighted), each of length k and padded (-inf, -1, 0),
    count (int32) and selected (int64)"""
    assert k >= 1 and first >= 0 and first + k <= MAX_K
    s, i = ranking(scores, ids, mask, radius, range_filter, id_base)
    part_s, part_i = s[first:first + k], i[first:first + k]
    raw = np.full(k, -np.inf, np.float32)
    rid = np.full(k, -1, np.int64)
    lv = np.zeros(k, np.int32)
    raw[:len(part_s)], rid[:len(part_i)] = part_s, part_i
    lv[:len(part_i)] = np.asarray(levels)[part_i - id_base]
    return (raw, rid, lv), reweight(raw, rid, lv), np.int32(len(part_i)), np.int64(len(i))


def _per_query(v, q):
    if v is None:
        return None
    v = np.asarray(v)
    return v.reshape(-1)[q] if v.size > 1 else v.reshape(-1)[0]


def wide_batch(scores, ids, levels, k, first=0, masks=None, radius=None, range_filter=None, id_base=0):
    """a batch: masks None or one entry per query (None, boolean array over rows); bounds None, scalars or one per query.
    Returns (raw f32, ids i64, levels i32), (adj f64, raw, ids, levels), count i32 [nq], selected i64 [nq]"""
    nq = len(scores)
    per = [wide_query(scores[q], ids[q], levels, k, first, None if masks is None else masks[q], _per_query(radius, q),
                      _per_query(range_filter, q), id_base) for q in range(nq)]
    raw = tuple(np.stack([p[0][j] for p in per]) for j in range(3))
    adj = tuple(np.stack([p[1][j] for p in per]) for j in range(4))
    return raw, adj, np.array([p[2] for p in per], np.int32), np.array([p[3] for p in per], np.int64)


def brute_force(row_scores, k, first=0, mask=None, radius=None, range_filter=None, id_base=0):
    """one query from its scores BY ROW (float32 [n]), without a ranking: a ranking row's rank is the number of ranking rows with
    a larger score, or the same score bits' order and a smaller row. Returns (raw, ids) of ranks first .. first + k - 1 padded,
    count, selected. Quadratic: for small n."""
    sc = np.asarray(row_scores, np.float32)
    n = len(sc)
    ranks = ~np.isnan(sc)
    if mask is not None:
        ranks &= np.asarray(mask, bool)
    if radius is not None:
        ranks &= sc > np.float32(radius)
    if range_filter is not None:
        ranks &= sc <= np.float32(range_filter)
    o = order_u32(sc).astype(np.int64)
    rows = np.nonzero(ranks)[0]
    raw = np.full(k, -np.inf, np.float32)
    rid = np.full(k, -1, np.int64)
    count = 0
    for r in rows:
        ahead = int(((o[rows] > o[r]) | ((o[rows] == o[r]) & (rows < r))).sum())
        if first <= ahead < first + k:
            raw[ahead - first], rid[ahead - first] = sc[r], r + id_base
            count += 1
    return raw, rid, np.int32(count), np.int64(len(rows))


def staged(row_scores, k, first=0, mask=None, radius=None, range_filter=None, id_base=0):
    """the device's stages on one query's scores by row: S (ordered scores, 0 where a row does not rank), the threshold by three
    radix digits (T, above, need, selected), the collect (everything above T, the `need` smallest rows equal to T, in row
    order) and the sort of (score, ~row) keys, descending. Returns (raw, ids) padded, count, selected, and the record
    (T, above, need, selected)."""
    sc = np.asarray(row_scores, np.float32)
    ranks = ~np.isnan(sc)
    if mask is not None:
        ranks &= np.asarray(mask, bool)
    if radius is not None:
        ranks &= sc > np.float32(radius)
    if range_filter is not None:
        ranks &= sc <= np.float32(range_filter)
    S = np.where(ranks, order_u32(sc), np.uint32(0)).astype(np.uint32)
    assert not (ranks & (S == 0)).any()   # 0 is a safe sentinel: only a NaN pattern orders to 0
    width = first + k
    live = S != 0
    selected = int(live.sum())
    remaining, above, prefix, pmask = min(width, selected), 0, 0, 0
    if remaining:
        for shift, bits in DIGITS:
            inside = live & ((S & np.uint32(pmask)) == np.uint32(prefix))
            hist = np.bincount((S[inside] >> np.uint32(shift)) & np.uint32((1 << bits) - 1), minlength=1 << bits)
            ahead = 0
            for digit in range((1 << bits) - 1, -1, -1):
                if ahead + hist[digit] >= remaining:
                    break
                ahead += hist[digit]
            above, remaining = above + ahead, remaining - ahead
            prefix |= digit << shift
            pmask |= ((1 << bits) - 1) << shift
        T, need = prefix, remaining
    else:
        T, need, above = 0xFFFFFFFF, 0, 0
    rows_above = np.nonzero(S > np.uint32(T))[0] if T != 0xFFFFFFFF else np.zeros(0, np.int64)
    rows_equal = np.nonzero(S == np.uint32(T))[0][:need]   # ascending rows: the smallest ids
    assert len(rows_above) == above and len(rows_equal) == need
    rows = np.concatenate([rows_above, rows_equal]).astype(np.int64)
    keys = (S[rows].astype(np.uint64) << np.uint64(32)) | (~rows.astype(np.uint32)).astype(np.uint64)
    rows = rows[np.argsort(keys)[::-1]][first:first + k]
    raw = np.full(k, -np.inf, np.float32)
    rid = np.full(k, -1, np.int64)
    raw[:len(rows)], rid[:len(rows)] = sc[rows], rows + id_base
    return raw, rid, np.int32(len(rows)), np.int64(selected), (T, above, need, selected)
