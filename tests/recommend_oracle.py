"""What a recommend search must return (include/icd_search.h), in numpy float32: the canonical score chain,
the target vector of `average_vector`, the fold of the examples' scores per strategy, what ranks, and the window with its raw and
reweighted forms (wide_oracle's). Beside it `brute_force`, which folds row by row with scalar float32 arithmetic and never builds
a ranking (per row: count the rows ahead).

An example is an int (a stored row's id) or a vector of dim floats. No device code and nothing of the package under test: numpy
only.
"""
import numpy as np

from wide_oracle import MAX_K, order_u32, reweight

MAX_EXAMPLES = 16
STRATEGIES = ("average_vector", "best_score", "sum_scores")
F = np.float32


def chain_scores(vector, corpus):
    """the canonical score of DESIGN.md section 2 for one vector and every row: acc = fmaf(row[d], vector[d], acc) over d ascending
    from +0.0f. numpy has no fmaf: the product of two float32 is exact in float64, the sum with acc is taken in float64 and rounded
    TO ODD there (two-sum: when it was inexact and the double's last bit is even, step one ulp towards the error), so that the
    final rounding to float32 is the one rounding of the exact value - fmaf's bits."""
    x = np.asarray(corpus, F).astype(np.float64)
    v = np.asarray(vector, F).astype(np.float64)
    acc = np.zeros(x.shape[0], F)
    with np.errstate(all="ignore"):
        for d in range(x.shape[1]):
            p, a = x[:, d] * v[d], acc.astype(np.float64)
            s = p + a
            bv = s - p
            err = (p - (s - bv)) + (a - bv)                        # exact: s + err = p + a
            fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
            s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
            acc = s.astype(F)
    return acc


def example_vector(example, corpus, id_base=0):
    if isinstance(example, (int, np.integer)):
        return np.asarray(corpus[int(example) - id_base], F)
    return np.asarray(example, F)


def example_rows(examples, id_base=0):
    """the rows a request's stored examples name: they do not rank"""
    return [int(e) - id_base for e in examples if isinstance(e, (int, np.integer))]


def target_vector(positive, negative, corpus, id_base=0):
    """average_vector's target: per component the positives summed in list order from +0.0f, one float32 divide by float32(P), the
    same over the negatives, t = mp + (mp - mn) when there are negatives, else mp"""
    assert len(positive) >= 1

    def mean(examples):
        acc = np.zeros(corpus.shape[1], F)
        for e in examples:
            acc = (acc + example_vector(e, corpus, id_base)).astype(F)
        return (acc / F(len(examples))).astype(F)
    with np.errstate(all="ignore"):
        mp = mean(positive)
        if not negative:
            return mp
        mn = mean(negative)
        return (mp + (mp - mn).astype(F)).astype(F)


def fold(strategy, pos_scores, neg_scores, n):
    """the combined score c [n] float32 from the examples' scores by row (lists of float32 [n], in list order) and `clean` [n]: no
    example score of the row is NaN"""
    assert strategy in ("best_score", "sum_scores")
    clean = np.ones(n, bool)
    for s in list(pos_scores) + list(neg_scores):
        clean &= ~np.isnan(s)
    with np.errstate(all="ignore"):
        if strategy == "sum_scores":
            acc = np.zeros(n, F)
            for s in pos_scores:
                acc = (acc + np.asarray(s, F)).astype(F)
            for s in neg_scores:
                acc = (acc - np.asarray(s, F)).astype(F)
            return acc, clean
        bp, bn = np.full(n, -np.inf, F), np.full(n, -np.inf, F)
        for s in pos_scores:
            bp = np.where(np.asarray(s, F) > bp, s, bp).astype(F)       # plain compares, in list order: +0.0 does not replace -0.0
        for s in neg_scores:
            bn = np.where(np.asarray(s, F) > bn, s, bn).astype(F)
        return np.where(bp > bn, bp, -((bn * bn).astype(F))).astype(F), clean


def combined(corpus, positive, negative, strategy, id_base=0, score_fn=chain_scores):
    """c [n] and clean [n] of one request; score_fn(vector, corpus) -> the canonical scores by row"""
    assert strategy in STRATEGIES and 1 <= len(positive) + len(negative) <= MAX_EXAMPLES
    n = corpus.shape[0]
    if strategy == "average_vector":
        c = np.asarray(score_fn(target_vector(positive, negative, corpus, id_base), corpus), F)
        return c, ~np.isnan(c)
    sp = [np.asarray(score_fn(example_vector(e, corpus, id_base), corpus), F) for e in positive]
    sn = [np.asarray(score_fn(example_vector(e, corpus, id_base), corpus), F) for e in negative]
    return fold(strategy, sp, sn, n)


def ranks_mask(c, clean, excluded_rows, mask=None, radius=None, range_filter=None):
    ok = clean & ~np.isnan(c)
    if mask is not None:
        ok &= np.asarray(mask, bool)
    ok[list(excluded_rows)] = False
    if radius is not None:
        ok &= c > F(radius)
    if range_filter is not None:
        ok &= c <= F(range_filter)
    return ok


def window(c, ok, levels, k, first=0, id_base=0):
    """((raw, ids, levels) in raw order, (adj, raw, ids, levels) reweighted), count, selected from the combined scores by row and
    the rows that rank: (c descending, the smaller row first among equal bits), ranks first .. first + k - 1, padded (-inf, -1, 0)"""
    assert k >= 1 and first >= 0 and first + k <= MAX_K
    rows = np.nonzero(ok)[0]
    o = order_u32(c[rows]).astype(np.int64)
    rows = rows[np.lexsort((rows, -o))]
    part = rows[first:first + k]
    raw, rid, lv = np.full(k, -np.inf, F), np.full(k, -1, np.int64), np.zeros(k, np.int32)
    raw[:len(part)], rid[:len(part)], lv[:len(part)] = c[part], part + id_base, np.asarray(levels)[part]
    return (raw, rid, lv), reweight(raw, rid, lv), np.int32(len(part)), np.int64(len(rows))


def recommend_query(corpus, levels, positive, negative, strategy, k, first=0, mask=None, radius=None, range_filter=None, id_base=0,
                    score_fn=chain_scores):
    c, clean = combined(corpus, positive, negative, strategy, id_base, score_fn)
    ok = ranks_mask(c, clean, example_rows(list(positive) + list(negative), id_base), mask, radius, range_filter)
    return window(c, ok, levels, k, first, id_base)


def _per(v, r):
    if v is None:
        return None
    v = np.asarray(v)
    return v.reshape(-1)[r] if v.size > 1 else v.reshape(-1)[0]


def recommend_batch(corpus, levels, positive, negative, strategy, k, first=0, masks=None, radius=None, range_filter=None, id_base=0,
                    score_fn=chain_scores):
    """a batch: positive / negative one list per request; masks None or one entry per request (None, boolean array over rows); bounds
    None, scalars or one per request. Returns (raw f32, ids i64, levels i32), (adj f64, raw, ids, levels), count i32 [nr], selected
    i64 [nr]"""
    per = [recommend_query(corpus, levels, positive[r], negative[r], strategy, k, first, None if masks is None else masks[r],
                           _per(radius, r), _per(range_filter, r), id_base, score_fn) for r in range(len(positive))]
    raw = tuple(np.stack([p[0][j] for p in per]) for j in range(3))
    adj = tuple(np.stack([p[1][j] for p in per]) for j in range(4))
    return raw, adj, np.array([p[2] for p in per], np.int32), np.array([p[3] for p in per], np.int64)


def brute_force(pos_scores, neg_scores, strategy, excluded_rows, k, first=0, mask=None, radius=None, range_filter=None, id_base=0):
    """one best_score / sum_scores request from its examples' scores by row, row by row in scalar float32 and without a ranking: a
    ranking row's rank is the number of ranking rows with a larger c, or the same bits and a smaller row. Returns (raw, ids) of
    ranks first .. first + k - 1 padded, count, selected. Quadratic: for small n."""
    n = len((list(pos_scores) + list(neg_scores))[0])
    c, ok = np.zeros(n, F), np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for i in range(n):
            sp, sn = [F(s[i]) for s in pos_scores], [F(s[i]) for s in neg_scores]
            if any(np.isnan(s) for s in sp + sn):
                continue
            if strategy == "sum_scores":
                acc = F(0.0)
                for s in sp:
                    acc = F(acc + s)
                for s in sn:
                    acc = F(acc - s)
                ci = acc
            else:
                bp = bn = F(-np.inf)
                for s in sp:
                    bp = s if s > bp else bp
                for s in sn:
                    bn = s if s > bn else bn
                ci = bp if bp > bn else F(-F(bn * bn))
            c[i] = ci
            ok[i] = (not np.isnan(ci) and (mask is None or bool(mask[i])) and i not in excluded_rows
                     and (radius is None or ci > F(radius)) and (range_filter is None or ci <= F(range_filter)))
    o = order_u32(c).astype(np.int64)
    rows = np.nonzero(ok)[0]
    raw, rid, count = np.full(k, -np.inf, F), np.full(k, -1, np.int64), 0
    for r in rows:
        ahead = int(((o[rows] > o[r]) | ((o[rows] == o[r]) & (rows < r))).sum())
        if first <= ahead < first + k:
            raw[ahead - first], rid[ahead - first] = c[r], r + id_base
            count += 1
    return raw, rid, np.int32(count), np.int64(len(rows))
