"""What a boosted search must return, from every query's canonical scores BY ROW: multiply the scores of
the rows inside each boost's mask by its weight - one np.float32 multiply per slot, slots in order -, drop NaN and -inf, stable-sort
by (boosted desc, id asc), then walk that ranking exactly as a masked search walks the raw one: mask_oracle.restrict, then
range_oracle.band_query (in_band, k, padding, reweight). The iterator's pages come from the same ranking.

No device code and nothing of the package under test: numpy only.
"""
import numpy as np

from mask_oracle import as_bool, restrict
from range_oracle import band_query, pages

MAX_BOOSTS = 4
# a pair of weights whose two orders round differently: fl(fl(0.3f * W1) * W2) and fl(fl(0.3f * W2) * W1) differ in the last bit
W1, W2 = np.float32(1.1), np.float32(0.7)


def by_row(s_all, i_all, n, id_base=0):
    """the oracle's full ranking (oracle.flat_ip_topk at k = n: scores and ids best first) -> scores[q, row]"""
    out = np.full((len(s_all), n), np.nan, np.float32)
    np.put_along_axis(out, np.asarray(i_all, np.int64) - id_base, np.asarray(s_all, np.float32), 1)
    return out


def boost_scores(scores, boosts):
    """one query: scores [n] by row, boosts a list of up to MAX_BOOSTS entries, each None (slot unused) or (mask, weight) with
    mask a boolean array [n] or a list of rows -> the boosted scores [n]. One IEEE fp32 multiply per used slot, in slot order."""
    s = np.array(scores, np.float32)
    n = len(s)
    boosts = [] if boosts is None else list(boosts)
    assert len(boosts) <= MAX_BOOSTS
    for b in boosts:
        if b is None:
            continue
        m, w = as_bool(b[0], n), np.float32(b[1])
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            prod = s[m] * w
        assert prod.dtype == np.float32
        s[m] = prod
    return s


def ranking(boosted, id_base=0):
    """boosted scores [n] by row -> (scores, ids) of the rows that can be hits (no NaN, no -inf), best first by (boosted desc, id asc)"""
    boosted = np.asarray(boosted, np.float32)
    rows = np.nonzero(~np.isnan(boosted) & ~np.isneginf(boosted))[0]
    order = np.argsort(-boosted[rows].astype(np.float64), kind="stable")   # (rows ascend: the stable sort breaks ties by id)
    return boosted[rows][order], (rows[order] + id_base).astype(np.int64)


def _restrict(scores, ids, mask, n, id_base):
    """mask_oracle.restrict over a ranking that may be shorter than the index (NaN and -inf rows are gone): the mask is over ROWS"""
    return (scores, ids) if mask is None else restrict(scores, ids, as_bool(mask, n), id_base)


def _per_query(v, q):
    if v is None:
        return None
    v = np.asarray(v)
    return v.reshape(-1)[q] if v.size > 1 else v.reshape(-1)[0]


def boosted_rankings(scores_by_row, boosts, id_base=0):
    """per query: ranking(boost_scores(...)); boosts has one entry (a list of slots, or None) per query"""
    assert len(boosts) == len(scores_by_row)
    return [ranking(boost_scores(scores_by_row[q], boosts[q]), id_base) for q in range(len(scores_by_row))]


def boosted_batch(scores_by_row, levels, boosts, k, masks=None, radius=None, range_filter=None, after=None, offset=0, id_base=0,
                  rankings=None):
    """a batch: ((raw, ids, levels) in raw order, (adj, raw, ids, levels) reweighted), each [nq, k], padded (-inf, -1, level 0).
    masks: None or one entry per query (None, boolean array or row list over ROWS); bounds: None, scalars or one value per query;
    after = (scores [nq], ids [nq]) or None - all on the BOOSTED score. rankings: boosted_rankings' result, to share it."""
    nq = len(scores_by_row)
    rk = boosted_rankings(scores_by_row, boosts, id_base) if rankings is None else rankings
    raws, adjs = [], []
    for q in range(nq):
        s, i = _restrict(rk[q][0], rk[q][1], None if masks is None else masks[q], len(scores_by_row[q]), id_base)
        a = None if after is None else (_per_query(after[0], q), _per_query(after[1], q))
        r, a2 = band_query(s, i, levels, k, _per_query(radius, q), _per_query(range_filter, q), a, offset, id_base)
        raws.append(r)
        adjs.append(a2)
    return tuple(np.stack([r[j] for r in raws]) for j in range(3)), tuple(np.stack([a[j] for a in adjs]) for j in range(4))


def boosted_pages(scores, boosts, batch_size, mask=None, radius=None, range_filter=None, limit=-1, id_base=0):
    """one query (scores [n] by row): the iterator's pages, lists of ids in raw order over the boosted ranking"""
    s, i = ranking(boost_scores(scores, boosts), id_base)
    s, i = _restrict(s, i, mask, len(scores), id_base)
    return pages(s, i, batch_size, radius, range_filter, limit)
