"""numpy oracle of the facet counts over a row mask (include/icd_search.h icd_rowmask_group_counts). Nothing
of the package: a mask - its words in icd_rowmask_pack's layout (bit r & 31 of word r >> 5 is row r), a boolean array over the rows,
or None for every row - and the rows' caller group ids give

    group_ids   the sorted distinct caller ids: column j counts the rows of group_ids[j]
    counts      int32 [G]: np.bincount of the set rows' dense group numbers
"""
import numpy as np


def pack(rows, n):
    """the words of a mask over n rows that holds `rows` (icd_rowmask_pack's layout, without its tile padding)"""
    words = np.zeros((n + 31) // 32, np.uint32)
    rows = np.asarray(rows, np.int64)
    np.bitwise_or.at(words, rows >> 5, (np.uint32(1) << (rows & 31).astype(np.uint32)))
    return words


def unpack(words, n):
    """bool [n] of a mask's words: bits at or behind n are dropped whatever they hold"""
    bits = np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8), bitorder="little")
    return bits[:n].astype(bool)


def dense(group_of):
    """(group_ids int32 [G], dense_of int64 [n]): the sorted distinct caller ids and every row's rank among them"""
    group_ids, dense_of = np.unique(np.asarray(group_of).reshape(-1), return_inverse=True)
    return group_ids.astype(np.int32), dense_of.reshape(-1).astype(np.int64)


def counts(mask, group_of, words=False):
    """int32 [G] of one query; mask: None, bool [n], or - words=True - uint32 words"""
    group_ids, dense_of = dense(group_of)
    n = dense_of.size
    if mask is None:
        keep = np.ones(n, bool)
    else:
        keep = unpack(mask, n) if words else np.asarray(mask, bool)[:n]
    return np.bincount(dense_of[keep], minlength=group_ids.size).astype(np.int32)


def counts_batch(masks, group_of, words=False):
    """int32 [nq, G] of a batch: what IcdIndex.group_counts returns"""
    G = dense(group_of)[0].size
    out = np.empty((len(masks), G), np.int32)
    for q, m in enumerate(masks):
        out[q] = counts(m, group_of, words)
    return out


def facets(row, values, limit=None, min_count=1):
    """the service's list of one row of counts: count descending, then the values' order; below min_count dropped; cut at limit"""
    order = sorted(range(len(row)), key=lambda j: (-int(row[j]), j))
    out = [{"value": values[j], "count": int(row[j])} for j in order if row[j] >= min_count]
    return out if limit is None else out[:limit]
