"""numpy oracle of the ordered select over a row mask (include/icd_search.h icd_rowmask_select). Nothing of
the package: a boolean array over the rows (or None: every row), an offset and a limit give

    total   the rows the mask holds
    taken   clamp(total - offset, 0, limit)
    ids     int64 [limit]: the rows of ranks offset .. offset + taken in ascending order, then -1
"""
import numpy as np


def select(mask, n, offset, limit):
    """(ids int64 [limit], total int, taken int) of one query; mask: bool [n] or None"""
    rows = np.arange(n, dtype=np.int64) if mask is None else np.flatnonzero(np.asarray(mask, bool)[:n]).astype(np.int64)
    total = int(rows.size)
    taken = int(min(max(total - int(offset), 0), int(limit)))
    ids = np.full(int(limit), -1, np.int64)
    ids[:taken] = rows[int(offset):int(offset) + taken]
    return ids, total, taken


def select_batch(masks, n, offsets, limit):
    """(ids int64 [nq, limit], total int64 [nq], taken int32 [nq]) of a batch: what IcdIndex.select_rows returns"""
    nq = len(masks)
    ids = np.empty((nq, int(limit)), np.int64)
    total, taken = np.empty(nq, np.int64), np.empty(nq, np.int32)
    for q, m in enumerate(masks):
        ids[q], total[q], taken[q] = select(m, n, 0 if offsets is None else offsets[q], limit)
    return ids, total, taken
