"""Probe of the sparse range search, one MI355X: the 40 474 golden titles through the analyzer and BM25, the
golden diagnosis strings as queries, device in / device out, device bounds, hipEvents, median of 25 after 5 warm-up steps.
For nq 1 / 16 / 1 000 and k 10 / 128, in the same run: icd_sparse_search twice (the spread between two repetitions of the plain
call), a floor (radius = every query's rank-10 score), and a ceiling plus a cursor page (range_filter = the rank-200 score, after =
the last hit of the page under it); each banded time and its ratio to the first plain time.
Usage: python scripts/probe/sparse_range.py > profiles/sparse_range_probe.log"""
import csv
import io
import lzma
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from rag_project_icd10_amd import _native  # noqa: E402
from rag_project_icd10_amd.services import range_search, sparse_text  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def median_ms(fn, steps=25, warmup=5):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def score_at_rank(index, sp, q, rank):
    """every query's raw score at `rank` of its hit ranking (-inf where it has fewer hits), walked with cursor pages"""
    band = range_search.SparseBandIndex(index, sp, None)
    raw, _ids, _lv = (np.asarray(x) for x in range_search.search_band(band, q, 1, offset=rank)[1:])
    return raw[:, 0].astype(np.float32)


def main():
    titles = [r["disease"] for r in csv.DictReader(io.StringIO(lzma.open(os.path.join(GOLDEN, "ICD_10v601.csv.xz")).read().decode("utf-8-sig")))]
    strings = [l.strip() for l in open(os.path.join(GOLDEN, "diagnosis_strings.txt"), encoding="utf-8") if l.strip()]
    strings = (strings * (1000 // len(strings) + 1))[:1000]
    tx = sparse_text.SparseTextIndex(titles)
    rng = np.random.default_rng(0)
    n = len(titles)
    index = _native.IcdIndex(rng.standard_normal((n, 32), dtype=np.float32), rng.integers(1, 4, n).astype(np.int32), device=0, max_nq=1024,
                             max_k=128, probe=False)
    sp = index.sparse(tx.row_off, tx.terms, tx.vals, tx.vocab_size, max_nq=1024, max_k=128)
    print(f"n={n} {sp.stats()} tile={_native.sparse_tile_rows()}")
    q_all = tx.encode_queries(strings)
    _native.check_sparse_rows(*q_all, tx.vocab_size, 64, "query")
    floor_all, ceil_all = score_at_rank(index, sp, q_all, 9), score_at_rank(index, sp, q_all, 199)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for nq in (1, 16, 1000):
        off = q_all[0][:nq + 1]
        q = (off, q_all[1][:off[-1]], q_all[2][:off[-1]])
        dq = (dev(off), dev(q[1].view(np.int32)), dev(q[2]))
        for k in (10, 128):
            floor, ceil = floor_all[:nq].copy(), ceil_all[:nq].copy()
            ceil[np.isneginf(ceil)] = np.inf   # (fewer than 200 hits: no ceiling)
            raw, ids, _ = index.search_sparse(sp, *q, k, range_filter=ceil)
            sc, cid = range_search._cursor_of(np.asarray(raw), np.asarray(ids), k)
            d_floor, d_ceil, d_after = dev(floor), dev(ceil), (dev(sc), dev(cid))
            plain = median_ms(lambda: index.search_sparse(sp, *dq, k, validate=False))
            again = median_ms(lambda: index.search_sparse(sp, *dq, k, validate=False))
            a = median_ms(lambda: index.search_sparse(sp, *dq, k, validate=False, radius=d_floor))
            b = median_ms(lambda: index.search_sparse(sp, *dq, k, validate=False, range_filter=d_ceil, after=d_after))
            print(f"nq={nq} k={k}: icd_sparse_search {plain:.3f} ms, repeated {again:.3f} ms (x{again / plain:.3f}); radius at rank 10 {a:.3f} ms "
                  f"(x{a / plain:.3f}); range_filter at rank 200 + after page {b:.3f} ms (x{b / plain:.3f})")
    sp.close()
    index.close()


if __name__ == "__main__":
    main()
