"""The look-ahead quad tests of the coarse sweep (csrc/coarse_flat_kernel.hpp, VAR bit 134217728): the
compares of a block of quads are issued ahead of the block's branches, so a quad may be appended from masks made against
a threshold that a compaction inside the block has since raised. That changes which candidates a list collects on its way,
never the top-k: every case runs in AUTO mode on the coarse path (dim 768, more than 16 queries) and is compared bit for
bit with the CPU oracle, on the shapes where the block walk could go wrong:
  - 129, 160 and 300 queries (partial waves and query tiles);
  - 128 m + 1 and 128 m + 127 rows for m = 9, 23 (pad rows inside a block of quads, one row or all but one of the last tile);
  - 12 000 rows (lists long enough to leave the bootstrap tiles: compactions fall inside blocks);
  - k = 1, 10, 32;
  - 200 exact duplicates of one row, queries equal to it (ties at the threshold across a block);
  - 20 families x 64 near-identical rows (dense appends: compaction in the middle of a block);
  - the list plan of icd_index_set_chunks.
The lists may only collect MORE than before, so no more queries may miss the certificate than on the parent: PARENT holds
(last_fallback, last_second_pass) of index.stats() after the same search on commit d390c38, one fresh index per case."""
import numpy as np
import pytest

from bench import family_rows
from conftest import unit_rows

pytestmark = pytest.mark.gpu

from rag_project_icd10_amd._native import MODE_AUTO, IcdIndex  # noqa: E402

DIM = 768
NQ_MAX = 300
# (corpus kind, rows, queries, k, chunks override or 0)
CASES = [
    ("gauss", 128 * 9 + 1, 129, 10, 0),
    ("gauss", 128 * 9 + 1, 300, 32, 0),
    ("gauss", 128 * 9 + 127, 160, 1, 0),
    ("gauss", 128 * 9 + 127, 300, 10, 0),
    ("gauss", 128 * 23 + 1, 300, 32, 0),
    ("gauss", 128 * 23 + 1, 160, 10, 0),
    ("gauss", 128 * 23 + 127, 129, 10, 0),
    ("gauss", 128 * 23 + 127, 300, 1, 0),
    ("gauss", 12000, 300, 10, 0),
    ("gauss", 12000, 160, 32, 0),
    ("gauss", 12000, 129, 1, 0),
    ("gauss", 12000, 300, 10, 20),
    ("dups", 128 * 23 + 127, 160, 10, 0),
    ("dups", 128 * 23 + 127, 300, 32, 0),
    ("dups", 128 * 23 + 127, 129, 1, 0),
    ("family", 20 * 64, 300, 1, 0),
    ("family", 20 * 64, 300, 10, 0),
    ("family", 20 * 64, 160, 32, 0),
]
# commit d390c38, measured with this file's own searches: case -> (last_fallback, last_second_pass)
PARENT = {case: (0, 0) for case in CASES}   # (every case certified every query in its first pass)
_data = {}
_want = {}


def _levels(n):
    return (np.arange(n) * 2654435761 % 3 + 1).astype(np.int32)


def _make(kind, n):
    """(corpus, the NQ_MAX queries a case takes its first nq of), built once and never changed"""
    if (kind, n) not in _data:
        if kind == "family":
            corpus, queries = family_rows(20, 64, DIM, 0.10, NQ_MAX, 11)
            assert len(corpus) == n
        else:
            corpus, queries = unit_rows(n, DIM, 41 + n), unit_rows(NQ_MAX, DIM, 42)
            if kind == "dups":   # 200 copies of row 7 spread over the corpus (every block of quads of some tile holds one); a third of the queries ARE that row
                corpus = corpus.copy()
                corpus[np.arange(200) * (n // 200) + 3] = corpus[7]
                queries = queries.copy()
                queries[::3] = corpus[7]
        corpus.setflags(write=False)
        queries.setflags(write=False)
        _data[(kind, n)] = (corpus, queries)
    return _data[(kind, n)]


def _oracle(oracle, kind, n, k):
    if (kind, n, k) not in _want:
        corpus, queries = _make(kind, n)
        s, i = oracle.flat_ip_topk(corpus, queries, k)
        s.setflags(write=False)
        i.setflags(write=False)
        _want[(kind, n, k)] = (s, i)
    return _want[(kind, n, k)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_lookahead_select_is_exact(oracle, case):
    kind, n, nq, k, chunks = case
    corpus, queries = _make(kind, n)
    s_all, i_all = _oracle(oracle, kind, n, k)
    s_w, i_w = s_all[:nq], i_all[:nq]
    rw = oracle.reweight(s_w, i_w, _levels(n))
    idx = IcdIndex(corpus, _levels(n), max_nq=NQ_MAX, max_k=32)
    try:
        assert idx.stats()["fast_path"] == 1
        if chunks:
            idx.set_chunks(chunks)
        q = np.ascontiguousarray(queries[:nq])
        s, i = idx.search(q, k, MODE_AUTO)
        st = idx.stats()
        print(f"LOOKAHEAD {case!r}: ({st['last_fallback']}, {st['last_second_pass']}),   # lists {st['last_chunks']}")
        assert np.array_equal(i, i_w), f"id mismatch rows {np.nonzero((i != i_w).any(1))[0][:5]}"
        assert s.tobytes() == s_w.tobytes()
        adj, raw, ids, lv = idx.search_reweighted(q, k, MODE_AUTO)
        assert np.array_equal(ids, rw[2]) and adj.tobytes() == rw[0].tobytes() and raw.tobytes() == rw[1].tobytes()
        assert np.array_equal(lv, rw[3])
        assert st["last_mode"] == MODE_AUTO and st["last_nq"] == nq
        assert st["last_fallback"] <= PARENT[case][0]
        assert st["last_second_pass"] <= PARENT[case][1]
    finally:
        idx.close()
