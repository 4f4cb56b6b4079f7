"""The sparse search's host side, no device: the analyzer, the BM25 weights, icd_sparse_pack and its
refusals, the host-only packer under the host sanitizers, AnnSearchRequest's anns_field."""
import os
import subprocess

import numpy as np
import pytest

import sparse_oracle as so
from rag_project_icd10_amd import _native
from rag_project_icd10_amd.services import sparse_text
from rag_project_icd10_amd.services.hybrid_search import AnnSearchRequest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TEXTS = ["2型糖尿病", "２型糖尿病　伴有并发症", "原发性高血压 I10", "E11.9, e11.9; Type-2 diabetes", "", "肺炎（未特指）", "糖尿病糖尿病", "a..b .5 x.y.z"]


def test_analyzer_on_fixed_strings():
    an = sparse_text.analyze
    assert an("") == [] and an(" ，。!? ") == []
    assert an("肺炎") == ["肺", "炎", "肺炎"]
    assert an("I10") == ["i10"] and an("E11.9") == ["e11.9"]
    assert an("E11.9,I10") == ["e11.9", "i10"]
    assert an("２型糖尿病") == ["2", "型", "糖", "尿", "病", "型糖", "糖尿", "尿病"]   # full-width digit -> ASCII, its own token
    assert an("Ｔｙｐｅ－２ DIABETES") == ["type", "2", "diabetes"]
    assert an("肺炎（未特指）x") == ["肺", "炎", "肺炎", "未", "特", "指", "未特", "特指", "x"]
    assert an("a..b .5 x.y.z") == ["a", "b", "5", "x.y.z"]
    assert an("高 血") == ["高", "血"]   # a separator breaks the pair
    for t in TEXTS:
        assert an(t) == so.analyze(t)


def test_bm25_weights_equal_the_oracle_bit_for_bit():
    ix = sparse_text.SparseTextIndex(TEXTS)
    vocab, row_off, terms, vals, idf = so.bm25(TEXTS)
    assert ix.vocab == vocab and ix.n == len(TEXTS)
    assert np.array_equal(ix.row_off, row_off) and np.array_equal(ix.terms, terms)
    assert ix.vals.dtype == np.float32 and ix.vals.tobytes() == vals.tobytes()
    assert ix.idf.tobytes() == idf.tobytes()
    _native.check_sparse_rows(ix.row_off, ix.terms, ix.vals, ix.vocab_size)
    for q in TEXTS + ["糖尿病 I10 unknown", "病病病"]:
        t, w = ix.encode_query(q)
        ot, ow = so.bm25_query(q, vocab, idf)
        assert np.array_equal(t, ot) and w.tobytes() == ow.tobytes()
    t, w = ix.encode_query("病病病")
    assert len(t) == 1 and w[0] == np.float32(ix.idf[t[0]] * 3.0)
    off, qt, qv = ix.encode_queries(["糖尿病", "", "I10"])
    assert off.tolist()[0] == 0 and off[2] == off[1] and off[-1] == len(qt) == len(qv)
    # one hand-computed weight: "肺炎（未特指）" has 8 tokens, tf("肺") = 1
    avgdl = sum(len(so.analyze(x)) for x in TEXTS) / len(TEXTS)
    want = np.float32(1 * 2.2 / (1 + 1.2 * (1 - 0.75 + 0.75 * 8 / avgdl)))
    row = 5
    at = int(row_off[row]) + [vocab[t] for t in terms[row_off[row]:row_off[row + 1]]].index("肺")
    assert ix.vals[at] == want


def test_query_longer_than_the_limit_keeps_the_heaviest_terms():
    texts = ["".join(chr(0x4E00 + i) for i in range(0, 80, 1)), "一"]
    ix = sparse_text.SparseTextIndex(texts)
    t, w = ix.encode_query(texts[0])
    assert len(t) == 64 and (np.diff(t.astype(np.int64)) > 0).all()
    ot, ow = so.bm25_query(texts[0], ix.vocab, ix.idf)
    assert np.array_equal(t, ot) and w.tobytes() == ow.tobytes()


def _random_rows(rng, n, vocab, density):
    row_off, terms, vals = [0], [], []
    for _ in range(n):
        t = np.flatnonzero(rng.random(vocab) < density)
        terms += t.tolist()
        vals += (rng.integers(1, 999, len(t)) / 16.0 * rng.choice([-1.0, 1.0], len(t))).tolist()
        row_off.append(len(terms))
    return np.array(row_off, np.int64), np.array(terms, np.uint32), np.array(vals, np.float32)


@pytest.mark.parametrize("n,vocab,density", [(1, 1, 1.0), (7, 1, 0.5), (100, 37, 0.1), (300, 5000, 0.002), (64, 5, 1.0), (9, 11, 0.0)])
def test_sparse_pack_equals_a_numpy_counting_sort(n, vocab, density):
    rng = np.random.default_rng(n * 1000 + vocab)
    row_off, terms, vals = _random_rows(rng, n, vocab, density)
    post_off, post_row, post_val = _native.sparse_pack(row_off, terms, vals, n, vocab)
    o_off, o_row, o_val = so.postings(row_off, terms, vals, vocab)
    assert np.array_equal(post_off, o_off) and np.array_equal(post_row, o_row) and post_val.tobytes() == o_val.tobytes()
    for t in range(min(vocab, 50)):
        assert (np.diff(post_row[post_off[t]:post_off[t + 1]].astype(np.int64)) > 0).all()


def test_sparse_pack_rejections():
    off = np.array([0, 2, 2, 3], np.int64)
    terms = np.array([1, 4, 0], np.uint32)
    vals = np.array([1.0, -2.0, 0.5], np.float32)
    _native.sparse_pack(off, terms, vals, 3, 5)
    bad = [
        (off, terms, vals, 3, 4, "vocabulary"),                                            # a term >= vocab
        (off, np.array([1, 1, 0], np.uint32), vals, 3, 5, "strictly increasing"),         # duplicate
        (off, np.array([4, 1, 0], np.uint32), vals, 3, 5, "strictly increasing"),         # unsorted
        (off, terms, np.array([1.0, 0.0, 0.5], np.float32), 3, 5, "non-zero"),
        (off, terms, np.array([1.0, np.nan, 0.5], np.float32), 3, 5, "finite"),
        (off, terms, np.array([np.inf, 1.0, 0.5], np.float32), 3, 5, "finite"),
        (np.array([0, 2, 1, 3], np.int64), terms, vals, 3, 5, "decrease"),
        (np.array([1, 2, 2, 3], np.int64), terms, vals, 3, 5, "start at 0"),
        (off, terms, vals, 2, 5, "offsets"),                                               # n does not match row_off
        (off, terms, vals, 3, 0, "vocab"),
    ]
    for o, t, v, n, vocab, word in bad:
        with pytest.raises(ValueError) as e:
            _native.sparse_pack(o, t, v, n, vocab)
        assert word in str(e.value), (word, str(e.value))
    # the C entry point itself: ICD_ERR_INVALID, and nothing written
    lib = _native.load_library()
    post_off = np.full(6, -7, np.int64)
    post_row = np.zeros(3, np.uint32)
    post_val = np.zeros(3, np.float32)
    dup = np.array([1, 1, 0], np.uint32)
    assert lib.icd_sparse_pack(off.ctypes.data, dup.ctypes.data, vals.ctypes.data, 3, 5, post_off.ctypes.data, post_row.ctypes.data, post_val.ctypes.data) == -1
    assert b"strictly increasing" in lib.icd_last_error() and (post_off == -7).all()
    assert lib.icd_sparse_pack(off.ctypes.data, terms.ctypes.data, vals.ctypes.data, 3, 5, None, post_row.ctypes.data, post_val.ctypes.data) == -1
    assert lib.icd_sparse_pack(off.ctypes.data, terms.ctypes.data, vals.ctypes.data, 1 << 31, 5, post_off.ctypes.data, post_row.ctypes.data, post_val.ctypes.data) == -1
    for name in ("check_sparse_rows",):
        with pytest.raises(ValueError):
            getattr(_native, name)(off, terms, vals, 5, max_terms=1, unit="query")
    assert _native.sparse_tile_rows() >= 256 and _native.sparse_tile_rows() & (_native.sparse_tile_rows() - 1) == 0
    # handles that are not: ICD_ERR_STATE before any device call
    assert lib.icd_sparse_destroy(None) == -5 and lib.icd_sparse_stats(None, None, None, None) == -5
    assert lib.icd_sparse_search(None, None, None, None, None, 1, 1, 0, None, 0, None, None, None, None, 0, None) == -5
    assert lib.icd_fusion_fuse_lists(None, None, None, None, 1, 1, 1, None, 0, 60.0, None, 0, 1, 0, None, None, None, None, None, 1, None) == -5


def test_oracle_search_equals_a_walk_over_row_dicts():
    """the vectorised oracle against the contract spelled out row by row: a dict per row, the query's terms in ascending order,
    np.float32 products and adds"""
    rng = np.random.default_rng(5)
    n, vocab = 60, 9
    row_off, terms, vals = _random_rows(rng, n, vocab, 0.4)
    vals[::3] = np.float32(1e8)
    vals[1::3] = np.float32(-1e8)
    q_off = np.array([0, 3, 3, 9], np.int64)
    q_terms = np.array([0, 4, 8, 0, 1, 2, 3, 4, 5], np.uint32)
    q_vals = np.array([1, -1, 1, 0.5, 1, 1, -2, 1, 3], np.float32)
    raw, ids, lv = so.search(row_off, terms, vals, vocab, q_off, q_terms, q_vals, 7)
    rows = so.rows_as_dicts(row_off, terms, vals)
    for q in range(3):
        scored = []
        for i, d in enumerate(rows):
            s, shared = np.float32(0.0), False
            for p in range(q_off[q], q_off[q + 1]):
                if int(q_terms[p]) in d:
                    s = np.float32(s + np.float32(q_vals[p] * d[int(q_terms[p])]))
                    shared = True
            if shared:
                scored.append((-float(s), i, s))
        scored.sort(key=lambda x: (x[0], x[1]))
        want = scored[:7]
        assert ids[q, :len(want)].tolist() == [w[1] for w in want] and (ids[q, len(want):] == -1).all()
        assert raw[q, :len(want)].tobytes() == np.array([w[2] for w in want], np.float32).tobytes()
        assert np.isneginf(raw[q, len(want):]).all() and (lv[q, len(want):] == 0).all()


def test_host_packer_under_the_host_sanitizers(tmp_path):
    """tests/sparse_pack_check.cpp: the host-only header that holds the packer, in a program of its own, with ASan and UBSan"""
    exe = str(tmp_path / "sparse_pack_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "rag_project_icd10_amd", "csrc"), os.path.join(ROOT, "tests", "sparse_pack_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sparse pack cases ok" in out.stdout


def test_ann_search_request_anns_field():
    dense = AnnSearchRequest(np.zeros(8, np.float32), 5)
    assert dense.anns_field == "vector"
    assert AnnSearchRequest("肺炎", 5, anns_field="sparse").anns_field == "sparse"
    assert AnnSearchRequest({3: 0.5, 7: 1.0}, 5, expr="level >= 2", anns_field="sparse").expr == "level >= 2"
    assert AnnSearchRequest(["肺炎", "I10"], 128, anns_field="sparse").limit == 128
    with pytest.raises(ValueError):
        AnnSearchRequest("肺炎", 5, anns_field="text")
    with pytest.raises(ValueError):
        AnnSearchRequest(np.zeros(8, np.float32), 5, anns_field="sparse")
    with pytest.raises(ValueError):
        AnnSearchRequest("肺炎", 5, param={"params": {"radius": 0.1}}, anns_field="sparse")
    with pytest.raises(ValueError):
        AnnSearchRequest("肺炎", 0, anns_field="sparse")
    with pytest.raises(TypeError):
        AnnSearchRequest("肺炎", 5, None, None, "sparse")   # keyword only: the positional signature is unchanged
    assert "anns_field='sparse'" in repr(AnnSearchRequest("肺炎", 5, anns_field="sparse")) and "anns_field='vector'" in repr(dense)
    from rag_project_icd10_amd.services import hybrid_search as hybrid
    assert hybrid.sparse_queries(AnnSearchRequest("肺炎", 5, anns_field="sparse")) == ["肺炎"]
    with pytest.raises(ValueError):   # the dense stack takes dense requests; the service routes sparse ones to the sparse index
        hybrid.stack_requests([dense, AnnSearchRequest("肺炎", 5, anns_field="sparse")])
    t, w = sparse_text.query_from_dict({7: 1.0, 3: 0.5}, 10)
    assert t.tolist() == [3, 7] and w.tolist() == [0.5, 1.0]
    for bad in ({10: 1.0}, {1: 0.0}, {1: float("nan")}, {i: 1.0 for i in range(65)}):
        with pytest.raises(ValueError):
            sparse_text.query_from_dict(bad, 10 if len(bad) < 65 else 100)
