"""Text -> sparse vectors for the sparse search: the analyzer and the BM25 weighting. Pure Python / numpy,
deterministic, no third-party segmenter. The device sees a plain sparse inner product; a caller with sparse vectors of its own
(SPLADE-style) skips this module and hands its CSR rows to IcdIndex.sparse.

Analyzer: NFKC, lower-case; every CJK character is a unigram and every adjacent pair of CJK characters a bigram; every maximal
run of ASCII letters or digits is one token, and a single '.' between two such runs joins them (`I10` and `E11.9` stay whole).
Everything else separates.

BM25 (Milvus's defaults k1 = 1.2, b = 0.75), in float64, rounded once to fp32:
    document weight  tf * (k1 + 1) / (tf + k1 * (1 - b + b * dl / avgdl))     at build time
    query weight     idf(t) * qtf,  idf = ln(1 + (N - df + 0.5) / (df + 0.5))  at call time
dl = tokens of the document, avgdl = their mean over the N documents (1.0 for a corpus without tokens). Operations in the order
written, ln = math.log.
"""
import math
import re
import unicodedata
from collections import Counter
from typing import Dict, Iterable, List, Sequence, Tuple

import numpy as np

K1 = 1.2
B = 0.75
MAX_QUERY_TERMS = 64   # include/icd_search.h ICD_SPARSE_MAX_QUERY_TERMS

_CJK = r"\u3400-\u4dbf\u4e00-\u9fff\uf900-\ufaff\U00020000-\U0003134f"
_TOKEN = re.compile(rf"([{_CJK}]+)|([a-z0-9]+(?:\.[a-z0-9]+)*)")


def analyze(text: str) -> List[str]:
    """The tokens of a text, in reading order (a CJK run: its unigrams, then its bigrams)"""
    out: List[str] = []
    for m in _TOKEN.finditer(unicodedata.normalize("NFKC", text or "").lower()):
        run = m.group(1)
        if run is None:
            out.append(m.group(2))
            continue
        out.extend(run)
        out.extend(run[i:i + 2] for i in range(len(run) - 1))
    return out


class SparseTextIndex:
    """Vocabulary, idf and the BM25 document vectors (CSR) of a corpus of texts"""

    def __init__(self, texts: Sequence[str]):
        counts = [Counter(analyze(t)) for t in texts]
        self.n = len(counts)
        self.vocab: List[str] = sorted(set().union(*counts)) if counts else []
        self.term_id: Dict[str, int] = {t: i for i, t in enumerate(self.vocab)}
        dl = np.array([sum(c.values()) for c in counts], np.float64)
        total = float(dl.sum())
        self.avgdl = total / self.n if total > 0 else 1.0
        df = np.zeros(len(self.vocab), np.int64)
        row_off = np.zeros(self.n + 1, np.int64)
        terms: List[int] = []
        vals: List[float] = []
        for i, c in enumerate(counts):
            ids = sorted(self.term_id[t] for t in c)
            for t in ids:
                tf = float(c[self.vocab[t]])
                df[t] += 1
                terms.append(t)
                vals.append(tf * (K1 + 1) / (tf + K1 * (1 - B + B * float(dl[i]) / self.avgdl)))
            row_off[i + 1] = len(terms)
        self.df = df
        self.idf = np.array([math.log(1 + (self.n - int(d) + 0.5) / (int(d) + 0.5)) for d in df], np.float64)
        self.row_off = row_off
        self.terms = np.asarray(terms, np.uint32)
        self.vals = np.asarray(vals, np.float64).astype(np.float32)

    @property
    def vocab_size(self) -> int:
        return max(len(self.vocab), 1)   # (an index needs a vocabulary of at least one term, used or not)

    def encode_query(self, text: str) -> Tuple[np.ndarray, np.ndarray]:
        """(terms uint32 ascending, weights float32) of a query text; terms outside the vocabulary are dropped. A query of more
        than MAX_QUERY_TERMS distinct terms keeps the heaviest (ties: the smaller term id)."""
        c = Counter(self.term_id[t] for t in analyze(text) if t in self.term_id)
        pairs = [(t, float(self.idf[t]) * float(qtf)) for t, qtf in c.items()]
        if len(pairs) > MAX_QUERY_TERMS:
            pairs = sorted(pairs, key=lambda p: (-p[1], p[0]))[:MAX_QUERY_TERMS]
        pairs.sort()
        t = np.array([p[0] for p in pairs], np.uint32)
        w = np.array([p[1] for p in pairs], np.float64).astype(np.float32)
        keep = w != 0   # (a weight that rounds to zero in fp32 is no pair)
        return t[keep], w[keep]

    def match_terms(self, terms: Iterable[str]) -> Tuple[np.ndarray, int]:
        """(known term ids uint32 ascending, |T|) of the distinct analysed terms T of a TEXT_MATCH predicate (DESIGN.md section
        17): terms outside the vocabulary are dropped for matching but still count in |T|. More than MAX_QUERY_TERMS known terms:
        ValueError - dropping any would change a set predicate."""
        distinct = set(analyze(terms)) if isinstance(terms, str) else set(terms)
        known = sorted(self.term_id[t] for t in distinct if t in self.term_id)
        if len(known) > MAX_QUERY_TERMS:
            raise ValueError(f"TEXT_MATCH: the text holds {len(known)} distinct known terms (at most {MAX_QUERY_TERMS})")
        return np.asarray(known, np.uint32), len(distinct)

    def match_rows(self, terms: Iterable[str], m=1) -> np.ndarray:
        """bool[n]: the rows that hold at least m of the distinct terms T (analysed term strings, or one text to analyse); m an int
        in 1 .. 64 or "all" = |T|, unknown terms included - an unknown term under "all" matches nothing. The host evaluation of
        TEXT_MATCH (filter_expr.Columns.set_text_matcher), over the rows' CSR."""
        known, total = self.match_terms(terms)
        need = total if m == "all" else m
        if isinstance(need, bool) or not isinstance(need, (int, np.integer)) or (m != "all" and not 1 <= need <= MAX_QUERY_TERMS):
            raise ValueError(f"minimum_should_match={m!r}: an int in 1 .. {MAX_QUERY_TERMS} or 'all'")
        if known.size == 0 or need > known.size or need < 1:
            return np.zeros(self.n, bool)
        hit = np.isin(self.terms, known)
        count = np.add.reduceat(np.append(hit, False).astype(np.int64), self.row_off[:-1]) if self.n else np.zeros(0, np.int64)
        count[self.row_off[:-1] == self.row_off[1:]] = 0   # (reduceat on an empty row reads its neighbour's first entry)
        return count >= need

    def encode_queries(self, texts: Iterable[str]):
        """CSR (q_off int64, q_terms uint32, q_vals float32) of several query texts"""
        enc = [self.encode_query(t) for t in texts]
        return csr_from_pairs(enc)


def csr_from_pairs(pairs: Sequence[Tuple[np.ndarray, np.ndarray]]):
    """[(terms, weights), ...] -> (off int64, terms uint32, vals float32)"""
    off = np.zeros(len(pairs) + 1, np.int64)
    for i, (t, _) in enumerate(pairs):
        off[i + 1] = off[i] + len(t)
    terms = np.concatenate([np.asarray(t, np.uint32) for t, _ in pairs]) if pairs else np.zeros(0, np.uint32)
    vals = np.concatenate([np.asarray(w, np.float32) for _, w in pairs]) if pairs else np.zeros(0, np.float32)
    return off, terms.astype(np.uint32), vals.astype(np.float32)


def query_from_dict(weights: Dict[int, float], vocab: int) -> Tuple[np.ndarray, np.ndarray]:
    """A {term_id: weight} dict as (terms ascending, weights): term ids in [0, vocab), weights finite and non-zero"""
    items = sorted((int(t), float(w)) for t, w in weights.items())
    if len(items) > MAX_QUERY_TERMS:
        raise ValueError(f"a sparse query carries at most {MAX_QUERY_TERMS} terms")
    for t, w in items:
        if not 0 <= t < vocab:
            raise ValueError(f"term {t} outside the vocabulary's [0, {vocab})")
        if not math.isfinite(w) or np.float32(w) == 0:
            raise ValueError(f"the weight of term {t} must be finite and non-zero")
    return np.array([t for t, _ in items], np.uint32), np.array([w for _, w in items], np.float32)


def text_match_expr(field: str, text: str, minimum_should_match=1) -> str:
    """The filter expression TEXT_MATCH(field, text, minimum_should_match=m) (services/filter_expr.py). minimum_should_match: an
    int in 1 .. 64, or "all": m = the number of distinct terms the analyzer makes of `text`, so that a caller need not count them
    (every term must then be in the row; a word the corpus does not know matches nothing)."""
    if minimum_should_match == "all":
        m = max(len(set(analyze(text))), 1)
    elif isinstance(minimum_should_match, bool) or not isinstance(minimum_should_match, (int, np.integer)):
        raise ValueError(f"minimum_should_match={minimum_should_match!r}: an int in 1 .. {MAX_QUERY_TERMS} or 'all'")
    else:
        m = int(minimum_should_match)
    if not 1 <= m <= MAX_QUERY_TERMS:
        raise ValueError(f"minimum_should_match={m}: must lie in 1 .. {MAX_QUERY_TERMS} (the text holds {len(set(analyze(text)))} distinct terms)")
    quoted = '"' + text.replace("\\", "\\\\").replace('"', '\\"') + '"'
    return f"TEXT_MATCH({field}, {quoted}, minimum_should_match={m})"
