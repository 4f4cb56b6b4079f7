"""Inputs shared by the tight-bound tests (test_tight_bound_gpu.py, test_tight_bound_cpu.py): dim 768, seeded, small.

Kinds: gauss (unit Gaussian rows), family (30 families x 124 near-identical rows in code order, bench.py's family_rows),
centred (rows sharing a common component: |mu|^2 = 0.36 of the mean squared norm, so the index centres its fp16 image),
tiny / huge (the Gaussian corpus scaled by 2^-20 / 2^20), dups (a fifth of the rows duplicated: exact ties at rank k)."""
import math

import numpy as np

from bench import family_rows
from conftest import unit_rows

DIM = 768
NQ = 300
KINDS = ("gauss", "family", "centred", "tiny", "huge", "dups")
_cache = {}


def _centred(n, seed):
    common = unit_rows(1, DIM, 900)[0]
    x = 0.8 * unit_rows(n, DIM, seed) + 0.6 * common[None, :]
    return np.ascontiguousarray(x, dtype=np.float32)


def make(kind):
    """(corpus, queries) of one kind, built once"""
    if kind in _cache:
        return _cache[kind]
    if kind == "family":
        corpus, queries = family_rows(30, 124, DIM, 0.10, NQ, 11)
    elif kind == "centred":
        corpus, queries = _centred(5000, 21), _centred(NQ, 22)
    else:
        corpus, queries = unit_rows(5000, DIM, 31), unit_rows(NQ, DIM, 32)
        if kind == "tiny":
            corpus = corpus * np.float32(2.0 ** -20)
        elif kind == "huge":
            corpus = corpus * np.float32(2.0 ** 20)
        elif kind == "dups":
            corpus = corpus.copy()
            corpus[5::5] = corpus[np.arange(5, 5000, 5) // 2]
    corpus.setflags(write=False)
    queries.setflags(write=False)
    _cache[kind] = (corpus, queries)
    return _cache[kind]


def scale_exp(m):
    return 1 - math.frexp(float(m))[1]   # m * 2^e in [1, 2)


def image(x):
    """fp16 image of already scaled float64 rows, and the residual norm per row the way convert_rows_kernel counts it (a
    component whose image is subnormal counts with the larger of its residual and itself)"""
    h = x.astype(np.float32).astype(np.float16).astype(np.float64)
    d = np.abs(x - h)
    d = np.where(np.abs(h) < 2.0 ** -14, np.maximum(d, np.abs(x)), d)
    return h, np.linalg.norm(d, axis=1)


def scaled(kind):
    """(q', c', cexp) in float64, scaled the way the library scales them: a power of two per query, ONE for the corpus, the
    column mean (float64 sum, rounded to fp32) subtracted in fp32 where the index would centre"""
    corpus, queries = make(kind)
    c = corpus.astype(np.float32)
    if kind == "centred":
        mu = c.mean(axis=0, dtype=np.float64).astype(np.float32)
        assert float(mu.astype(np.float64) @ mu) >= 0.25 * float((c.astype(np.float64) ** 2).sum(axis=1).mean())
        c = c - mu[None, :]   # (one fp32 subtraction per component, as the kernel does)
    cexp = scale_exp(np.abs(c).max())
    c = c.astype(np.float64) * 2.0 ** cexp
    q = queries.astype(np.float64)
    q = q * np.array([2.0 ** scale_exp(m) for m in np.abs(q).max(axis=1)])[:, None]
    return q, c, cexp
