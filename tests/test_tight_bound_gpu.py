"""The certificate's measured error bound (csrc/cert_bound.hpp) on the GPU: a smaller window changes
which rows finalize rescans, never the top-k. Every result is compared bit for bit with the CPU oracle (flat_ip_topk +
reweight), as tests/test_gpu_parity.py does, on the shapes where the bound could go wrong: Gaussian unit rows, families
of near-identical rows, a centred image, rows scaled by 2^-20 and 2^20, duplicate rows (ties at rank k).

A tighter bound certifies at least what the looser one did, so no more queries may reach the exact re-search than on the
parent: PARENT_FALLBACK holds `last_fallback` of index.stats() after the same search on commit 101feda (the bound
1.2e-3 |q'| rmax'), one fresh index per case."""
import numpy as np
import pytest

import tight_bound_data as data

pytestmark = pytest.mark.gpu

from rag_project_icd10_amd._native import MODE_AUTO, IcdIndex  # noqa: E402

KS = (1, 10, 32)
# commit 101feda, measured with this file's own searches: (kind, k) -> last_fallback
PARENT_FALLBACK = {
    ("gauss", 1): 0, ("gauss", 10): 0, ("gauss", 32): 0,
    ("family", 1): 0, ("family", 10): 0, ("family", 32): 0,
    ("centred", 1): 0, ("centred", 10): 0, ("centred", 32): 0,
    ("tiny", 1): 0, ("tiny", 10): 0, ("tiny", 32): 0,
    ("huge", 1): 0, ("huge", 10): 0, ("huge", 32): 0,
    ("dups", 1): 0, ("dups", 10): 0, ("dups", 32): 0,
}
_want = {}


def _levels(n):
    return (np.arange(n) * 2654435761 % 3 + 1).astype(np.int32)


def _oracle(oracle, kind, k):
    if (kind, k) not in _want:
        corpus, queries = data.make(kind)
        s, i = oracle.flat_ip_topk(corpus, queries, k)
        _want[(kind, k)] = (s, i, oracle.reweight(s, i, _levels(len(corpus))))
    return _want[(kind, k)]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", data.KINDS)
def test_tight_bound_is_exact(oracle, kind, k):
    corpus, queries = data.make(kind)
    levels = _levels(len(corpus))
    s_w, i_w, rw = _oracle(oracle, kind, k)
    idx = IcdIndex(corpus, levels, max_nq=data.NQ, max_k=32)
    try:
        st0 = idx.stats()
        assert st0["fast_path"] == 1
        assert st0["centered"] == (1 if kind == "centred" else 0)
        s, i = idx.search(queries, k, MODE_AUTO)
        assert np.array_equal(i, i_w), f"id mismatch rows {np.nonzero((i != i_w).any(1))[0][:5]}"
        assert s.tobytes() == s_w.tobytes()
        adj, raw, ids, lv = idx.search_reweighted(queries, k, MODE_AUTO)
        st = idx.stats()
        print(f"FALLBACK {kind} {k} first={st['last_fallback']} second_pass={st['last_second_pass']} wide={st['wide_mode']}")
        assert np.array_equal(ids, rw[2]) and adj.tobytes() == rw[0].tobytes() and raw.tobytes() == rw[1].tobytes()
        assert np.array_equal(lv, rw[3])
        assert st["last_mode"] == MODE_AUTO
        assert st["last_fallback"] <= PARENT_FALLBACK[(kind, k)]
    finally:
        idx.close()


@pytest.mark.parametrize("kind", data.KINDS)
def test_measured_terms_match_an_independent_computation(kind):
    """What convert_rows_kernel measures - the norm and the fp16 residual norm of every query, the largest of both over the
    corpus - against numpy in float64 (tight_bound_data.image: the same rounding, the same rule for subnormal image
    components). The kernel's values must never be BELOW the float64 ones (they multiply an error bound) and are above by
    at most 1e-5: 22 fp32 roundings of a sum of positive terms (1.4e-6 of the square, half of that of the root), the root's
    ulp, and the factors 1 + 1e-6 / 1 + 2e-6 they are rounded up with - 3.1e-6 in all. A residual that left out the
    subnormal rule would be low by up to 4e-4 on the one row in ten that has such a component.
    The centred corpus is compared within 1e-3 instead: the library's column mean comes from its own fp32 summation, so a
    few components of c - mu round the other way."""
    corpus, queries = data.make(kind)
    q, c, cexp = data.scaled(kind)
    _, cres = data.image(c)
    _, qres = data.image(q)
    cmax, dcmax, qnorm = np.linalg.norm(c, axis=1).max(), cres.max(), np.linalg.norm(q, axis=1)
    idx = IcdIndex(corpus, _levels(len(corpus)), max_nq=data.NQ, max_k=32)
    try:
        idx.search(queries, 10, MODE_AUTO)
        t = idx.cert_terms(data.NQ)
    finally:
        idx.close()
    print(f"TERMS {kind} cexp {t['cexp']} cmax {t['cmax']:.8g} / {cmax:.8g} dcmax {t['dcmax']:.8g} / {dcmax:.8g} "
          f"qres ratio {float((t['qres'] / qres).min()):.8f} .. {float((t['qres'] / qres).max()):.8f} "
          f"qnorm ratio {float((t['qnorm'] / qnorm).min()):.8f} .. {float((t['qnorm'] / qnorm).max()):.8f}")
    assert t["cexp"] == cexp
    if kind == "centred":
        assert abs(t["cmax"] / cmax - 1) <= 1e-3 and abs(t["dcmax"] / dcmax - 1) <= 1e-3
    else:
        assert cmax <= t["cmax"] <= cmax * (1 + 1e-5)
        assert dcmax <= t["dcmax"] <= dcmax * (1 + 1e-5)
    assert (t["qres"] >= qres).all() and (t["qres"] <= qres * (1 + 1e-5)).all()
    assert (t["qnorm"] >= qnorm).all() and (t["qnorm"] <= qnorm * (1 + 1e-5)).all()
