"""The device-side rescoring of queries WITH NER entities (run with -m gpu on an MI355X): icd_hier_rescore_entities at
k = 1 ... 128 against the host method batch_calculate_similarities(query, entities, hits), byte-identical to
icd_hier_rescore when every entity list is empty; match_diagnoses_batch(..., entities=) against the one-at-a-time calls;
match_multiple_diagnoses with an NER service on the device path against the host path."""
import numpy as np
import pytest

import test_rescoring_gpu as tr
from test_entity_rescoring_cpu import _CHAPTERS, CHAPTERS, synthetic_entities
from test_rescoring_gpu import services  # noqa: F401  (the module-scoped fixture: synthetic encoder, 6 000- and 70-row stores)

pytestmark = pytest.mark.gpu

from rag_project_icd10_amd import _native  # noqa: E402
from rag_project_icd10_amd.services.hierarchical_similarity_service import SimilarityFactors  # noqa: E402


def _ca(table, code):
    c = code[:1]
    return table[13 + CHAPTERS.index(c)] if c and c in CHAPTERS else 0.0


@pytest.mark.parametrize("k,weights,id_base,nstr", tr.RESCORE_CASES)
def test_entity_rescoring_matches_host_at_every_k(k, weights, id_base, nstr):
    """icd_hier_rescore_entities against batch_calculate_similarities(text, entities, hits), string by string: final order,
    enhanced score, the record's score after the uncertainty boost, the boost, the six factors (bit for bit), -1 / -inf
    behind the hits; with every entity list empty, the same bytes as icd_hier_rescore"""
    import torch
    strings, hs, ids, adj, raw, nhit, (d_ids, d_adj, _d_raw), plain = tr._rescored(k, weights, id_base, nstr)
    ents = [synthetic_entities(i, s) for i, s in enumerate(strings)]
    tags = torch.from_numpy(np.asarray([hs.row_tag(c) for c in tr._row_codes()], np.uint8)).cuda()
    outs = hs.rescore_live_hits_batch(strings, d_adj, d_ids, tags, id_base=id_base, entities=ents)
    empty = hs.rescore_live_hits_batch(strings, d_adj, d_ids, tags, id_base=id_base, entities=[{} for _ in strings])
    torch.cuda.synchronize()
    for a, b in zip(empty, plain):
        assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    order, enh, score, vs, hb, boost = (t.cpu().numpy() for t in outs)
    codes = tr._row_codes()
    sc = 0.3 if hs.embedding_service else 0.5
    ca_winners = em_winners = 0
    for q, text in enumerate(strings):
        n = int(nhit[q])
        hits = []
        for j in range(n):
            r = int(ids[q, j]) - id_base
            code = codes[r] if 0 <= r < tr.NROWS else tr._outside_code(int(ids[q, j]))
            hits.append({"code": code, "title": f"合成{r}", "score": float(adj[q, j]), "original_score": float(raw[q, j]),
                         "metadata": {"level": 1 + r % 3, "parent_code": "", "category_path": "", "semantic_text": "",
                                      "has_complication": False, "main_code": "", "secondary_code": ""}})
        pos = {h["code"]: j for j, h in enumerate(hits)}
        want = hs.batch_calculate_similarities(text, ents[q], [dict(h) for h in hits])
        assert len(want) == n
        assert (order[q, n:] == -1).all() and (enh[q, n:] == -np.inf).all() and (score[q, n:] == -np.inf).all(), (text, n)
        assert (vs[q, n:] == 0).all() and (hb[q, n:] == 0).all() and (boost[q, n:] == 0).all(), (text, n)
        table = hs.query_params_entities(text, ents[q])
        for j, (rec, s_host, f_host) in enumerate(want):
            assert order[q, j] == pos[rec["code"]], (text, j)
            assert enh[q, j] == s_host == rec["enhanced_score"], (text, j)
            assert score[q, j] == rec["score"], (text, j)
            assert boost[q, j] == rec.get("uncertainty_boost", 0.0), (text, j)
            ca = _ca(table, rec["code"])
            assert SimilarityFactors(vs[q, j], hb[q, j], table[12], sc, ca, table[1]) == f_host, (text, j)
            ca_winners += ca > 0
            em_winners += table[12] > 0
    assert ca_winners > 0 and em_winners > 0, (ca_winners, em_winners)


def test_entity_rescoring_refuses_k_outside_1_to_128():
    import torch
    qp = torch.zeros((4, 22), dtype=torch.float64)
    tags = torch.zeros(16, dtype=torch.uint8, device="cuda")
    with pytest.raises(_native.IcdError, match="k=129"):
        _native.hier_rescore(torch.zeros((4, 129), dtype=torch.float64, device="cuda"),
                             torch.zeros((4, 129), dtype=torch.int64, device="cuda"), tags, qp, [0.2, 0.15, 0.08, 0.04, 0.03, 0.5, 0.045])


def _check_batch_with_entities(svc, md, ms, strings, top_k, ents):
    batched = md.match_diagnoses_batch(strings, top_k=top_k, confidence_statistics=True, entities=ents)
    assert len(batched) == len(strings) and all(m.candidates for m in batched)
    cs = md.confidence_service
    ca_winners = 0
    for i, s in enumerate(strings):
        hits = ms.search(svc["vecs"][i], top_k=2 * top_k)
        one = md._match_from_hits(s, hits, top_k, ents[i])
        got = batched[i]
        assert got.model_dump(exclude={"confidence_factors"}) == one.model_dump(exclude={"confidence_factors"}), (s, top_k)
        recs = [{"score": c.score} for c in one.candidates]
        cf = got.confidence_factors
        assert cf["model_uncertainty"] == cs._assess_model_uncertainty(recs), (s, top_k)
        assert cf["prediction_variance"] == cs._calculate_prediction_variance(None, recs), (s, top_k)
        ca_winners += sum(c.similarity_factors.category_alignment > 0 for c in got.candidates)
    assert ca_winners > 0
    return batched


@pytest.mark.parametrize("top_k", [1, 5, 32, 33, 50])
def test_match_diagnoses_batch_with_entities_equals_one_at_a_time(services, top_k):  # noqa: F811
    strings = services["strings"]
    ents = [synthetic_entities(i, s) for i, s in enumerate(strings)]
    _check_batch_with_entities(services, services["md"], services["ms"], strings, top_k, ents)


def test_match_diagnoses_batch_with_entities_on_a_70_row_store(services):  # noqa: F811
    strings = services["strings"]
    ents = [synthetic_entities(i, s) for i, s in enumerate(strings)]
    _check_batch_with_entities(services, services["md70"], services["ms70"], strings, 50, ents)


def _requests(strings):
    """multi-diagnosis texts of golden strings with chapter keywords, under the delimiters the splitter knows"""
    keyed = [s for s in strings if any(kw in s for _n, kws, _w in _CHAPTERS.values() for kw in kws)]
    out = [keyed[0], keyed[1] + "，" + keyed[2], "；".join(keyed[3:6]), "、".join(keyed[6:14]), strings[0], "疑似" + keyed[14]]
    return out


@pytest.mark.parametrize("ner_kind", ["rules", "synthetic_model"])
def test_match_multiple_diagnoses_with_ner_takes_the_device_path(services, ner_kind, monkeypatch):  # noqa: F811
    """with an NER service the request rescoring runs on the device (_match_from_hits, the host path's rescoring, raises if
    called) and gives what the host path gives (forced by supports_device_rescoring = lambda: False)"""
    from rag_project_icd10_amd.services.medical_ner_service import MedicalNERService
    from rag_project_icd10_amd.services.multi_diagnosis_service import MultiDiagnosisService
    if ner_kind == "rules":
        ner = MedicalNERService(use_model=False)
    else:
        monkeypatch.setenv("ICD_NER_ALLOW_SYNTHETIC", "1")
        ner = MedicalNERService()
        assert ner.synthetic and ner.ner_pipeline is not None
        # random weights seldom tag a chapter keyword: the seeded keyword entities are added to what the classifier finds
        one, many = ner.extract_medical_entities, ner.extract_medical_entities_batch

        def add(text, ents):
            out = {k: list(v) for k, v in ents.items()}
            for kind, lst in synthetic_entities(len(text), text).items():
                out.setdefault(kind, []).extend(lst)
            return out

        monkeypatch.setattr(ner, "extract_medical_entities", lambda t, **kw: add(t, one(t, **kw)))
        monkeypatch.setattr(ner, "extract_medical_entities_batch", lambda ts, **kw: [add(t, e) for t, e in zip(ts, many(ts, **kw))])
    es, ms = services["es"], services["ms"]
    texts = _requests(list(services["strings"]))
    md_dev = MultiDiagnosisService(es, ms, ner_service=ner)
    md_host = MultiDiagnosisService(es, ms, ner_service=ner)

    def boom(*a, **k):
        raise AssertionError("host rescoring called on the device path")

    monkeypatch.setattr(md_dev, "_match_from_hits", boom)
    assert ms.supports_device_rescoring()
    ca_winners = 0
    for top_k in (1, 5, 50):
        for text in texts:
            dev = md_dev.match_multiple_diagnoses(text, top_k=top_k)
            ms.supports_device_rescoring = lambda: False
            try:
                host = md_host.match_multiple_diagnoses(text, top_k=top_k)
            finally:
                del ms.supports_device_rescoring
            assert [m.model_dump() for m in dev["matches"]] == [m.model_dump() for m in host["matches"]], (text, top_k)
            assert {k: v for k, v in dev.items() if k != "matches"} == {k: v for k, v in host.items() if k != "matches"}
            assert dev["total_matches"] > 0
            ca_winners += sum(c.similarity_factors.category_alignment > 0 for m in dev["matches"] for c in m.candidates)
    assert ca_winners > 0
