#!/usr/bin/env python3
"""A/B of the hybrid and sparse entry points between two trees of this project on one MI355X (for a change that must not move
their speed): one process measures one tree and appends one JSON line of medians to --out.

  python scripts/probe/hybrid_sparse_ab.py --tree PARENT_CHECKOUT --label parent --out runs.jsonl    (built: make -C .../csrc)
  python scripts/probe/hybrid_sparse_ab.py --tree . --label result --out runs.jsonl
  ... alternating, several times each, then
  python scripts/probe/hybrid_sparse_ab.py --report runs.jsonl > profiles/NAME.log

ms; a figure is the process's median of 25 calls after 5 warm-up between hipEvents (device in / device out), or of 15 calls after
3 warm-up by wall clock with a device synchronisation on either side ("host" and "service" rows).
hybrid / fuse_lists rows: scripts/probe/hybrid_search.py's corpus (40 474 x 768 random unit rows), requests and k = 10, its (a)
rows at nq 1 / 16 / 1 000, (R, L) = (2, 10) and (8, 128); fuse_lists on random best-first lists of the same shape.
search_sparse rows: scripts/probe/sparse_search.py's index (the 40 474 golden titles, BM25) and queries (the golden diagnosis
strings), k = 10; range: radius 0.5; grouped: 997 groups, 5 groups x 2. service rows: MilvusService on the golden slice's store,
1 000 title queries through search_sparse_batch; 64 queries of one dense and one sparse request through hybrid_search_batch (RRF).
The report's verdict: the median of the result's medians against [min, max] of the parent's."""
import argparse
import csv
import io
import json
import lzma
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree")
ap.add_argument("--label")
ap.add_argument("--out")
ap.add_argument("--report")
args = ap.parse_args()
if args.report:
    runs = [json.loads(line) for line in open(args.report)]
    P, R = ([r for r in runs if r["label"] == lab] for lab in ("parent", "result"))
    print(f"parent and result alternating, {len(P)} and {len(R)} processes; ms, each figure a process's median (see scripts/probe/hybrid_sparse_ab.py)")
    count = {"inside": 0, "below": 0, "above": 0}
    for key in P[0]:
        if key == "label":
            continue
        p, q = [r[key] for r in P], [r[key] for r in R]
        med = statistics.median(q)
        verdict = "inside" if min(p) <= med <= max(p) else "below" if med < min(p) else "above"
        count[verdict] += 1
        print(f"{key:62s} | parent {min(p):8.4f} .. {max(p):8.4f} (median {statistics.median(p):8.4f}) | result {min(q):8.4f} .. {max(q):8.4f} "
              f"median {med:8.4f} {verdict}" + (f" by {med - max(p):.4f}" if verdict == "above" else ""))
    print(f"{count['inside']} rows inside the parent's spread, {count['below']} below, {count['above']} above")
    sys.exit(0)
sys.path.insert(0, os.path.abspath(args.tree))
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(REPO, "tests", "golden")
import torch  # noqa: E402
from rag_project_icd10_amd import _native  # noqa: E402
from rag_project_icd10_amd._native import IcdIndex  # noqa: E402
from rag_project_icd10_amd.services import sparse_text  # noqa: E402
assert os.path.abspath(_native.__file__).startswith(os.path.abspath(args.tree)), _native.__file__

res = {"label": args.label}

def ev_ms(f, steps=25, warm=5):
    for _ in range(warm): f()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record(); b.synchronize(); ts.append(a.elapsed_time(b))
    return statistics.median(ts)

def wall_ms(f, steps=15, warm=3):
    for _ in range(warm): f()
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); f(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)

# scripts/probe/hybrid_search.py's corpus and requests, its (a) rows
N, DIM, K = 40474, 768, 10
rng = np.random.default_rng(77)
corpus = rng.standard_normal((N, DIM), dtype=np.float32); corpus /= np.linalg.norm(corpus, axis=1, keepdims=True)
base = corpus[rng.integers(0, N, 1000)]
qb = np.repeat(base[:, None, :], 8, axis=1) + 0.1 * rng.standard_normal((1000, 8, DIM), dtype=np.float32)
index = IcdIndex(corpus, rng.integers(1, 4, N).astype(np.int32), max_nq=8000, max_k=128)
fusion = index.fusion(8000)
dq = torch.from_numpy(np.ascontiguousarray(qb, np.float32)).cuda()
for nq in (1, 16, 1000):
    for R, L in ((2, 10), (8, 128)):
        qs = dq[:nq, :R].contiguous()
        w = [1.0 / (r + 1) for r in range(R)]
        res[f"hybrid rrf nq={nq} R={R} L={L}"] = ev_ms(lambda: index.search_hybrid(qs, [L] * R, K, fusion, ranker="rrf"))
        res[f"hybrid weighted-atan nq={nq} R={R} L={L}"] = ev_ms(lambda: index.search_hybrid(qs, [L] * R, K, fusion, ranker="weighted", weights=w, norm="atan"))
        sc = torch.rand((nq, R, L), device="cuda").sort(dim=2, descending=True).values.contiguous()
        ids = torch.randint(0, N, (nq, R, L), device="cuda")
        res[f"fuse_lists rrf nq={nq} R={R} L={L}"] = ev_ms(lambda: index.fuse_lists(fusion, sc, ids, [L] * R, K))
# scripts/probe/sparse_search.py's index and queries, its (a) rows, and the host caller's form
titles = [r["disease"] for r in csv.DictReader(io.StringIO(lzma.open(os.path.join(GOLDEN, "ICD_10v601.csv.xz")).read().decode("utf-8-sig")))]
strings = [l.strip() for l in open(os.path.join(GOLDEN, "diagnosis_strings.txt"), encoding="utf-8") if l.strip()]
strings = (strings * (1000 // len(strings) + 1))[:1000]
tx = sparse_text.SparseTextIndex(titles)
sp = index.sparse(tx.row_off, tx.terms, tx.vals, tx.vocab_size, max_nq=1024, max_k=128)
q_all = tx.encode_queries(strings)
group_of = (np.arange(N) % 997).astype(np.int32)
grouping = index.grouping(group_of, max_nq=1024)
for nq in (1, 16, 1000):
    off = q_all[0][:nq + 1]
    hq = (off.copy(), q_all[1][:off[-1]].copy(), q_all[2][:off[-1]].copy())
    d = (torch.from_numpy(hq[0]).cuda(), torch.from_numpy(hq[1].view(np.int32)).cuda(), torch.from_numpy(hq[2]).cuda())
    res[f"search_sparse device nq={nq} k=10"] = ev_ms(lambda: index.search_sparse(sp, *d, 10, validate=False))
    res[f"search_sparse host nq={nq} k=10"] = wall_ms(lambda: index.search_sparse(sp, *hq, 10))
    res[f"search_sparse range device nq={nq} k=10"] = ev_ms(lambda: index.search_sparse(sp, *d, 10, validate=False, radius=0.5))
    res[f"search_sparse grouped device nq={nq} k=5x2"] = ev_ms(lambda: index.search_sparse(sp, *d, 5, validate=False, grouping=grouping, group_size=2))
for x in (grouping, sp, fusion, index): x.close()

# the service: search_sparse_batch (arrays and hit dicts) and a mixed hybrid_search_batch on the golden slice's store, 1 000 queries
os.environ.update(MILVUS_DB_PATH=tempfile.mkdtemp(), MILVUS_COLLECTION_NAME="icd10_ab", EMBEDDING_MODEL_NAME="shibing624/text2vec-base-chinese", ICD_EMBEDDING_ALLOW_SYNTHETIC="1")
from rag_project_icd10_amd.tools.build_database import DatabaseBuilder  # noqa: E402
from rag_project_icd10_amd.services import hybrid_search as hy  # noqa: E402
b = DatabaseBuilder(); b.initialize_services()
recs = b.load_csv_data(os.path.join(GOLDEN, "csv_slice.csv"))
assert b.vectorize_and_index(recs) is True
ms = b.milvus_service
sp2, tx2 = ms.build_sparse_index()
texts = [recs[i % len(recs)]["preferred_zh"] for i in range(1000)]
q = tx2.encode_queries(texts)
res["service search_sparse_batch nq=1000 k=10 arrays"] = wall_ms(lambda: ms.search_sparse_batch(*q, 10))
res["service search_sparse_batch nq=1000 k=10 as_dicts"] = wall_ms(lambda: ms.search_sparse_batch(*q, 10, as_dicts=True))
dim = ms._ready_index().dim
vec = np.random.default_rng(3).standard_normal((64, dim)).astype(np.float32)
reqs = [hy.AnnSearchRequest(vec, 10), hy.AnnSearchRequest(texts[:64], 10, anns_field="sparse")]
res["service hybrid_search_batch dense+sparse nq=64 as_dicts"] = wall_ms(lambda: ms.hybrid_search_batch(reqs, hy.RRFRanker(60), 10, as_dicts=True))
res["service hybrid_search_batch dense+sparse nq=64 grouped as_dicts"] = wall_ms(lambda: ms.hybrid_search_batch(reqs, hy.RRFRanker(60), 5, as_dicts=True, group_by_field="level", group_size=2))
ms.disconnect()
with open(args.out, "a") as f:
    f.write(json.dumps(res) + "\n")
print(json.dumps(res), flush=True)
