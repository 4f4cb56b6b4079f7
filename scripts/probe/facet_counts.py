"""Probe of the facet counts over row masks, one MI355X. Two shapes:
  corpus   the 40 474 golden rows, 1 000 cached masks - mask_select.py's: `level >= L and code like "P%"` over the corpus's distinct
           three-character code prefixes, L in 1 .. 3 - counted per `category` and per `parent_code` (filter_expr.Columns.group_ids)
  shard    10 000 000 rows - section 19.7's shape - and 64 random masks of densities 1e-4 .. 0.5, counted per 1 000 groups in
           contiguous blocks of rows and per 20 000 hashed groups
For each, medians of 15 after 3 warm-up steps, the routes alternating step by step:
  device time              IcdIndex.group_counts(on_device=True) between two events: the memset and the launch
  wall (host outputs)      the same call with host outputs, as MilvusService.facet_batch makes it, ended by its own synchronisation
  host route, wall         what the parent had: IcdRowMask.words() per mask (icd_rowmask_read: a device synchronisation and n / 8
                           bytes to the host) plus numpy's unpackbits and bincount over the rows' group numbers
The two routes' counts are compared first. FC_LDS_GROUPS is a compile-time bound: build a second library with
`make -C rag_project_icd10_amd/csrc OUT=<dir> EXTRA=-DICD_FC_LDS_GROUPS=<bound>` and run the probe once per library
(ICD_SEARCH_LIB=<dir>/libicdsearch.so, --bound <bound> labels the log).
Usage: python scripts/probe/facet_counts.py [--bound N] >> profiles/facet_counts_probe.log"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from rag_project_icd10_amd import _native  # noqa: E402
from rag_project_icd10_amd.services import filter_expr as fe  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
STEPS, WARMUP = 15, 3


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def device(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def host_route(masks, dense_of, G):
    n = dense_of.size
    out = np.empty((len(masks), G), np.int32)
    for q, m in enumerate(masks):
        bits = np.unpackbits(m.words().view(np.uint8), bitorder="little")[:n]
        out[q] = np.bincount(dense_of[bits.view(bool)], minlength=G)
    return out


def show(name, ms, count):
    print(f"    {name}: median {np.median(ms):.3f} ms (min {np.min(ms):.3f}, max {np.max(ms):.3f}) for {count} masks", flush=True)


def run(index, masks, name, group_of, bound):
    grouping = index.grouping(group_of, max_nq=64)
    G = grouping.groups
    dense_of = np.unique(group_of, return_inverse=True)[1].reshape(-1)
    count = len(masks)
    got = index.group_counts(masks, grouping)
    want = host_route(masks, dense_of, G)
    assert got.dtype == want.dtype and np.array_equal(got, want) and np.array_equal(got, index.group_counts(masks, grouping, on_device=True).cpu().numpy())
    assert np.array_equal(got.sum(axis=1, dtype=np.int64), index.count_rows(masks))
    print(f"  {name}: G = {G} ({'LDS histogram' if G <= bound else 'global adds'} at FC_LDS_GROUPS = {bound}); the two routes agree on {count} masks, "
          f"non-zero groups per mask min {int((got > 0).sum(axis=1).min())}, median {int(np.median((got > 0).sum(axis=1)))}, max {int((got > 0).sum(axis=1).max())}")
    arms = {
        "device time": lambda: device(lambda: index.group_counts(masks, grouping, on_device=True)),
        "wall (host outputs)": lambda: wall(lambda: index.group_counts(masks, grouping)),
        "host route, wall (icd_rowmask_read + numpy)": lambda: wall(lambda: host_route(masks, dense_of, G)),
    }
    times = {k: [] for k in arms}
    for step in range(WARMUP + STEPS):
        for k, fn in arms.items():
            ms, _ = fn()
            if step >= WARMUP:
                times[k].append(ms)
    for k, ms in times.items():
        show(k, ms, count)
    grouping.close()


def main():
    import lzma
    import tempfile
    from rag_project_icd10_amd.tools.build_database import DatabaseBuilder
    ap = argparse.ArgumentParser()
    ap.add_argument("--bound", type=int, default=_native.FACET_LDS_GROUPS, help="the FC_LDS_GROUPS the loaded library was built with")
    ap.add_argument("--skip-shard", action="store_true")
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}; library {os.environ.get('ICD_SEARCH_LIB', _native.LIB_PATH)}; FC_LDS_GROUPS = {args.bound}; "
          f"segment {_native.SELECT_SEGMENT_ROWS} rows; medians of {STEPS} after {WARMUP} warm-up steps")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "ICD_10v601.csv")
        with open(path, "wb") as f:
            f.write(lzma.open(os.path.join(GOLDEN, "ICD_10v601.csv.xz")).read())
        recs = DatabaseBuilder.__new__(DatabaseBuilder).load_csv_data(path)
    n = len(recs)
    cols = fe.Columns.from_records(recs)
    prefixes = sorted({r["code"][:3] for r in recs})
    exprs = [f'level >= {lv} and code like "{p}%"' for lv in (1, 2, 3) for p in prefixes][:1000]
    assert len(exprs) == 1000
    rng = np.random.default_rng(0)
    index = _native.IcdIndex(rng.standard_normal((n, 32), dtype=np.float32), cols["level"].astype(np.int32), device=0, max_nq=1024, max_k=16, probe=False)
    masks = [index.rowmask(cols.select(e)) for e in exprs]
    print(f"corpus: n = {n} rows ({-(-n // _native.SELECT_SEGMENT_ROWS)} segments), {len(masks)} masks of {n // 8} bytes")
    for field in ("category", "parent_code"):
        run(index, masks, field, cols.group_ids(field)[0], args.bound)
    for m in masks:
        m.close()
    index.close()
    if args.skip_shard:
        return

    n = 10_000_000
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = torch.randn((n, 32), generator=g, device="cuda", dtype=torch.float32)
    index = _native.IcdIndex(rows, None, device=0, max_nq=1024, max_k=16, probe=False)
    del rows
    masks = []
    for q in range(64):
        density = (1e-4, 1e-2, 0.1, 0.5)[q % 4]
        keep = torch.rand(n, generator=g, device="cuda") < density
        masks.append(index.rowmask(torch.nonzero(keep).reshape(-1)))
    print(f"shard: n = {n} rows ({-(-n // _native.SELECT_SEGMENT_ROWS)} segments), {len(masks)} masks of {n // 8} bytes")
    r = np.arange(n, dtype=np.int64)
    run(index, masks, "1 000 groups in blocks of rows", (r // (n // 1000)).astype(np.int32), args.bound)
    run(index, masks, "20 000 hashed groups", (r * 2654435761 % 20000).astype(np.int32), args.bound)


if __name__ == "__main__":
    main()
