"""Probe of the filter programs, one MI355X: the 40 474 golden rows' eight filter columns, 1 000 distinct
expressions in two groups of 500 -
  scalar    `level >= L and code like "P%"` over the corpus's distinct three-character code prefixes, L in 1 .. 3
  text      `code like "P%" or TEXT_MATCH(preferred_zh, "<golden diagnosis string>")`
Wall-clock medians of 15 after 3 warm-up steps, each ended by a device synchronisation (both routes hand finished masks to the
host), the two routes alternating step by step:
  compile         filter_expr.device_program over the group (parse included; the 512-entry parse cache does not hold 1 000)
  device          IcdIndex.filter_masks over the group's packed programs: one launch
  device + rows   ... and every mask's row count read back (IcdRowMask.stats), as the service does for scalar-only masks
  host            the parent's route: Columns.select (parse, numpy over all rows) + IcdIndex.rowmask per expression
The two routes' masks are compared word for word first.
Usage: python scripts/probe/filter_masks.py > profiles/filter_masks_probe.log"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from rag_project_icd10_amd import _native  # noqa: E402
from rag_project_icd10_amd.services import filter_expr as fe  # noqa: E402
from rag_project_icd10_amd.services import sparse_text  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
STEPS, WARMUP = 15, 3


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def show(name, ms, count):
    print(f"{name}: median {np.median(ms):.2f} ms (min {np.min(ms):.2f}, max {np.max(ms):.2f}) for {count} expressions", flush=True)


def main():
    import lzma
    import tempfile
    from rag_project_icd10_amd.tools.build_database import DatabaseBuilder
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "ICD_10v601.csv")
        with open(path, "wb") as f:
            f.write(lzma.open(os.path.join(GOLDEN, "ICD_10v601.csv.xz")).read())
        recs = DatabaseBuilder.__new__(DatabaseBuilder).load_csv_data(path)
    strings = [l.strip() for l in open(os.path.join(GOLDEN, "diagnosis_strings.txt"), encoding="utf-8") if l.strip()]
    n = len(recs)
    cols = fe.Columns.from_records(recs)
    tx = sparse_text.SparseTextIndex([r["preferred_zh"] for r in recs])
    cols.set_text_matcher("preferred_zh", tx.match_rows)
    rng = np.random.default_rng(0)
    index = _native.IcdIndex(rng.standard_normal((n, 32), dtype=np.float32), cols["level"].astype(np.int32), device=0, max_nq=1024, max_k=128, probe=False)
    sp = index.sparse(tx.row_off, tx.terms, tx.vals, tx.vocab_size, max_nq=1024, max_k=128)
    t0 = time.perf_counter()
    dev = index.columns(cols.device_columns())
    print(f"n={n} columns {dev.stats()} built and uploaded in {(time.perf_counter() - t0) * 1e3:.1f} ms (once per store generation) "
          f"tile={_native.sparse_tile_rows()}", flush=True)
    prefixes = sorted({r["code"][:3] for r in recs})
    assert len(prefixes) >= 500
    text = {"preferred_zh": tx}
    groups = {
        "scalar": [f'level >= {1 + i % 3} and code like "{prefixes[i * len(prefixes) // 500]}%"' for i in range(500)],
        "text": [f'code like "{prefixes[i * len(prefixes) // 500]}%" or ' + sparse_text.text_match_expr("preferred_zh", strings[i % len(strings)][:24])
                 for i in range(500)],
    }
    for name, exprs in groups.items():
        assert len(set(fe.compile(e) for e in exprs)) == len(exprs)
        use_sp = sp if name == "text" else None

        def compile_all():
            return [fe.device_program(e, cols, text) for e in exprs]

        def device(progs, rows=False):
            masks = index.filter_masks(dev, use_sp, *fe.pack_programs(progs))
            if rows:
                for m in masks:
                    m.stats()
            return masks

        def host():
            return [index.rowmask(cols.select(e)) for e in exprs]

        progs = compile_all()
        assert all(p is not None for p in progs), "an expression of the probe was refused"
        a, b = device(progs, rows=True), host()
        counts = [m.rows for m in a]
        assert all(np.array_equal(x.words(), y.words()) for x, y in zip(a, b)) and counts == [m.rows for m in b]
        print(f"[{name}] the two routes' masks agree word for word; rows per mask: median {int(np.median(counts))} max {max(counts)} "
              f"empty {counts.count(0)}; program words: mean {np.mean([len(p) for p in progs]):.1f} max {max(len(p) for p in progs)}", flush=True)
        for m in a + b:
            m.close()
        t = {"compile": [], "device": [], "device + rows": [], "host": []}
        for step in range(WARMUP + STEPS):   # the routes alternate within every step
            ms_c, progs = timed(compile_all)
            ms_d, ma = timed(lambda: device(progs))
            ms_r, mr = timed(lambda: device(progs, rows=True))
            ms_h, mh = timed(host)
            for m in ma + mr + mh:
                m.close()
            if step >= WARMUP:
                for k, v in zip(t, (ms_c, ms_d, ms_r, ms_h)):
                    t[k].append(v)
        for k, v in t.items():
            show(f"[{name}] {k}", v, len(exprs))
        print(f"[{name}] device (compile + masks + rows) against host: {np.median(t['host']) / (np.median(t['compile']) + np.median(t['device + rows'])):.1f} x", flush=True)


if __name__ == "__main__":
    main()
