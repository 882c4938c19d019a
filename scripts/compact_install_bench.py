#!/usr/bin/env python3
"""DB.Compact() with the compacted table installed from the merge's buffers in HBM against the same with reflect
forced to reload the table from its files. One database of --tables tables is built once; every
measured call runs on a fresh copy of it, opened with CompactOnDevice(), so each call merges the same inputs.

    python scripts/compact_install_bench.py [--tables 11] [--entries 20000] [--value-bytes 1024] [--repeats 5] [--warmup 1]

Prints one JSON line: per mode the median, the least and the most milliseconds of Compact(), and of its two halves
(execute: merge, encode, file writes; reflect: directory swap, the new reader, the new stack)."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "go-sstables_amd"))


def build(path, tables, entries, value_bytes, seed=1):
    import numpy as np

    import simpledb as DB

    rng = np.random.default_rng(seed)
    db, err = DB.NewSimpleDB(path, DB.MemstoreSizeBytes(1 << 40), DB.DisableCompactions())
    assert err is None and db.Open() is None
    space = 4 * entries  # keys overlap between tables: about a fifth of a table's keys is in the next one too
    for _ in range(tables):
        ids = rng.choice(space, size=entries, replace=False)
        values = rng.integers(0, 256, size=(entries, value_bytes), dtype=np.uint8)
        dead = rng.random(entries) < 0.1
        b = DB.WriteBatch()
        for i in range(entries):
            key = b"key%012d" % ids[i]
            if dead[i]:
                b.DeleteBytes(key)
            else:
                b.PutBytes(key, values[i].tobytes())
        assert db.Apply(b) is None
        assert db._rotate_wal_and_flush_memstore(compact=False) is None
    assert len(db.readers) == tables
    assert db.Close() is None


def one(template, install):
    import torch

    import simpledb as DB

    work = tempfile.mkdtemp(prefix="compact_bench_")
    try:
        path = os.path.join(work, "db")
        shutil.copytree(template, path)
        db, err = DB.NewSimpleDB(path, DB.CompactOnDevice(), DB.CompactionFileThreshold(1 << 30))
        assert err is None and db.Open() is None
        db.installCompactedFromDevice = install
        db.compactionFileThreshold = DB.NumSSTablesToTriggerCompaction
        n_in = len(db.readers)
        torch.cuda.synchronize(db.device)
        t0 = time.perf_counter()
        m, err = db._execute_compaction()
        torch.cuda.synchronize(db.device)
        t1 = time.perf_counter()
        assert err is None and m is not None and len(m.sstablePaths) == n_in, (m, err)
        err = db._reflect_compaction_result(m)
        torch.cuda.synchronize(db.device)
        t2 = time.perf_counter()
        assert err is None and len(db.readers) == 1, err
        n_out = db.readers[0].MetaData().numRecords
        db.compactionFileThreshold = 1 << 30
        assert db.Close() is None
        return (t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, n_out
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=11)
    ap.add_argument("--entries", type=int, default=20000)
    ap.add_argument("--value-bytes", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    root = tempfile.mkdtemp(prefix="compact_bench_template_")
    try:
        template = os.path.join(root, "db")
        os.mkdir(template)
        build(template, args.tables, args.entries, args.value_bytes)
        out = {"tables": args.tables, "entries_per_table": args.entries, "value_bytes": args.value_bytes,
               "repeats": args.repeats, "warmup": args.warmup}
        runs = {"hbm_install": [], "reload": []}
        for k in range(args.warmup + args.repeats):  # the two modes alternate, so drift touches both alike
            for mode, install in (("hbm_install", True), ("reload", False)):
                r = one(template, install)
                if k >= args.warmup:
                    runs[mode].append(r)
        for mode, rs in runs.items():
            out["records_out"] = rs[0][3]
            for j, part in enumerate(("compact_ms", "execute_ms", "reflect_ms")):
                xs = [r[j] for r in rs]
                out[f"{mode}_{part}"] = {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2),
                                         "max": round(max(xs), 2)}
        print(json.dumps(out))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
