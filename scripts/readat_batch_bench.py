#!/usr/bin/env python3
"""Batched ReadNextAt on one GPU: rio_device_read_at_plan + rio_device_read_at_copy over random record starts of a
device-resident file. One JSON line per file, recorded and not gated.

Files: C2 (1 000 000 x 1 KiB text-like records, Snappy) and C1 (100 000 x 1 KiB ref-random records, uncompressed), as
bench.py generates them. Queries: 65 536 record starts drawn at random (with replacement) from the file.

batch      plan + copy between two device events on the context's stream, after a warm-up, the median of `--runs`
           runs; lookups/s and GiB/s of decoded bytes from it. The plan and the copy are also timed apart.
loop       rio_device_read_at over the first 1 024 of the same offsets: the one device path before the batch, a
           launch, a synchronise and a D2H of the result per record. per-record time x 65 536 is the comparison.
verified   the batch's statuses are all RIO_OK and its bytes equal the whole-file decode's records.

    python scripts/readat_batch_bench.py [--queries 65536] [--runs 20] [--warmup 3] [--loop 1024] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "go-sstables_amd"))

HOST_INDEX_LOOKUPS_PER_S = 29.5e6  # README: ReadNextAt from the reader's decoded index, 16 host threads


def one_file(name, n_rec, rec_len, comp, kind, args, torch, np, L, dev):
    from recordio import generate
    from recordio.device import DeviceDecoder, to_device_file

    lib, ctx = L.lib(), L.default_ctx(0)
    img = generate(n_rec, rec_len, comp, kind=kind, seed=1, threads=min(16, os.cpu_count() or 1))
    d_file, flen = to_device_file(img)
    b, info = DeviceDecoder(0).decode(d_file, flen)
    assert info["n_records"] == n_rec and info["status"] in L.EOF_CLASS, info
    starts, arena_off = b.rec_off[:n_rec], b.out_off[:n_rec + 1]
    q = args.queries
    pick = torch.from_numpy(np.random.default_rng(7).integers(0, n_rec, size=q)).to(dev)
    d_offs = starts[pick].contiguous()
    d_hits = torch.zeros(q * ctypes.sizeof(L.ReadAtHit), dtype=torch.uint8, device=dev)
    d_off = torch.zeros(q + 1, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(device=0)  # a stream of its own: the calls and the events that time them share it
    sp = ctypes.c_void_p(s.cuda_stream)
    torch.cuda.synchronize(0)

    def plan():
        rc = lib.rio_device_read_at_plan(ctx, d_file.data_ptr(), flen, d_offs.data_ptr(), q, d_hits.data_ptr(),
                                         d_off.data_ptr(), sp)
        assert rc == 0, rc

    plan()
    torch.cuda.synchronize(0)
    need = int(d_off[q].item())
    d_out = torch.zeros(need + L.RIO_DEVICE_PAD, dtype=torch.uint8, device=dev)

    def copy():
        rc = lib.rio_device_read_at_copy(ctx, d_file.data_ptr(), flen, q, d_hits.data_ptr(), d_off.data_ptr(),
                                         d_out.data_ptr(), need, sp)
        assert rc == 0, rc

    copy()
    torch.cuda.synchronize(0)
    # verified: against the whole-file decode
    hits = d_hits.cpu().numpy().view(np.dtype([("status", "<i4"), ("nil", "<i4"), ("len", "<u8"), ("d0", "<u8"),
                                               ("d1", "<u8"), ("hdr_len", "<u8"), ("payload_off", "<u8")]))
    lens = (arena_off[pick + 1] - arena_off[pick])
    ok = bool((hits["status"] == 0).all()) and bool((torch.from_numpy(hits["len"].astype(np.int64)).to(dev) == lens).all())
    idx = torch.repeat_interleave(arena_off[pick] - d_off[:q], lens) + torch.arange(need, device=dev)
    ok = ok and bool(torch.equal(b.out[idx], d_out[:need]))
    del idx

    def timed(fn):
        ms = []
        for i in range(args.warmup + args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            e1.synchronize()
            if i >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        return ms

    both = timed(lambda: (plan(), copy()))
    plan_ms, copy_ms = timed(plan), timed(copy)
    # the single-record device path, one call per offset
    offs = d_offs[:args.loop].cpu().numpy().astype(np.uint64)
    one = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    ln, nil = ctypes.c_uint64(), ctypes.c_int()
    for o in offs[:32]:
        lib.rio_device_read_at(ctx, d_file.data_ptr(), flen, int(o), one.data_ptr(), one.numel(), ctypes.byref(ln),
                               ctypes.byref(nil), None, None)
    t0 = time.perf_counter()
    for o in offs:
        rc = lib.rio_device_read_at(ctx, d_file.data_ptr(), flen, int(o), one.data_ptr(), one.numel(), ctypes.byref(ln),
                                    ctypes.byref(nil), None, None)
        assert rc == 0, rc
    per_rec_us = (time.perf_counter() - t0) / len(offs) * 1e6
    med = statistics.median(both)
    return {
        "file": name, "records": n_rec, "record_len": rec_len, "compression": comp, "queries": q, "decoded_bytes": need,
        "verified": ok, "runs": args.runs, "batch_ms_median": med, "batch_ms_min": min(both), "batch_ms_max": max(both),
        "plan_ms_median": statistics.median(plan_ms), "copy_ms_median": statistics.median(copy_ms),
        "lookups_per_s": q / (med * 1e-3), "decoded_gib_per_s": need / (med * 1e-3) / 2**30,
        "loop_records": len(offs), "loop_us_per_record": per_rec_us, "loop_ms_for_all_queries": per_rec_us * q * 1e-3,
        "batch_over_loop": per_rec_us * q * 1e-3 / med,
        "host_index_lookups_per_s": HOST_INDEX_LOOKUPS_PER_S,
        "batch_over_host_index": q / (med * 1e-3) / HOST_INDEX_LOOKUPS_PER_S,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop", type=int, default=1024)
    ap.add_argument("--out")
    args = ap.parse_args()
    import numpy as np
    import torch

    from recordio import _lib as L

    dev = "cuda:0"
    lines = [one_file("C2", 1_000_000, 1024, 2, 1, args, torch, np, L, dev),
             one_file("C1", 100_000, 1024, 0, 0, args, torch, np, L, dev)]
    text = "\n".join(json.dumps(ln) for ln in lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
