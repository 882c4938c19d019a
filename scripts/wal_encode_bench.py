#!/usr/bin/env python3
"""Batched writes on one GPU: an op log of 1 M ops (16-byte keys, 1 KiB values, every eighth op a delete) that is
in HBM already, encoded into one WAL file image as simpledb.append_batch does it: rio_wal_ops_encode (length
pass + scan + result, then the two write launches), rio_device_encode (none and Snappy), and the image's copy to
page-locked host memory. Prints one JSON line: milliseconds per stage between stream events. The length pass and
scan are timed by a call without a record arena (records_cap = 0 launches no write kernel); "write" is the full
call minus that, a difference of two measured means, not an event pair of its own. The write kernels' GB/s counts
bytes read + bytes written, the figure scripts/wal_recover_bench.py prints for rio_wal_ops_gather (the same copy
shape), so the two lines compare directly.

In the same run the host route this replaces is timed on --host-ops ops of the same mix: the loop of
proto.marshal_upsert / marshal_delete + Appender.Append (code this feature does not touch), scaled per op.

verified: the result block's counts and byte total equal the closed form for the mix, and on the --host-ops ops
append_batch leaves the directory (names and bytes) the host loop leaves.

    python scripts/wal_encode_bench.py [--ops 1000000] [--steps 5] [--warmup 2] [--host-ops 50000]
"""
import argparse
import ctypes
import json
import os
import shutil
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "go-sstables_amd"))

KEY_LEN, VALUE_LEN, PATTERNS, DELETE_EVERY = 16, 1024, 8, 8
# addition { keyBytes, valueBytes }: 0a <1045> 1a 10 <key> 22 80 08 <value>; deleteTombStone { keyBytes }: 12 12 12 10 <key>
UPSERT_LEN, DELETE_LEN = 3 + 2 + KEY_LEN + 3 + VALUE_LEN, 2 + 2 + KEY_LEN


def source_tree_hash():
    """sha1 of the product sources, as bench.py's source_tree_hash: the tree a line was measured on."""
    import glob
    import hashlib

    h = hashlib.sha1()
    pats = [("go-sstables_amd", "csrc", "*.hip"), ("go-sstables_amd", "csrc", "*.cpp"), ("go-sstables_amd", "csrc", "*.h"),
            ("include", "*.h")]
    for f in sorted(sum((glob.glob(os.path.join(HERE, *p)) for p in pats), [])):
        h.update(os.path.relpath(f, HERE).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def device_log(torch, np, MS, device, n, seed):
    """The op log in HBM: op i deletes key i when i % DELETE_EVERY == DELETE_EVERY - 1, else upserts it."""
    dev = f"cuda:{device}"
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 256, (n, KEY_LEN), dtype=np.uint8)
    keys[:, :8] = np.arange(n, dtype=">u8").view(np.uint8).reshape(n, 8)
    patterns = np.stack([np.random.default_rng(1000 + t).integers(0, 256, VALUE_LEN, dtype=np.uint8) for t in range(PATTERNS)])
    is_del = (np.arange(n) % DELETE_EVERY) == DELETE_EVERY - 1
    up = np.nonzero(~is_del)[0]
    pad = torch.zeros(64, dtype=torch.uint8, device=dev)
    d_keys = torch.cat([torch.from_numpy(keys.reshape(-1)).to(dev), pad])
    d_values = torch.cat([torch.from_numpy(patterns).to(dev)[torch.from_numpy(up % PATTERNS).to(dev)].reshape(-1), pad])
    key_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * KEY_LEN
    val_off = torch.from_numpy(np.concatenate([[0], np.cumsum(np.where(is_del, 0, VALUE_LEN))]).astype(np.int64)).to(dev)
    flags = torch.from_numpy(np.concatenate([is_del.astype(np.uint8), [0]]).astype(np.uint8)).to(dev)
    n_del = int(is_del.sum())
    ops = MS.DeviceOps(device, d_keys, key_off, d_values, val_off, flags, n, n * KEY_LEN, (n - n_del) * VALUE_LEN, KEY_LEN)
    return ops, keys, patterns, is_del


def host_loop(np, P, W, R, L, path, keys, patterns, is_del, comp, max_size):
    """marshal + Append, record by record: -> marshal ms, append ms."""
    os.makedirs(path)
    opts, err = W.NewWriteAheadLogOptions(W.BasePath(path), W.MaximumWalFileSizeBytes(max_size),
                                          W.WriterFactory(lambda p: R.NewFileWriter(p, comp)))
    assert err is None, err
    a, err = W.NewAppender(opts)
    assert err is None, err
    kb = [keys[i].tobytes() for i in range(len(keys))]
    vals = [patterns[t].tobytes() for t in range(PATTERNS)]
    t0 = time.time()
    recs = [P.marshal_delete(kb[i]) if is_del[i] else P.marshal_upsert(kb[i], vals[i % PATTERNS]) for i in range(len(kb))]
    t1 = time.time()
    for r in recs:
        err = a.Append(r)
        assert err is None, err
    assert a.Close() is None
    return (t1 - t0) * 1e3, (time.time() - t1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=1_000_000)
    ap.add_argument("--host-ops", type=int, default=50_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch

    import memstore as MS
    import recordio as R
    import simpledb as DB
    import wal as W
    from recordio import _lib as L
    from simpledb import proto as P

    n, device = args.ops, args.device
    dev = f"cuda:{device}"
    lib = L.lib()
    ctx = L.default_ctx(device)
    with torch.cuda.device(device), torch.cuda.stream(torch.cuda.Stream(device=device)):
        t0 = time.time()
        ops, keys, patterns, is_del = device_log(torch, np, MS, device, n, 7)
        torch.cuda.synchronize(device)
        gen_s = time.time() - t0
        n_del = int(is_del.sum())
        total = (n - n_del) * UPSERT_LEN + n_del * DELETE_LEN
        rcap = int(lib.rio_wal_ops_encode_bound(n, ops.view.key_bytes, ops.view.value_bytes))
        records = torch.empty(rcap + L.RIO_DEVICE_PAD, dtype=torch.uint8, device=dev)
        rec_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        res = torch.empty(L.RIO_WALENC_RESULT_WORDS, dtype=torch.int64, device=dev)
        icap = max(int(lib.rio_encode_bound(n, total, c)) for c in (L.COMP_NONE, L.COMP_SNAPPY))
        img = torch.empty(icap, dtype=torch.uint8, device=dev)
        out_off, out_len = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
        host_img = torch.empty(icap, dtype=torch.uint8, pin_memory=True)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        view = ctypes.addressof(ops.view)

        def run():
            ev = []

            def mark(name):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                ev.append((name, e))

            def ok(rc):
                assert rc == L.RIO_OK, L.strerror(rc)

            mark("start")
            ok(lib.rio_wal_ops_encode(ctx, view, None, 0, rec_off.data_ptr(), res.data_ptr(), st))
            mark("len_scan")
            ok(lib.rio_wal_ops_encode(ctx, view, records.data_ptr(), rcap, rec_off.data_ptr(), res.data_ptr(), st))
            mark("encode_call")
            ok(lib.rio_device_encode(ctx, records.data_ptr(), rec_off.data_ptr(), None, n, total, L.COMP_NONE, img.data_ptr(),
                                     icap, out_off.data_ptr(), out_len.data_ptr(), st))
            mark("recordio_encode_none")
            ok(lib.rio_device_encode(ctx, records.data_ptr(), rec_off.data_ptr(), None, n, total, L.COMP_SNAPPY, img.data_ptr(),
                                     icap, out_off.data_ptr(), out_len.data_ptr(), st))
            mark("recordio_encode_snappy")
            flen = int(out_len.item())
            mark("length_read")
            host_img[:flen].copy_(img[:flen], non_blocking=True)
            mark("d2h")
            torch.cuda.synchronize(device)
            ms = {name: ev[k - 1][1].elapsed_time(e) for k, (name, e) in enumerate(ev) if k}
            ms["write"] = ms["encode_call"] - ms["len_scan"]
            return ms, flen

        for _ in range(args.warmup):
            run()
        steps = [run() for _ in range(args.steps)]
        flen = steps[-1][1]
        mean = {k: sum(s[0][k] for s in steps) / len(steps) for k in steps[0][0]}
        r = [x & 0xFFFFFFFFFFFFFFFF for x in res.cpu().tolist()]
        ok = r == [n, total, n - n_del, n_del, KEY_LEN, 0xFFFFFFFFFFFFFFFF, 0, 0]

        # the host route on the first --host-ops ops, and append_batch on the same ops
        m = min(args.host_ops, n)
        tmp = tempfile.mkdtemp(prefix="wal_encode_bench_")
        try:
            marshal_ms, append_ms = host_loop(np, P, W, R, L, os.path.join(tmp, "host"), keys[:m], patterns, is_del[:m],
                                              L.COMP_SNAPPY, 16 << 20)
            os.makedirs(os.path.join(tmp, "dev"))
            opts, _ = W.NewWriteAheadLogOptions(W.BasePath(os.path.join(tmp, "dev")), W.MaximumWalFileSizeBytes(16 << 20),
                                                W.WriterFactory(lambda p: R.NewFileWriter(p, L.COMP_SNAPPY)))
            a, err = W.NewAppender(opts)
            assert err is None, err
            batch = DB.WriteBatch()
            vals = [patterns[t].tobytes() for t in range(PATTERNS)]
            for i in range(m):
                batch.DeleteBytes(keys[i].tobytes()) if is_del[i] else batch.PutBytes(keys[i].tobytes(), vals[i % PATTERNS])
            w0 = time.time()
            _, err = DB.append_batch(a, batch, device)
            batch_ms = (time.time() - w0) * 1e3
            assert err is None and a.Close() is None, err
            names = sorted(os.listdir(os.path.join(tmp, "host")))
            ok = ok and names == sorted(os.listdir(os.path.join(tmp, "dev"))) and len(names) >= 2
            for name in names:
                x, y = (open(os.path.join(tmp, d, name), "rb").read() for d in ("host", "dev"))
                ok = ok and x == y
        finally:
            shutil.rmtree(tmp, ignore_errors=True)

    stage = lambda k: round(mean[k], 3)  # noqa: E731
    moved = n * KEY_LEN + (n - n_del) * VALUE_LEN
    host_us = (marshal_ms + append_ms) * 1e3 / m
    dev_ms = mean["encode_call"] + mean["recordio_encode_snappy"] + mean["length_read"] + mean["d2h"]
    out = {
        "bench": "wal_encode",
        "shape": f"{n} ops: {KEY_LEN}-byte keys x 1 KiB values, every {DELETE_EVERY}th op a delete; one WAL image",
        "n_ops": n, "record_bytes": total, "image_bytes_snappy": flen,
        "stage_ms": {"len_scan": stage("len_scan"), "write": stage("write"), "encode_call": stage("encode_call"),
                     "recordio_encode_none": stage("recordio_encode_none"), "recordio_encode_snappy": stage("recordio_encode_snappy"),
                     "length_read": stage("length_read"), "d2h_pinned": stage("d2h")},
        "write_copy_gb_per_s": round(2 * moved / 1e9 / (mean["write"] / 1e3), 1),
        "device_total_ms_snappy": round(dev_ms, 3),
        "host_route": {"ops": m, "marshal_ms": round(marshal_ms, 1), "append_ms": round(append_ms, 1),
                       "us_per_op": round(host_us, 2), "scaled_to_n_ms": round(host_us * n / 1e3, 1),
                       "append_batch_same_ops_wall_ms": round(batch_ms, 1)},
        "host_over_device": round(host_us * n / 1e3 / dev_ms, 1),
        "steps": args.steps, "warmup": args.warmup, "generate_s": round(gen_s, 1), "tree": source_tree_hash(),
        "verified": bool(ok),
    }
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
