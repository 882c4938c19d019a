#!/usr/bin/env python3
"""Memstore flush on one GPU: an op log of 1M ops with 20-byte SHA1 keys and 1 KiB values, every fourth op
rewriting an earlier key (750 000 survivors), flushed by memstore.flush_ops_on_device (Flush's mode: no
tombstones in this log), Snappy data file out. Prints one JSON line: per-stage milliseconds between HIP
events: inside the plan (rio_sst_flush_stage_ms: check, the length pass, each chunk pass, keep, crc), then
gather, data encode, index entries, index encode as scripts/compact_bench.py reports them, the two host
round trips as intervals of their own, the whole sequence, and `verified`.

verified: the two output files are decoded and CRC-validated by the device reader path (load_table of
compact_bench.py: every entry in the writer's layout, every value's CRC-64 equal to its entry's checksum),
the table holds one entry per distinct key, and a SHA-1 over (key, value) of the keys whose first byte is a
multiple of 64 equals the host model's: sorted sampled keys, each with the value of its last op.

    python scripts/flush_bench.py [--ops 1000000] [--steps 5] [--warmup 2]
"""
import argparse
import ctypes
import hashlib
import json
import os
import struct
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "go-sstables_amd"))
sys.path.insert(0, os.path.join(HERE, "scripts"))

STAGES = ("plan", "result_read", "gather", "data_encode", "index_entries", "entries_length_read", "index_encode")
HOST_GAPS = ("result_read", "entries_length_read")
KEY_LEN, VALUE_LEN, PATTERNS = 20, 1024, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch

    from compact_bench import load_table
    from memstore import flush_ops_on_device
    from recordio import _lib as L
    from recordio.device import DeviceDecoder

    n, device = args.ops, args.device
    dev = f"cuda:{device}"
    lib = L.lib()
    dec = DeviceDecoder(device)
    t0 = time.time()
    # op j writes a new key unless j % 4 == 3, which rewrites a key written before it
    rng = np.random.default_rng(7)
    fresh = np.arange(n) % 4 != 3
    made = np.cumsum(fresh)  # keys written up to and including op j
    ids = np.where(fresh, made - 1, (rng.random(n) * np.maximum(made, 1)).astype(np.int64))
    n_keys = int(made[-1]) if n else 0
    digests = np.frombuffer(b"".join(hashlib.sha1(struct.pack(">I", i)).digest() for i in range(n_keys)),
                            dtype=np.uint8).reshape(n_keys, KEY_LEN)
    patterns = np.stack([np.random.default_rng(1000 + t).integers(0, 256, VALUE_LEN, dtype=np.uint8) for t in range(PATTERNS)])
    last = np.full(n_keys, -1, dtype=np.int64)
    np.maximum.at(last, ids, np.arange(n))  # the last op of every key
    with torch.cuda.device(device):
        pad = torch.zeros(L.RIO_DEVICE_PAD, dtype=torch.uint8, device=dev)
        keys = torch.cat([torch.from_numpy(digests[ids].reshape(-1)).to(dev), pad])
        values = torch.cat([torch.from_numpy(patterns).to(dev)[torch.arange(n, device=dev) % PATTERNS].reshape(-1), pad])
        key_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * KEY_LEN
        val_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * VALUE_LEN
        flags = torch.zeros(n + 1, dtype=torch.uint8, device=dev)
    view = L.OpsView(keys=keys.data_ptr(), key_off=key_off.data_ptr(), values=values.data_ptr(), val_off=val_off.data_ptr(),
                     flags=flags.data_ptr(), n=n, key_bytes=n * KEY_LEN, value_bytes=n * VALUE_LEN)
    gen_s = time.time() - t0

    def run(marks=None):
        ev = []

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append(e)

        if marks is not None:
            mark("start")
        c = flush_ops_on_device(dec.ctx, device, view, L.RIO_FLUSH_SKIP_TOMBSTONES, L.COMP_SNAPPY,
                                mark if marks is not None else None, max_key_len=KEY_LEN)
        if c.status is not None:
            raise RuntimeError(f"flush refused: op {c.unsorted_table}")
        if marks is not None:
            marks.append(ev)
        return c

    chunks = (KEY_LEN + 7) // 8
    plan_stages = ["check", "sort_length"] + [f"sort_chunk{c}" for c in reversed(range(chunks))] + ["keep", "crc"]
    with torch.cuda.device(device), torch.cuda.stream(torch.cuda.Stream(device=device)):
        for _ in range(args.warmup):
            c = run()
        torch.cuda.synchronize(device)
        lib.rio_ctx_set_timing(dec.ctx, 1)  # the plan records its stage events
        per_step, plan_steps, wall = [], [], []
        for _ in range(args.steps):
            marks = []
            w0 = time.time()
            c = run(marks)
            torch.cuda.synchronize(device)
            wall.append((time.time() - w0) * 1e3)
            ev = marks[0]
            ms = [ev[k].elapsed_time(ev[k + 1]) for k in range(len(STAGES))]
            per_step.append(ms + [ev[0].elapsed_time(ev[-1])])
            buf = (ctypes.c_float * len(plan_stages))()
            got = lib.rio_sst_flush_stage_ms(dec.ctx, buf, len(plan_stages))
            plan_steps.append(list(buf)[:got])
        lib.rio_ctx_set_timing(dec.ctx, 0)
        mean = [sum(s[k] for s in per_step) / len(per_step) for k in range(len(STAGES) + 1)]
        plan_ok = all(len(p) == len(plan_stages) for p in plan_steps)
        plan_mean = [sum(p[k] for p in plan_steps) / len(plan_steps) for k in range(len(plan_stages))] if plan_ok else []

        # verification through the reader path
        dn, ixn = int(c.data_len.item()), int(c.index_len.item())
        out = load_table(dec, lib, device, c.index_img[:ixn].cpu().numpy(), c.data_img[:dn].cpu().numpy())
        ok = plan_ok and out["n"] == c.n_out == n_keys
        key_off_o, key_len_o = out["key_off"][:out["n"]].cpu().numpy(), out["key_len"][:out["n"]].cpu().numpy()
        ok = ok and bool((key_len_o == KEY_LEN).all())
        arena = out["ib"].out[:out["index_bytes"]].cpu().numpy()
        okeys = arena[key_off_o[:, None] + np.arange(KEY_LEN)[None, :]]
        pick = np.nonzero(okeys[:, 0] % 64 == 0)[0]
        doff = out["db"].out_off[:out["n"] + 1]
        pj = torch.from_numpy(pick).to(dev)
        ok = ok and bool(((doff[pj + 1] - doff[pj]) == VALUE_LEN).all().item())
        vals = out["db"].out[(doff[pj][:, None] + torch.arange(VALUE_LEN, device=dev)[None, :])].cpu().numpy()
        got = hashlib.sha1()
        for r, j in enumerate(pick):
            got.update(okeys[j].tobytes())
            got.update(vals[r].tobytes())
        sample = sorted((digests[i].tobytes(), int(last[i]) % PATTERNS) for i in np.nonzero(digests[:, 0] % 64 == 0)[0])
        want = hashlib.sha1()
        for k, p in sample:
            want.update(k)
            want.update(patterns[p].tobytes())
        ok = ok and len(pick) == len(sample) and got.hexdigest() == want.hexdigest()

    whole = mean[-1]
    stage_ms = {k: round(v, 3) for k, v in zip(plan_stages, plan_mean)}
    stage_ms.update({k: round(v, 3) for k, v in zip(STAGES, mean) if k not in HOST_GAPS and k != "plan"})
    log_bytes = n * (KEY_LEN + VALUE_LEN)
    res = {
        "bench": "memstore_flush", "shape": f"{n} ops x {KEY_LEN}-byte SHA1 keys x 1 KiB values, every fourth op a rewrite",
        "mode": "Flush", "data_compression": "snappy", "n_ops": n, "n_out": c.n_out, "value_bytes_out": c.value_bytes,
        "log_bytes": log_bytes, "output_table_bytes": dn + ixn, "sort_passes": chunks + 1, "stage_ms": stage_ms,
        "plan_ms": round(mean[0], 3), "host_gap_ms": {k: round(v, 3) for k, v in zip(STAGES, mean) if k in HOST_GAPS},
        "whole_ms": round(whole, 3), "whole_ms_min": round(min(s[-1] for s in per_step), 3),
        "wall_ms": round(sum(wall) / len(wall), 3), "gib_per_s": round(log_bytes / 2**30 / (whole / 1e3), 2),
        "steps": args.steps, "warmup": args.warmup, "generate_s": round(gen_s, 1), "sample_keys": len(sample),
        "verified": bool(ok),
    }
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
