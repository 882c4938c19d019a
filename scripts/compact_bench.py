#!/usr/bin/env python3
"""Compaction of the C5 table set on one GPU: 8 tables x 1.25M SHA1 keys x 1 KiB values with overlapping
key ranges (table t holds the keys of indices [t * n / 2, t * n / 2 + n): half of each table is shared with
the next one), MergeCompact + ScanReduceLatestWins, Snappy data file out. Prints one JSON line: per-stage
milliseconds between HIP events recorded on the stream after each stage is enqueued (plan, gather, data
encode, index entries, index encode), the two host round trips between them as intervals of their own
(`host_gap_ms`: the stream idles while the host reads the plan's result block and the entries arena's
length), the whole sequence from the first event to the last (host gaps included), GiB/s of input table
bytes over that whole, and `verified`.

verified: the two output files are decoded and CRC-validated by the device reader path (rio_device_decode,
rio_sst_index_parse, rio_sst_validate: every entry in the writer's layout, every value's CRC-64 equal to
its entry's checksum), and a SHA-1 over (key, value) of the keys whose first byte is a multiple of 64 (a
1/64 sample of SHA1 keys) equals the host model's: sorted sampled keys, each with the value of the
highest table that holds it.

    python scripts/compact_bench.py [--keys 1250000] [--tables 8] [--steps 5] [--warmup 2]
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

# events in the order compact_on_device records them; the two *_read intervals are host round trips (the
# stream idles while the host reads 64 and 8 bytes), kept apart from the stages that follow them
STAGES = ("plan", "result_read", "gather", "data_encode", "index_entries", "entries_length_read", "index_encode")
HOST_GAPS = ("result_read", "entries_length_read")


def table_images(key_rows, value):
    """data.rio (Snappy v4) and index.rio (uncompressed v4) as sstable_writer.go writes them for sorted
    20-byte keys that all carry `value` (bench.py's C5 generator with the keys given)."""
    import numpy as np

    from sstables.proto import encode_index_entry
    from sstables.writer import _Image, crc64_iso

    one = _Image(2)
    one.write(value)
    img = one.bytes()
    rec = img[8:]
    n = len(key_rows)
    data = np.frombuffer(img[:8] + rec * n, dtype=np.uint8)
    cs = crc64_iso(value)
    hdr = {}  # an uncompressed v4 record's header depends only on its length
    parts = [_Image(0).bytes()]
    for i, k in enumerate(key_rows):
        e = encode_index_entry(k, 8 + i * len(rec), cs)
        h = hdr.get(len(e))
        if h is None:
            w = _Image(0)
            w.write(e)
            h = hdr[len(e)] = w.bytes()[8:-len(e)]
        parts.append(h)
        parts.append(e)
    return np.frombuffer(b"".join(parts), dtype=np.uint8), data


def load_table(dec, lib, device, index_img, data_img):
    """The device side of NewSSTableReader: both files decoded, index parsed, values CRC-validated."""
    import torch

    from recordio import _lib as L
    from recordio.device import header_codec, to_device_file

    T = {}
    d_index, li = to_device_file(index_img, device)
    d_data, ld = to_device_file(data_img, device)
    T["ib"], ii = dec.decode(d_index, li, comp=header_codec(index_img))
    T["db"], di = dec.decode(d_data, ld, comp=header_codec(data_img))
    n = ii["n_records"]
    if ii["status"] not in L.EOF_CLASS or di["status"] not in L.EOF_CLASS or di["n_records"] != n:
        raise RuntimeError(f"table decode failed: {ii} {di}")
    i64 = dict(dtype=torch.int64, device=f"cuda:{device}")
    for k in ("key_off", "key_len", "value_off", "checksum", "crc"):
        T[k] = torch.empty(max(n, 1), **i64)
    pres, vres = torch.empty(2, **i64), torch.empty(2, **i64)
    st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    rc = lib.rio_sst_index_parse(dec.ctx, T["ib"].out.data_ptr(), T["ib"].out_off.data_ptr(), n, T["key_off"].data_ptr(),
                                 T["key_len"].data_ptr(), T["value_off"].data_ptr(), T["checksum"].data_ptr(),
                                 pres.data_ptr(), st)
    rc = rc or lib.rio_sst_validate(dec.ctx, T["db"].out.data_ptr(), T["db"].out_off.data_ptr(), T["db"].rec_off.data_ptr(),
                                    n, T["value_off"].data_ptr(), T["checksum"].data_ptr(), n, T["crc"].data_ptr(),
                                    vres.data_ptr(), st)
    torch.cuda.synchronize(device)
    if rc or int(pres[0].item()) != -1 or vres.tolist() != [-1, -1]:
        raise RuntimeError(f"table validation failed: rc {rc} {pres.tolist()} {vres.tolist()}")
    T["n"], T["index_bytes"], T["data_bytes"] = n, ii["total_out_bytes"], di["total_out_bytes"]
    T["view"] = L.SstView(index=T["ib"].out.data_ptr(), key_off=T["key_off"].data_ptr(), key_len=T["key_len"].data_ptr(),
                          data=T["db"].out.data_ptr(), data_off=T["db"].out_off.data_ptr(), flags=T["db"].flags.data_ptr(),
                          crc=T["crc"].data_ptr(), n=n, index_bytes=T["index_bytes"], data_bytes=T["data_bytes"])
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1_250_000)
    ap.add_argument("--tables", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch

    from recordio import _lib as L
    from recordio.device import DeviceDecoder
    from sstables.merger import compact_on_device

    n, nt, device = args.keys, args.tables, args.device
    lib = L.lib()
    dec = DeviceDecoder(device)
    t0 = time.time()
    half = n // 2
    universe = [hashlib.sha1(struct.pack(">I", i)).digest() for i in range(half * (nt - 1) + n)]
    values = [np.random.default_rng(1000 + t).integers(0, 256, 1024, dtype=np.uint8).tobytes() for t in range(nt)]
    tables, in_bytes, model = [], 0, {}
    for t in range(nt):
        keys = sorted(universe[t * half:t * half + n])
        index_img, data_img = table_images(keys, values[t])
        in_bytes += len(index_img) + len(data_img)
        tables.append(load_table(dec, lib, device, index_img, data_img))
        for k in keys:
            if k[0] % 64 == 0:
                model[k] = t  # list order is the context: the highest table wins
    del universe
    gen_s = time.time() - t0
    views = (L.SstView * nt)(*[T["view"] for T in tables])

    def run(marks=None):
        ev = []

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append(e)

        if marks is not None:
            mark("start")
        c = compact_on_device(dec.ctx, device, views, L.RIO_MERGE_LATEST_WINS, L.COMP_SNAPPY,
                              mark if marks is not None else None)
        if c.status is not None:
            raise RuntimeError(f"compaction refused: {c.status}")
        if marks is not None:
            marks.append(ev)
        return c

    # a real stream: events recorded on it bracket the stages
    with torch.cuda.device(device), torch.cuda.stream(torch.cuda.Stream(device=device)):
        for _ in range(args.warmup):
            c = run()
        torch.cuda.synchronize(device)
        per_step, wall = [], []
        for _ in range(args.steps):
            marks = []
            w0 = time.time()
            c = run(marks)
            torch.cuda.synchronize(device)
            wall.append((time.time() - w0) * 1e3)
            ev = marks[0]
            ms = [ev[k].elapsed_time(ev[k + 1]) for k in range(len(STAGES))]
            per_step.append(ms + [ev[0].elapsed_time(ev[-1])])
        mean = [sum(s[k] for s in per_step) / len(per_step) for k in range(len(STAGES) + 1)]

        # verification through the reader path
        dn, ixn = int(c.data_len.item()), int(c.index_len.item())
        out = load_table(dec, lib, device, c.index_img[:ixn].cpu().numpy(), c.data_img[:dn].cpu().numpy())
        ok = out["n"] == c.n_out
        key_off, key_len = out["key_off"][:out["n"]].cpu().numpy(), out["key_len"][:out["n"]].cpu().numpy()
        ok = ok and bool((key_len == 20).all())
        arena = out["ib"].out[:out["index_bytes"]].cpu().numpy()
        keys = arena[key_off[:, None] + np.arange(20)[None, :]]
        pick = np.nonzero(keys[:, 0] % 64 == 0)[0]
        doff = out["db"].out_off[:out["n"] + 1]
        pj = torch.from_numpy(pick).to(f"cuda:{device}")
        ok = ok and bool(((doff[pj + 1] - doff[pj]) == 1024).all().item())
        vals = out["db"].out[(doff[pj][:, None] + torch.arange(1024, device=f"cuda:{device}")[None, :])].cpu().numpy()
        got = hashlib.sha1()
        for r, j in enumerate(pick):
            got.update(keys[j].tobytes())
            got.update(vals[r].tobytes())
        want = hashlib.sha1()
        for k in sorted(model):
            want.update(k)
            want.update(values[model[k]])
        ok = ok and len(pick) == len(model) and got.hexdigest() == want.hexdigest()

    whole = mean[-1]
    res = {
        "bench": "compaction", "shape": f"{nt} tables x {n} keys x 1 KiB, half of each table shared with the next",
        "mode": "LatestWins", "data_compression": "snappy", "n_in": sum(T["n"] for T in tables), "n_out": c.n_out,
        "value_bytes_out": c.value_bytes, "input_table_bytes": in_bytes, "output_table_bytes": dn + ixn,
        "stage_ms": {k: round(v, 3) for k, v in zip(STAGES, mean) if k not in HOST_GAPS},
        "host_gap_ms": {k: round(v, 3) for k, v in zip(STAGES, mean) if k in HOST_GAPS}, "whole_ms": round(whole, 3),
        "whole_ms_min": round(min(s[-1] for s in per_step), 3), "wall_ms": round(sum(wall) / len(wall), 3),
        "gib_per_s": round(in_bytes / 2**30 / (whole / 1e3), 2), "steps": args.steps, "warmup": args.warmup,
        "generate_s": round(gen_s, 1), "sample_keys": len(model), "verified": bool(ok),
    }
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
