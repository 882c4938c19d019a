#!/usr/bin/env python3
"""Bloom filters and point lookups on one GPU. Three parts, one JSON line:

compaction   the C5 table set of scripts/compact_bench.py (8 tables x 1.25M SHA1 keys x 1 KiB values, half of
             each table shared with the next; MergeCompact + ScanReduceLatestWins, Snappy out), run without and
             with the output table's filter in alternating steps of one process. The filter is sized as
             simpledb/compaction.go:79 sizes it: NewOptimal(total input records, 0.01). Stage milliseconds are
             intervals between HIP events recorded on the stream after each stage is enqueued; `bloom` (zero
             fill of the bits, upload of the hash keys, rio_sst_bloom_add) is an interval of its own between
             `gather` and `data_encode`.
flush        the 1M-op log of scripts/flush_bench.py (750 000 survivors), the same way; the filter is sized for
             the survivors (flush.go:35,55).
lookup       table 0 of the set (1.25M keys) with a filter built from its keys: rio_bloom_contains, and
             rio_sst_lookup gated and ungated, for 1M query keys of which half are in the table.

`atomics_per_s` = keys x k / the bloom interval. verified: the filter's bits fetched from the device equal the
host model's (numpy restatement of FNV-1 and the probes over the survivors' keys read back from the output
index), every hit vector equals the model's entry for entry, and the lookup's entries equal numpy's
searchsorted over the table's keys.

    python scripts/bloom_bench.py [--keys 1250000] [--tables 8] [--ops 1000000] [--queries 1000000]
                                  [--steps 5] [--warmup 2] [--out FILE]
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
STAGES_BLOOM = STAGES[:3] + ("bloom",) + STAGES[3:]
KEY_LEN = 20


def model_words(m, hash_keys, rows):
    """Bit words of a filter holding every row of `rows` (uint8 [n, key_len]): FNV-1, probes (h ^ key_j) mod m."""
    import numpy as np

    h = np.full(rows.shape[0], 0xCBF29CE484222325, dtype=np.uint64)
    for c in range(rows.shape[1]):
        h = (h * np.uint64(0x100000001B3)) ^ rows[:, c].astype(np.uint64)
    words = np.zeros((m + 63) // 64, dtype=np.uint64)
    for hk in hash_keys:
        idx = (h ^ np.uint64(hk)) % np.uint64(m)
        np.bitwise_or.at(words, (idx >> np.uint64(6)).astype(np.int64), np.uint64(1) << (idx & np.uint64(63)))
    return words, h


def model_hits(words, m, hash_keys, h):
    import numpy as np

    hit = np.ones(h.shape[0], dtype=bool)
    for hk in hash_keys:
        idx = (h ^ np.uint64(hk)) % np.uint64(m)
        hit &= ((words[(idx >> np.uint64(6)).astype(np.int64)] >> (idx & np.uint64(63))) & np.uint64(1)).astype(bool)
    return hit


def timed(run, stages, steps, warmup, torch, device):
    """Mean stage intervals of `steps` runs of run(mark) -> Compaction, after `warmup` unmarked runs."""
    for _ in range(warmup):
        c = run(None)
    torch.cuda.synchronize(device)
    per_step = []
    for _ in range(steps):
        ev = []

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append(e)

        mark("start")
        c = run(mark)
        torch.cuda.synchronize(device)
        assert len(ev) == len(stages) + 1, (len(ev), stages)
        per_step.append([ev[k].elapsed_time(ev[k + 1]) for k in range(len(stages))] + [ev[0].elapsed_time(ev[-1])])
    mean = [sum(s[k] for s in per_step) / len(per_step) for k in range(len(stages) + 1)]
    out = {k: round(v, 3) for k, v in zip(stages, mean)}
    out["whole"] = round(mean[-1], 3)
    out["whole_min"] = round(min(s[-1] for s in per_step), 3)
    out["whole_max"] = round(max(s[-1] for s in per_step), 3)
    return c, out


def output_keys(dec, lib, device, c, load_table, np):
    """The written table's keys, read back through the reader path: uint8 [n_out, KEY_LEN]."""
    dn, ixn = int(c.data_len.item()), int(c.index_len.item())
    out = load_table(dec, lib, device, c.index_img[:ixn].cpu().numpy(), c.data_img[:dn].cpu().numpy())
    key_off = out["key_off"][:out["n"]].cpu().numpy()
    arena = out["ib"].out[:out["index_bytes"]].cpu().numpy()
    return arena[key_off[:, None] + np.arange(KEY_LEN)[None, :]], out["n"]


def filter_section(c, ms, rows, n_rows, np):
    flt, d = c.bloom
    got = d.bits.cpu().numpy().view(np.uint64)
    want, _ = model_words(flt.m, flt.keys, rows)
    ok = n_rows == c.n_out and bool(np.array_equal(got, want))
    return {"m": flt.m, "k": flt.k, "filter_bytes": int(got.nbytes), "keys": c.n_out, "bloom_ms": ms["bloom"],
            "atomics_per_s": round(c.n_out * flt.k / (ms["bloom"] / 1e3)), "gather_ms": ms["gather"],
            "bloom_over_gather": round(ms["bloom"] / ms["gather"], 3), "bits_equal_model": ok}, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1_250_000)
    ap.add_argument("--tables", type=int, default=8)
    ap.add_argument("--ops", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    from compact_bench import load_table, table_images
    from memstore import flush_ops_on_device
    from recordio import _lib as L
    from recordio.device import DeviceDecoder
    from sstables import _WriterOpts, writer_filter
    from sstables.merger import compact_on_device

    n, nt, device = args.keys, args.tables, args.device
    dev = f"cuda:{device}"
    lib = L.lib()
    dec = DeviceDecoder(device)
    res = {"bench": "bloom", "steps": args.steps, "warmup": args.warmup}
    all_ok = True

    def new_filter(expected):
        f, err = writer_filter(_WriterOpts(basePath="bench", enableBloomFilter=True, bloomExpectedNumberOfElements=expected))
        if err is not None:
            raise err
        return f

    # ---- compaction -------------------------------------------------------------------------------------------
    t0 = time.time()
    half = n // 2
    universe = [hashlib.sha1(struct.pack(">I", i)).digest() for i in range(half * (nt - 1) + n)]
    values = [np.random.default_rng(1000 + t).integers(0, 256, 1024, dtype=np.uint8).tobytes() for t in range(nt)]
    tables, table0_keys = [], None
    for t in range(nt):
        keys = sorted(universe[t * half:t * half + n])
        if t == 0:
            table0_keys = np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(n, KEY_LEN)
        index_img, data_img = table_images(keys, values[t])
        tables.append(load_table(dec, lib, device, index_img, data_img))
    absent_keys = np.frombuffer(b"".join(hashlib.sha1(struct.pack(">I", (1 << 30) + i)).digest()
                                         for i in range(args.queries // 2)), dtype=np.uint8).reshape(-1, KEY_LEN)
    del universe
    gen_s = time.time() - t0
    views = (L.SstView * nt)(*[T["view"] for T in tables])
    n_in = sum(T["n"] for T in tables)

    def compaction(flt):
        def run(mark):
            c = compact_on_device(dec.ctx, device, views, L.RIO_MERGE_LATEST_WINS, L.COMP_SNAPPY, mark,
                                  flt=new_filter(n_in) if flt else None)
            if c.status is not None:
                raise RuntimeError(f"compaction refused: {c.status}")
            return c
        return run

    with torch.cuda.device(device), torch.cuda.stream(torch.cuda.Stream(device=device)):
        # two plain runs: the second against the first is the run-to-run spread of the stages that were there before
        _, plain_a = timed(compaction(False), STAGES, args.steps, args.warmup, torch, device)
        c, with_f = timed(compaction(True), STAGES_BLOOM, args.steps, args.warmup, torch, device)
        _, plain_b = timed(compaction(False), STAGES, args.steps, 1, torch, device)
        rows, n_rows = output_keys(dec, lib, device, c, load_table, np)
        sec, ok = filter_section(c, with_f, rows, n_rows, np)
        all_ok = all_ok and ok
        res["compaction"] = {"shape": f"{nt} tables x {n} keys x 1 KiB, half of each table shared with the next", "n_in": n_in,
                             "n_out": c.n_out, "expected_elements": n_in, "stage_ms_without_filter": plain_a,
                             "stage_ms_without_filter_again": plain_b, "stage_ms_with_filter": with_f, "filter": sec,
                             "generate_s": round(gen_s, 1)}
        del c, rows

        # ---- lookups on table 0 -------------------------------------------------------------------------------
        T = tables[0]
        nq = args.queries
        rng = np.random.default_rng(11)
        present = table0_keys[rng.integers(0, n, nq - absent_keys.shape[0])]
        q_rows = np.concatenate([present, absent_keys])[rng.permutation(nq)]
        f = new_filter(n)
        words, _ = model_words(f.m, f.keys, table0_keys)
        _, qh = model_words(2, [], q_rows)  # the queries' hashes
        want_hit = model_hits(words, f.m, f.keys, qh)
        fixed = np.dtype(f"S{KEY_LEN}")  # fixed-length byte strings order and compare as bytes.Compare does
        tk, qk = table0_keys.copy().view(fixed).ravel(), q_rows.copy().view(fixed).ravel()
        pos = np.searchsorted(tk, qk)
        found = (pos < n) & (tk[np.minimum(pos, n - 1)] == qk)
        want_entry = np.where(found, pos, -1).astype(np.int64)
        d_bits = torch.zeros((f.m + 63) // 64, dtype=torch.int64, device=dev)
        d_hk = torch.from_numpy(np.asarray(f.keys, dtype=np.uint64).view(np.int64).copy()).to(dev)
        bv = L.BloomView(bits=d_bits.data_ptr(), hash_keys=d_hk.data_ptr(), m=f.m, k=f.k)
        d_tk = torch.from_numpy(table0_keys.reshape(-1).copy()).to(dev)
        d_toff = torch.arange(n + 1, dtype=torch.int64, device=dev) * KEY_LEN
        d_q = torch.from_numpy(q_rows.reshape(-1).copy()).to(dev)
        d_qoff = torch.arange(nq + 1, dtype=torch.int64, device=dev) * KEY_LEN
        d_hit = torch.empty(nq, dtype=torch.uint8, device=dev)
        d_entry = torch.empty(nq, dtype=torch.int64, device=dev)
        d_pfx = torch.empty(n, dtype=torch.int64, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)

        def check(rc, what):
            if rc:
                raise RuntimeError(f"{what}: {L.strerror(rc)}")

        calls = {
            "add": lambda: check(lib.rio_bloom_add(dec.ctx, ctypes.byref(bv), d_tk.data_ptr(), d_toff.data_ptr(), n, n * KEY_LEN,
                                                   st), "rio_bloom_add"),
            "key_prefixes": lambda: check(lib.rio_sst_key_prefixes(dec.ctx, ctypes.byref(T["view"]), d_pfx.data_ptr(), st),
                                          "rio_sst_key_prefixes"),
            "contains": lambda: check(lib.rio_bloom_contains(dec.ctx, ctypes.byref(bv), d_q.data_ptr(), d_qoff.data_ptr(), nq,
                                                             nq * KEY_LEN, d_hit.data_ptr(), st), "rio_bloom_contains"),
            "lookup_gated": lambda: check(lib.rio_sst_lookup(dec.ctx, ctypes.byref(T["view"]), d_pfx.data_ptr(), ctypes.byref(bv),
                                                             d_q.data_ptr(), d_qoff.data_ptr(), nq, nq * KEY_LEN,
                                                             d_entry.data_ptr(), st), "rio_sst_lookup"),
            "lookup_ungated": lambda: check(lib.rio_sst_lookup(dec.ctx, ctypes.byref(T["view"]), d_pfx.data_ptr(), None,
                                                               d_q.data_ptr(), d_qoff.data_ptr(), nq, nq * KEY_LEN,
                                                               d_entry.data_ptr(), st), "rio_sst_lookup"),
        }
        look = {"table_keys": n, "queries": nq, "present": int(found.sum()), "m": f.m, "k": f.k,
                "model_false_positives": int((want_hit & ~found).sum())}
        for name, call in calls.items():
            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize(device)
            ms = []
            for _ in range(args.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if name == "add":
                    d_bits.zero_()  # outside the interval: every step builds the filter from zero bits
                e0.record()
                call()
                e1.record()
                torch.cuda.synchronize(device)
                ms.append(e0.elapsed_time(e1))
            look[name + "_ms"] = round(sum(ms) / len(ms), 4)
            look[name + "_ms_min"] = round(min(ms), 4)
            if name == "add":
                ok = bool(np.array_equal(d_bits.cpu().numpy().view(np.uint64), words))
                look["add_atomics_per_s"] = round(n * f.k / (look["add_ms"] / 1e3))
            elif name == "contains":
                ok = bool(np.array_equal(d_hit.cpu().numpy().astype(bool), want_hit))
                look["contains_keys_per_s"] = round(nq / (look["contains_ms"] / 1e3))
            elif name == "lookup_gated":
                ok = bool(np.array_equal(d_entry.cpu().numpy(), np.where(want_hit, want_entry, -1)))
                look["lookup_gated_keys_per_s"] = round(nq / (look["lookup_gated_ms"] / 1e3))
            elif name == "lookup_ungated":
                ok = bool(np.array_equal(d_entry.cpu().numpy(), want_entry))
                look["lookup_ungated_keys_per_s"] = round(nq / (look["lookup_ungated_ms"] / 1e3))
            else:
                ok = True
            look[name + "_equals_model"] = ok
            all_ok = all_ok and ok
        res["lookup"] = look
        del tables, views, d_tk, d_q

        # ---- flush ------------------------------------------------------------------------------------------------
        no = args.ops
        rng = np.random.default_rng(7)
        fresh = np.arange(no) % 4 != 3
        made = np.cumsum(fresh)
        ids = np.where(fresh, made - 1, (rng.random(no) * np.maximum(made, 1)).astype(np.int64))
        n_keys = int(made[-1]) if no else 0
        digests = np.frombuffer(b"".join(hashlib.sha1(struct.pack(">I", i)).digest() for i in range(n_keys)),
                                dtype=np.uint8).reshape(n_keys, KEY_LEN)
        patterns = np.stack([np.random.default_rng(1000 + t).integers(0, 256, 1024, dtype=np.uint8) for t in range(8)])
        pad = torch.zeros(L.RIO_DEVICE_PAD, dtype=torch.uint8, device=dev)
        keys = torch.cat([torch.from_numpy(digests[ids].reshape(-1)).to(dev), pad])
        vals = torch.cat([torch.from_numpy(patterns).to(dev)[torch.arange(no, device=dev) % 8].reshape(-1), pad])
        key_off = torch.arange(no + 1, dtype=torch.int64, device=dev) * KEY_LEN
        val_off = torch.arange(no + 1, dtype=torch.int64, device=dev) * 1024
        flags = torch.zeros(no + 1, dtype=torch.uint8, device=dev)
        view = L.OpsView(keys=keys.data_ptr(), key_off=key_off.data_ptr(), values=vals.data_ptr(), val_off=val_off.data_ptr(),
                         flags=flags.data_ptr(), n=no, key_bytes=no * KEY_LEN, value_bytes=no * 1024)

        def flush(flt):
            def run(mark):
                c = flush_ops_on_device(dec.ctx, device, view, L.RIO_FLUSH_SKIP_TOMBSTONES, L.COMP_SNAPPY, mark,
                                        max_key_len=KEY_LEN, flt=new_filter(n_keys) if flt else None)
                if c.status is not None:
                    raise RuntimeError(f"flush refused: op {c.unsorted_table}")
                return c
            return run

        _, plain_a = timed(flush(False), STAGES, args.steps, args.warmup, torch, device)
        c, with_f = timed(flush(True), STAGES_BLOOM, args.steps, args.warmup, torch, device)
        _, plain_b = timed(flush(False), STAGES, args.steps, 1, torch, device)
        rows, n_rows = output_keys(dec, lib, device, c, load_table, np)
        sec, ok = filter_section(c, with_f, rows, n_rows, np)
        all_ok = all_ok and ok and c.n_out == n_keys
        res["flush"] = {"shape": f"{no} ops x {KEY_LEN}-byte SHA1 keys x 1 KiB values, every fourth op a rewrite", "n_out": c.n_out,
                        "expected_elements": n_keys, "stage_ms_without_filter": plain_a, "stage_ms_without_filter_again": plain_b,
                        "stage_ms_with_filter": with_f, "filter": sec}

    res["verified"] = bool(all_ok)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
