#!/usr/bin/env python3
"""A stack of loaded tables on one GPU (rio_sst_stack_*, csrc/rio_stack.hip). One JSON line.

Shape: the C5 table set of scripts/compact_bench.py (T = 8 tables x 1.25M 20-byte SHA1 keys x 1 KiB values, half
of each table shared with the next, so a key's newest table is known from its number), every table with a filter
NewOptimal(keys, 0.01) built from its own keys, and 1M query keys in three mixes:
  newest       every query is a key of the newest table
  spread       the queries' newest tables are spread evenly over the T tables
  half_absent  half of the queries are in no table, the others spread evenly
lookup       per mix, gated and ungated: the fused rio_sst_stack_lookup, and in the same process what the library
             offered before it for the same question: T chained rio_sst_lookup launches, newest first, and a
             combine of their T result arrays (torch.where per table) into the stack's source words. The chain is
             timed whole, and its launches and its combine each alone, so the searches can be read without the
             combine's elementwise launches.
values       rio_sst_stack_value_plan and rio_sst_stack_value_copy over the `spread` mix's source words (every
             query found: queries x 1 KiB of values).
scan_range   a ScanRange over a tenth of the key space, stage by stage: bounds (both ends), their read-back,
             rio_sst_merge_plan over the cut views, the result read, rio_sst_merge_gather, rio_sst_keys_gather.
Intervals are between HIP events on the stream; every figure is the mean of --steps runs after --warmup runs,
with the smallest and largest run beside it. verified: the source words equal numpy's (searchsorted over each
table's keys and the construction's newest table), the chained baseline's equal them too, the gathered values and
the scan's keys equal the model's.

    python scripts/super_bench.py [--keys 1250000] [--tables 8] [--queries 1000000] [--steps 10] [--warmup 3]
                                  [--out FILE]
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

KEY_LEN = 20
VALUE_LEN = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1_250_000)
    ap.add_argument("--tables", type=int, default=8)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    from compact_bench import load_table, table_images
    from recordio import _lib as L
    from recordio.device import DeviceDecoder
    from sstables import bloom

    n, nt, nq, device = args.keys, args.tables, args.queries, args.device
    dev = f"cuda:{device}"
    lib = L.lib()
    dec = DeviceDecoder(device)
    BITS = L.RIO_MERGE_ENTRY_BITS
    fixed = np.dtype(f"S{KEY_LEN}")  # fixed-length byte strings order and compare as bytes.Compare does
    res = {"bench": "super", "steps": args.steps, "warmup": args.warmup, "library": os.path.basename(L.LIB_PATH),
           "shape": f"{nt} tables x {n} keys x {VALUE_LEN} B values, half of each table shared with the next; {nq} queries"}

    def check(rc, what):
        if rc:
            raise RuntimeError(f"{what}: {L.strerror(rc)}")

    def timed(call):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize(device)
        ms = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize(device)
            ms.append(e0.elapsed_time(e1))
        return {"ms": round(sum(ms) / len(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}

    # ---- the tables -------------------------------------------------------------------------------------------
    t0 = time.time()
    half = n // 2
    n_uni = half * (nt - 1) + n
    universe = np.frombuffer(b"".join(hashlib.sha1(struct.pack(">I", i)).digest() for i in range(n_uni)),
                             dtype=np.uint8).reshape(n_uni, KEY_LEN)
    values = [np.random.default_rng(1000 + t).integers(0, 256, VALUE_LEN, dtype=np.uint8).tobytes() for t in range(nt)]
    with torch.cuda.device(device), torch.cuda.stream(torch.cuda.Stream(device=device)):
        st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        tables, sorted_keys = [], []
        for t in range(nt):
            rows = universe[t * half:t * half + n]
            tk = np.sort(rows.copy().view(fixed).ravel())
            sorted_keys.append(tk)
            raw = tk.tobytes()  # element by element, numpy would strip a digest's trailing zero bytes
            index_img, data_img = table_images([raw[i:i + KEY_LEN] for i in range(0, n * KEY_LEN, KEY_LEN)], values[t])
            T = load_table(dec, lib, device, index_img, data_img)
            T["pfx"] = torch.empty(n, dtype=torch.int64, device=dev)
            check(lib.rio_sst_key_prefixes(dec.ctx, ctypes.byref(T["view"]), T["pfx"].data_ptr(), st), "rio_sst_key_prefixes")
            f, err = bloom.NewOptimal(n, 0.01)
            if err is not None:
                raise err
            T["filter"] = bloom.DeviceFilter(torch.zeros((f.m + 63) // 64, dtype=torch.int64, device=dev),
                                             torch.from_numpy(np.asarray(f.keys, dtype=np.uint64).view(np.int64).copy()).to(dev),
                                             f.m, f.k)
            d_tk = torch.from_numpy(np.frombuffer(tk.tobytes(), dtype=np.uint8).copy()).to(dev)
            d_toff = torch.arange(n + 1, dtype=torch.int64, device=dev) * KEY_LEN
            check(lib.rio_bloom_add(dec.ctx, T["filter"].ref(), d_tk.data_ptr(), d_toff.data_ptr(), n, n * KEY_LEN, st),
                  "rio_bloom_add")
            torch.cuda.synchronize(device)
            tables.append(T)
        res["generate_s"] = round(time.time() - t0, 1)
        res["filter"] = {"m": tables[0]["filter"].m, "k": tables[0]["filter"].k}

        views = (L.SstView * nt)(*[T["view"] for T in tables])
        pfx = (ctypes.c_uint64 * nt)(*[T["pfx"].data_ptr() for T in tables])
        filters = (L.BloomView * nt)(*[T["filter"].view for T in tables])
        stored = (ctypes.c_uint64 * nt)(*[T["checksum"].data_ptr() for T in tables])
        stack = ctypes.c_void_p()
        check(lib.rio_sst_stack_create(dec.ctx, ctypes.addressof(views), ctypes.addressof(pfx), ctypes.addressof(filters),
                                       ctypes.addressof(stored), nt, nq, ctypes.byref(stack), st), "rio_sst_stack_create")

        # ---- the query mixes: universe numbers (-1: absent), their newest table by construction ----------------
        rng = np.random.default_rng(11)
        absent = np.frombuffer(b"".join(hashlib.sha1(struct.pack(">I", (1 << 30) + i)).digest() for i in range(nq // 2)),
                               dtype=np.uint8).reshape(-1, KEY_LEN)

        def spread(count):  # universe numbers whose newest table is t, the same count for every t
            per = count // nt
            u = [rng.integers(t * half, (t + 1) * half if t < nt - 1 else n_uni, per) for t in range(nt)]
            u.append(rng.integers(0, half, count - per * nt))
            return np.concatenate(u)

        mixes = {"newest": rng.integers((nt - 1) * half, n_uni, nq), "spread": spread(nq),
                 "half_absent": np.concatenate([spread(nq - absent.shape[0]), np.full(absent.shape[0], -1)])}
        d_qoff = torch.arange(nq + 1, dtype=torch.int64, device=dev) * KEY_LEN
        d_src = torch.empty(nq, dtype=torch.int64, device=dev)
        d_entry = [torch.empty(nq, dtype=torch.int64, device=dev) for _ in range(nt)]
        all_ok = True
        res["lookup"] = {}
        kept_src = None
        for name, u in mixes.items():
            order = rng.permutation(nq)
            u = u[order]
            q_rows = np.where((u >= 0)[:, None], universe[np.maximum(u, 0)], 0)
            if name == "half_absent":
                q_rows[u < 0] = absent
            qk = q_rows.copy().view(fixed).ravel()
            newest = np.minimum(np.maximum(u, 0) // half, nt - 1)
            want = np.full(nq, -1, dtype=np.int64)
            for t in range(nt):
                sel = (u >= 0) & (newest == t)
                pos = np.searchsorted(sorted_keys[t], qk[sel])
                assert bool((sorted_keys[t][pos] == qk[sel]).all())
                want[sel] = (t << BITS) | pos
            d_q = torch.from_numpy(q_rows.reshape(-1).copy()).to(dev)
            sec = {"present": int((u >= 0).sum()), "per_table": np.bincount(newest[u >= 0], minlength=nt).tolist()}
            for gated in (0, 1):
                def fused():
                    check(lib.rio_sst_stack_lookup(stack, gated, d_q.data_ptr(), d_qoff.data_ptr(), nq, nq * KEY_LEN,
                                                   d_src.data_ptr(), st), "rio_sst_stack_lookup")

                chain_out = [None]

                def chain_lookups():  # what the library offered before: one launch per table, newest first
                    for t in range(nt - 1, -1, -1):
                        T = tables[t]
                        check(lib.rio_sst_lookup(dec.ctx, ctypes.byref(T["view"]), T["pfx"].data_ptr(),
                                                 T["filter"].ref() if gated else None, d_q.data_ptr(), d_qoff.data_ptr(), nq,
                                                 nq * KEY_LEN, d_entry[t].data_ptr(), st), "rio_sst_lookup")

                def combine():  # the T result arrays into the stack's source words (torch.where per table)
                    out = torch.full((nq,), -1, dtype=torch.int64, device=dev)
                    for t in range(nt - 1, -1, -1):
                        out = torch.where((out == -1) & (d_entry[t] != -1), d_entry[t] | (t << BITS), out)
                    chain_out[0] = out

                def chained():
                    chain_lookups()
                    combine()

                tag = "gated" if gated else "ungated"
                d_src.fill_(-7)
                f_ms = timed(fused)
                ok_f = bool(np.array_equal(d_src.cpu().numpy(), want))
                c_ms = timed(chained)
                ok_c = bool(np.array_equal(chain_out[0].cpu().numpy(), want))
                l_ms, k_ms = timed(chain_lookups), timed(combine)  # the chain's two parts, each timed alone
                sec[tag] = {"fused": f_ms, "fused_lookups_per_s": round(nq / (f_ms["ms"] / 1e3)), "chained": c_ms,
                            "chained_lookups_per_s": round(nq / (c_ms["ms"] / 1e3)), "chained_lookups_only": l_ms,
                            "chained_combine_only": k_ms, "chained_over_fused": round(c_ms["ms"] / f_ms["ms"], 3),
                            "chained_lookups_only_over_fused": round(l_ms["ms"] / f_ms["ms"], 3),
                            "fused_equals_model": ok_f, "chained_equals_model": ok_c}
                all_ok = all_ok and ok_f and ok_c
            if name == "spread":
                fused()
                kept_src = (d_src.clone(), newest.copy())
            res["lookup"][name] = sec
            del d_q

        # ---- values of the spread mix ---------------------------------------------------------------------------
        src, newest = kept_src
        status = torch.empty(nq, dtype=torch.uint8, device=dev)
        val_off = torch.empty(nq + 1, dtype=torch.int64, device=dev)
        total = nq * VALUE_LEN
        out = torch.empty(total + L.RIO_DEVICE_PAD, dtype=torch.uint8, device=dev)
        plan_ms = timed(lambda: check(lib.rio_sst_stack_value_plan(stack, src.data_ptr(), nq, 1, status.data_ptr(),
                                                                   val_off.data_ptr(), st), "rio_sst_stack_value_plan"))
        copy_ms = timed(lambda: check(lib.rio_sst_stack_value_copy(stack, src.data_ptr(), nq, val_off.data_ptr(),
                                                                   out.data_ptr(), total, st), "rio_sst_stack_value_copy"))
        vals = torch.from_numpy(np.frombuffer(b"".join(values), dtype=np.uint8).reshape(nt, VALUE_LEN).copy()).to(dev)
        ok = (int(val_off[nq].item()) == total and bool((status == L.RIO_GET_VALUE).all().item())
              and bool(torch.equal(out[:total].view(nq, VALUE_LEN), vals[torch.from_numpy(newest).to(dev)])))
        all_ok = all_ok and ok
        res["values"] = {"queries": nq, "value_bytes": total, "plan": plan_ms, "copy": copy_ms,
                         "copy_bytes_per_s": round(total / (copy_ms["ms"] / 1e3)),
                         "plan_and_copy_bytes_per_s": round(total / ((plan_ms["ms"] + copy_ms["ms"]) / 1e3)),
                         "equals_model": ok}
        del out, vals

        # ---- one ScanRange over a tenth of the key space ----------------------------------------------------------
        lo, hi = b"\x40" + b"\0" * (KEY_LEN - 1), b"\x59\x99" + b"\xff" * (KEY_LEN - 2)
        d_b = torch.from_numpy(np.frombuffer(lo + hi, dtype=np.uint8).copy()).to(dev)
        d_boff = torch.tensor([0, KEY_LEN, 2 * KEY_LEN], dtype=torch.int64, device=dev)
        pos = torch.empty(2 * nt, dtype=torch.int64, device=dev)
        stages = ("bounds", "bounds_read", "plan", "result_read", "gather", "keys_gather")
        i64 = lambda k: torch.empty(max(k, 1), dtype=torch.int64, device=dev)  # noqa: E731
        u8 = lambda k: torch.empty(max(k, 1), dtype=torch.uint8, device=dev)  # noqa: E731
        last = {}

        def scan(mark):
            check(lib.rio_sst_stack_bounds(stack, d_b.data_ptr(), d_boff.data_ptr(), 1, 2 * KEY_LEN, 0, pos.data_ptr(), st),
                  "rio_sst_stack_bounds")
            check(lib.rio_sst_stack_bounds(stack, d_b.data_ptr(), d_boff.data_ptr() + 8, 1, 2 * KEY_LEN, 1,
                                           pos.data_ptr() + 8 * nt, st), "rio_sst_stack_bounds")
            mark()
            h = pos.cpu().tolist()
            mark()
            cut = (L.SstView * nt)()
            for t in range(nt):
                a, b = h[t], max(h[t], h[nt + t])
                v = L.SstView.from_buffer_copy(views[t])
                v.key_off, v.key_len, v.data_off, v.crc = (p + 8 * a for p in (v.key_off, v.key_len, v.data_off, v.crc))
                v.flags = v.flags + a
                v.n = b - a
                cut[t] = v
            n_in = sum(v.n for v in cut)
            s, keep_, r = i64(n_in), u8(n_in), i64(L.RIO_MERGE_RESULT_WORDS)
            check(lib.rio_sst_merge_plan(dec.ctx, ctypes.addressof(cut), nt, L.RIO_MERGE_LATEST_WINS, s.data_ptr(),
                                         keep_.data_ptr(), r.data_ptr(), st), "rio_sst_merge_plan")
            mark()
            rr = r.cpu().tolist()
            mark()
            k, vb, kb = rr[L.RIO_MERGE_R_N_OUT], rr[L.RIO_MERGE_R_VALUE_BYTES], rr[L.RIO_MERGE_R_KEY_BYTES]
            out_src, voff, fl, koff = i64(k), i64(k + 1), u8(k), i64(k + 1)
            vv, kk = u8(vb + L.RIO_DEVICE_PAD), u8(kb + L.RIO_DEVICE_PAD)
            check(lib.rio_sst_merge_gather(dec.ctx, s.data_ptr(), keep_.data_ptr(), k, out_src.data_ptr(), vv.data_ptr(),
                                           vv.numel(), voff.data_ptr(), fl.data_ptr(), st), "rio_sst_merge_gather")
            mark()
            check(lib.rio_sst_keys_gather(dec.ctx, out_src.data_ptr(), k, kk.data_ptr(), kk.numel(), koff.data_ptr(), st),
                  "rio_sst_keys_gather")
            mark()
            last.update(n_in=n_in, n_out=k, value_bytes=vb, key_bytes=kb, keys=kk, unsorted=rr[L.RIO_MERGE_R_UNSORTED])

        for _ in range(args.warmup):
            scan(lambda: None)
        torch.cuda.synchronize(device)
        per = []
        for _ in range(args.steps):
            ev = []

            def mark():
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                ev.append(e)

            mark()
            scan(mark)
            torch.cuda.synchronize(device)
            per.append([ev[k].elapsed_time(ev[k + 1]) for k in range(len(stages))] + [ev[0].elapsed_time(ev[-1])])
        uk = universe.copy().view(fixed).ravel()
        inside = np.sort(uk[(uk >= np.bytes_(lo)) & (uk <= np.bytes_(hi))])
        got = last["keys"][:last["key_bytes"]].cpu().numpy()
        ok = (last["unsorted"] == -1 and last["n_out"] == inside.shape[0] and last["key_bytes"] == KEY_LEN * inside.shape[0]
              and got.tobytes() == inside.tobytes())
        all_ok = all_ok and ok
        sec = {s_: round(sum(p[k] for p in per) / len(per), 3) for k, s_ in enumerate(stages)}
        whole = [p[-1] for p in per]
        res["scan_range"] = {"entries_in_range": last["n_in"], "n_out": last["n_out"], "value_bytes": last["value_bytes"],
                             "key_bytes": last["key_bytes"], "stage_ms": sec, "whole_ms": round(sum(whole) / len(whole), 3),
                             "whole_ms_min": round(min(whole), 3), "whole_ms_max": round(max(whole), 3), "equals_model": ok}
        lib.rio_sst_stack_free(stack)

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
