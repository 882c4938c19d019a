#!/usr/bin/env python3
"""Batched GetBytes on one GPU: a memstore's op log over a stack of loaded tables (rio_mem_index_build, rio_mem_lookup,
rio_db_value_plan / _copy; csrc/rio_memidx.hip, csrc/rio_db.hip). One JSON line.

Shape: scripts/super_bench.py's stack (T = 8 tables x 1.25M 20-byte SHA1 keys x 1 KiB values, half of each table
shared with the next) under a write store of 1M ops over 1M distinct keys in random order: half of them keys of the
oldest table's first half, the others keys no table holds; every 16th op a tombstone, the others 1 KiB values.
index_build   rio_mem_index_build over the log, with the flush plan's stage times (rio_sst_flush_stage_ms: check, the
              length pass, the chunk passes, keep) from one more build with timing on.
index_extend  the same log with its last 1 Ki, 16 Ki, 128 Ki and 512 Ki ops as the tail, every fourth tail op rewriting a
              key of the first part: rio_mem_index_extend over the index of the first part against rio_mem_index_build
              over the whole log, alternated run by run (the old index is restored outside the timed interval); the
              tail plan's stage times and what follows it (rank, scan, place, copy back) from one more extend with
              timing on. --only index_extend runs this entry alone, without the tables.
mem_lookup    rio_mem_lookup alone for three mixes of 1M queries: all in the memstore, none, half; beside each, in the
              same process, rio_sst_lookup (no filter) of the same queries against ONE table that holds the memstore's
              1M keys: the same search without the order indirection.
sequence      the whole device sequence for a mix of memstore keys (half) and keys spread over the tables: stack
              lookup, mem lookup, value plan, the 8-byte read, value copy; stage by stage and whole.
host_loop     DBReadView.GetBytes, the reference's host sequence and all the library offered before, over
              --host-queries queries, per query. Its tables are written to disk and opened by NewSSTableReader, so
              they are SMALLER than the device shape's (--host-keys keys per table, 64-byte values); the memstore is
              the same log in a host MemStore. Python's cost per key hardly depends on the tables' size.
Intervals are between HIP events on the stream; every figure is the mean of --steps runs after --warmup runs, with
the smallest and largest run beside it. verified: the memstore words equal numpy's for every query of every mix, the
table lookups equal them too, and the sequence's statuses and bytes equal tests/db_model.py's get_bytes on a sample.

    python scripts/db_get_bench.py [--keys 1250000] [--tables 8] [--ops 1000000] [--queries 1000000] [--steps 10]
                                   [--warmup 3] [--host-queries 50000] [--host-keys 20000] [--out FILE]
"""
import argparse
import ctypes
import hashlib
import json
import os
import struct
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "go-sstables_amd"))
sys.path.insert(0, os.path.join(HERE, "scripts"))
sys.path.insert(0, os.path.join(HERE, "tests"))

KEY_LEN = 20
VALUE_LEN = 1024


def sha_rows(np, start, count):
    return np.frombuffer(b"".join(hashlib.sha1(struct.pack(">I", start + i)).digest() for i in range(count)),
                         dtype=np.uint8).reshape(count, KEY_LEN)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=1_250_000)
    ap.add_argument("--tables", type=int, default=8)
    ap.add_argument("--ops", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-queries", type=int, default=50_000)
    ap.add_argument("--host-keys", type=int, default=20_000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--only", choices=["index_extend"], default=None, help="run this entry alone (no tables are made)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import db_model as dm
    from compact_bench import load_table, table_images
    from recordio import _lib as L
    from recordio.device import DeviceDecoder

    n, nt, nq, n_ops, device = args.keys, args.tables, args.queries, args.ops, args.device
    dev = f"cuda:{device}"
    lib = L.lib()
    dec = DeviceDecoder(device)
    ctx = dec.ctx
    fixed = np.dtype(f"S{KEY_LEN}")
    res = {"bench": "db_get", "steps": args.steps, "warmup": args.warmup, "library": os.path.basename(L.LIB_PATH),
           "shape": f"{nt} tables x {n} keys x {VALUE_LEN} B values; a write store of {n_ops} ops over {n_ops} keys; {nq} queries"}

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

    def finish(all_ok):
        res["verified"] = bool(all_ok)
        line = json.dumps(res)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
        return 0 if all_ok else 1

    t0 = time.time()
    full = args.only is None
    half = n // 2
    n_uni = half * (nt - 1) + n
    in_tables = min(n_ops // 2, half * 4 // 5)  # memstore keys the oldest table holds too
    universe = sha_rows(np, 0, n_uni if full else in_tables)
    values = [np.random.default_rng(1000 + t).integers(0, 256, VALUE_LEN, dtype=np.uint8).tobytes() for t in range(nt)]
    mem_value = np.random.default_rng(999).integers(0, 256, VALUE_LEN, dtype=np.uint8)
    all_ok = True
    with torch.cuda.device(device), torch.cuda.stream(torch.cuda.Stream(device=device)):
        st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731

        def one_table(rows, value):
            tk = np.sort(rows.copy().view(fixed).ravel())
            raw = tk.tobytes()
            index_img, data_img = table_images([raw[i:i + KEY_LEN] for i in range(0, len(raw), KEY_LEN)], value)
            T = load_table(dec, lib, device, index_img, data_img)
            T["pfx"] = torch.empty(len(tk), dtype=torch.int64, device=dev)
            check(lib.rio_sst_key_prefixes(ctx, ctypes.byref(T["view"]), T["pfx"].data_ptr(), st), "rio_sst_key_prefixes")
            torch.cuda.synchronize(device)
            return T, tk

        if full:
            tables = [one_table(universe[t * half:t * half + n], values[t])[0] for t in range(nt)]
            views = (L.SstView * nt)(*[T["view"] for T in tables])
            pfx = (ctypes.c_uint64 * nt)(*[T["pfx"].data_ptr() for T in tables])
            stored = (ctypes.c_uint64 * nt)(*[T["checksum"].data_ptr() for T in tables])
            stack = ctypes.c_void_p()
            check(lib.rio_sst_stack_create(ctx, ctypes.addressof(views), ctypes.addressof(pfx), None, ctypes.addressof(stored),
                                           nt, nq, ctypes.byref(stack), st), "rio_sst_stack_create")

        # ---- the write store's log: op i holds mem key perm[i]; every 16th op is a tombstone ------------------------
        rng = np.random.default_rng(17)
        mem_rows = np.concatenate([universe[:in_tables], sha_rows(np, 1 << 29, n_ops - in_tables)])
        perm = rng.permutation(n_ops)          # log position -> mem key
        op_of_key = np.empty(n_ops, dtype=np.int64)
        op_of_key[perm] = np.arange(n_ops)     # mem key -> log position (keys are distinct: its latest op)
        nil = (np.arange(n_ops) % 16) == 15
        vlen = np.where(nil, 0, VALUE_LEN).astype(np.int64)
        val_off = np.zeros(n_ops + 1, dtype=np.int64)
        np.cumsum(vlen, out=val_off[1:])
        pad = np.zeros(L.RIO_DEVICE_PAD, dtype=np.uint8)
        d_keys = up(np.concatenate([mem_rows[perm].reshape(-1), pad]))
        d_key_off = torch.arange(n_ops + 1, dtype=torch.int64, device=dev) * KEY_LEN
        d_values = torch.cat([up(mem_value).repeat(int((~nil).sum())), up(pad)])
        d_val_off, d_flags = up(val_off), up(np.where(nil, L.RIO_FLAG_NIL, 0).astype(np.uint8))
        ops = L.OpsView(keys=d_keys.data_ptr(), key_off=d_key_off.data_ptr(), values=d_values.data_ptr(),
                        val_off=d_val_off.data_ptr(), flags=d_flags.data_ptr(), n=n_ops, key_bytes=n_ops * KEY_LEN,
                        value_bytes=int(val_off[-1]))
        order, ipfx = (torch.empty(n_ops, dtype=torch.int64, device=dev) for _ in range(2))
        result = torch.empty(L.RIO_MERGE_RESULT_WORDS, dtype=torch.int64, device=dev)
        res["generate_s"] = round(time.time() - t0, 1)

        def build():
            check(lib.rio_mem_index_build(ctx, ctypes.addressof(ops), KEY_LEN, order.data_ptr(), ipfx.data_ptr(),
                                          result.data_ptr(), st), "rio_mem_index_build")

        b_ms = timed(build)
        lib.rio_ctx_set_timing(ctx, 1)
        build()
        stage = (ctypes.c_float * 16)()
        k = lib.rio_sst_flush_stage_ms(ctx, stage, 16)
        lib.rio_ctx_set_timing(ctx, 0)
        names = ["check", "length_pass"] + [f"chunk_{c}" for c in range((KEY_LEN + 7) // 8 - 1, -1, -1)] + ["keep"]
        words = result.cpu().tolist()
        ok = words[L.RIO_MERGE_R_N_OUT] == n_ops and words[L.RIO_MERGE_R_UNSORTED] == -1
        sorted_mem = np.argsort(mem_rows.copy().view(fixed).ravel(), kind="stable")
        ok = ok and bool(np.array_equal(order.cpu().numpy(), op_of_key[sorted_mem]))
        all_ok = all_ok and ok
        res["index_build"] = dict(b_ms, ops=n_ops, distinct_keys=n_ops, ops_per_s=round(n_ops / (b_ms["ms"] / 1e3)),
                                  flush_plan_stage_ms={names[i]: round(stage[i], 4) for i in range(min(k, len(names)))},
                                  equals_model=bool(ok))

        # ---- rio_mem_index_extend against the build of the same final log ------------------------------------------
        res["index_extend"] = {}
        log_rows = mem_rows[perm]  # op -> key
        rng_ext = np.random.default_rng(23)  # its own generator: the later entries' draws stay as they were
        W = L.RIO_MERGE_RESULT_WORDS
        old_idx = [torch.empty(n_ops, dtype=torch.int64, device=dev) for _ in range(2)] + [torch.empty(W, dtype=torch.int64, device=dev)]
        ext_idx = [torch.empty_like(t_) for t_ in old_idx]
        bld_idx = [torch.empty_like(t_) for t_ in old_idx]
        for tail in (1 << 10, 1 << 14, 1 << 17, 1 << 19):
            if tail >= n_ops:
                continue
            n_old = n_ops - tail
            rewrites = np.arange(n_old, n_ops)[::4]  # every fourth tail op writes a key of the first part again
            rows = log_rows.copy()
            rows[rewrites] = log_rows[rng_ext.integers(0, n_old, rewrites.shape[0])]
            d_keys_t = up(np.concatenate([rows.reshape(-1), pad]))
            whole_log = L.OpsView(keys=d_keys_t.data_ptr(), key_off=d_key_off.data_ptr(), values=d_values.data_ptr(),
                                  val_off=d_val_off.data_ptr(), flags=d_flags.data_ptr(), n=n_ops, key_bytes=n_ops * KEY_LEN,
                                  value_bytes=int(val_off[-1]))
            first_part = L.OpsView(keys=d_keys_t.data_ptr(), key_off=d_key_off.data_ptr(), values=d_values.data_ptr(),
                                   val_off=d_val_off.data_ptr(), flags=d_flags.data_ptr(), n=n_old, key_bytes=n_old * KEY_LEN,
                                   value_bytes=int(val_off[n_old]))
            check(lib.rio_mem_index_build(ctx, ctypes.addressof(first_part), KEY_LEN, old_idx[0].data_ptr(), old_idx[1].data_ptr(),
                                          old_idx[2].data_ptr(), st), "rio_mem_index_build")

            def extend():
                check(lib.rio_mem_index_extend(ctx, ctypes.addressof(whole_log), n_old, KEY_LEN, ext_idx[0].data_ptr(),
                                               ext_idx[1].data_ptr(), ext_idx[2].data_ptr(), st), "rio_mem_index_extend")

            def rebuild():
                check(lib.rio_mem_index_build(ctx, ctypes.addressof(whole_log), KEY_LEN, bld_idx[0].data_ptr(),
                                              bld_idx[1].data_ptr(), bld_idx[2].data_ptr(), st), "rio_mem_index_build")

            def pair(ev):
                for dst, src_ in zip(ext_idx, old_idx):  # the old index again, outside the timed interval
                    dst.copy_(src_)
                for call in (extend, rebuild):
                    ev.append(torch.cuda.Event(enable_timing=True))
                    ev[-1].record()
                    call()
                    ev.append(torch.cuda.Event(enable_timing=True))
                    ev[-1].record()

            for _ in range(args.warmup):
                pair([])
            torch.cuda.synchronize(device)
            e_ms, r_ms = [], []
            for _ in range(args.steps):
                ev = []
                pair(ev)
                torch.cuda.synchronize(device)
                e_ms.append(ev[0].elapsed_time(ev[1]))
                r_ms.append(ev[2].elapsed_time(ev[3]))
            words = ext_idx[2].cpu().tolist()
            nk = words[L.RIO_MERGE_R_N_OUT]
            ok = (words == bld_idx[2].cpu().tolist() and nk == n_ops - rewrites.shape[0] and words[L.RIO_MERGE_R_UNSORTED] == -1
                  and torch.equal(ext_idx[0][:nk], bld_idx[0][:nk]) and torch.equal(ext_idx[1][:nk], bld_idx[1][:nk]))
            all_ok = all_ok and ok
            # the tail plan's stages and the rest of the call, from one more extend with timing on
            for dst, src_ in zip(ext_idx, old_idx):
                dst.copy_(src_)
            lib.rio_ctx_set_timing(ctx, 1)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            extend()
            ev[1].record()
            torch.cuda.synchronize(device)
            k = lib.rio_sst_flush_stage_ms(ctx, stage, 16)
            lib.rio_ctx_set_timing(ctx, 0)
            plan = {names[i]: round(stage[i], 4) for i in range(min(k, len(names)))}
            stat = lambda ms: {"ms": round(sum(ms) / len(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}  # noqa: E731
            res["index_extend"][f"tail_{tail}"] = {
                "tail_ops": tail, "rewrites": int(rewrites.shape[0]), "old_ops": n_old, "extend": stat(e_ms), "rebuild": stat(r_ms),
                "extend_over_rebuild": round(sum(e_ms) / sum(r_ms), 4), "tail_plan_stage_ms": plan,
                "timed_extend_ms": round(ev[0].elapsed_time(ev[1]), 4),
                "after_plan_ms": round(ev[0].elapsed_time(ev[1]) - sum(stage[i] for i in range(k)), 4), "verified": bool(ok)}
            del d_keys_t
        if not full:
            return finish(all_ok)

        index = (L.MemIndex * 1)(L.MemIndex(ops=ops, order=order.data_ptr(), pfx=ipfx.data_ptr(), result=result.data_ptr()))
        # one table of the memstore's keys: the same search without the indirection
        twin, twin_keys = one_table(mem_rows, values[0])
        twin_pos = np.empty(n_ops, dtype=np.int64)
        twin_pos[sorted_mem] = np.arange(n_ops)  # mem key -> entry of the twin table

        # ---- rio_mem_lookup alone: three mixes (mem key numbers, -1: absent) ---------------------------------------
        absent = sha_rows(np, 1 << 30, nq)
        mixes = {"all_in_memstore": rng.integers(0, n_ops, nq), "none_in_memstore": np.full(nq, -1),
                 "half_in_memstore": rng.permutation(np.concatenate([rng.integers(0, n_ops, nq // 2), np.full(nq - nq // 2, -1)]))}
        d_qoff = torch.arange(nq + 1, dtype=torch.int64, device=dev) * KEY_LEN
        d_mem = torch.empty(nq, dtype=torch.int64, device=dev)
        d_entry = torch.empty(nq, dtype=torch.int64, device=dev)
        res["mem_lookup"] = {}
        for name, u in mixes.items():
            q_rows = np.where((u >= 0)[:, None], mem_rows[np.maximum(u, 0)], absent)
            d_q = up(q_rows.reshape(-1))
            m_ms = timed(lambda: check(lib.rio_mem_lookup(ctx, ctypes.addressof(index), 1, d_q.data_ptr(), d_qoff.data_ptr(), nq,
                                                          nq * KEY_LEN, d_mem.data_ptr(), st), "rio_mem_lookup"))
            t_ms = timed(lambda: check(lib.rio_sst_lookup(ctx, ctypes.byref(twin["view"]), twin["pfx"].data_ptr(), None,
                                                          d_q.data_ptr(), d_qoff.data_ptr(), nq, nq * KEY_LEN,
                                                          d_entry.data_ptr(), st), "rio_sst_lookup"))
            ok_m = bool(np.array_equal(d_mem.cpu().numpy(), np.where(u >= 0, op_of_key[np.maximum(u, 0)], -1)))
            ok_t = bool(np.array_equal(d_entry.cpu().numpy(), np.where(u >= 0, twin_pos[np.maximum(u, 0)], -1)))
            all_ok = all_ok and ok_m and ok_t
            res["mem_lookup"][name] = {"present": int((u >= 0).sum()), "mem_lookup": m_ms,
                                       "mem_lookups_per_s": round(nq / (m_ms["ms"] / 1e3)), "table_lookup_same_keys": t_ms,
                                       "mem_over_table": round(m_ms["ms"] / t_ms["ms"], 3), "mem_equals_model": ok_m,
                                       "table_equals_model": ok_t}
            del d_q

        # ---- the whole sequence: half memstore keys, half keys spread over the tables -------------------------------
        per = (nq - nq // 2) // nt
        tab_u = np.concatenate([rng.integers(max(t * half, in_tables), (t + 1) * half if t < nt - 1 else n_uni, per)
                                for t in range(nt)])
        mem_u = rng.integers(0, n_ops, nq - tab_u.shape[0])
        is_mem = rng.permutation(np.concatenate([np.ones(mem_u.shape[0], bool), np.zeros(tab_u.shape[0], bool)]))
        q_rows = np.empty((nq, KEY_LEN), dtype=np.uint8)
        q_rows[is_mem], q_rows[~is_mem] = mem_rows[mem_u], universe[tab_u]
        d_q = up(q_rows.reshape(-1))
        reader = ctypes.c_void_p()
        check(lib.rio_db_reader_create(ctx, stack, nq, ctypes.byref(reader)), "rio_db_reader_create")
        d_tab = torch.empty(nq, dtype=torch.int64, device=dev)
        status = torch.empty(nq, dtype=torch.uint8, device=dev)
        d_voff = torch.empty(nq + 1, dtype=torch.int64, device=dev)
        out = torch.empty(nq * VALUE_LEN + L.RIO_DEVICE_PAD, dtype=torch.uint8, device=dev)
        stages = ("stack_lookup", "mem_lookup", "value_plan", "size_read", "value_copy")
        p_idx = ctypes.addressof(index)
        last = {}

        def sequence(mark):
            check(lib.rio_sst_stack_lookup(stack, 0, d_q.data_ptr(), d_qoff.data_ptr(), nq, nq * KEY_LEN, d_tab.data_ptr(), st),
                  "rio_sst_stack_lookup")
            mark()
            check(lib.rio_mem_lookup(ctx, p_idx, 1, d_q.data_ptr(), d_qoff.data_ptr(), nq, nq * KEY_LEN, d_mem.data_ptr(), st),
                  "rio_mem_lookup")
            mark()
            check(lib.rio_db_value_plan(reader, p_idx, 1, d_tab.data_ptr(), d_mem.data_ptr(), nq, 1, status.data_ptr(),
                                        d_voff.data_ptr(), st), "rio_db_value_plan")
            mark()
            total = int(d_voff[nq].item())
            mark()
            check(lib.rio_db_value_copy(reader, p_idx, 1, d_tab.data_ptr(), d_mem.data_ptr(), status.data_ptr(), nq,
                                        d_voff.data_ptr(), out.data_ptr(), min(total, nq * VALUE_LEN), st), "rio_db_value_copy")
            mark()
            last["total"] = total

        for _ in range(args.warmup):
            sequence(lambda: None)
        torch.cuda.synchronize(device)
        runs = []
        for _ in range(args.steps):
            ev = []

            def mark():
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                ev.append(e)

            mark()
            sequence(mark)
            torch.cuda.synchronize(device)
            runs.append([ev[j].elapsed_time(ev[j + 1]) for j in range(len(stages))] + [ev[0].elapsed_time(ev[-1])])
        whole = [r[-1] for r in runs]
        # the model on a sample: dict tables that hold the sampled keys, a store that holds the sampled ops
        sample = rng.choice(nq, 2000, replace=False)
        h_status, h_off = status.cpu().numpy(), d_voff.cpu().numpy()
        newest = np.minimum(tab_u // half, nt - 1)
        mem_no, tab_no = np.cumsum(is_mem) - 1, np.cumsum(~is_mem) - 1
        w, model_tables, ok = dm.ModelStore(), [dict() for _ in range(nt)], True
        for i in sample:
            q = q_rows[i].tobytes()
            if is_mem[i]:
                u = mem_u[mem_no[i]]
                w.tombstone(q) if nil[op_of_key[u]] else w.upsert(q, mem_value.tobytes())
                if u < in_tables:
                    model_tables[0][q] = values[0]
            else:
                model_tables[newest[tab_no[i]]][q] = values[newest[tab_no[i]]]
        for i in sample:
            v, err = dm.get_bytes(model_tables, w, None, q_rows[i].tobytes())
            got = bytes(out[h_off[i]:h_off[i + 1]].cpu().numpy())
            want_status = L.RIO_GET_NOT_FOUND if err else (L.RIO_GET_MEM_VALUE if is_mem[i] else L.RIO_GET_VALUE)
            ok = ok and h_status[i] == want_status and got == (v or b"")
        ok = bool(ok and last["total"] == int(h_off[nq]))
        all_ok = all_ok and ok
        res["sequence"] = {"queries": nq, "in_memstore": int(is_mem.sum()), "value_bytes": last["total"],
                           "stage_ms": {s_: round(sum(r[j] for r in runs) / len(runs), 4) for j, s_ in enumerate(stages)},
                           "whole_ms": round(sum(whole) / len(whole), 4), "whole_ms_min": round(min(whole), 4),
                           "whole_ms_max": round(max(whole), 4), "queries_per_s": round(nq / (sum(whole) / len(whole) / 1e3)),
                           "sample_equals_model": ok}
        lib.rio_db_reader_free(reader)
        lib.rio_sst_stack_free(stack)
        del out, tables, twin

        # ---- the host loop: DBReadView.GetBytes over real readers of smaller tables and the same log ----------------
        if args.host_queries:
            import memstore as M
            import simpledb as DB
            import sstables as S
            from sstables.writer import write_sstable

            hk, hq = args.host_keys, args.host_queries
            ms = M.NewMemStore(device)
            mv = mem_value.tobytes()
            for i in range(n_ops):
                key = mem_rows[perm[i]].tobytes()
                ms.Tombstone(key) if nil[i] else ms.Upsert(key, mv)
            with tempfile.TemporaryDirectory() as tmp:
                readers = []
                for t in range(nt):
                    rows = sorted(universe[j].tobytes() for j in range(t * (hk // 2), t * (hk // 2) + hk))
                    write_sstable(os.path.join(tmp, f"t{t}"), [(key, values[t][:64]) for key in rows])
                    r, err = S.NewSSTableReader(S.ReadBasePath(os.path.join(tmp, f"t{t}")))
                    if err is not None:
                        raise err
                    readers.append(r)
                view = DB.DBReadView(S.NewSuperSSTableReader(readers), ms)
                qs = [q_rows[i].tobytes() for i in range(hq)]
                view.GetBytes(qs[0])
                t1 = time.perf_counter()
                for q in qs:
                    view.GetBytes(q)
                host_s = time.perf_counter() - t1
                got = view.GetBatch(qs[:2000])
                ok = all((a == b_ and (ea is None) == (eb is None)) for (a, ea), (b_, eb) in zip(got, [view.GetBytes(q) for q in qs[:2000]]))
                all_ok = all_ok and ok
                res["host_loop"] = {"queries": hq, "tables": f"{nt} x {hk} keys x 64 B values (smaller than the device shape's)",
                                    "seconds": round(host_s, 3), "us_per_query": round(host_s / hq * 1e6, 2),
                                    "device_sequence_us_per_query": round(sum(whole) / len(whole) * 1e3 / nq, 4),
                                    "get_batch_equals_loop": bool(ok)}
                view.Close()

    return finish(all_ok)


if __name__ == "__main__":
    sys.exit(main())
