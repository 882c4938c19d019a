#!/usr/bin/env python3
"""What DB.Apply adds to a batch on one GPU: rio_mem_size_scan beside the rio_mem_index_extend it stands next to
(csrc/rio_memsize.hip, csrc/rio_memidx.hip). Both sort the batch. One JSON line.

Shape: DESIGN.md §6's extend shape. A write store of --ops ops over as many distinct 20-byte keys (every 16th op a
tombstone, the others --value-len byte values), indexed by rio_mem_index_build; then batches of 1 Ki and 16 Ki ops
behind it, every fourth batch op writing a key of the store again, every 16th a delete.
size_scan     rio_mem_size_scan of the batch (offsets from 0, as WriteBatch.upload leaves it) over the store's index,
              without a limit.
index_extend  rio_mem_index_extend of the store's index by the same ops as the log's tail (the old index is restored
              outside the timed interval).
The two are alternated run by run in one process. Intervals are between HIP events on the stream; every figure is
the mean of --steps runs after --warmup runs, with the smallest and largest run beside it. verified: the scan's SIZE
word and its last d_size word equal numpy's sum of the deltas, CUT is ~0, and the extend's key count is the model's.

    python scripts/db_apply_times.py [--ops 1000000] [--value-len 64] [--steps 10] [--warmup 3] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "go-sstables_amd"))

KEY_LEN = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=1_000_000)
    ap.add_argument("--value-len", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    from recordio import _lib as L

    n_store, vlen, device = args.ops, args.value_len, args.device
    dev = f"cuda:{device}"
    lib, ctx = L.lib(), L.default_ctx(device)
    W, none = L.RIO_MERGE_RESULT_WORDS, (1 << 64) - 1
    res = {"bench": "db_apply_times", "steps": args.steps, "warmup": args.warmup, "library": os.path.basename(L.LIB_PATH),
           "shape": f"a write store of {n_store} ops over {n_store} keys of {KEY_LEN} B, {vlen} B values; batches behind it"}

    def check(rc, what):
        if rc:
            raise RuntimeError(f"{what}: {L.strerror(rc)}")

    def stat(ms):
        return {"ms": round(sum(ms) / len(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}

    rng = np.random.default_rng(17)
    tails = (1 << 10, 1 << 14)
    n_all = n_store + max(tails)
    # distinct keys: a counter in the first 8 bytes under random bytes
    rows = rng.integers(0, 256, (n_all, KEY_LEN), dtype=np.uint8)
    rows[:, :8] = np.frombuffer(rng.permutation(n_all).astype(">u8").tobytes(), dtype=np.uint8).reshape(n_all, 8)
    all_ok = True
    with torch.cuda.device(device), torch.cuda.stream(torch.cuda.Stream(device=device)):
        st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        pad = np.zeros(L.RIO_DEVICE_PAD, dtype=np.uint8)
        for tail in tails:
            n = n_store + tail
            log_rows = rows[:n].copy()
            rewrites = np.arange(n_store, n)[::4]  # every fourth batch op writes a key of the store again
            targets = rng.choice(n_store, rewrites.shape[0], replace=False)
            log_rows[rewrites] = rows[targets]
            nil = (np.arange(n) % 16) == 15
            lens = np.where(nil, 0, vlen).astype(np.int64)
            val_off = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(lens, out=val_off[1:])
            d_keys = up(np.concatenate([log_rows.reshape(-1), pad]))
            d_key_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * KEY_LEN
            d_values = torch.zeros(int(val_off[-1]) + L.RIO_DEVICE_PAD, dtype=torch.uint8, device=dev)
            d_val_off, d_flags = up(val_off), up(np.where(nil, L.RIO_FLAG_NIL, 0).astype(np.uint8))

            def view(k):
                """The first k ops of the log."""
                return L.OpsView(keys=d_keys.data_ptr(), key_off=d_key_off.data_ptr(), values=d_values.data_ptr(),
                                 val_off=d_val_off.data_ptr(), flags=d_flags.data_ptr(), n=k, key_bytes=k * KEY_LEN,
                                 value_bytes=int(val_off[k]))

            store_ops, whole_log = view(n_store), view(n)
            # the batch as WriteBatch.upload leaves it: its own offsets from 0 over the tail of the arenas
            b_key_off = d_key_off[n_store:] - n_store * KEY_LEN
            b_val_off = d_val_off[n_store:] - int(val_off[n_store])
            batch = L.OpsView(keys=d_keys.data_ptr() + n_store * KEY_LEN, key_off=b_key_off.data_ptr(),
                              values=d_values.data_ptr() + int(val_off[n_store]), val_off=b_val_off.data_ptr(),
                              flags=d_flags.data_ptr() + n_store, n=tail, key_bytes=tail * KEY_LEN,
                              value_bytes=int(val_off[n] - val_off[n_store]))
            old_idx = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2)] + [torch.empty(W, dtype=torch.int64, device=dev)]
            ext_idx = [torch.empty_like(t_) for t_ in old_idx]
            check(lib.rio_mem_index_build(ctx, ctypes.addressof(store_ops), KEY_LEN, old_idx[0].data_ptr(), old_idx[1].data_ptr(),
                                          old_idx[2].data_ptr(), st), "rio_mem_index_build")
            store = L.MemIndex(ops=store_ops, order=old_idx[0].data_ptr(), pfx=old_idx[1].data_ptr(), result=old_idx[2].data_ptr())
            size0 = n_store * KEY_LEN + int(lens[:n_store].sum())
            d_size = torch.empty(tail, dtype=torch.int64, device=dev)
            d_result = torch.empty(L.RIO_SIZE_RESULT_WORDS, dtype=torch.int64, device=dev)

            def scan():
                check(lib.rio_mem_size_scan(ctx, ctypes.addressof(store), size0, ctypes.addressof(batch), KEY_LEN, none,
                                            d_size.data_ptr(), d_result.data_ptr(), st), "rio_mem_size_scan")

            def extend():
                check(lib.rio_mem_index_extend(ctx, ctypes.addressof(whole_log), n_store, KEY_LEN, ext_idx[0].data_ptr(),
                                               ext_idx[1].data_ptr(), ext_idx[2].data_ptr(), st), "rio_mem_index_extend")

            def pair(ev):
                for dst, src_ in zip(ext_idx, old_idx):  # the old index again, outside the timed interval
                    dst.copy_(src_)
                for call in (scan, extend):
                    ev.append(torch.cuda.Event(enable_timing=True))
                    ev[-1].record()
                    call()
                    ev.append(torch.cuda.Event(enable_timing=True))
                    ev[-1].record()

            for _ in range(args.warmup):
                pair([])
            torch.cuda.synchronize(device)
            s_ms, e_ms = [], []
            for _ in range(args.steps):
                ev = []
                pair(ev)
                torch.cuda.synchronize(device)
                s_ms.append(ev[0].elapsed_time(ev[1]))
                e_ms.append(ev[2].elapsed_time(ev[3]))
            # the model: a new key adds its length and its value's, a delete of one its length; a key of the store
            # changes the size by the value lengths' difference (a tombstone's length is 0)
            t_nil, t_len = nil[n_store:], lens[n_store:]
            delta = np.where(t_nil, KEY_LEN, KEY_LEN + t_len).astype(np.int64)
            delta[::4] = t_len[::4] - lens[targets]
            want = size0 + int(delta.sum())
            r = [x & none for x in d_result.cpu().tolist()]
            ok = (r[L.RIO_SIZE_R_CUT] == none and r[L.RIO_SIZE_R_FIRST_BAD] == none and r[L.RIO_SIZE_R_SIZE] == want
                  and int(d_size[-1].item()) == want and r[L.RIO_SIZE_R_KEY_END] == tail * KEY_LEN)
            words = ext_idx[2].cpu().tolist()
            ok = ok and words[L.RIO_MERGE_R_N_OUT] == n - rewrites.shape[0] and words[L.RIO_MERGE_R_UNSORTED] == -1
            all_ok = all_ok and ok
            res[f"batch_{tail}"] = {"batch_ops": tail, "rewrites": int(rewrites.shape[0]), "store_ops": n_store,
                                    "size_scan": stat(s_ms), "index_extend": stat(e_ms),
                                    "scan_over_extend": round(sum(s_ms) / sum(e_ms), 4), "verified": bool(ok)}
            del d_keys, d_values
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
