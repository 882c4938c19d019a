"""MemStore mirror (memstore/memstore.go) whose flush runs on the device.

Point semantics (Add / Get / Upsert / Delete / Tombstone, the size estimate) live in a host dict from key
to its latest value. Every mutating call also appends to an op log: a key arena, a value arena, offsets and
flags, in application order and not deduplicated. Flush / FlushWithTombstones ship the log and run
rio_sst_flush_plan (rio_flush.hip: order by (key, op index), keep the latest op of every key, drop nil
ones under Flush), then the back end merge-compaction uses (sstables.merger.encode_planned: gather, data
encode, index entries, index encode). The three files are byte-identical to what the reference's
SSTableStreamWriter writes for the same sorted pairs. None is Go's nil; b"" is an empty non-nil key or
value. Functions return Go-style error values. There is no CPU fallback.

Batched point reads search the log where it lies on the device: DeviceMemIndex makes an uploaded log searchable
in place (rio_mem_index_build, csrc/rio_memidx.hip: the flush plan's order compacted to the latest op of every
key, 16 bytes per distinct key, no key or value copied), MemStore.GetBatch / ContainsBatch answer what loops of
Get / Contains answer through it. At the first batched read after the log has grown, the new ops alone are uploaded
behind the device copy of the log (DeviceOpLog) and the index is extended by them (rio_mem_index_extend: a sort of
the new ops and a merge into the old order). DeviceMemStore is the memstore that lives on the device only: batches
that append_batch left there are appended (rio_ops_append) and indexed without a host copy. Its size estimate comes
from rio_mem_size_scan (csrc/rio_memsize.hip): the raw estimatedSize after every op of a batch, and the put at which
db.PutBytes would rotate (ApplyUntilFull).
"""
from __future__ import annotations

import ctypes
import struct

from recordio import _lib as L
from recordio.errors import GoError

KeyAlreadyExists = GoError("key already exists")  # memstore.go:10-14
KeyNotFound = GoError("key not found")
KeyTombstoned = GoError("key was tombstoned")
KeyNil = GoError("key was nil")
ValueNil = GoError("value was nil")

_NONE = 0xFFFFFFFFFFFFFFFF


def _key(key) -> bytes:
    return b"" if key is None else bytes(key)  # a nil []byte compares as the empty key


def _f32(x: float) -> float:
    return struct.unpack("f", struct.pack("f", x))[0]


def flush_ops_on_device(ctx, device: int, ops_view, mode: int, comp: int, mark=None,
                        max_key_len: int = L.RIO_FLUSH_MAX_KEY_LEN, flt=None):
    """rio_sst_flush_plan over a device-resident op log (an OpsView), then gather, data encode, index
    entries and index encode on torch's current stream; returns the merger's Compaction (status "unsorted"
    with unsorted_table = the first rejected op when the log is inconsistent or a key is longer than
    max_key_len). max_key_len bounds the key lengths and sets the sort's pass count: pass the longest key's
    length. `mark(name)` and `flt` (the table's bloom filter to build) as for sstables.merger.compact_on_device."""
    import torch

    from sstables.merger import check_status, encode_planned, on_device_stream

    mark = mark or (lambda name: None)
    dev = f"cuda:{device}"
    n = int(ops_view.n)

    def run(st):
        src = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        keep = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        res = torch.empty(L.RIO_MERGE_RESULT_WORDS, dtype=torch.int64, device=dev)
        check_status(L.lib().rio_sst_flush_plan(ctx, ctypes.addressof(ops_view), mode, max_key_len, src.data_ptr(),
                                          keep.data_ptr(), res.data_ptr(), st), "rio_sst_flush_plan")
        mark("plan")
        return encode_planned(ctx, device, st, src, keep, res, comp, mark, False, flt)

    return on_device_stream(device, run)


class DeviceOps:
    """An op log in device memory: the tensors (kept alive here) and the OpsView over them."""

    def __init__(self, device: int, keys, key_off, values, val_off, flags, n: int, key_bytes: int, value_bytes: int,
                 max_key_len: int):
        self.device, self.n, self.max_key_len = device, n, max_key_len
        self.keys, self.key_off, self.values, self.val_off, self.flags = keys, key_off, values, val_off, flags
        self.view = L.OpsView(keys=keys.data_ptr(), key_off=key_off.data_ptr(), values=values.data_ptr(),
                              val_off=val_off.data_ptr(), flags=flags.data_ptr(), n=n, key_bytes=key_bytes,
                              value_bytes=value_bytes)


def upload_ops(device: int, keys: bytearray, key_off, values: bytearray, val_off, flags: bytearray,
               max_key_len: int) -> DeviceOps:
    """The host arrays of an op log (MemStore's, simpledb.WriteBatch's) to device `device`, with the pad
    bytes rio_ops_view asks for past each arena. Call under torch.cuda.device(device)."""
    import numpy as np
    import torch

    dev = f"cuda:{device}"
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    pad = bytearray(L.RIO_DEVICE_PAD)
    return DeviceOps(device,
                     up(np.frombuffer(keys + pad, dtype=np.uint8)), up(np.asarray(key_off, dtype=np.int64)),
                     up(np.frombuffer(values + pad, dtype=np.uint8)), up(np.asarray(val_off, dtype=np.int64)),
                     up(np.frombuffer(flags + bytearray(1), dtype=np.uint8)), len(flags), len(keys), len(values),
                     max_key_len)


class DeviceOpLog:
    """A growable op log in device memory: the five arrays of rio_ops_view with capacity (key_off / val_off hold
    ops_cap + 1 words, flags ops_cap bytes, keys keys_cap and values values_cap bytes, the arenas' pad included), and
    what DeviceOps has: `view` (over the ops so far), `n`, `max_key_len`. append() adds a batch that is on the device
    (rio_ops_append: two copies device to device and the offsets' rebase, nothing read back); append_host() copies a
    host tail to its place. Arrays that are too short double, their contents copied device to device."""

    def __init__(self, device: int = 0, ops_cap: int = 1024, keys_cap: int = 1 << 16, values_cap: int = 1 << 16):
        import torch

        self.device = device
        self.n = self.key_bytes = self.value_bytes = self.max_key_len = 0
        self.ops_cap = max(int(ops_cap), 1)
        self.keys_cap, self.values_cap = (max(int(c), L.RIO_DEVICE_PAD) for c in (keys_cap, values_cap))
        dev = f"cuda:{device}"
        with torch.cuda.device(device):
            self.keys = torch.zeros(self.keys_cap, dtype=torch.uint8, device=dev)
            self.values = torch.zeros(self.values_cap, dtype=torch.uint8, device=dev)
            self.key_off = torch.zeros(self.ops_cap + 1, dtype=torch.int64, device=dev)
            self.val_off = torch.zeros(self.ops_cap + 1, dtype=torch.int64, device=dev)
            self.flags = torch.zeros(self.ops_cap, dtype=torch.uint8, device=dev)

    @property
    def view(self):
        return L.OpsView(keys=self.keys.data_ptr(), key_off=self.key_off.data_ptr(), values=self.values.data_ptr(),
                         val_off=self.val_off.data_ptr(), flags=self.flags.data_ptr(), n=self.n, key_bytes=self.key_bytes,
                         value_bytes=self.value_bytes)

    def _reserve(self, n: int, key_bytes: int, value_bytes: int):
        """Room for n ops, key_bytes and value_bytes in all (and the arenas' pad)."""
        import torch

        def fit(cap, need):
            while cap < need:
                cap *= 2
            return cap

        def moved(old, size, used):
            new = torch.zeros(size, dtype=old.dtype, device=old.device)
            new[:used].copy_(old[:used])
            return new

        ops_cap = fit(self.ops_cap, n)
        keys_cap = fit(self.keys_cap, key_bytes + L.RIO_DEVICE_PAD)
        values_cap = fit(self.values_cap, value_bytes + L.RIO_DEVICE_PAD)
        if ops_cap != self.ops_cap:
            self.key_off, self.val_off = moved(self.key_off, ops_cap + 1, self.n + 1), moved(self.val_off, ops_cap + 1, self.n + 1)
            self.flags = moved(self.flags, ops_cap, self.n)
        if keys_cap != self.keys_cap:
            self.keys = moved(self.keys, keys_cap, self.key_bytes)
        if values_cap != self.values_cap:
            self.values = moved(self.values, values_cap, self.value_bytes)
        self.ops_cap, self.keys_cap, self.values_cap = ops_cap, keys_cap, values_cap

    def append(self, batch):
        """`batch` behind the log: a DeviceOps (what simpledb.append_batch returns), a DeviceOpLog, or a
        simpledb.WriteBatch, which is uploaded first."""
        import torch

        from sstables.merger import check_status, on_device_stream

        with torch.cuda.device(self.device):
            ops = batch.upload(self.device) if hasattr(batch, "upload") else batch
            bv = ops.view
            n, kb, vb = int(bv.n), int(bv.key_bytes), int(bv.value_bytes)
            if n == 0:
                return self
            self._reserve(self.n + n, self.key_bytes + kb, self.value_bytes + vb)
            lv = self.view
            on_device_stream(self.device, lambda st: check_status(
                L.lib().rio_ops_append(L.default_ctx(self.device), ctypes.addressof(lv), self.ops_cap, self.keys_cap,
                                       self.values_cap, ctypes.addressof(bv), st), "rio_ops_append"))
        self.n, self.key_bytes, self.value_bytes = self.n + n, self.key_bytes + kb, self.value_bytes + vb
        self.max_key_len = max(self.max_key_len, int(getattr(ops, "max_key_len", L.RIO_FLUSH_MAX_KEY_LEN)))
        return self

    def append_host(self, keys, key_off, values, val_off, flags):
        """A host tail behind the log, in upload_ops's shapes (offsets from 0, n + 1 of them). The host knows the
        log's lengths, so the offsets are rebased here and no kernel runs."""
        import numpy as np
        import torch

        n = len(flags)
        if n == 0:
            return self
        ko, vo = np.asarray(key_off, dtype=np.int64), np.asarray(val_off, dtype=np.int64)
        kb, vb = len(keys), len(values)
        with torch.cuda.device(self.device):
            self._reserve(self.n + n, self.key_bytes + kb, self.value_bytes + vb)

            def put(dst, at, arr):
                if len(arr):
                    dst[at:at + len(arr)].copy_(torch.from_numpy(arr))

            put(self.keys, self.key_bytes, np.frombuffer(bytearray(keys), dtype=np.uint8))
            put(self.values, self.value_bytes, np.frombuffer(bytearray(values), dtype=np.uint8))
            put(self.flags, self.n, np.frombuffer(bytearray(flags), dtype=np.uint8))
            put(self.key_off, self.n + 1, ko[1:] + self.key_bytes)
            put(self.val_off, self.n + 1, vo[1:] + self.value_bytes)
        self.n, self.key_bytes, self.value_bytes = self.n + n, self.key_bytes + kb, self.value_bytes + vb
        self.max_key_len = max(self.max_key_len, int(np.diff(ko).max()))
        return self


def upload_queries(device: int, keys):
    """Query keys as the arena every lookup takes: (uint8 arena, int64 offsets[n + 1], arena length) on `device`."""
    import numpy as np
    import torch

    arena = b"".join(keys)
    off = np.zeros(len(keys) + 1, dtype=np.int64)
    np.cumsum([len(k) for k in keys], out=off[1:])
    dev = f"cuda:{device}"
    d_keys = torch.from_numpy(np.frombuffer(arena + b"\0", dtype=np.uint8).copy()).to(dev)
    return d_keys, torch.from_numpy(off).to(dev), len(arena)


def index_array(indexes):
    """The rio_mem_index array of `indexes` (DeviceMemIndex, oldest first: the write store last)."""
    return (L.MemIndex * len(indexes))(*[i.view for i in indexes])


def read_piece(ctx, device: int, st, reader, stack, idx, p_keys, p_off, n: int, nbytes: int):
    """One batch of DB.GetBytes on stream `st`: rio_sst_stack_lookup (stack: the handle or None), rio_mem_lookup,
    rio_db_value_plan, the 8-byte read that sizes the values, rio_db_value_copy. idx: index_array(...); reader: a
    rio_db_reader over `stack`. Returns (mem_src, tab_src or None, status, val_off, values) as device tensors."""
    import torch

    from sstables.merger import check_status

    lib, dev, k = L.lib(), f"cuda:{device}", len(idx)
    p_idx = ctypes.addressof(idx)
    tab = None
    if stack is not None:
        tab = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        check_status(lib.rio_sst_stack_lookup(stack, 0, p_keys, p_off, n, nbytes, tab.data_ptr(), st), "rio_sst_stack_lookup")
    p_tab = None if tab is None else tab.data_ptr()
    mem = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    val_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    check_status(lib.rio_mem_lookup(ctx, p_idx, k, p_keys, p_off, n, nbytes, mem.data_ptr(), st), "rio_mem_lookup")
    check_status(lib.rio_db_value_plan(reader, p_idx, k, p_tab, mem.data_ptr(), n, 1, status.data_ptr(),
                                       val_off.data_ptr(), st), "rio_db_value_plan")
    total = int(val_off[n].item())  # the one round trip: the value arena's size
    values = torch.empty(total + L.RIO_DEVICE_PAD, dtype=torch.uint8, device=dev)
    check_status(lib.rio_db_value_copy(reader, p_idx, k, p_tab, mem.data_ptr(), status.data_ptr(), n, val_off.data_ptr(),
                                       values.data_ptr(), total, st), "rio_db_value_copy")
    return mem[:n], None if tab is None else tab[:n], status[:n], val_off, values[:total]


class DeviceMemIndex:
    """A searchable snapshot of an op log in device memory (rio_mem_index_build): `order` (the op of every distinct
    key's latest op, keys ascending) and `pfx` (those keys' 8-byte prefixes), n_keys in the result block ON THE
    DEVICE. The log is not copied; the DeviceOps is kept alive here. Get / Contains / GetBatch / ContainsBatch are
    MemStore's (memstore.go:92-123), answered by rio_mem_lookup: a log that never was on the host can be read."""

    def __init__(self, ops: DeviceOps):
        self.device = ops.device
        self.order = self.pfx = self.result = None
        self._reader, self._reader_cap = None, 0
        self.rebuild(ops)

    def rebuild(self, ops: DeviceOps):
        """Index `ops` (the log grown longer, or another log) into the same buffers while it fits them."""
        import torch

        from sstables import UnsupportedError
        from sstables.merger import check_status, on_device_stream

        dev, n = f"cuda:{self.device}", int(ops.n)
        with torch.cuda.device(self.device):
            if self.result is None:
                self.result = torch.zeros(L.RIO_MERGE_RESULT_WORDS, dtype=torch.int64, device=dev)
            if self.order is None or n > self.order.numel():
                self.order = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
                self.pfx = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
            self.ops, self._rejected, self._n = ops, None, n
            self.err = None
            if ops.max_key_len > L.RIO_FLUSH_MAX_KEY_LEN:  # the device rejects the log too: n_keys = 0
                self.err = UnsupportedError(f"a key of {ops.max_key_len} bytes: the device orders keys of up to "
                                            f"{L.RIO_FLUSH_MAX_KEY_LEN}")
            bound = min(int(ops.max_key_len), L.RIO_FLUSH_MAX_KEY_LEN)
            view = ops.view
            on_device_stream(self.device, lambda st: check_status(
                L.lib().rio_mem_index_build(L.default_ctx(self.device), ctypes.addressof(view), bound,
                                            self.order.data_ptr(), self.pfx.data_ptr(), self.result.data_ptr(), st),
                "rio_mem_index_build"))
        return self

    def extend(self, ops):
        """Index `ops`, the SAME log grown longer than at the last rebuild / extend (a DeviceOpLog after append, or a
        longer DeviceOps over the same ops), from the index as it stands: rio_mem_index_extend sorts the new ops alone
        and merges them in. order / pfx double while they are too short, their contents kept. A rejection is sticky:
        only rebuild() clears it."""
        import torch

        from sstables import UnsupportedError
        from sstables.merger import check_status, on_device_stream

        n, n_old = int(ops.n), self._n
        if n < n_old:
            raise GoError(f"memstore index: a log of {n} ops cannot extend an index of {n_old}")
        with torch.cuda.device(self.device):
            if n > self.order.numel():
                cap = self.order.numel()
                while cap < n:
                    cap *= 2
                for name in ("order", "pfx"):
                    old = getattr(self, name)
                    new = torch.empty(cap, dtype=torch.int64, device=old.device)
                    new[:n_old].copy_(old[:n_old])  # n_keys <= n_old
                    setattr(self, name, new)
            self.ops, self._rejected, self._n = ops, None, n
            if self.err is None and ops.max_key_len > L.RIO_FLUSH_MAX_KEY_LEN:
                self.err = UnsupportedError(f"a key of {ops.max_key_len} bytes: the device orders keys of up to "
                                            f"{L.RIO_FLUSH_MAX_KEY_LEN}")
            bound = min(int(ops.max_key_len), L.RIO_FLUSH_MAX_KEY_LEN)
            view = ops.view
            on_device_stream(self.device, lambda st: check_status(
                L.lib().rio_mem_index_extend(L.default_ctx(self.device), ctypes.addressof(view), n_old, bound,
                                             self.order.data_ptr(), self.pfx.data_ptr(), self.result.data_ptr(), st),
                "rio_mem_index_extend"))
        return self

    @property
    def view(self):
        return L.MemIndex(ops=self.ops.view, order=self.order.data_ptr(), pfx=self.pfx.data_ptr(),
                          result=self.result.data_ptr())

    def result_words(self):
        """The build's result block, read from the device."""
        return [x & _NONE for x in self.result.cpu().tolist()]

    def n_keys(self) -> int:
        return self.result_words()[L.RIO_MERGE_R_N_OUT]

    def rejected(self):
        """None, or the error of a log the build refused (read from the device once per build)."""
        if self._rejected is None:
            bad = self.result_words()[L.RIO_MERGE_R_UNSORTED]
            self._rejected = False if bad == _NONE else GoError(f"memstore index: op {bad} of the log was rejected")
        return self.err or self._rejected or None

    def _free_reader(self):
        if self._reader is not None:
            h, self._reader = self._reader, None
            L.lib().rio_db_reader_free(h)

    def __del__(self):
        try:
            self._free_reader()
        except Exception:  # interpreter shutdown: the library may be gone
            pass

    def _get(self, keys):
        """(mem_src, status, val_off, values) on the host for keys (bytes), through a reader without tables."""
        import torch

        from sstables.merger import check_status, on_device_stream

        n = len(keys)
        with torch.cuda.device(self.device):
            ctx = L.default_ctx(self.device)
            if n > self._reader_cap:
                self._free_reader()
                h, cap = ctypes.c_void_p(), max(n, 1024)
                check_status(L.lib().rio_db_reader_create(ctx, None, cap, ctypes.byref(h)), "rio_db_reader_create")
                self._reader, self._reader_cap = h, cap

            def run(st):
                d_keys, d_off, nbytes = upload_queries(self.device, keys)
                return read_piece(ctx, self.device, st, self._reader, None, index_array([self]), d_keys.data_ptr(),
                                  d_off.data_ptr(), n, nbytes)

            mem, _, status, val_off, values = on_device_stream(self.device, run)
            return ([x & _NONE for x in mem.cpu().tolist()], status.cpu().tolist(), val_off.cpu().tolist(),
                    bytes(values.cpu().numpy()))

    def GetBatch(self, keys):  # noqa: N802
        """[(value, err)] per key: what a loop of MemStore.Get returns (KeyNotFound / KeyTombstoned themselves)."""
        keys = [_key(k) for k in keys]
        err = self.rejected()
        if err is not None:
            return [(None, err) for _ in keys]
        if not keys:
            return []
        mem, status, off, val = self._get(keys)
        return [(val[off[i]:off[i + 1]], None) if s == L.RIO_GET_MEM_VALUE
                else (None, KeyNotFound if mem[i] == _NONE else KeyTombstoned) for i, s in enumerate(status)]

    def ContainsBatch(self, keys):  # noqa: N802
        """[found] per key: what a loop of MemStore.Contains returns. A log the device refuses raises its error
        (a bool cannot carry it)."""
        keys = [_key(k) for k in keys]
        err = self.rejected()
        if err is not None:
            raise err
        if not keys:
            return []
        return [s == L.RIO_GET_MEM_VALUE for s in self._get(keys)[1]]

    def Get(self, key):  # noqa: N802
        return self.GetBatch([key])[0]

    def Contains(self, key) -> bool:  # noqa: N802
        return self.ContainsBatch([key])[0]


class _Iterator:
    """SkipListSStableIterator (memstore/sstable_iterator.go): keys ascending, nil for a tombstoned key."""

    def __init__(self, items):
        self.items, self.i = items, 0

    def Next(self):  # noqa: N802
        from sstables import Done

        if self.i >= len(self.items):
            return None, None, Done
        k, v = self.items[self.i]
        self.i += 1
        return k, v, None


class MemStore:
    def __init__(self, device: int = 0):
        self.device = device
        self._latest = {}  # key -> latest value, None when tombstoned
        self._size = 0     # estimatedSize
        # the op log
        self._keys, self._values = bytearray(), bytearray()
        self._key_off, self._val_off = [0], [0]
        self._flags = bytearray()
        self._max_key_len = 0
        self._idx, self._idx_n = None, -1  # DeviceMemIndex over the device log, and the log length it covers
        self._dev_log = None               # DeviceOpLog: the ops uploaded so far

    def _index(self) -> "DeviceMemIndex":
        """The device index of the log as it stands. Only the ops added since the last index are uploaded
        (DeviceOpLog.append_host) and the index is extended by them (rio_mem_index_extend), whatever their share of
        the log: DESIGN.md §6 has the extend below the rebuild for every measured tail."""
        import numpy as np

        n = len(self._flags)
        if self._idx is None or self._idx_n != n:
            if self._dev_log is None:
                self._dev_log = DeviceOpLog(self.device, ops_cap=max(n, 1024), keys_cap=max(2 * len(self._keys), 1 << 16),
                                            values_cap=max(2 * len(self._values), 1 << 16))
            log = self._dev_log
            a, kb, vb = log.n, log.key_bytes, log.value_bytes
            log.append_host(self._keys[kb:], np.asarray(self._key_off[a:], dtype=np.int64) - kb, self._values[vb:],
                            np.asarray(self._val_off[a:], dtype=np.int64) - vb, self._flags[a:])
            self._idx = DeviceMemIndex(log) if self._idx is None else self._idx.extend(log)
            self._idx_n = n
        return self._idx

    def GetBatch(self, keys):  # noqa: N802
        """[(value, err)] per key, equal to a loop of Get; the search runs on the device. A memstore with a key
        longer than RIO_FLUSH_MAX_KEY_LEN returns UnsupportedError per key, as its flush does."""
        return self._index().GetBatch(keys)

    def ContainsBatch(self, keys):  # noqa: N802
        """[found] per key, equal to a loop of Contains; raises UnsupportedError for such a memstore."""
        return self._index().ContainsBatch(keys)

    def _log(self, key: bytes, value):
        self._keys += key
        self._key_off.append(len(self._keys))
        if value is not None:
            self._values += value
        self._val_off.append(len(self._values))
        self._flags.append(L.RIO_FLAG_NIL if value is None else 0)
        self._max_key_len = max(self._max_key_len, len(key))

    def _upsert(self, key, value, error_if_exists: bool):
        if key is None:
            return KeyNil
        if value is None:
            return ValueNil
        key, value = bytes(key), bytes(value)
        if key in self._latest:
            prev = self._latest[key]
            if prev is not None and error_if_exists:
                return KeyAlreadyExists
            self._size += len(value) - (0 if prev is None else len(prev))
        else:
            self._size += len(key) + len(value)
        self._latest[key] = value
        self._log(key, value)
        return None

    def Add(self, key, value):  # noqa: N802
        return self._upsert(key, value, True)

    def Upsert(self, key, value):  # noqa: N802
        return self._upsert(key, value, False)

    def Contains(self, key) -> bool:  # noqa: N802
        return self._latest.get(_key(key)) is not None

    def IsTombstoned(self, key) -> bool:  # noqa: N802
        key = _key(key)
        return key in self._latest and self._latest[key] is None

    def Get(self, key):  # noqa: N802
        key = _key(key)
        if key not in self._latest:
            return None, KeyNotFound
        v = self._latest[key]
        if v is None:
            return None, KeyTombstoned
        return v, None

    def _delete(self, key, error_if_not_found: bool):
        key = _key(key)
        if key not in self._latest:
            return KeyNotFound if error_if_not_found else None
        prev = self._latest[key]
        self._size -= 0 if prev is None else len(prev)
        self._latest[key] = None
        self._log(key, None)
        return None

    def Delete(self, key):  # noqa: N802
        return self._delete(key, True)

    def DeleteIfExists(self, key):  # noqa: N802
        return self._delete(key, False)

    def Tombstone(self, key):  # noqa: N802
        key = _key(key)
        if key in self._latest:
            return self._delete(key, False)
        self._latest[key] = None
        self._size += len(key)
        self._log(key, None)
        return None

    def EstimatedSizeInBytes(self) -> int:  # noqa: N802
        # uint64(1.15 * float32(m.estimatedSize)): the product of two float32 values, rounded to float32
        return int(_f32(_f32(1.15) * _f32(float(self._size))))

    def Size(self) -> int:  # noqa: N802
        return len(self._latest)

    def SStableIterator(self):  # noqa: N802
        return _Iterator(sorted(self._latest.items()))

    def Flush(self, *writer_options):  # noqa: N802
        """MemStore.Flush: keys whose latest op is a tombstone are left out."""
        return self._flush(L.RIO_FLUSH_SKIP_TOMBSTONES, writer_options)

    def FlushWithTombstones(self, *writer_options):  # noqa: N802
        """MemStore.FlushWithTombstones: tombstoned keys are written with nil values."""
        return self._flush(L.RIO_FLUSH_WITH_TOMBSTONES, writer_options)

    def _op_key(self, op: int) -> bytes:
        return bytes(self._keys[self._key_off[op]:self._key_off[op + 1]])

    def _flush(self, mode, writer_options):
        return _flush_log(self.device, lambda: upload_ops(self.device, self._keys, self._key_off, self._values, self._val_off,
                                                          self._flags, self._max_key_len),
                          self._max_key_len, mode, writer_options, self._op_key)


def _flush_log(device: int, ops_of, max_key_len: int, mode, writer_options, op_key):
    """MemStore.Flush / FlushWithTombstones of an op log: the writer options' errors first, then ops_of() (the log on
    the device: anything with `view`, made under torch.cuda.device(device)) through flush_ops_on_device into the
    table's three files. op_key(op) -> the key bytes of op, for the table's min / max keys."""
    import torch

    from sstables import UnsupportedError, _WriterOpts, writer_filter
    from sstables.merger import write_table_files

    o = _WriterOpts()
    for f in writer_options:
        f(o)
    if not o.basePath:
        return GoError("basePath was not supplied")  # sstable_writer.go:232
    if o.dataCompressionType not in (L.COMP_NONE, L.COMP_SNAPPY):
        return UnsupportedError(f"output data compression {o.dataCompressionType}: the device encodes none and snappy")
    flt, err = writer_filter(o)  # sstable_writer.go:239-241, :78-83
    if err is not None:
        return err
    if max_key_len > L.RIO_FLUSH_MAX_KEY_LEN:
        return UnsupportedError(f"a key of {max_key_len} bytes: the device flush orders keys of up to "
                                f"{L.RIO_FLUSH_MAX_KEY_LEN}")
    with torch.cuda.device(device):
        ops = ops_of()
        view = ops.view
        c = flush_ops_on_device(L.default_ctx(device), device, view, mode, o.dataCompressionType,
                                max_key_len=max_key_len, flt=flt)
        if c.status is not None:
            return GoError(f"memstore flush '{o.basePath}': op {c.unsorted_table} of the log was rejected")
        lo = hi = b""
        if c.n_out:
            first, last = (int(x) & _NONE for x in c.out_src[[0, c.n_out - 1]].cpu().tolist())
            lo, hi = op_key(first), op_key(last)
        write_table_files(o.basePath, c, lo, hi)
    return None


def NewMemStore(device: int = 0) -> MemStore:  # noqa: N802
    return MemStore(device)


class SizePlan:
    """What rio_mem_size_scan found for a batch over a DeviceMemStore (DeviceMemStore.PlanUntilFull): the ops the
    store takes before db.PutBytes would rotate (`n_applied`; `cut`: whether it rotates after them), the raw size
    after them and where the batch's arenas split."""

    def __init__(self, ops, n_applied: int, cut: bool, size: int, key_end: int, value_end: int):
        self.ops, self.n_applied, self.cut = ops, n_applied, cut
        self.size, self.key_end, self.value_end = size, key_end, value_end


class DeviceMemStore:
    """The memstore kept on the device: a DeviceOpLog and the DeviceMemIndex over it. Apply(batch) appends a batch's
    op log (what simpledb.append_batch returns, without a host copy; a DeviceOpLog; or a simpledb.WriteBatch, which is
    uploaded) and extends the index by it; the reads are the index's, Size() is its n_keys word, Flush /
    FlushWithTombstones go through flush_ops_on_device over the log where it lies. There is no host dict: the point
    calls that need one (Add's KeyAlreadyExists, Delete's KeyNotFound) are MemStore's. The size estimate is kept
    without one: rio_mem_size_scan (csrc/rio_memsize.hip) gives the raw estimatedSize after every op of a batch from
    the index as it stands, so EstimatedSizeInBytes() is what a loop of RWMemstore.Upsert / Delete over every batch
    so far leaves, and ApplyUntilFull(batch, max_size) stops where db.PutBytes would rotate (db.go:299)."""

    def __init__(self, device: int = 0, **caps):
        self.device = device
        self.log = DeviceOpLog(device, **caps)
        self._idx = None
        self._size = 0            # estimatedSize (raw, before the 1.15 scaling) ...
        self._size_result = None  # ... or the result block of the last Apply's scan, not read back yet

    def _raw_size(self) -> int:
        if self._size_result is not None:
            r, self._size_result = self._size_result, None
            self._size = int(r[L.RIO_SIZE_R_SIZE].item()) & _NONE
        return self._size

    def EstimatedSizeInBytes(self) -> int:  # noqa: N802
        # uint64(1.15 * float32(m.estimatedSize)), as MemStore.EstimatedSizeInBytes
        return int(_f32(_f32(1.15) * _f32(float(self._raw_size()))))

    def _scan(self, ops, max_size: int):
        """rio_mem_size_scan of `ops` over the store as it stands -> (d_size, d_result) on the device. Call under
        torch.cuda.device(self.device), before the ops are appended."""
        import torch

        from sstables.merger import check_status, on_device_stream

        dev, n = f"cuda:{self.device}", int(ops.view.n)
        d_size = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        d_result = torch.empty(L.RIO_SIZE_RESULT_WORDS, dtype=torch.int64, device=dev)
        size0 = self._raw_size()
        store = None if self._idx is None else self._idx.view
        bv = ops.view
        bound = min(int(getattr(ops, "max_key_len", L.RIO_FLUSH_MAX_KEY_LEN)), L.RIO_FLUSH_MAX_KEY_LEN)
        on_device_stream(self.device, lambda st: check_status(
            L.lib().rio_mem_size_scan(L.default_ctx(self.device), None if store is None else ctypes.addressof(store), size0,
                                      ctypes.addressof(bv), bound, max_size & _NONE, d_size.data_ptr(),
                                      d_result.data_ptr(), st), "rio_mem_size_scan"))
        return d_size, d_result

    def _append(self, ops):
        self.log.append(ops)
        self._idx = DeviceMemIndex(self.log) if self._idx is None else self._idx.extend(self.log)

    def Apply(self, batch):  # noqa: N802
        import torch

        with torch.cuda.device(self.device):
            ops = batch.upload(self.device) if hasattr(batch, "upload") else batch
            if int(ops.view.n):  # no cut: the block's SIZE word is the size after the whole batch, read when asked for
                self._size_result = self._scan(ops, _NONE)[1]
        self._append(ops)
        return None

    def PlanUntilFull(self, batch, max_size: int):  # noqa: N802
        """The scan alone -> (SizePlan, err): how many ops of `batch` (a DeviceOps with its tensors, a DeviceOpLog, or a
        simpledb.WriteBatch, which is uploaded) a loop of db.PutBytes / db.DeleteBytes applies before it rotates a
        memstore of max_size bytes. The store is not changed; ApplyPlanned(plan) applies those ops. One host read:
        the scan's 64-byte result block."""
        import torch

        with torch.cuda.device(self.device):
            ops = batch.upload(self.device) if hasattr(batch, "upload") else batch
            n = int(ops.view.n)
            if n == 0:
                return SizePlan(ops, 0, False, self._raw_size(), 0, 0), None
            r = [x & _NONE for x in self._scan(ops, max_size)[1].cpu().tolist()]
        if r[L.RIO_SIZE_R_FIRST_BAD] != _NONE:
            return None, GoError(f"memstore size scan: op {r[L.RIO_SIZE_R_FIRST_BAD]} of the batch was rejected")
        cut = r[L.RIO_SIZE_R_CUT]
        return SizePlan(ops, n if cut == _NONE else cut + 1, cut != _NONE, r[L.RIO_SIZE_R_SIZE], r[L.RIO_SIZE_R_KEY_END],
                        r[L.RIO_SIZE_R_VALUE_END]), None

    def ApplyPlanned(self, plan: "SizePlan"):  # noqa: N802
        """Appends the plan's first n_applied ops (a prefix view of the batch's arrays) and returns the rest of the
        batch as a DeviceOps, or None: slices of the batch's tensors, the offsets rebased to 0 as rio_ops_append asks."""
        import torch

        ops, k = plan.ops, plan.n_applied
        n = int(ops.view.n)
        if k == 0:
            return None if n == 0 else ops
        kb, vb = int(ops.view.key_bytes), int(ops.view.value_bytes)
        with torch.cuda.device(self.device):
            head = ops if k == n else DeviceOps(self.device, ops.keys, ops.key_off, ops.values, ops.val_off, ops.flags, k,
                                                plan.key_end, plan.value_end, ops.max_key_len)
            self._append(head)
            self._size, self._size_result = plan.size, None
            if k == n:
                return None
            return DeviceOps(self.device, ops.keys[plan.key_end:], ops.key_off[k:n + 1] - plan.key_end,
                             ops.values[plan.value_end:], ops.val_off[k:n + 1] - plan.value_end, ops.flags[k:], n - k,
                             kb - plan.key_end, vb - plan.value_end, ops.max_key_len)

    def ApplyUntilFull(self, batch, max_size: int):  # noqa: N802
        """Applies the ops of `batch` up to and including the put after which db.PutBytes rotates (db.go:299), or the
        whole batch -> (n_applied, rest): rest is a DeviceOps over the remaining ops, or None. A batch the device
        rejects raises its error and leaves the store as it was."""
        plan, err = self.PlanUntilFull(batch, max_size)
        if err is not None:
            raise err
        return plan.n_applied, self.ApplyPlanned(plan)

    def _index(self) -> "DeviceMemIndex":
        if self._idx is None:
            self._idx = DeviceMemIndex(self.log)
        return self._idx

    def GetBatch(self, keys):  # noqa: N802
        return self._index().GetBatch(keys)

    def ContainsBatch(self, keys):  # noqa: N802
        return self._index().ContainsBatch(keys)

    def Get(self, key):  # noqa: N802
        return self._index().Get(key)

    def Contains(self, key) -> bool:  # noqa: N802
        return self._index().Contains(key)

    def Size(self) -> int:  # noqa: N802
        """The distinct keys, tombstoned ones included (MemStore.Size): the index's n_keys, read from the device."""
        return self._index().n_keys()

    def _op_key(self, op: int) -> bytes:
        a, b = self.log.key_off[op:op + 2].cpu().tolist()
        return bytes(self.log.keys[a:b].cpu().numpy())

    def Flush(self, *writer_options):  # noqa: N802
        return _flush_log(self.device, lambda: self.log, self.log.max_key_len, L.RIO_FLUSH_SKIP_TOMBSTONES, writer_options,
                          self._op_key)

    def FlushWithTombstones(self, *writer_options):  # noqa: N802
        return _flush_log(self.device, lambda: self.log, self.log.max_key_len, L.RIO_FLUSH_WITH_TOMBSTONES, writer_options,
                          self._op_key)
