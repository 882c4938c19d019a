"""SuperSSTableReader mirror (sstables/super_sstable_reader.go:11-182) over tables loaded on the device.

A stack of open SSTableReaders, oldest first (the reference's order: position is age, the last reader is the
newest). Contains / Get are the reference's loops over the readers' own calls, on the host. ContainsBatch /
GetBatch answer a batch of keys in one device lookup over the whole stack (rio_sst_stack_lookup, csrc/
rio_stack.hip) and bring the found values out with one gather (rio_sst_stack_value_plan / _value_copy): one
upload of the query arena, one 8-byte read to size the value arena, one read-back. Scan / ScanStartingAt /
ScanRange cut every table on the device (rio_sst_stack_bounds), merge the cut views with the compaction's
plan (rio_sst_merge_plan, RIO_MERGE_LATEST_WINS: the iterator's rule that a key whose newest value is nil
yields nothing while an empty value stays, sstable_merger.go:86,102) and gather values and keys
(rio_sst_merge_gather, rio_sst_keys_gather). The readers' key prefixes and device filters are built at the
first batched call, the stack handle with them. Bytes comparator only. What the device path does not take
(readers that are not open SSTableReaders on one device, tables the merge refuses) returns UnsupportedError:
the adapter keeps the reference reader for it. There is no CPU fallback.
"""
from __future__ import annotations

import ctypes

from recordio import _lib as L
from recordio.errors import GoError

from . import proto

_NONE = 0xFFFFFFFFFFFFFFFF
_ENTRY_MASK = (1 << L.RIO_MERGE_ENTRY_BITS) - 1
DEFAULT_MAX_BATCH = 1 << 20  # queries per stack call; longer batches are split (8 bytes of scratch per query)


def BytesComparator(a, b) -> int:  # noqa: N802
    """skiplist.BytesComparator: bytes.Compare, the only order the device searches and merges in."""
    a, b = bytes(a or b""), bytes(b or b"")
    return (a > b) - (a < b)


class _ListIterator:
    """SSTableIteratorI over the entries a device scan brought back."""

    def __init__(self, items):
        self.items, self.i = items, 0

    def Next(self):  # noqa: N802
        from . import Done

        if self.i >= len(self.items):
            return None, None, Done
        k, v = self.items[self.i]
        self.i += 1
        return k, v, None


class DeviceScan(tuple):
    """(keys, key_off, values, val_off, flags, n_out): a scan's entries as device tensors. Entry j is key
    keys[key_off[j]:key_off[j + 1]] with value values[val_off[j]:val_off[j + 1]]; flags[j] & RIO_FLAG_NIL never
    occurs under latest-wins (such keys are dropped)."""


class SuperSSTableReader:
    def __init__(self, readers, comp=None, max_batch: int = DEFAULT_MAX_BATCH):
        """comp: None or BytesComparator (the reference's default). Another comparator orders MetaData's keys as the
        reference's does; the scans, which merge in byte order on the device, return UnsupportedError for it."""
        self.readers = list(readers)
        self.comp = BytesComparator if comp is None else comp
        self.max_batch = int(max_batch)
        self._stack = None  # rio_sst_stack handle and what it points into, created at the first batched call
        self._keep = None

    # ---- the reference's host loops ---------------------------------------------------------------------------

    def Contains(self, key: bytes):  # noqa: N802
        """super_sstable_reader.go:18-32: newest to oldest, the first table that holds the key answers."""
        for r in reversed(self.readers):
            found, err = r.Contains(key)
            if err is not None:
                return False, err
            if found:
                return True, None
        return False, None

    def Get(self, key: bytes):  # noqa: N802
        """super_sstable_reader.go:34-49: NotFound goes on to the older reader, any other error is returned, a
        nil or empty value of a newer table is the answer."""
        from . import NotFound

        for r in reversed(self.readers):
            v, err = r.Get(key)
            if err is not None:
                if err is NotFound:
                    continue
                return None, err
            return v, None
        return None, NotFound

    def MetaData(self) -> proto.MetaData:  # noqa: N802
        """super_sstable_reader.go:140-169 as written: the sums, the last reader's version, and MinKey and MaxKey
        BOTH replaced whenever the running one compares lower (so MinKey ends as the largest of the readers'
        MinKeys, as MaxKey ends as the largest of their MaxKeys)."""
        s = proto.MetaData()
        for r in self.readers:
            m = r.MetaData()
            s.numRecords += m.numRecords
            s.dataBytes += m.dataBytes
            s.indexBytes += m.indexBytes
            s.totalBytes += m.totalBytes
            s.version = m.version
            if self.comp(s.minKey, m.minKey) < 0:
                s.minKey = m.minKey
            if self.comp(s.maxKey, m.maxKey) < 0:
                s.maxKey = m.maxKey
        return s

    def BasePath(self) -> str:  # noqa: N802
        return ",".join(r.BasePath() for r in self.readers)

    def Close(self):  # noqa: N802
        """Closes every reader (errors.Join of their errors) and frees the stack."""
        self._free_stack()
        errs = [e for e in (r.Close() for r in self.readers) if e is not None]
        return GoError("\n".join(str(e) for e in errs)) if errs else None

    def __del__(self):
        try:
            self._free_stack()
        except Exception:  # interpreter shutdown: the library may be gone
            pass

    # ---- the stack on the device --------------------------------------------------------------------------------

    def _free_stack(self):
        if self._stack is not None:
            h, self._stack, self._keep = self._stack, None, None
            L.lib().rio_sst_stack_free(h)

    def _unsupported(self):
        from . import SSTableReader, UnsupportedError

        rs = self.readers
        if not rs or len(rs) > L.RIO_MERGE_MAX_TABLES:
            return UnsupportedError(f"a stack of {len(rs)} tables (1 .. {L.RIO_MERGE_MAX_TABLES})")
        for r in rs:
            if not isinstance(r, SSTableReader) or r.t is None:
                return UnsupportedError("the stack's readers are open SSTableReaders of NewSSTableReader")
            if r.opts.device != rs[0].opts.device:
                return UnsupportedError("the stack's readers are on different devices")
            if r.t.n_index > r.t.n_data:
                return UnsupportedError(f"sstable '{r.opts.basePath}': a value of the table cannot be read")
        return None

    @property
    def _device(self) -> int:
        return self.readers[0].opts.device

    def _ensure_stack(self, st):
        """The readers' prefixes and device filters, then the stack handle (once)."""
        import torch

        from .merger import check_status, table_view

        if self._stack is not None:
            return
        device = self._device
        lib, ctx = L.lib(), L.default_ctx(device)
        T = len(self.readers)
        views = (L.SstView * T)(*[table_view(r.t) for r in self.readers])
        pfx, filters, stored = (ctypes.c_uint64 * T)(), (L.BloomView * T)(), (ctypes.c_uint64 * T)()
        for t, r in enumerate(self.readers):
            if r._pfx is None:
                r._pfx = torch.empty(max(r.t.n_index, 1), dtype=torch.int64, device=f"cuda:{device}")
                check_status(lib.rio_sst_key_prefixes(ctx, ctypes.byref(views[t]), r._pfx.data_ptr(), st),
                             "rio_sst_key_prefixes")
            pfx[t] = r._pfx.data_ptr()
            f = r.bloomFilter
            if f is not None and f.k <= L.RIO_BLOOM_MAX_K:  # a larger k: ContainsBatch refuses, Get asks no filter
                if r._dfilter is None:
                    r._dfilter = f.on_device(device)
                filters[t] = r._dfilter.view
            # hash checks on reads are a reader's option: a reader without them has no stored checksums here
            stored[t] = 0 if r.opts.skipHashCheckOnRead else r.t.checksum.data_ptr()
        h = ctypes.c_void_p()
        check_status(lib.rio_sst_stack_create(ctx, ctypes.addressof(views), ctypes.addressof(pfx),
                                              ctypes.addressof(filters), ctypes.addressof(stored), T, self.max_batch,
                                              ctypes.byref(h), st), "rio_sst_stack_create")
        self._stack, self._keep = h, views

    @staticmethod
    def _arena(keys):
        import numpy as np

        arena = b"".join(keys)
        off = np.zeros(len(keys) + 1, dtype=np.int64)
        np.cumsum([len(k) for k in keys], out=off[1:])
        return arena, off

    def _upload(self, keys):
        import numpy as np
        import torch

        arena, off = self._arena(keys)
        dev = f"cuda:{self._device}"
        d_keys = torch.from_numpy(np.frombuffer(arena + b"\0", dtype=np.uint8).copy()).to(dev)
        return d_keys, torch.from_numpy(off).to(dev), len(arena)

    def _pieces(self, n):
        return [(a, min(a + self.max_batch, n)) for a in range(0, n, self.max_batch)]

    def ContainsBatch(self, keys):  # noqa: N802
        """[(found, err)] per key: what a loop of Contains returns, in one device lookup over the stack."""
        import torch

        from . import UnsupportedError
        from .merger import check_status, on_device_stream

        keys = [bytes(k) for k in keys]
        err = self._unsupported()
        if err is None:
            for r in self.readers:
                if r.bloomFilter is not None and r.bloomFilter.k > L.RIO_BLOOM_MAX_K:
                    err = UnsupportedError(f"a bloom filter of {r.bloomFilter.k} probes: the device takes up to "
                                           f"{L.RIO_BLOOM_MAX_K}")
                    break
        if err is not None:
            return [(False, err) for _ in keys]
        n = len(keys)
        if n == 0:
            return []
        lib = L.lib()
        with torch.cuda.device(self._device):
            def run(st):
                self._ensure_stack(st)
                d_keys, d_off, nbytes = self._upload(keys)
                src = torch.empty(n, dtype=torch.int64, device=d_keys.device)
                for a, b in self._pieces(n):
                    check_status(lib.rio_sst_stack_lookup(self._stack, 1, d_keys.data_ptr(), d_off.data_ptr() + 8 * a,
                                                          b - a, nbytes, src.data_ptr() + 8 * a, st),
                                 "rio_sst_stack_lookup")
                return src

            src = on_device_stream(self._device, run)
            return [(x != -1, None) for x in src.cpu().tolist()]

    def GetBatchOnDevice(self, d_keys, d_key_off, n: int):  # noqa: N802
        """(src, status, val_off, values) as device tensors for n <= max_batch query keys that are already on the
        device (uint8 arena d_keys, int64 offsets d_key_off[n + 1]); nothing is copied back but the 8 bytes that
        size `values`. src[i] = table << 40 | entry or -1, status[i] one of RIO_GET_*, value i =
        values[val_off[i]:val_off[i + 1]]."""
        import torch

        from .merger import on_device_stream

        err = self._unsupported()
        if err is None and any(r.t.v0 for r in self.readers):
            # v0 values are DataEntry ranges inside the data records, which the value kernels do not unwrap
            from . import UnsupportedError

            err = UnsupportedError("a stack with a v0 table answers GetBatch on the host: no device values")
        if err is not None:
            raise err
        with torch.cuda.device(self._device):
            def run(st):
                self._ensure_stack(st)
                return self._get_piece(st, d_keys.data_ptr(), d_key_off.data_ptr(), n, d_keys.numel())

            return on_device_stream(self._device, run)

    def _get_piece(self, st, p_keys, p_off, n, nbytes):
        import torch

        from .merger import check_status

        lib = L.lib()
        dev = f"cuda:{self._device}"
        src = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        val_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        check_status(lib.rio_sst_stack_lookup(self._stack, 0, p_keys, p_off, n, nbytes, src.data_ptr(), st),
                     "rio_sst_stack_lookup")
        check_status(lib.rio_sst_stack_value_plan(self._stack, src.data_ptr(), n, 1, status.data_ptr(),
                                                  val_off.data_ptr(), st), "rio_sst_stack_value_plan")
        total = int(val_off[n].item())  # the one round trip: the value arena's size
        values = torch.empty(total + L.RIO_DEVICE_PAD, dtype=torch.uint8, device=dev)
        check_status(lib.rio_sst_stack_value_copy(self._stack, src.data_ptr(), n, val_off.data_ptr(), values.data_ptr(),
                                                  total, st), "rio_sst_stack_value_copy")
        return src[:n], status[:n], val_off, values[:total]

    def GetBatch(self, keys):  # noqa: N802
        """[(value, err)] per key: what a loop of Get returns. The search and the value gather run on the device;
        an entry whose read fails (RIO_GET_HOST) gets its error from the owning reader's getValueAtOffset."""
        import torch

        from . import NotFound
        from .merger import on_device_stream

        keys = [bytes(k) for k in keys]
        err = self._unsupported()
        if err is not None:
            return [(None, err) for _ in keys]
        if any(r.t.v0 for r in self.readers):
            # v0 tables keep their values in DataEntry ranges, not in data_off: the host loop answers
            return [self.Get(k) for k in keys]
        n = len(keys)
        if n == 0:
            return []
        with torch.cuda.device(self._device):
            def run(st):
                self._ensure_stack(st)
                d_keys, d_off, nbytes = self._upload(keys)
                return [self._get_piece(st, d_keys.data_ptr(), d_off.data_ptr() + 8 * a, b - a, nbytes)
                        for a, b in self._pieces(n)]

            out = []
            for src, status, val_off, values in on_device_stream(self._device, run):
                h_src, h_status, h_off = src.cpu().tolist(), status.cpu().tolist(), val_off.cpu().tolist()
                h_val = bytes(values.cpu().numpy())
                for i, s in enumerate(h_status):
                    if s == L.RIO_GET_VALUE:
                        out.append((h_val[h_off[i]:h_off[i + 1]], None))
                    elif s == L.RIO_GET_NIL:
                        out.append((None, None))
                    elif s == L.RIO_GET_HOST:
                        w = h_src[i] & _NONE
                        r = self.readers[w >> L.RIO_MERGE_ENTRY_BITS]
                        v, e = r._value_at(w & _ENTRY_MASK, r.opts.skipHashCheckOnRead)
                        out.append((None, e) if e is not None else (v, None))  # Get drops the value beside an error
                    else:
                        out.append((None, NotFound))
            return out

    # ---- scans ------------------------------------------------------------------------------------------------

    def Scan(self):  # noqa: N802
        return self._scan(None, None, False)

    def ScanStartingAt(self, key: bytes):  # noqa: N802
        return self._scan(bytes(key), None, False)

    def ScanRange(self, key_lower: bytes, key_higher: bytes):  # noqa: N802
        return self._scan(bytes(key_lower), bytes(key_higher), False)

    def ScanOnDevice(self):  # noqa: N802
        return self._scan(None, None, True)

    def ScanStartingAtOnDevice(self, key: bytes):  # noqa: N802
        return self._scan(bytes(key), None, True)

    def ScanRangeOnDevice(self, key_lower: bytes, key_higher: bytes):  # noqa: N802
        return self._scan(bytes(key_lower), bytes(key_higher), True)

    def _cuts(self, st, lo, hi):
        """[(start, end)] per table: IteratorStartingAt's / IteratorBetween's entries (both ends inclusive)."""
        import torch

        from .merger import check_status

        T = len(self.readers)
        ends = [r.t.n_index for r in self.readers]
        if lo is None:
            return [(0, e) for e in ends]
        lib = L.lib()
        d_keys, d_off, nbytes = self._upload([lo] if hi is None else [lo, hi])
        pos = torch.empty(2 * T, dtype=torch.int64, device=d_keys.device)
        check_status(lib.rio_sst_stack_bounds(self._stack, d_keys.data_ptr(), d_off.data_ptr(), 1, nbytes, 0,
                                              pos.data_ptr(), st), "rio_sst_stack_bounds")
        if hi is not None:
            check_status(lib.rio_sst_stack_bounds(self._stack, d_keys.data_ptr(), d_off.data_ptr() + 8, 1, nbytes, 1,
                                                  pos.data_ptr() + 8 * T, st), "rio_sst_stack_bounds")
        h = pos.cpu().tolist()
        if hi is not None:
            ends = h[T:]
        return [(s, max(s, e)) for s, e in zip(h[:T], ends)]

    def _scan(self, lo, hi, on_device):
        import torch

        from . import UnsupportedError
        from .merger import check_status, on_device_stream, refuse_inputs, table_view

        err = self._unsupported()
        if err is None and self.comp is not BytesComparator:
            err = UnsupportedError("the device scans merge in byte order: BytesComparator only")
        if err is not None:
            return None, err
        if lo is not None and hi is not None and lo > hi:
            return self.readers[0].ScanRange(lo, hi)  # the reference asks the readers in order: the first one's error
        err = refuse_inputs(self.readers)
        if err is not None:
            return None, err
        device = self._device
        dev = f"cuda:{device}"
        lib, ctx = L.lib(), L.default_ctx(device)
        i64 = lambda n: torch.empty(max(n, 1), dtype=torch.int64, device=dev)  # noqa: E731
        u8 = lambda n: torch.empty(max(n, 1), dtype=torch.uint8, device=dev)  # noqa: E731

        def run(st):
            if lo is not None:  # a plain Scan cuts nothing: it needs no stack
                self._ensure_stack(st)
            cuts = self._cuts(st, lo, hi)
            T = len(self.readers)
            views = (L.SstView * T)()
            for t, (r, (a, b)) in enumerate(zip(self.readers, cuts)):
                v = table_view(r.t)
                # the table's view with every array advanced by the start; data_off keeps n + 1 entries
                v.key_off, v.key_len, v.data_off, v.crc = (p + 8 * a for p in (v.key_off, v.key_len, v.data_off, v.crc))
                v.flags = v.flags + a
                v.n = b - a
                views[t] = v
            n_in = sum(v.n for v in views)
            src, keep, res = i64(n_in), u8(n_in), i64(L.RIO_MERGE_RESULT_WORDS)
            check_status(lib.rio_sst_merge_plan(ctx, ctypes.addressof(views), T, L.RIO_MERGE_LATEST_WINS, src.data_ptr(),
                                                keep.data_ptr(), res.data_ptr(), st), "rio_sst_merge_plan")
            r = [x & _NONE for x in res.cpu().tolist()]
            if r[L.RIO_MERGE_R_UNSORTED] != _NONE:
                return UnsupportedError(f"sstable '{self.readers[r[L.RIO_MERGE_R_UNSORTED]].opts.basePath}': keys are "
                                        "not strictly ascending")
            n, vbytes, kbytes = r[L.RIO_MERGE_R_N_OUT], r[L.RIO_MERGE_R_VALUE_BYTES], r[L.RIO_MERGE_R_KEY_BYTES]
            out_src, val_off, flags, key_off = i64(n), i64(n + 1), u8(n), i64(n + 1)
            values, keys = u8(vbytes + L.RIO_DEVICE_PAD), u8(kbytes + L.RIO_DEVICE_PAD)
            check_status(lib.rio_sst_merge_gather(ctx, src.data_ptr(), keep.data_ptr(), n, out_src.data_ptr(),
                                                  values.data_ptr(), values.numel(), val_off.data_ptr(), flags.data_ptr(),
                                                  st), "rio_sst_merge_gather")
            check_status(lib.rio_sst_keys_gather(ctx, out_src.data_ptr(), n, keys.data_ptr(), keys.numel(),
                                                 key_off.data_ptr(), st), "rio_sst_keys_gather")
            return DeviceScan((keys[:kbytes], key_off, values[:vbytes], val_off, flags[:n], n))

        with torch.cuda.device(device):
            out = on_device_stream(device, run)
            if isinstance(out, GoError):
                return None, out
            if on_device:
                return out, None
            keys, key_off, values, val_off, flags, n = out
            hk, hv = bytes(keys.cpu().numpy()), bytes(values.cpu().numpy())
            ko, vo = key_off.cpu().tolist(), val_off.cpu().tolist()
            return _ListIterator([(hk[ko[j]:ko[j + 1]], hv[vo[j]:vo[j + 1]]) for j in range(n)]), None


def NewSuperSSTableReader(readers, comp=None, max_batch: int = DEFAULT_MAX_BATCH):  # noqa: N802
    """super_sstable_reader.go:180-182. comp: None or BytesComparator for the device scans."""
    return SuperSSTableReader(readers, comp, max_batch)
