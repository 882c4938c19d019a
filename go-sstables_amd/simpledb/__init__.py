"""simpledb's crash recovery on the device: a WAL directory to one SSTable.

recover_wal mirrors replayAndSetupWriteAheadLog (simpledb/recovery.go:208-268) without the DB object. The
reference joins its stages with one host loop: proto.Unmarshal of every WAL record into a WalMutation, then
memStore.Upsert / Tombstone, then FlushWithTombstones. Here the decoded WAL stays in HBM: rio_wal_ops_plan /
rio_wal_ops_gather (csrc/rio_walops.hip) turn the decoded records into the op log rio_sst_flush_plan takes, and
the flush's back end writes the table. The host reads the plan's 64-byte result block, then what the flush
reads.

The write side is batched the same way: a WriteBatch holds db.PutBytes / db.DeleteBytes calls (db.go:256-347) as
the memstore's op log, append_batch marshals every op into its WalMutation record on the device
(rio_wal_ops_encode, csrc/rio_walenc.hip), frames the records into WAL file images (rio_device_encode) and
writes them through wal.Appender.AppendFramed; the same device arrays then go to memstore.flush_ops_on_device.

The read side is DBReadView: db.GetBytes (db.go:197-242) over a table stack and the memstore pair (RWMemstore,
rw_memstore.go), one key at a time on the host as the reference runs it, and a batch of keys on the device
(rio_sst_stack_lookup, rio_mem_lookup, rio_db_value_plan / _copy; csrc/rio_memidx.hip, csrc/rio_db.hip). A store
may be a memstore.DeviceMemIndex: a log that append_batch returned or wal_ops_on_device recovered is read without
ever having been on the host.

The DB object ties them together: NewSimpleDB / Open / Apply / Put / Get / Close (db.go, flush.go,
recovery.go:117-277). DB.Apply(WriteBatch) leaves what a loop of PutBytes / DeleteBytes leaves: the op at which the
loop rotates the WAL and the memstore (db.go:299, the size check after every put) comes from rio_mem_size_scan
(csrc/rio_memsize.hip) over the device memstore. The flush runs inline.

Compaction (compaction.go, sstable_manager.go, recovery.go:22-114) is opt-in, CompactOnDevice(): the selection
(candidate_tables_for_compaction) and the crash-safe directory protocol (repair_compactions, the compaction_successful
record) are host functions that need no GPU; the merge is SSTableMerger.MergeCompact over the DB's own resident readers,
and the compacted table enters the stack from the buffers the merge left in HBM (sstables._DeviceTable.from_compaction),
without reading its files back. Functions return Go-style error values. There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
import shutil
import struct
import tempfile
import types

from recordio import _lib as L
from recordio.errors import EOF, ErrUnsupported, GoError, errors_is, wrap

from . import proto

_NONE = 0xFFFFFFFFFFFFFFFF
# protobuf-go's error prefix; it varies the space after the colon per binary (U+0020 or U+00A0): U+0020 here
_PROTO_PREFIX = "proto: "


def _record_error(cls: int, record):
    """The error `process` returns for the record the plan refused (recovery.go:215-239)."""
    from memstore import ValueNil

    if cls == L.RIO_WAL_BAD_VALUE_NIL:
        return ValueNil
    if cls in (L.RIO_WAL_BAD_PROTO, L.RIO_WAL_BAD_UTF8):
        try:
            proto.unmarshal_wal_mutation(record)
        except proto.InvalidUTF8Error as e:
            return GoError(_PROTO_PREFIX + str(e))
        except proto.WireError:
            pass
        return GoError(_PROTO_PREFIX + "cannot parse invalid wire-format data")
    return GoError("the decoded record's range leaves its arena")


def _cut(path, buf, info):
    """The replayer's rules for one decoded file (wal.Replayer._replay_device / _deliver): -> (records to
    replay, the error that ends the replay after them or None)."""
    from recordio.reader import _open_error, read_next_error
    from wal import _EOF_CLASS

    st = info["status"]
    if st in (L.RIO_ERR_VERSION, L.RIO_ERR_COMPRESSION_TYPE, L.RIO_ERR_SHORT_FILE_HEADER):
        return 0, wrap(f"error while opening WAL reader under '{path}'",
                       _open_error(st, path, info["detail0"], "file", os.path.getsize(path)))
    if st == L.RIO_ERR_UNSUPPORTED:
        return 0, wrap(f"error while reading WAL records under '{path}'", ErrUnsupported)
    n = info["n_records"]
    if info["n_bad"] and info["first_bad"] < n:
        bad = info["first_bad"]
        if int(buf.flags[bad].item()) & L.RIO_FLAG_EOF:  # gzip's bare io.EOF ends this file (replayer.go:60-63)
            return bad, None
        return bad, wrap(f"error while reading WAL records under '{path}'",
                         read_next_error(L.RIO_ERR_DECOMPRESS, path, 0, 0))
    if st not in _EOF_CLASS:
        err = read_next_error(st, path, info["detail0"], info["detail1"])
        if not errors_is(err, EOF):
            return n, wrap(f"error while reading WAL records under '{path}'", err)
    return n, None


def wal_ops_on_device(ctx, device: int, segments, mark=None):
    """rio_wal_ops_plan, the result read and rio_wal_ops_gather on torch's current stream. `segments` is a
    ctypes array of WalSegment. Returns (result words, tensors): the tensors are None when a record was
    refused, else a dict of keys / key_off / values / val_off / flags / op_rec and the OpsView over them.
    `mark(name)` as for sstables.merger.compact_on_device."""
    import torch

    from sstables.merger import check_status, on_device_stream

    mark = mark or (lambda name: None)
    lib, dev = L.lib(), f"cuda:{device}"
    i64 = lambda n: torch.empty(max(n, 1), dtype=torch.int64, device=dev)  # noqa: E731
    u8 = lambda n: torch.empty(max(n, 1), dtype=torch.uint8, device=dev)  # noqa: E731

    def run(st):
        res = i64(L.RIO_WAL_RESULT_WORDS)
        check_status(lib.rio_wal_ops_plan(ctx, ctypes.addressof(segments), len(segments), res.data_ptr(), st),
                     "rio_wal_ops_plan")
        mark("wal_plan")
        r = [x & _NONE for x in res.cpu().tolist()]  # the one host round trip: the gather's outputs are sized here
        mark("wal_result_read")
        if r[L.RIO_WAL_R_FIRST_BAD] != _NONE:
            return r, None
        n, kb, vb = r[L.RIO_WAL_R_N_OPS], r[L.RIO_WAL_R_KEY_BYTES], r[L.RIO_WAL_R_VALUE_BYTES]
        t = dict(keys=u8(kb + L.RIO_DEVICE_PAD), key_off=i64(n + 1), values=u8(vb + L.RIO_DEVICE_PAD),
                 val_off=i64(n + 1), flags=u8(n), op_rec=i64(n))
        check_status(lib.rio_wal_ops_gather(ctx, n, t["keys"].data_ptr(), kb, t["key_off"].data_ptr(),
                                            t["values"].data_ptr(), vb, t["val_off"].data_ptr(), t["flags"].data_ptr(),
                                            t["op_rec"].data_ptr(), st), "rio_wal_ops_gather")
        mark("wal_gather")
        t["view"] = L.OpsView(keys=t["keys"].data_ptr(), key_off=t["key_off"].data_ptr(), values=t["values"].data_ptr(),
                              val_off=t["val_off"].data_ptr(), flags=t["flags"].data_ptr(), n=n, key_bytes=kb,
                              value_bytes=vb)
        return r, t

    return on_device_stream(device, run)


def recover_wal(base_path: str, table_path: str, device: int = 0, compression: int = L.COMP_SNAPPY,
                bloom_filter: bool = False, bloom_fp_probability: float = 0.01):
    """Replay the WAL directory `base_path` into one SSTable at `table_path` (FlushWithTombstones), then
    empty the directory (recovery.go:208-268). Returns (num_records, wrote_table, err). The error is the
    earliest in replay order, with wal.Replayer's texts and wrapping; on any error no table is written and the
    directory is left untouched. No table is written when no record holds an op (executeFlush skips an empty
    memstore, flush.go:37). bloom_filter: also write the table's bloom.bf.gz, sized for the memstore's
    size (its distinct keys), as executeFlush sizes it (flush.go:35,55); off by default here."""
    import torch

    from memstore import flush_ops_on_device
    from recordio.device import DeviceDecoder, to_device_file
    from sstables import UnsupportedError, _WriterOpts, writer_filter
    from sstables.merger import write_table_files
    from wal import _wal_files

    if compression not in (L.COMP_NONE, L.COMP_SNAPPY):
        return 0, False, UnsupportedError(f"output data compression {compression}: the device encodes none and snappy")
    flt = None
    if bloom_filter:
        _, err = writer_filter(_WriterOpts(basePath=table_path, enableBloomFilter=True,
                                           bloomFpProbability=bloom_fp_probability))
        if err is not None:  # a probability NewOptimal refuses, before anything is read
            return 0, False, err

        def flt(n_out):  # FlushWithTombstones keeps every key of the memstore: n_out is its size
            return writer_filter(_WriterOpts(basePath=table_path, enableBloomFilter=True, bloomExpectedNumberOfElements=n_out,
                                             bloomFpProbability=bloom_fp_probability))[0]
    try:
        paths = _wal_files(base_path)
    except OSError as e:
        return 0, False, GoError(f"error while walking WAL structure under '{base_path}': {e}")
    with torch.cuda.device(device):
        ctx = L.default_ctx(device)
        dec = DeviceDecoder(device)
        # upload and decode, device-resident; a file that cannot be read ends the replay where it stands
        files, tail_err = [], None
        for path in paths:
            try:
                with open(path, "rb") as fh:
                    files.append(to_device_file(fh.read(), device))
            except OSError as e:
                tail_err = GoError(f"error while creating WAL reader under '{path}': {e}")
                break
        decoded = []
        batch = 16  # rio_device_decode_batch's file limit
        for k in range(0, len(files), batch):
            decoded += dec.decode_batch(files[k:k + batch])  # loops on RIO_ERR_CAPACITY
        segs, seg_paths = [], []
        for path, (buf, info) in zip(paths, decoded):
            n, err = _cut(path, buf, info)
            segs.append(L.WalSegment(out=buf.out.data_ptr(), out_off=buf.out_off.data_ptr(), flags=buf.flags.data_ptr(),
                                     n=n, out_bytes=info["total_out_bytes"]))
            seg_paths.append(path)
            if err is not None:
                tail_err = err
                break
        if not segs:
            if tail_err is not None:
                return 0, False, tail_err
            return 0, False, _reset_dir(base_path)
        segments = (L.WalSegment * len(segs))(*segs)
        r, t = wal_ops_on_device(ctx, device, segments)
        bad = r[L.RIO_WAL_R_FIRST_BAD]
        if bad != _NONE:  # a refused record comes before the error that ended the replay after the records
            cls, g = r[L.RIO_WAL_R_BAD_CLASS], bad
            for s, (path, (buf, _)) in enumerate(zip(seg_paths, decoded)):
                if g < segs[s].n:
                    break
                g -= segs[s].n
            record = None
            if cls != L.RIO_WAL_BAD_RANGE and not int(buf.flags[g].item()) & L.RIO_FLAG_NIL:
                o0, o1 = buf.out_off[g:g + 2].cpu().tolist()
                record = bytes(buf.out[o0:o1].cpu().numpy())
            err = wrap(f"error while processing WAL record under '{path}'", _record_error(cls, record))
            # numRecords counts a record once it unmarshals (recovery.go:222), before the memstore refuses it
            return bad + (cls == L.RIO_WAL_BAD_VALUE_NIL), False, err
        n_records = r[L.RIO_WAL_R_N_RECORDS]
        if tail_err is not None:
            return n_records, False, tail_err
        wrote = False
        if r[L.RIO_WAL_R_N_OPS]:
            max_key = r[L.RIO_WAL_R_MAX_KEY_LEN]
            if max_key > L.RIO_FLUSH_MAX_KEY_LEN:
                return n_records, False, UnsupportedError(
                    f"a key of {max_key} bytes: the device flush orders keys of up to {L.RIO_FLUSH_MAX_KEY_LEN}")
            c = flush_ops_on_device(ctx, device, t["view"], L.RIO_FLUSH_WITH_TOMBSTONES, compression, max_key_len=max_key,
                                    flt=flt)
            if c.status is not None:
                return n_records, False, GoError(f"memstore flush '{table_path}': op {c.unsorted_table} of the log was rejected")
            ends = [int(x) & _NONE for x in c.out_src[[0, c.n_out - 1]].cpu().tolist()]
            off = t["key_off"][[ends[0], ends[0] + 1, ends[1], ends[1] + 1]].cpu().tolist()
            lo, hi = (bytes(t["keys"][off[k]:off[k + 1]].cpu().numpy()) for k in (0, 2))
            write_table_files(table_path, c, lo, hi)
            wrote = True
        torch.cuda.synchronize(device)
    err = _reset_dir(base_path)
    return n_records, wrote, err


ErrEmptyKeyValue = GoError("neither empty keys nor values are allowed")  # db.go:37


class WriteBatch:
    """A batch of db.PutBytes / db.DeleteBytes calls (db.go:244-347) kept as the op log MemStore keeps:
    key arena, value arena, offsets and flags in application order. append_batch encodes it into WAL files
    on the device and hands back the device arrays for memstore.flush_ops_on_device."""

    def __init__(self):
        self._keys, self._values = bytearray(), bytearray()
        self._key_off, self._val_off = [0], [0]
        self._flags = bytearray()
        self._max_key_len = 0

    def __len__(self):
        return len(self._flags)

    def _log(self, key: bytes, value):
        self._keys += key
        self._key_off.append(len(self._keys))
        if value is not None:
            self._values += value
        self._val_off.append(len(self._values))
        self._flags.append(L.RIO_FLAG_NIL if value is None else 0)
        self._max_key_len = max(self._max_key_len, len(key))

    def PutBytes(self, key, value):  # noqa: N802
        """db.PutBytes (db.go:256): never refused; a nil key or value marshals as the empty one."""
        self._log(bytes(key or b""), bytes(value or b""))
        return None

    def DeleteBytes(self, key):  # noqa: N802
        """db.DeleteBytes (db.go:311): never refused."""
        self._log(bytes(key or b""), None)
        return None

    def Put(self, key: str, value: str):  # noqa: N802
        """db.Put (db.go:244)."""
        if len(key) == 0 or len(value) == 0:
            return ErrEmptyKeyValue
        return self.PutBytes(key.encode(), value.encode())

    def Delete(self, key: str):  # noqa: N802
        """db.Delete (db.go:306)."""
        return self.DeleteBytes(key.encode())

    def upload(self, device: int = 0):
        """-> memstore.DeviceOps: the batch in device memory. Call under torch.cuda.device(device)."""
        from memstore import upload_ops

        return upload_ops(device, self._keys, self._key_off, self._values, self._val_off, self._flags, self._max_key_len)


def wal_records_on_device(ctx, device: int, ops_view, mark=None):
    """rio_wal_ops_encode on torch's current stream: the WalMutation record of every op of `ops_view` (an
    OpsView). Returns (records, rec_off, result): the record arena (with RIO_DEVICE_PAD bytes past the
    bound), its n + 1 offsets and the result words as a list; reading those 64 bytes is the one host round
    trip. `mark(name)` as for sstables.merger.compact_on_device."""
    import torch

    from sstables.merger import check_status, on_device_stream

    mark = mark or (lambda name: None)
    lib, dev = L.lib(), f"cuda:{device}"
    n = int(ops_view.n)
    cap = int(lib.rio_wal_ops_encode_bound(n, ops_view.key_bytes, ops_view.value_bytes))

    def run(st):
        records = torch.empty(cap + L.RIO_DEVICE_PAD, dtype=torch.uint8, device=dev)
        rec_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        res = torch.empty(L.RIO_WALENC_RESULT_WORDS, dtype=torch.int64, device=dev)
        check_status(lib.rio_wal_ops_encode(ctx, ctypes.addressof(ops_view), records.data_ptr(), cap, rec_off.data_ptr(),
                                            res.data_ptr(), st), "rio_wal_ops_encode")
        mark("wal_encode")
        r = [x & _NONE for x in res.cpu().tolist()]
        mark("wal_encode_result_read")
        return records, rec_off, r

    return on_device_stream(device, run)


def wal_image_on_device(batch, comp: int, device: int = 0, mark=None):
    """The part of append_batch before the write: upload, rio_wal_ops_encode, rio_device_encode with compression
    `comp` (none or snappy), the image and its offsets to the host. `batch` is a WriteBatch, a memstore.DeviceOps
    or an OpsView whose arrays the caller keeps alive. Returns (ops, framed, err): ops is the memstore.DeviceOps;
    framed is None for an empty batch, else (image, out_rec_off, raw_len) as wal.Appender.AppendFramed takes them
    (a v4 file image of every op's WalMutation record, each record's offset in it, each record's length before
    framing)."""
    import torch

    from sstables.merger import check_status, on_device_stream

    mark = mark or (lambda name: None)
    lib, dev = L.lib(), f"cuda:{device}"
    with torch.cuda.device(device):
        ctx = L.default_ctx(device)
        if isinstance(batch, WriteBatch):
            ops = batch.upload(device)
        elif isinstance(batch, L.OpsView):  # the caller keeps the arrays alive
            ops = types.SimpleNamespace(view=batch)
        else:
            ops = batch
        mark("upload")
        n = int(ops.view.n)
        if n == 0:
            return ops, None, None
        records, rec_off, r = wal_records_on_device(ctx, device, ops.view, mark)
        if r[L.RIO_WALENC_R_FIRST_BAD] != _NONE:
            return ops, None, GoError(f"append batch: op {r[L.RIO_WALENC_R_FIRST_BAD]} of the log was rejected")
        total = r[L.RIO_WALENC_R_BYTES]
        cap = int(lib.rio_encode_bound(n, total, comp))

        def run(st):
            img = torch.empty(cap, dtype=torch.uint8, device=dev)
            out_off, out_len = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
            check_status(lib.rio_device_encode(ctx, records.data_ptr(), rec_off.data_ptr(), None, n, total, comp,
                                               img.data_ptr(), cap, out_off.data_ptr(), out_len.data_ptr(), st),
                         "rio_device_encode(wal)")
            mark("recordio_encode")
            flen = int(out_len.item())
            image, offs, raw = img[:flen].cpu().numpy(), out_off.cpu().numpy(), rec_off.cpu().numpy()
            mark("d2h")
            return image, offs, raw

        image, offs, raw = on_device_stream(device, run)
    return ops, (image, offs, raw[1:] - raw[:-1]), None


def append_batch(appender, batch, device: int = 0, mark=None):
    """The WAL half of a loop of db.PutBytes / db.DeleteBytes over `batch` (a WriteBatch, or a
    memstore.DeviceOps that is on the device already): upload, rio_wal_ops_encode, rio_device_encode with
    the appender's writer's compression, the image and its offsets to the host (wal_image_on_device),
    wal.Appender.AppendFramed. The directory is what the host loop of proto.marshal_upsert / marshal_delete +
    Append leaves. Returns (ops, err): ops is the memstore.DeviceOps, whose view memstore.flush_ops_on_device
    takes as it is."""
    from recordio.writer import FileWriter
    from sstables import UnsupportedError

    w = appender.currentWriter
    if not isinstance(w, FileWriter) or w.compression not in (L.COMP_NONE, L.COMP_SNAPPY):
        return None, UnsupportedError("append_batch writes through a recordio.FileWriter with compression none or snappy")
    ops, framed, err = wal_image_on_device(batch, w.compression, device, mark)
    if err is not None or framed is None:
        return ops, err
    return ops, appender.AppendFramed(*framed)


def _reset_dir(base_path: str):
    """os.RemoveAll + os.MkdirAll(0700) of the WAL directory (recovery.go:260-268)."""
    try:
        shutil.rmtree(base_path)
    except FileNotFoundError:
        pass
    except OSError as e:
        return GoError(str(e))
    try:
        os.makedirs(base_path, mode=0o700, exist_ok=True)
    except OSError as e:
        return GoError(str(e))
    return None


ErrNotFound = GoError("ErrNotFound")  # db.go:35


class RWMemstore:
    """simpledb/rw_memstore.go: two memstores, one for reading (the one being flushed), one for writing; the one
    that writes takes precedence for the same key. The stores are memstore.MemStores, or anything with their
    calls (a memstore.DeviceMemIndex for the read paths)."""

    def __init__(self, readStore, writeStore):  # noqa: N803
        self.readStore, self.writeStore = readStore, writeStore

    def Contains(self, key) -> bool:  # noqa: N802
        return self.writeStore.Contains(key) or self.readStore.Contains(key)

    def Get(self, key):  # noqa: N802
        """rw_memstore.go:22-36: only the write store's KeyNotFound asks the read store; its tombstone answers."""
        from memstore import KeyNotFound

        v, err = self.writeStore.Get(key)
        if err is not None:
            if err is KeyNotFound:
                return self.readStore.Get(key)
            return None, err
        return v, None

    def Add(self, key, value):  # noqa: N802
        return self.writeStore.Add(key, value)

    def Upsert(self, key, value):  # noqa: N802
        return self.writeStore.Upsert(key, value)

    def Delete(self, key):  # noqa: N802
        from memstore import KeyNotFound

        err = self.writeStore.Delete(key)
        if err is KeyNotFound:
            return self.Tombstone(key)
        return err

    def DeleteIfExists(self, key):  # noqa: N802
        return self.Delete(key)

    def Tombstone(self, key):  # noqa: N802
        return self.writeStore.Tombstone(key)

    def EstimatedSizeInBytes(self) -> int:  # noqa: N802
        return self.writeStore.EstimatedSizeInBytes()

    def SStableIterator(self):  # noqa: N802
        return self.writeStore.SStableIterator()

    def Flush(self, *opts):  # noqa: N802
        return self.writeStore.Flush(*opts)

    def Size(self) -> int:  # noqa: N802
        return self.writeStore.Size()


class _NoReadStore:
    """The read store of a view that has none: holds no key."""

    def Get(self, key):  # noqa: N802
        from memstore import KeyNotFound

        return None, KeyNotFound

    def Contains(self, key) -> bool:  # noqa: N802
        return False


class DBReadView:
    """DB.GetBytes / Get (db.go:184-242) over `tables` (a sstables.SuperSSTableReader, or None for a database
    without tables yet), the write memstore and the read memstore (the one being flushed, or None). A store is a
    memstore.MemStore, a memstore.DeviceMemStore or a memstore.DeviceMemIndex. GetBytes / Get run the reference's host sequence; GetBatch /
    GetBatchOnDevice answer a batch on the device. The open / closed checks of db.go:201-207 belong to the DB
    object, which this is not; bytes comparator only."""

    def __init__(self, tables, write_store, read_store=None, max_batch: int = 1 << 20):
        self.tables, self.write_store, self.read_store = tables, write_store, read_store
        self.max_batch = int(max_batch) if tables is None else min(int(max_batch), tables.max_batch)
        self.memstore = RWMemstore(_NoReadStore() if read_store is None else read_store, write_store)
        self._reader, self._reader_stack = None, None

    # ---- the reference's host sequence --------------------------------------------------------------------------

    def GetBytes(self, key):  # noqa: N802
        """db.go:197-242: the tables first (their error is returned before the memstore is asked), then the
        memstore, which wins with a value and hides the key with a tombstone."""
        from memstore import KeyNotFound, KeyTombstoned
        from sstables import NotFound

        key = bytes(key or b"")
        tab_val, tab_missing = None, True
        if self.tables is not None:
            tab_val, err = self.tables.Get(key)
            if err is not None:
                if err is not NotFound:
                    return None, err
            elif tab_val is not None and len(tab_val) != 0:
                tab_missing = False
        mem_val, err = self.memstore.Get(key)
        if err is not None:
            if err is KeyNotFound:
                return (None, ErrNotFound) if tab_missing else (tab_val, None)
            if err is KeyTombstoned:
                return None, ErrNotFound
            return None, err
        return mem_val, None

    def Get(self, key: str):  # noqa: N802
        """db.Get (db.go:184-195)."""
        v, err = self.GetBytes(key.encode())
        if err is not None:
            return "", err
        return v.decode(errors="surrogateescape"), None

    # ---- the batch on the device --------------------------------------------------------------------------------

    @property
    def _device(self) -> int:
        return self.tables._device if self.tables is not None and self.tables.readers else self.write_store.device

    def _indexes(self):
        """The stores' device indexes, oldest first (the write store last)."""
        stores = [s for s in (self.read_store, self.write_store) if s is not None]
        return [s._index() if hasattr(s, "_index") else s for s in stores]  # a MemStore or a DeviceMemStore

    def _host_only(self):
        """The stack's own rule: None, or why its batches are answered on the host."""
        from sstables import UnsupportedError

        if self.tables is None:
            return None
        err = self.tables._unsupported()
        if err is None and any(r.t.v0 for r in self.tables.readers):
            err = UnsupportedError("a stack with a v0 table answers GetBatch on the host: no device values")
        return err

    def _free_reader(self):
        if self._reader is not None:
            h, self._reader = self._reader, None
            L.lib().rio_db_reader_free(h)

    def Close(self):  # noqa: N802
        """Frees the reader handle; the tables and the stores are the caller's."""
        self._free_reader()
        return None

    def __del__(self):
        try:
            self._free_reader()
        except Exception:  # interpreter shutdown: the library may be gone
            pass

    def _ensure_reader(self, st):
        """The tables' stack, then the reader over it (again when the stack was freed and made anew)."""
        from sstables.merger import check_status

        stack = None
        if self.tables is not None:
            self.tables._ensure_stack(st)
            stack = self.tables._stack
        key = None if stack is None else stack.value
        if self._reader is None or self._reader_stack != key:
            self._free_reader()
            h = ctypes.c_void_p()
            check_status(L.lib().rio_db_reader_create(L.default_ctx(self._device), stack, self.max_batch, ctypes.byref(h)),
                         "rio_db_reader_create")
            self._reader, self._reader_stack = h, key
        return stack

    def GetBatchOnDevice(self, d_keys, d_key_off, n: int):  # noqa: N802
        """(mem_src, tab_src, status, val_off, values) as device tensors for n <= max_batch query keys already on
        the device (uint8 arena d_keys, int64 offsets d_key_off[n + 1]); the only host read is the 8 bytes that
        size `values`. mem_src[i] = store << 40 | op or -1 (store 1 = the write store when there are two),
        tab_src[i] = table << 40 | entry or -1 (None without tables), status[i] one of RIO_GET_* (RIO_GET_MEM_VALUE:
        the memstore's value), value i = values[val_off[i]:val_off[i + 1]]."""
        import torch

        from memstore import index_array, read_piece
        from sstables.merger import on_device_stream

        err = self._host_only()
        idx = self._indexes()
        for i in idx:
            err = err or i.err
        if err is not None:
            raise err
        device = self._device
        with torch.cuda.device(device):
            def run(st):
                stack = self._ensure_reader(st)
                return read_piece(L.default_ctx(device), device, st, self._reader, stack, index_array(idx),
                                  d_keys.data_ptr(), d_key_off.data_ptr(), n, d_keys.numel())

            return on_device_stream(device, run)

    def GetBatch(self, keys):  # noqa: N802
        """[(value, err)] per key, equal to a loop of GetBytes, in pieces of max_batch. A RIO_GET_HOST entry gets
        its error from the owning reader, as SuperSSTableReader.GetBatch does."""
        import torch

        from memstore import index_array, read_piece, upload_queries
        from sstables.merger import on_device_stream

        keys = [bytes(k or b"") for k in keys]
        if self._host_only() is not None:
            return [self.GetBytes(k) for k in keys]
        idx = self._indexes()
        for i in idx:
            err = i.rejected()
            if err is not None:
                return [(None, err) for _ in keys]
        n = len(keys)
        if n == 0:
            return []
        device = self._device
        with torch.cuda.device(device):
            def run(st):
                stack = self._ensure_reader(st)
                d_keys, d_off, nbytes = upload_queries(device, keys)
                arr, ctx = index_array(idx), L.default_ctx(device)
                return [read_piece(ctx, device, st, self._reader, stack, arr, d_keys.data_ptr(), d_off.data_ptr() + 8 * a,
                                   min(a + self.max_batch, n) - a, nbytes) for a in range(0, n, self.max_batch)]

            out = []
            for _, tab, status, val_off, values in on_device_stream(device, run):
                h_status, h_off, h_val = status.cpu().tolist(), val_off.cpu().tolist(), bytes(values.cpu().numpy())
                h_tab = None
                for i, s in enumerate(h_status):
                    if s in (L.RIO_GET_VALUE, L.RIO_GET_MEM_VALUE):
                        out.append((h_val[h_off[i]:h_off[i + 1]], None))
                    elif s == L.RIO_GET_HOST:
                        h_tab = tab.cpu().tolist() if h_tab is None else h_tab
                        w = h_tab[i] & _NONE
                        r = self.tables.readers[w >> L.RIO_MERGE_ENTRY_BITS]
                        _, e = r._value_at(w & ((1 << L.RIO_MERGE_ENTRY_BITS) - 1), r.opts.skipHashCheckOnRead)
                        # a read the host can make after all: the key's answer by the host sequence
                        out.append((None, e) if e is not None else self.GetBytes(keys[len(out)]))
                    else:
                        out.append((None, ErrNotFound))
            return out


# ---- the DB object (db.go, flush.go, recovery.go:117-277) ---------------------------------------------------------

SSTablePrefix = "sstable"  # db.go:20-25
SSTablePattern = SSTablePrefix + "_%015d"
SSTableCompactionPathPrefix = SSTablePrefix + "_compaction"
CompactionFinishedSuccessfulFileName = "compaction_successful"
WriteAheadFolder = "wal"
MemStoreMaxSizeBytes = 1024 * 1024 * 1024
NumSSTablesToTriggerCompaction = 10
DefaultCompactionMaxSizeBytes = 5 * 1024 * 1024 * 1024
DefaultCompactionRatio = struct.unpack("f", struct.pack("f", 0.2))[0]  # float32(0.2)

ErrNotOpenedYet = GoError("database has not been opened yet, please call Open() first")  # db.go:34-36
ErrAlreadyOpen = GoError("database is already open")
ErrAlreadyClosed = GoError("database is already closed")


class ExtraOptions:
    """db.go:414-425, the fields this DB reads; `device` is not in the reference."""

    def __init__(self):
        self.memstoreSizeBytes = MemStoreMaxSizeBytes
        self.enableCompactions = True
        self.compactionFileThreshold = NumSSTablesToTriggerCompaction
        self.compactionMaxSizeBytes = DefaultCompactionMaxSizeBytes
        self.compactionRatio = DefaultCompactionRatio
        self.compactionRunInterval = 5.0  # accepted and unused: a pass runs where a table is added, not on a ticker
        self.compactOnDevice = False
        self.device = 0


def MemstoreSizeBytes(n: int):  # noqa: N802
    """db.go:431: the size of the memstore after which it is written to disk."""
    def f(o): o.memstoreSizeBytes = n
    return f


def DisableCompactions():  # noqa: N802
    """db.go:438. Compactions run only under CompactOnDevice(), and not when this was passed too."""
    def f(o): o.enableCompactions = False
    return f


def CompactOnDevice():  # noqa: N802
    """Not in the reference: the opt-in to compactions. Without it a database with a compaction directory stays with
    the reference (Open returns UnsupportedError) and no compaction runs."""
    def f(o): o.compactOnDevice = True
    return f


def CompactionRunInterval(seconds: float):  # noqa: N802
    """db.go:458: accepted and ignored, there is no ticker here."""
    def f(o): o.compactionRunInterval = seconds
    return f


def CompactionRatio(ratio: float):  # noqa: N802
    """db.go:472: the share of tombstones from which a table is a candidate whatever its size; float32."""
    if not 0.0 <= ratio <= 1.0:  # a NaN too; Go panics
        raise ValueError("invalid compaction ratio: %f, must be between 0 and 1" % ratio)
    def f(o): o.compactionRatio = struct.unpack("f", struct.pack("f", ratio))[0]
    return f


def CompactionFileThreshold(n: int):  # noqa: N802
    """db.go:483: a pass compacts only more candidates than this."""
    def f(o): o.compactionFileThreshold = n
    return f


def CompactionMaxSizeBytes(n: int):  # noqa: N802
    """db.go:492: a table of fewer totalBytes than this is a candidate."""
    def f(o): o.compactionMaxSizeBytes = n
    return f


# ---- compaction, the parts that need no GPU (sstable_manager.go:115-185, compaction.go:148-172, recovery.go:22-114) ----

def _u64_to_f32(n: int) -> float:
    """Go's float32(uint64): round to nearest, ties to even, on the integer (a double in between rounds twice)."""
    if n < 1 << 24:
        return float(n)
    shift = n.bit_length() - 24
    q, r, half = n >> shift, n & ((1 << shift) - 1), 1 << (shift - 1)
    if r > half or (r == half and q & 1):
        q += 1
    return float(q << shift)


def flood_fill(a):
    """floodFill (sstable_manager.go:158-185): the values enclosed by true values become true as well."""
    a = list(a)
    sel = [i for i, x in enumerate(a) if x]
    if sel:
        a[sel[0]:sel[-1] + 1] = [True] * (sel[-1] + 1 - sel[0])
    return a


def candidate_tables_for_compaction(tables, compaction_max_size_bytes: int, compaction_ratio: float):
    """candidateTablesForCompaction (sstable_manager.go:115-156) over `tables` = [(base path, MetaData)], oldest first
    -> (the selected paths, the sum of their numRecords). A table is selected below the size limit, or (when it holds a
    record) from the tombstone ratio on, float32(nullValues) / float32(numRecords) >= ratio as Go computes it; the
    gaps between selected tables are filled so that the lineage is kept."""
    ratio = struct.unpack("f", struct.pack("f", compaction_ratio))[0]
    selected = []
    for _, m in tables:
        s = m.totalBytes < compaction_max_size_bytes
        if m.numRecords > 0:
            # the double quotient of two float32 values, rounded to float32, is the float32 quotient
            q = struct.unpack("f", struct.pack("f", _u64_to_f32(m.nullValues) / _u64_to_f32(m.numRecords)))[0]
            s = s or q >= ratio
        selected.append(s)
    selected = flood_fill(selected)
    paths = [p for (p, _), s in zip(tables, selected) if s]
    return paths, sum(m.numRecords for (_, m), s in zip(tables, selected) if s)


def save_compaction_metadata(write_folder: str, m):
    """saveCompactionMetadata (compaction.go:148-172): the one marshalled record in a recordio file with the writer's
    defaults (the current version, uncompressed) -> err."""
    from recordio.writer import NewFileWriter

    try:
        record = proto.marshal_compaction_metadata(m)
    except ValueError as e:
        return GoError(_PROTO_PREFIX + str(e))
    w, err = NewFileWriter(os.path.join(write_folder, CompactionFinishedSuccessfulFileName), L.COMP_NONE)
    if err is None:
        err = w.Open()
    if err is not None:
        return err
    _, err = w.Write(record)
    cerr = w.Close()
    return err or cerr


def _crc32c(b: bytes) -> int:
    c = 0xFFFFFFFF
    for x in b:
        c ^= x
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 & -(c & 1))
    return c ^ 0xFFFFFFFF


def _first_record_on_host(img: bytes):
    """The first record of a recordio file image in the writer's default form (version 4, uncompressed), read on the
    host: readRecordHeaderV4 (common_reader.go:110-151) and the payload. None for a nil record; raises ValueError for
    anything the reader would refuse, a file without a record included."""
    from sstables.proto import _varint

    pos = 8
    if pos >= len(img):
        raise ValueError("EOF")
    magic, pos = _varint(img, pos)
    if magic != 0x130691:
        raise ValueError("magic number mismatch")
    if pos >= len(img):
        raise ValueError("unexpected EOF")
    nil, pos = img[pos], pos + 1
    size, pos = _varint(img, pos)
    _, pos = _varint(img, pos)
    actual = _crc32c(img[8:pos])
    expected, pos = _varint(img, pos)
    if actual != expected:
        raise ValueError("header checksum mismatch")
    if size > len(img) - pos:
        raise ValueError("unexpected EOF")
    return None if nil == 1 else img[pos:pos + size]


def read_compaction_metadata(path: str):
    """The CompactionMetadata of a compaction_successful file -> (metadata, err). The file as saveCompactionMetadata
    writes it is read on the host, so that repair_compactions needs no GPU: recordio.reader decodes on the device.
    A file of another version or with a compression goes through recordio.reader."""
    try:
        with open(path, "rb") as fh:
            img = fh.read()
    except OSError as e:
        return None, GoError(str(e))
    try:
        if len(img) >= 8 and img[:8] == struct.pack("<II", 4, L.COMP_NONE):
            record = _first_record_on_host(img)
        else:
            from recordio.reader import NewFileReaderWithPath

            r, err = NewFileReaderWithPath(path)
            if err is None:
                err = r.Open()
            if err is not None:
                return None, err
            record, err = r.ReadNext()
            r.Close()
            if err is not None:
                return None, err
        return proto.unmarshal_compaction_metadata(record), None
    except ValueError as e:  # the wire format's and the UTF-8 error too
        return None, GoError(str(e))


def repair_compactions(base_path: str):
    """repairCompactions (recovery.go:22-114) -> err. Every directory under base_path whose name starts with
    SSTableCompactionPathPrefix: without a readable metadata record it is deleted (the compaction can be attempted
    again); with one the compaction is finished: the replacement path removed, the write folder renamed to it, the
    other inputs removed. Needs no GPU."""
    to_finish, to_delete = [], []

    def onerror(e):
        raise e

    try:
        for root, _, _ in os.walk(base_path, onerror=onerror):
            if os.path.basename(root).startswith(SSTableCompactionPathPrefix):
                m, err = read_compaction_metadata(os.path.join(root, CompactionFinishedSuccessfulFileName))
                if err is not None:
                    to_delete.append(root)
                else:
                    to_finish.append(m)
        for p in to_delete:
            _remove_all(p)
        for m in to_finish:
            write_path, replacement = os.path.join(base_path, m.writePath), os.path.join(base_path, m.replacementPath)
            _remove_all(replacement)
            os.rename(write_path, replacement)
            for p in m.sstablePaths:
                if p != m.replacementPath:
                    _remove_all(os.path.join(base_path, p))
    except OSError as e:
        return GoError(str(e))
    return None


def _remove_all(path: str):
    """os.RemoveAll: a path that does not exist is no error."""
    try:
        shutil.rmtree(path)
    except FileNotFoundError:
        pass
    except NotADirectoryError:
        os.remove(path)


def OnDevice(device: int):  # noqa: N802
    """Not in the reference: the GPU that holds the memstore and the tables."""
    def f(o): o.device = device
    return f


class DB:
    """simpledb.DB (db.go:81-347) with the write path batched: Apply(WriteBatch) leaves the directory and the reads
    that a loop of PutBytes / DeleteBytes over the batch leaves, rotations included. The memstore is a
    memstore.DeviceMemStore, the WAL records are marshalled and framed on the device (wal_image_on_device), and the
    op at which the loop would rotate comes from rio_mem_size_scan (DeviceMemStore.PlanUntilFull), once per
    segment. The flush runs inline in the writing call (flush.go's goroutine is not mirrored: there is never a read
    store, and a failed flush is returned); one writer at a time, there is no lock. Under CompactOnDevice() one
    compaction pass (executeCompaction + reflectCompactionResult, one tick of the reference's ticker) runs inline at
    the end of Open and after every rotation that added a table, and on demand (Compact); its error is returned by the
    call that triggered it."""

    def __init__(self, basePath: str, opts: ExtraOptions):  # noqa: N803
        self.basePath = basePath
        self.memstoreMaxSize = int(opts.memstoreSizeBytes)
        self.enableCompactions = opts.enableCompactions
        self.compactOnDevice = opts.compactOnDevice
        self.compactionFileThreshold = int(opts.compactionFileThreshold)
        self.compactedMaxSizeBytes = int(opts.compactionMaxSizeBytes)
        self.compactionRatio = opts.compactionRatio
        self.installCompactedFromDevice = True  # False: reflect reloads the compacted table from its files
        self._compacted = None  # (write path, the merge's Compaction) between execute and reflect
        self.device = opts.device
        self.currentGeneration = 0
        self.open = self.closed = False
        self.wal = None       # the wal.Appender
        self.readers = []     # sstableManager.allSSTableReaders, oldest first
        self.tables = None    # the SuperSSTableReader over them, None without a table
        self.memStore = None  # the write store
        self.view = None      # DBReadView over tables and memStore

    # ---- Open / Close ---------------------------------------------------------------------------------------------

    def _table_dirs(self):
        """reconstructSSTables' walk (recovery.go:120-130): every directory under basePath, itself included, whose
        name starts with SSTablePrefix; sorted."""
        def onerror(e):
            raise e

        out = []
        for root, _, _ in os.walk(self.basePath, onerror=onerror):
            if os.path.basename(root).startswith(SSTablePrefix):
                out.append(root)
        return sorted(out)

    def _restack(self):
        """A new stack over the readers and a new read view over it and the write store."""
        from sstables import NewSuperSSTableReader

        if self.view is not None:
            self.view.Close()
        if self.tables is not None:
            self.tables._free_stack()
        self.tables = NewSuperSSTableReader(self.readers) if self.readers else None
        self.view = DBReadView(self.tables, self.memStore)

    def _add_table(self, path: str):
        from sstables import NewSSTableReader, ReadBasePath, ReadOnDevice

        reader, err = NewSSTableReader(ReadBasePath(path), ReadOnDevice(self.device))
        if err is None:
            self.readers.append(reader)
        return err

    def Open(self):  # noqa: N802
        from memstore import DeviceMemStore
        from recordio.writer import NewFileWriter
        from sstables import UnsupportedError
        from wal import BasePath, MaximumWalFileSizeBytes, NewAppender, NewWriteAheadLogOptions, WriterFactory

        if self.open:
            return ErrAlreadyOpen
        if self._compaction_active():  # db.go:122: before the tables are reconstructed
            err = repair_compactions(self.basePath)
            if err is not None:
                return err
        try:
            paths = self._table_dirs()
        except OSError as e:
            return GoError(str(e))
        for p in paths:  # repairCompactions' and the compactor's directories: such a database stays with the reference
            if os.path.basename(p).startswith(SSTableCompactionPathPrefix):
                return UnsupportedError(f"'{p}': a database with a compaction directory is opened by the reference")
        # reconstructSSTables
        for p in paths:
            suffix = os.path.basename(p)[len(SSTablePrefix) + 1:]
            if not (suffix.isascii() and suffix.isdigit()) or int(suffix) >= 1 << 64:
                return GoError(f'strconv.ParseUint: parsing "{suffix}": invalid syntax')
            err = self._add_table(p)
            if err is not None:
                return err
            self.currentGeneration = max(self.currentGeneration, int(suffix))
        # replayAndSetupWriteAheadLog: the replay flushes into the next generation (executeFlush) when it held an op
        wal_base = os.path.join(self.basePath, WriteAheadFolder)
        try:
            os.makedirs(wal_base, mode=0o700, exist_ok=True)
        except OSError as e:
            return GoError(f"could not mkdir WAL dir at {wal_base}: {e}")
        table = os.path.join(self.basePath, SSTablePattern % (self.currentGeneration + 1))
        _, wrote, err = recover_wal(wal_base, table, device=self.device, bloom_filter=True)
        if err is not None:
            return err
        if wrote:
            self.currentGeneration += 1
            err = self._add_table(table)
            if err is not None:
                return err
        # we rotate in lockstep with the memstore flushes: the size limit is set far above them (recovery.go:193-195)
        o, err = NewWriteAheadLogOptions(BasePath(wal_base), MaximumWalFileSizeBytes(self.memstoreMaxSize * 100),
                                         WriterFactory(lambda path: NewFileWriter(path, L.COMP_SNAPPY)))
        if err is not None:
            return err
        self.wal, err = NewAppender(o)
        if err is not None:
            return err
        self.memStore = DeviceMemStore(self.device)
        self._restack()
        self.open = True
        _, err = self._compaction_pass()
        return err

    def _check(self):
        if not self.open:
            return ErrNotOpenedYet
        if self.closed:
            return ErrAlreadyClosed
        return None

    def Close(self):  # noqa: N802
        """db.go:150-187: the last rotation and flush, then the WAL (its fresh, header-only file stays) and the
        readers."""
        err = self._check()
        if err is not None:
            return err
        self.closed = True
        err = self._rotate_wal_and_flush_memstore(compact=False)
        if err is not None:
            return err
        errs = [self.wal.Close(), self.view.Close(), None if self.tables is None else self.tables.Close()]
        errs = [e for e in errs if e is not None]
        return GoError("\n".join(str(e) for e in errs)) if errs else None

    # ---- writes -----------------------------------------------------------------------------------------------------

    def _rotate_wal_and_flush_memstore(self, compact: bool = True):
        """rotateWalAndFlushMemstore and executeFlush (flush.go:32-108), inline. compact: a compaction pass follows a
        rotation that added a table (Close passes False: the reference stops its ticker before the last flush)."""
        from memstore import DeviceMemStore
        from sstables import BloomExpectedNumberOfElements, EnableBloomFilter, WriteBasePath

        wal_path, err = self.wal.Rotate()
        if err is not None:
            return err
        store = self.memStore
        if store.log.n == 0:  # nothing to write: the WAL file stays (flush.go:37-40); the empty store serves on
            return None
        self.memStore = DeviceMemStore(self.device)
        gen = self.currentGeneration = self.currentGeneration + 1
        path = os.path.join(self.basePath, SSTablePattern % gen)
        try:
            os.makedirs(path, mode=0o700, exist_ok=True)
        except OSError as e:
            return GoError(str(e))
        err = store.FlushWithTombstones(WriteBasePath(path), EnableBloomFilter(), BloomExpectedNumberOfElements(store.Size()))
        if err is not None:
            return err
        try:
            os.remove(wal_path)
        except OSError as e:
            return GoError(str(e))
        err = self._add_table(path)
        if err is not None:
            return err
        self._restack()
        if compact:
            _, err = self._compaction_pass()
            return err
        return None

    # ---- compaction (compaction.go:57-146, sstable_manager.go:24-85) ----------------------------------------------

    def _compaction_active(self) -> bool:
        return self.compactOnDevice and self.enableCompactions

    def _index_of_reader(self, name: str) -> int:
        for i, r in enumerate(self.readers):
            if os.path.basename(r.BasePath()) == name:
                return i
        return -1

    def _execute_compaction(self):
        """executeCompaction (compaction.go:57-146) -> (CompactionMetadata or None when nothing was compacted, err).
        The inputs are the DB's own readers, resident in HBM; the table is written into a fresh write folder with its
        compaction_successful record. On an error the write folder is removed."""
        from sstables import (BloomExpectedNumberOfElements, EnableBloomFilter, NewSSTableMerger,
                              ScanReduceLatestWinsSkipTombstones, _WriterOpts)

        paths, num_records = candidate_tables_for_compaction([(r.BasePath(), r.MetaData()) for r in self.readers],
                                                             self.compactedMaxSizeBytes, self.compactionRatio)
        if len(paths) <= self.compactionFileThreshold:
            return None, None
        paths.sort()  # make sure we're always compacting with the right order in mind (compaction.go:65)
        try:
            write_folder = tempfile.mkdtemp(prefix=SSTableCompactionPathPrefix, dir=self.basePath)
        except OSError as e:
            return None, GoError(str(e))
        by_path = {r.BasePath(): r for r in self.readers}
        merger = NewSSTableMerger(data_compression=_WriterOpts().dataCompressionType)  # the flush's
        try:
            err = merger.MergeCompact([by_path[p] for p in paths], write_folder, ScanReduceLatestWinsSkipTombstones,
                                      writer_options=(EnableBloomFilter(), BloomExpectedNumberOfElements(num_records)))
        except OSError as e:
            err = GoError(str(e))
        except GoError as e:
            err = e
        names = [os.path.basename(p) for p in paths]  # relative to the base path, to be portable (compaction.go:125)
        m = proto.CompactionMetadata(writePath=os.path.basename(write_folder), replacementPath=names[0], sstablePaths=names)
        if err is None:
            err = save_compaction_metadata(write_folder, m)
        if err is not None:
            shutil.rmtree(write_folder, ignore_errors=True)
            return None, err
        self._compacted = (m.writePath, merger.compaction)
        return m, None

    def _reflect_compaction_result(self, m):
        """reflectCompactionResult (sstable_manager.go:24-85) -> err: the inputs' directories go, the write folder takes
        the replacement's name, the new reader takes the replacement's place in the readers and the other inputs leave
        them. The new reader is made from the buffers the merge left in HBM when they are at hand (a metadata that
        _execute_compaction has just returned) and reads no file; else the table is loaded from its files."""
        import torch

        from sstables import NewSSTableReader, ReadBasePath, ReadOnDevice, SSTableReader, _DeviceTable, _Opts

        replacement = os.path.join(self.basePath, m.replacementPath)
        held, self._compacted = self._compacted, None
        reader = None
        if self.installCompactedFromDevice and held is not None and held[0] == m.writePath:
            c = held[1]
            try:
                with torch.cuda.device(self.device):
                    t = _DeviceTable.from_compaction(replacement, self.device, c, c.data_file, c.index_file)
            except GoError as e:
                return e
            reader = SSTableReader(_Opts(basePath=replacement, device=self.device), c.meta, t, c.filter)
        del held
        i = self._index_of_reader(m.replacementPath)
        if i < 0:
            return GoError(f"couldn't find replacement sstable in current readers. Path: {m.replacementPath}")
        others = [p for p in m.sstablePaths if p != m.replacementPath]
        gone = [self._index_of_reader(p) for p in others]
        for p, k in zip(others, gone):
            if k < 0:
                return GoError(f"couldn't find sstable in current readers. Path: {p}")
        try:
            for p in m.sstablePaths:
                if self._index_of_reader(p) >= 0:
                    _remove_all(os.path.join(self.basePath, p))
            os.rename(os.path.join(self.basePath, m.writePath), replacement)
        except OSError as e:
            return GoError(str(e))
        if reader is None:
            reader, err = NewSSTableReader(ReadBasePath(replacement), ReadOnDevice(self.device))
            if err is not None:
                return err
        old = [self.readers[k] for k in [i] + gone]
        readers = list(self.readers)
        readers[i] = reader
        self.readers = [r for k, r in enumerate(readers) if k not in gone]
        self._restack()  # the old stack's views go before the tables they point into
        for r in old:
            r.Close()
        return None

    def _compaction_pass(self):
        """One tick of backgroundCompaction (compaction.go:32-46) -> (metadata or None, err); nothing when compaction
        is not active."""
        if not self._compaction_active():
            return None, None
        m, err = self._execute_compaction()
        if err is not None or m is None:
            return None, err
        err = self._reflect_compaction_result(m)
        if err is not None:
            shutil.rmtree(os.path.join(self.basePath, m.writePath), ignore_errors=True)
            return None, err
        return m, None

    def Compact(self):  # noqa: N802
        """Not in the reference: one compaction pass on demand -> (the CompactionMetadata of what was compacted or None,
        err). UnsupportedError without CompactOnDevice(); nothing runs under DisableCompactions()."""
        from sstables import UnsupportedError

        err = self._check()
        if err is not None:
            return None, err
        if not self.compactOnDevice:
            return None, UnsupportedError("compactions run under CompactOnDevice() only")
        return self._compaction_pass()

    def Apply(self, batch: "WriteBatch"):  # noqa: N802
        """What a loop of PutBytes / DeleteBytes over the batch leaves: per op the WAL record, the memstore op and,
        after a put, the size check and the rotation (db.go:256-347). Per segment (the ops up to and including the
        put that rotates): the segment's framed records to the WAL, its ops to the memstore, the rotation."""
        from sstables import UnsupportedError

        err = self._check()
        if err is not None:
            return err
        n = len(batch)
        if n == 0:
            return None
        if batch._max_key_len > L.RIO_FLUSH_MAX_KEY_LEN:  # before anything is written
            return UnsupportedError(f"a key of {batch._max_key_len} bytes: the device orders keys of up to "
                                    f"{L.RIO_FLUSH_MAX_KEY_LEN}")
        ops, framed, err = wal_image_on_device(batch, self.wal.currentWriter.compression, self.device)
        if err is not None:
            return err
        image, offs, raw = framed
        a = 0
        while ops is not None:
            plan, err = self.memStore.PlanUntilFull(ops, self.memstoreMaxSize)
            if err is not None:
                return err
            b = a + plan.n_applied
            err = self.wal.AppendFramed(image if b == n else image[:int(offs[b])], offs[a:b], raw[a:b])
            if err is not None:
                return err
            ops = self.memStore.ApplyPlanned(plan)
            if plan.cut:
                err = self._rotate_wal_and_flush_memstore()
                if err is not None:
                    return err
            a = b
        return None

    def PutBytes(self, key, value):  # noqa: N802
        b = WriteBatch()
        b.PutBytes(key, value)
        return self.Apply(b)

    def DeleteBytes(self, key):  # noqa: N802
        b = WriteBatch()
        b.DeleteBytes(key)
        return self.Apply(b)

    def Put(self, key: str, value: str):  # noqa: N802
        if len(key) == 0 or len(value) == 0:
            return ErrEmptyKeyValue
        return self.PutBytes(key.encode(), value.encode())

    def Delete(self, key: str):  # noqa: N802
        return self.DeleteBytes(key.encode())

    # ---- reads ------------------------------------------------------------------------------------------------------

    def GetBytes(self, key):  # noqa: N802
        err = self._check()
        if err is not None:
            return None, err
        return self.view.GetBytes(key)

    def Get(self, key: str):  # noqa: N802
        err = self._check()
        if err is not None:
            return "", err
        return self.view.Get(key)

    def GetBatch(self, keys):  # noqa: N802
        """[(value, err)] per key, equal to a loop of GetBytes."""
        err = self._check()
        if err is not None:
            return [(None, err) for _ in keys]
        return self.view.GetBatch(keys)

    def GetBatchOnDevice(self, d_keys, d_key_off, n: int):  # noqa: N802
        """DBReadView.GetBatchOnDevice over the current tables and write store; raises the open / closed error."""
        err = self._check()
        if err is not None:
            raise err
        return self.view.GetBatchOnDevice(d_keys, d_key_off, n)


def NewSimpleDB(basePath: str, *extraOptions):  # noqa: N802,N803
    """db.go:351-410: the directory must exist -> (DB, err)."""
    try:
        os.listdir(basePath)
    except OSError as e:
        return None, GoError(f"open {basePath}: {(e.strerror or str(e)).lower()}")
    o = ExtraOptions()
    for f in extraOptions:
        f(o)
    return DB(basePath, o), None
