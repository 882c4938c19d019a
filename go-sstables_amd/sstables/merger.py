"""SSTableMerger mirror (sstables/sstable_merger.go:36-169) over tables loaded on the device.

Merge / MergeCompact take SSTableReaders from NewSSTableReader (their decoded files, parsed index and
per-value CRC-64 are resident in HBM) and write one table: the k-way merge, the reduce, the value
gather and the IndexEntry records run in rio_compact.hip (rio_sst_merge_plan / rio_sst_merge_gather /
rio_sst_index_encode), both output files are encoded by rio_device_encode. The host reads the plan's
64-byte result block, the two file images and the first and last key. The reducers are the two the
reference ships (super_sstable_reader.go:107-131); any other callable returns UnsupportedError: the
adapter keeps the reference merger for it. There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os

from recordio import _lib as L
from recordio.errors import GoError

from . import bloom, proto

_NONE = 0xFFFFFFFFFFFFFFFF
_ENTRY_MASK = (1 << L.RIO_MERGE_ENTRY_BITS) - 1


class _Reducer:
    """One of the reference's ReduceFuncs (func(key, values, context) (key, value)); callable with the
    reference's semantics, and recognised by MergeCompact, which runs it on the device."""

    def __init__(self, name: str, mode: int):
        self.__name__ = name
        self.mode = mode

    def __call__(self, key, values, context):
        # super_sstable_reader.go:109-121: the value whose context is the largest (the first one on a tie)
        max_ctx, idx = 0, 0
        for i, x in enumerate(context):
            if x > max_ctx:
                max_ctx, idx = x, i
        val = values[idx]
        if self.mode == L.RIO_MERGE_LATEST_WINS_SKIP_TOMBSTONES and (val is None or len(val) == 0):
            return None, None  # :125-131
        return key, val

    def __repr__(self):
        return self.__name__


ScanReduceLatestWins = _Reducer("ScanReduceLatestWins", L.RIO_MERGE_LATEST_WINS)
ScanReduceLatestWinsSkipTombstones = _Reducer("ScanReduceLatestWinsSkipTombstones",
                                              L.RIO_MERGE_LATEST_WINS_SKIP_TOMBSTONES)


def table_view(t) -> L.SstView:
    """rio_sst_view of a loaded _DeviceTable (entry i pairs with data record i: the writer's layout)."""
    return L.SstView(
        index=t.ib.out.data_ptr(), key_off=t.key_off.data_ptr(), key_len=t.key_len.data_ptr(),
        data=t.db.out.data_ptr(), data_off=t.db.out_off.data_ptr(), flags=t.db.flags.data_ptr(),
        crc=t.crc.data_ptr(), n=t.n_index, index_bytes=t.index_info["total_out_bytes"],
        data_bytes=t.data_info["total_out_bytes"])


class Compaction:
    """Device buffers and host figures of one merge (compact_on_device)."""

    status = None  # None, "unsorted" or "duplicate"
    n_out = value_bytes = null_values = key_bytes = 0
    first_dup = unsorted_table = _NONE
    out_src = data_img = data_len = index_img = index_len = None
    bloom = None  # (host Filter, DeviceFilter) when the table gets a bloom.bf.gz
    # the table as it stands decoded in HBM once encode_planned is through: the gathered values (arena, n + 1 offsets,
    # per-value flags), the IndexEntry records (arena, n + 1 offsets) and each record's offset in its file image.
    # _DeviceTable.from_compaction loads the table from them
    values = val_off = val_flags = entries = ent_off = data_rec_off = index_rec_off = None
    ent_bytes = 0
    # what write_table_files wrote: the MetaData, the host bloom Filter (None without one), the two file images
    meta = filter = data_file = index_file = None


def on_device_stream(device: int, fn):
    """fn(stream handle) on torch's current stream of `device`; when that is the null stream, on a stream of
    our own ordered after and before it (the null stream's handle would select the context's own stream,
    which torch's copies do not follow)."""
    import torch

    cur = torch.cuda.current_stream(device)
    if cur.cuda_stream == 0:
        side = torch.cuda.Stream(device=device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            out = fn(ctypes.c_void_p(side.cuda_stream))
        cur.wait_stream(side)
        return out
    return fn(ctypes.c_void_p(cur.cuda_stream))


def check_status(rc, what):
    if rc:
        raise GoError(f"{what}: {L.strerror(rc)}")


def encode_planned(ctx, device: int, st, src, keep, res, comp: int, mark, refuse_dup: bool, flt=None) -> Compaction:
    """What follows a plan (rio_sst_merge_plan or rio_sst_flush_plan, whose view the context holds): result
    read, gather, [filter build,] data encode, index entries, index encode, on stream `st`. src / keep / res
    are the plan's outputs. Shared by compact_on_device and memstore.flush_ops_on_device.
    flt: None, an empty sstables.bloom.Filter (sstables.writer_filter), or a callable n_out -> Filter: its
    bits are built on the device from the survivors' keys (rio_sst_bloom_add: one Add per WriteNext,
    sstable_writer.go:114-118) and fetched with the file images by write_table_files. The gathered values, the
    IndexEntry records and the records' file offsets stay on the returned Compaction (the written table, decoded)."""
    import torch

    lib = L.lib()
    dev = f"cuda:{device}"
    i64 = lambda n: torch.empty(max(n, 1), dtype=torch.int64, device=dev)  # noqa: E731
    u8 = lambda n: torch.empty(max(n, 1), dtype=torch.uint8, device=dev)  # noqa: E731
    c = Compaction()
    # the one host round trip before the files are fetched: rio_device_encode takes n by value
    r = [x & _NONE for x in res.cpu().tolist()]
    mark("result_read")
    c.n_out, c.value_bytes, c.null_values = r[L.RIO_MERGE_R_N_OUT], r[L.RIO_MERGE_R_VALUE_BYTES], r[L.RIO_MERGE_R_NULL_VALUES]
    c.first_dup, c.unsorted_table, c.key_bytes = r[L.RIO_MERGE_R_FIRST_DUP], r[L.RIO_MERGE_R_UNSORTED], r[L.RIO_MERGE_R_KEY_BYTES]
    if c.unsorted_table != _NONE:
        c.status = "unsorted"
        return c
    if refuse_dup and c.first_dup != _NONE:
        c.status = "duplicate"
        return c
    n = c.n_out
    c.out_src, val_off, val_flags = i64(n), i64(n + 1), u8(n)
    values = u8(c.value_bytes + L.RIO_DEVICE_PAD)
    check_status(lib.rio_sst_merge_gather(ctx, src.data_ptr(), keep.data_ptr(), n, c.out_src.data_ptr(), values.data_ptr(),
                                    values.numel(), val_off.data_ptr(), val_flags.data_ptr(), st), "rio_sst_merge_gather")
    mark("gather")
    if flt is not None:
        if callable(flt):
            flt = flt(n)
        # zero-filled bits and the hash keys go up; nothing comes back before the files are fetched
        words = torch.zeros((flt.m + 63) // 64, dtype=torch.int64, device=dev)
        hk = torch.tensor([x - (1 << 64) if x >> 63 else x for x in flt.keys], dtype=torch.int64).to(dev, non_blocking=True)
        d = bloom.DeviceFilter(words, hk, flt.m, flt.k)
        check_status(lib.rio_sst_bloom_add(ctx, d.ref(), c.out_src.data_ptr(), n, st), "rio_sst_bloom_add")
        c.bloom = (flt, d)
        mark("bloom")
    cap = int(lib.rio_encode_bound(n, c.value_bytes, comp))
    c.data_img, data_rec_off, c.data_len = u8(cap), i64(n), i64(1)
    check_status(lib.rio_device_encode(ctx, values.data_ptr(), val_off.data_ptr(), val_flags.data_ptr(), n, c.value_bytes, comp,
                                 c.data_img.data_ptr(), cap, data_rec_off.data_ptr(), c.data_len.data_ptr(), st),
           "rio_device_encode(data)")
    mark("data_encode")
    ecap = int(lib.rio_index_entries_bound(n, c.key_bytes)) + L.RIO_DEVICE_PAD
    entries, ent_off = u8(ecap), i64(n + 1)
    check_status(lib.rio_sst_index_encode(ctx, c.out_src.data_ptr(), data_rec_off.data_ptr(), n, entries.data_ptr(),
                                    ecap - L.RIO_DEVICE_PAD, ent_off.data_ptr(), st), "rio_sst_index_encode")
    mark("index_entries")
    ent_bytes = int(ent_off[n].item())  # rio_device_encode sizes its scratch from the arena length
    mark("entries_length_read")
    icap = int(lib.rio_encode_bound(n, ent_bytes, L.COMP_NONE))
    c.index_img, index_rec_off, c.index_len = u8(icap), i64(n), i64(1)
    check_status(lib.rio_device_encode(ctx, entries.data_ptr(), ent_off.data_ptr(), None, n, ent_bytes, L.COMP_NONE,
                                 c.index_img.data_ptr(), icap, index_rec_off.data_ptr(), c.index_len.data_ptr(), st),
           "rio_device_encode(index)")
    mark("index_encode")
    c.values, c.val_off, c.val_flags = values, val_off, val_flags
    c.entries, c.ent_off, c.ent_bytes = entries, ent_off, ent_bytes
    c.data_rec_off, c.index_rec_off = data_rec_off, index_rec_off
    return c


def compact_on_device(ctx, device: int, views, mode: int, comp: int, mark=None, flt=None) -> Compaction:
    """Plan, gather, data encode, index entries, index encode on torch's current stream. `views` is a
    ctypes array of SstView. `mark(name)` is called after each stage is enqueued and after each of the two
    host reads (benchmarks record an event there, so the host gaps are intervals of their own). The file images stay on the device; data_len / index_len are 1-element tensors.
    flt: the table's bloom filter to build, as for encode_planned."""
    import torch

    mark = mark or (lambda name: None)
    dev = f"cuda:{device}"
    n_in = sum(v.n for v in views)

    def run(st):
        src = torch.empty(max(n_in, 1), dtype=torch.int64, device=dev)
        keep = torch.empty(max(n_in, 1), dtype=torch.uint8, device=dev)
        res = torch.empty(L.RIO_MERGE_RESULT_WORDS, dtype=torch.int64, device=dev)
        check_status(L.lib().rio_sst_merge_plan(ctx, ctypes.addressof(views), len(views), mode, src.data_ptr(), keep.data_ptr(),
                                          res.data_ptr(), st), "rio_sst_merge_plan")
        mark("plan")
        return encode_planned(ctx, device, st, src, keep, res, comp, mark, mode == L.RIO_MERGE_ALL, flt)

    return on_device_stream(device, run)


def write_table_files(path: str, c: Compaction, min_key: bytes, max_key: bytes):
    """data.rio, index.rio and meta.pb.bin of a finished Compaction (its images are fetched here), and
    bloom.bf.gz when the compaction built a filter (header n = numRecords: one Add per written key)."""
    from . import BloomFileName, DataFileName, IndexFileName, MetaFileName

    dn, ixn = int(c.data_len.item()), int(c.index_len.item())
    data = bytes(c.data_img[:dn].cpu().numpy())
    index = bytes(c.index_img[:ixn].cpu().numpy())
    meta = proto.MetaData(version=1, numRecords=c.n_out, nullValues=c.null_values)
    if c.n_out:
        meta.minKey, meta.maxKey = min_key, max_key
    meta.dataBytes, meta.indexBytes, meta.totalBytes = len(data), len(index), len(data) + len(index)
    os.makedirs(path, exist_ok=True)
    for name, b in ((DataFileName, data), (IndexFileName, index), (MetaFileName, meta.marshal())):
        with open(os.path.join(path, name), "wb") as fh:
            fh.write(b)
    if c.bloom is not None:
        flt, d = c.bloom
        out = bloom.Filter(flt.m, flt.keys, bytearray(d.bits.cpu().numpy().tobytes()), c.n_out)
        err = out.WriteFile(os.path.join(path, BloomFileName))
        if err is not None:
            raise err
        c.filter = out
    c.meta, c.data_file, c.index_file = meta, data, index


def refuse_inputs(readers):
    """The UnsupportedError with which the device merge hands `readers` back to the reference merger, or None.
    Shared by the merger and by SuperSSTableReader's scans, which are merges of the stack's tables."""
    from . import SSTableReader, UnsupportedError

    if not readers or len(readers) > L.RIO_MERGE_MAX_TABLES:
        return UnsupportedError(f"merge of {len(readers)} tables (1 .. {L.RIO_MERGE_MAX_TABLES})")
    for r in readers:
        if not isinstance(r, SSTableReader) or r.t is None:
            return UnsupportedError("merge inputs are open SSTableReaders of NewSSTableReader")
        if r.meta.version == 0 or r.t.v0:
            return UnsupportedError(f"sstable '{r.opts.basePath}': v0 tables are merged by the reference merger")
        if r.opts.device != readers[0].opts.device:
            return UnsupportedError("merge inputs are on different devices")
        t = r.t
        if t.n_index > t.n_data or t.value_bad != _NONE:
            return UnsupportedError(f"sstable '{r.opts.basePath}': a value of the table cannot be read")
        # a value that fails its stored checksum (a reader opened with SkipHashCheckOnLoad): with hash checks on
        # reads the reference's scan reports it (sstable_iterator.go:100-108), so the table goes back to the
        # reference merger; without them the value is merged as the reference merges it, and the new index
        # carries the CRC-64 of the value as read (what WriteNext computes, sstable_writer.go:120-124)
        if t.bad_crc != _NONE and not r.opts.skipHashCheckOnRead:
            return UnsupportedError(f"sstable '{r.opts.basePath}': a value fails its checksum and hash checks "
                                    "on reads are enabled")
    return None


class SSTableMerger:
    def __init__(self, comp=None, data_compression: int = L.COMP_SNAPPY):
        """comp: bytes comparator only (skiplist.BytesComparator, the reference's default)."""
        self.data_compression = data_compression
        self.compaction = None  # the last written table's Compaction: its buffers stay in HBM while this holds them

    def Merge(self, readers, writer_path: str, data_compression=None, writer_options=()):  # noqa: N802
        """SSTableMerger.Merge (sstable_merger.go:41-68): every entry of every table, nil values too. Two
        tables holding one key give WriteNext's error; no file is written then (the reference leaves the
        table written up to that key behind). writer_options: the output writer's bloom options
        (sstables.EnableBloomFilter, BloomExpectedNumberOfElements, BloomFalsePositiveProbability)."""
        return self._run(readers, writer_path, L.RIO_MERGE_ALL, data_compression, writer_options)

    def MergeCompact(self, readers, writer_path: str, reduce, data_compression=None, writer_options=()):  # noqa: N802
        """SSTableMerger.MergeCompact (sstable_merger.go:146-165) with one of the reference's reducers;
        the reader's position in `readers` is its context (super_sstable_reader.go:88-97). writer_options as
        for Merge (simpledb/compaction.go:79 sizes the filter for every compaction)."""
        from . import UnsupportedError

        if not isinstance(reduce, _Reducer):
            return UnsupportedError("MergeCompact on the device runs ScanReduceLatestWins / "
                                    "ScanReduceLatestWinsSkipTombstones only")
        return self._run(readers, writer_path, reduce.mode, data_compression, writer_options)

    def _run(self, readers, path, mode, comp, writer_options=()):
        import torch

        from . import UnsupportedError, _WriterOpts, writer_filter

        o = _WriterOpts(basePath=path)
        for f in writer_options:
            f(o)
        flt, err = writer_filter(o)
        if err is not None:
            return err

        comp = self.data_compression if comp is None else comp
        if comp not in (L.COMP_NONE, L.COMP_SNAPPY):
            return UnsupportedError(f"output data compression {comp}: the device encodes none and snappy")
        readers = list(readers)
        err = refuse_inputs(readers)
        if err is not None:
            return err
        device = readers[0].opts.device
        views = (L.SstView * len(readers))(*[table_view(r.t) for r in readers])
        with torch.cuda.device(device):
            c = compact_on_device(L.default_ctx(device), device, views, mode, comp, flt=flt)
            if c.status == "unsorted":
                return UnsupportedError(f"sstable '{readers[c.unsorted_table].opts.basePath}': keys are not strictly "
                                        "ascending")
            if c.status == "duplicate":
                return GoError(f"sstables.WriteNext '{path}': the same key cannot be written more than once")
            lo = hi = b""
            if c.n_out:
                first, last = (int(x) & _NONE for x in c.out_src[[0, c.n_out - 1]].cpu().tolist())
                lo = readers[first >> L.RIO_MERGE_ENTRY_BITS].t.key(first & _ENTRY_MASK)
                hi = readers[last >> L.RIO_MERGE_ENTRY_BITS].t.key(last & _ENTRY_MASK)
            write_table_files(path, c, lo, hi)
            self.compaction = c
        return None


def NewSSTableMerger(comp=None, data_compression: int = L.COMP_SNAPPY):  # noqa: N802
    return SSTableMerger(comp, data_compression)
