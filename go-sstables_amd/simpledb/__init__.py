"""simpledb's crash recovery on the device: a WAL directory to one SSTable.

recover_wal mirrors replayAndSetupWriteAheadLog (simpledb/recovery.go:208-268) without the DB object. The
reference joins its stages with one host loop: proto.Unmarshal of every WAL record into a WalMutation, then
memStore.Upsert / Tombstone, then FlushWithTombstones. Here the decoded WAL stays in HBM: rio_wal_ops_plan /
rio_wal_ops_gather (csrc/rio_walops.hip) turn the decoded records into the op log rio_sst_flush_plan takes, and
the flush's back end writes the table. The host reads the plan's 64-byte result block, then what the flush
reads. Functions return Go-style error values. There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
import shutil

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
