"""ctypes binding of librio.so (include/rio.h).

The library is built in-tree (go-sstables_amd/librio.so) by __graft_entry__.build() /
`make -C go-sstables_amd/csrc`. Loading it needs no GPU; every decode entry point needs one and
fails loudly (RIO_ERR_HIP) without it. There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_uint8, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# RIO_LIB_PATH: load an experiment build (csrc/Makefile `variant`) instead of the in-tree library
LIB_PATH = os.environ.get("RIO_LIB_PATH") or os.path.normpath(os.path.join(_HERE, "..", "librio.so"))

# status codes (rio.h rio_status)
RIO_OK = 0
RIO_EOF = 1
RIO_EOF_ZERO_TAIL = 2
RIO_EOF_HEADER = 3
RIO_EOF_PAYLOAD = 4
RIO_ERR_UNEXPECTED_EOF = 5
RIO_ERR_MAGIC = 6
RIO_ERR_HEADER_CRC = 7
RIO_ERR_VARINT_OVERFLOW = 8
RIO_ERR_HEADER_TOO_LONG = 9
RIO_ERR_DECOMPRESS = 10
RIO_ERR_VERSION = 11
RIO_ERR_COMPRESSION_TYPE = 12
RIO_ERR_SHORT_FILE_HEADER = 13
RIO_ERR_INVALID_OFFSET = 14
RIO_ERR_UNSUPPORTED = 15
RIO_ERR_CAPACITY = 16
RIO_ERR_ARG = 17
RIO_ERR_HIP = 18
RIO_ERR_STATE = 19
RIO_ERR_IO = 20
RIO_ERR_PROTO = 21
RIO_EOF_CODEC = 22

EOF_CLASS = (RIO_EOF, RIO_EOF_ZERO_TAIL, RIO_EOF_HEADER, RIO_EOF_PAYLOAD, RIO_EOF_CODEC)

RIO_FLAG_NIL = 1
RIO_FLAG_CORRUPT = 2
RIO_FLAG_EOF = 4
RIO_DEVICE_PAD = 64
RIO_VALUE_NIL = 0xFFFFFFFFFFFFFFFF  # rio_sst_data_entries: DataEntry without a value field
RIO_VALUE_BAD = 0xFFFFFFFFFFFFFFFE  # rio_sst_data_entries: not a valid DataEntry
RIO_SST_V0_VALUES = 1
RIO_COMP_UNKNOWN = 0xFFFFFFFF
COMP_NONE, COMP_GZIP, COMP_SNAPPY, COMP_LZW = 0, 1, 2, 3


class FileInfo(ctypes.Structure):
    _fields_ = [
        ("version", c_uint32),
        ("compression", c_uint32),
        ("n_records", c_uint64),
        ("total_out_bytes", c_uint64),
        ("status", ctypes.c_int32),
        ("reserved0", c_uint32),
        ("status_offset", c_uint64),
        ("detail0", c_uint64),
        ("detail1", c_uint64),
        ("n_chunks", c_uint64),
        ("n_repairs", c_uint64),
        ("first_bad", c_uint64),
        ("n_bad", c_uint64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved0"}


class SstInfo(ctypes.Structure):
    """rio_sst_info (include/rio.h)."""

    _fields_ = [
        ("index", FileInfo),
        ("data", FileInfo),
        ("n_entries", c_uint64),
        ("first_bad_proto", c_uint64),
        ("first_bad_crc", c_uint64),
        ("first_unplaced", c_uint64),
        ("index_bad", c_uint64),
        ("first_bad_value", c_uint64),
    ]


RIO_MERGE_MAX_TABLES = 256
RIO_MERGE_ENTRY_BITS = 40
RIO_MERGE_ALL, RIO_MERGE_LATEST_WINS, RIO_MERGE_LATEST_WINS_SKIP_TOMBSTONES = 0, 1, 2
RIO_MERGE_RESULT_WORDS = 8
(RIO_MERGE_R_N_OUT, RIO_MERGE_R_VALUE_BYTES, RIO_MERGE_R_NULL_VALUES, RIO_MERGE_R_FIRST_DUP, RIO_MERGE_R_UNSORTED,
 RIO_MERGE_R_KEY_BYTES) = range(6)


class SstView(ctypes.Structure):
    """rio_sst_view (include/rio.h): one loaded table's device arrays."""

    _fields_ = [
        ("index", c_void_p),
        ("key_off", c_void_p),
        ("key_len", c_void_p),
        ("data", c_void_p),
        ("data_off", c_void_p),
        ("flags", c_void_p),
        ("crc", c_void_p),
        ("n", c_uint64),
        ("index_bytes", c_uint64),
        ("data_bytes", c_uint64),
    ]


RIO_BLOOM_MAX_K = 64


class BloomView(ctypes.Structure):
    """rio_bloom_view (include/rio.h): a filter's bits and hash keys on the device."""

    _fields_ = [
        ("bits", c_void_p),
        ("hash_keys", c_void_p),
        ("m", c_uint64),
        ("k", c_uint32),
    ]


RIO_GET_VALUE, RIO_GET_NOT_FOUND, RIO_GET_NIL, RIO_GET_HOST = 0, 1, 2, 3  # rio_sst_stack_value_plan's status bytes

RIO_FLUSH_WITH_TOMBSTONES, RIO_FLUSH_SKIP_TOMBSTONES = 0, 1
RIO_FLUSH_MAX_KEY_LEN = 1024


class OpsView(ctypes.Structure):
    """rio_ops_view (include/rio.h): a memstore's op log on the device."""

    _fields_ = [
        ("keys", c_void_p),
        ("key_off", c_void_p),
        ("values", c_void_p),
        ("val_off", c_void_p),
        ("flags", c_void_p),
        ("n", c_uint64),
        ("key_bytes", c_uint64),
        ("value_bytes", c_uint64),
    ]


RIO_DB_MAX_MEMSTORES = 2
RIO_GET_MEM_VALUE = 4  # rio_db_value_plan: a memstore's value answers


class MemIndex(ctypes.Structure):
    """rio_mem_index (include/rio.h): an op log with its searchable order, by value."""

    _fields_ = [
        ("ops", OpsView),
        ("order", c_void_p),
        ("pfx", c_void_p),
        ("result", c_void_p),
    ]


RIO_SIZE_RESULT_WORDS = 8  # rio_mem_size_scan's result block
RIO_SIZE_R_CUT, RIO_SIZE_R_SIZE, RIO_SIZE_R_KEY_END, RIO_SIZE_R_VALUE_END, RIO_SIZE_R_FIRST_BAD = range(5)

RIO_WAL_MAX_SEGMENTS = 4096
RIO_WAL_RESULT_WORDS = 8
(RIO_WAL_R_N_RECORDS, RIO_WAL_R_N_OPS, RIO_WAL_R_KEY_BYTES, RIO_WAL_R_VALUE_BYTES, RIO_WAL_R_MAX_KEY_LEN,
 RIO_WAL_R_FIRST_BAD, RIO_WAL_R_BAD_CLASS) = range(7)
RIO_WAL_BAD_PROTO, RIO_WAL_BAD_UTF8, RIO_WAL_BAD_VALUE_NIL, RIO_WAL_BAD_RANGE = 1, 2, 3, 4
RIO_WALENC_RESULT_WORDS = 8
(RIO_WALENC_R_N_RECORDS, RIO_WALENC_R_BYTES, RIO_WALENC_R_N_UPSERTS, RIO_WALENC_R_N_DELETES, RIO_WALENC_R_MAX_KEY_LEN,
 RIO_WALENC_R_FIRST_BAD, RIO_WALENC_R_BAD_CLASS) = range(7)


class WalSegment(ctypes.Structure):
    """rio_wal_segment (include/rio.h): one decoded WAL file on the device."""

    _fields_ = [
        ("out", c_void_p),
        ("out_off", c_void_p),
        ("flags", c_void_p),
        ("n", c_uint64),
        ("out_bytes", c_uint64),
    ]


class IndexHit(ctypes.Structure):
    """rio_index_hit (include/rio.h)."""

    _fields_ = [
        ("offset", c_uint64),
        ("value_offset", c_uint64),
        ("checksum", c_uint64),
        ("status", ctypes.c_int32),
        ("found", ctypes.c_int32),
    ]


class ReadAtHit(ctypes.Structure):
    """rio_read_at_hit (include/rio.h): one query of a batched ReadNextAt."""

    _fields_ = [
        ("status", ctypes.c_int32),
        ("nil", ctypes.c_int32),
        ("len", c_uint64),
        ("detail0", c_uint64),
        ("detail1", c_uint64),
        ("hdr_len", c_uint64),
        ("payload_off", c_uint64),
    ]


RIO_SEEK_END_OTHER = (1 << 63) - 1
RIO_SEEK_END_EOF = RIO_SEEK_END_OTHER - 1


class ReaderIndexInfo(ctypes.Structure):
    """struct rio_reader_index_info (include/rio.h)."""

    _fields_ = [
        ("n_records", c_uint64),
        ("n_positions", c_uint64),
        ("positions", POINTER(c_uint64)),
        ("ends", POINTER(c_uint64)),
    ]


# name -> (restype, argtypes)
_SIGS = {
    "rio_strerror": (c_char_p, [c_int]),
    "rio_status_is_eof": (c_int, [c_int]),
    "rio_build_info": (c_char_p, []),
    "rio_ctx_create": (c_int, [c_int, POINTER(c_void_p)]),
    "rio_ctx_destroy": (None, [c_void_p]),
    "rio_ctx_device": (c_int, [c_void_p]),
    "rio_ctx_acquire": (c_int, [c_int, POINTER(c_void_p)]),
    "rio_ctx_release": (None, [c_void_p]),
    "rio_device_count": (c_int, [POINTER(c_int)]),
    "rio_frame": (c_int, [c_void_p, c_void_p, c_uint64, POINTER(FileInfo)]),
    "rio_host_register": (c_int, [c_void_p, c_uint64]),
    "rio_host_unregister": (c_int, [c_void_p]),
    "rio_decode": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_uint64, POINTER(FileInfo)]),
    "rio_device_decode": (
        c_int,
        [c_void_p, c_void_p, c_uint64, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p],
    ),
    "rio_device_decode_ex": (
        c_int,
        [c_void_p, c_void_p, c_uint64, c_uint32, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p,
         c_void_p],
    ),
    "rio_ctx_reserve": (c_int, [c_void_p, c_uint64, c_uint64, c_uint32]),
    "rio_ctx_arena_bytes": (c_uint64, [c_void_p]),
    "rio_device_decode_batch": (
        c_int,
        [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
         c_void_p],
    ),
    "rio_max_records": (c_uint64, [c_uint64]),
    "rio_ctx_last_stage_ms": (c_int, [c_void_p, POINTER(c_float), c_int]),
    "rio_ctx_set_timing": (c_int, [c_void_p, c_int]),
    "rio_device_read_at": (
        c_int,
        [c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_uint64, POINTER(c_uint64), POINTER(c_int),
         POINTER(c_uint64), POINTER(c_uint64)],
    ),
    "rio_device_read_at_plan": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p]),
    "rio_device_read_at_copy": (
        c_int, [c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p]),
    "rio_reader_new_file": (c_int, [c_void_p, c_char_p, POINTER(c_void_p)]),
    "rio_reader_new_mmap": (c_int, [c_void_p, c_char_p, POINTER(c_void_p)]),
    "rio_reader_open": (c_int, [c_void_p]),
    "rio_reader_close": (c_int, [c_void_p]),
    "rio_reader_free": (None, [c_void_p]),
    "rio_reader_header": (c_int, [c_void_p, POINTER(c_uint32), POINTER(c_uint32)]),
    "rio_reader_size": (c_uint64, [c_void_p]),
    "rio_reader_last_detail": (None, [c_void_p, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
    "rio_reader_read_next": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_uint64), POINTER(c_int)]),
    "rio_reader_skip_next": (c_int, [c_void_p]),
    "rio_reader_read_next_at": (c_int, [c_void_p, c_uint64, POINTER(c_void_p), POINTER(c_uint64), POINTER(c_int)]),
    "rio_reader_read_next_at_batch": (
        c_int, [c_void_p, c_void_p, c_uint64, POINTER(ReadAtHit), POINTER(c_void_p), POINTER(POINTER(c_uint64))]),
    "rio_reader_seek_next": (
        c_int, [c_void_p, c_uint64, POINTER(c_uint64), POINTER(c_void_p), POINTER(c_uint64), POINTER(c_int)]),
    "rio_reader_set_seek_len": (c_int, [c_void_p, c_uint64]),
    "rio_reader_index_info": (c_int, [c_void_p, POINTER(ReaderIndexInfo)]),
    "rio_reader_file_info": (c_int, [c_void_p, POINTER(FileInfo)]),
    "rio_writer_new": (c_int, [c_char_p, c_uint32, POINTER(c_void_p)]),
    "rio_writer_write": (c_int, [c_void_p, c_void_p, c_uint64, POINTER(c_uint64)]),
    "rio_writer_size": (c_uint64, [c_void_p]),
    "rio_writer_close": (c_int, [c_void_p]),
    "rio_encode_record_v4": (c_uint64, [c_void_p, c_uint64, c_uint32, c_void_p, c_uint64]),
    "rio_encode_file_header": (None, [c_void_p, c_uint32, c_uint32]),
    "rio_snappy_max_encoded_len": (c_uint64, [c_uint64]),
    "rio_snappy_encode": (c_uint64, [c_void_p, c_uint64, c_void_p, c_uint64]),
    "rio_generate": (c_uint64, [c_void_p, c_uint64, c_uint32, c_uint64, c_uint64, c_int, c_uint64, c_int]),
    "rio_generate_bound": (c_uint64, [c_uint32, c_uint64, c_uint64]),
    "rio_sst_index_parse": (
        c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rio_sst_validate": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p]),
    "rio_sst_data_entries": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p]),
    "rio_sst_validate_view": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p,
         c_void_p]),
    "rio_sst_open": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_uint64, POINTER(c_void_p), POINTER(SstInfo)]),
    "rio_sst_open_ex": (
        c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_uint64, c_uint32, POINTER(c_void_p), POINTER(SstInfo)]),
    "rio_sst_entry": (
        c_int,
        [c_void_p, c_uint64, POINTER(c_void_p), POINTER(c_uint64), POINTER(c_void_p), POINTER(c_uint64), POINTER(c_int),
         POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
    "rio_sst_free": (None, [c_void_p]),
    "rio_replay_open": (c_int, [c_int, c_void_p, c_uint64, c_uint32, c_uint32, POINTER(c_void_p)]),
    "rio_replay_next": (
        c_int, [c_void_p, POINTER(c_uint64), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), POINTER(FileInfo)]),
    "rio_replay_free": (None, [c_void_p]),
    "rio_replay_open_devices": (c_int, [c_void_p, c_uint32, c_void_p, c_uint64, c_uint32, c_uint32, POINTER(c_void_p)]),
    "rio_fileset_decode": (c_int, [c_void_p, c_uint32, c_void_p, c_uint64, POINTER(c_void_p)]),
    "rio_fileset_get": (c_int, [c_void_p, c_uint64, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p),
                                POINTER(c_void_p), POINTER(FileInfo), POINTER(c_int)]),
    "rio_fileset_free": (None, [c_void_p]),
    "rio_stream_open": (c_int, [c_int, c_char_p, c_uint64, c_uint32, POINTER(c_void_p)]),
    "rio_stream_open_host": (c_int, [c_int, c_void_p, c_uint64, c_uint64, c_uint32, POINTER(c_void_p)]),
    "rio_stream_next": (c_int, [c_void_p, POINTER(c_uint64), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p),
                                POINTER(c_void_p), POINTER(FileInfo)]),
    "rio_stream_free": (None, [c_void_p]),
    "rio_reader_set_window": (c_int, [c_void_p, c_uint64]),
    "rio_encode_bound": (c_uint64, [c_uint64, c_uint64, c_uint32]),
    "rio_device_encode": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_uint32, c_void_p, c_uint64, c_void_p,
                c_void_p, c_void_p]),
    "rio_encode_file": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint32, c_void_p, c_uint64, c_void_p,
                POINTER(c_uint64)]),
    "rio_device_index_search": (
        c_int, [c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p]),
    "rio_index_open": (c_int, [c_void_p, c_void_p, c_uint64, POINTER(c_void_p)]),
    "rio_index_search": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p]),
    "rio_index_free": (None, [c_void_p]),
    "rio_sst_merge_plan": (c_int, [c_void_p, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rio_sst_merge_gather": (
        c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p]),
    "rio_sst_index_encode": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_uint64, c_void_p, c_void_p]),
    "rio_index_entry_len": (c_uint64, [c_uint64, c_uint64, c_uint64]),
    "rio_index_entries_bound": (c_uint64, [c_uint64, c_uint64]),
    "rio_bloom_optimal": (c_int, [c_uint64, ctypes.c_double, POINTER(c_uint64), POINTER(c_uint64)]),
    "rio_bloom_add": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p]),
    "rio_sst_bloom_add": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p]),
    "rio_bloom_contains": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p]),
    "rio_sst_key_prefixes": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "rio_sst_lookup": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p]),
    "rio_sst_stack_create": (
        c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_uint64, POINTER(c_void_p), c_void_p]),
    "rio_sst_stack_free": (None, [c_void_p]),
    "rio_sst_stack_lookup": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p]),
    "rio_sst_stack_value_plan": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_void_p, c_void_p, c_void_p]),
    "rio_sst_stack_value_copy": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_uint64, c_void_p]),
    "rio_sst_stack_bounds": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_uint32, c_void_p, c_void_p]),
    "rio_sst_keys_gather": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_uint64, c_void_p, c_void_p]),
    "rio_sst_flush_plan": (c_int, [c_void_p, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rio_sst_flush_stage_ms": (c_int, [c_void_p, POINTER(c_float), c_int]),
    "rio_mem_index_build": (c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rio_mem_index_extend": (c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rio_ops_append": (c_int, [c_void_p, c_void_p, c_uint64, c_uint64, c_uint64, c_void_p, c_void_p]),
    "rio_mem_lookup": (c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p]),
    "rio_mem_size_scan": (
        c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_uint32, c_uint64, c_void_p, c_void_p, c_void_p]),
    "rio_db_reader_create": (c_int, [c_void_p, c_void_p, c_uint64, POINTER(c_void_p)]),
    "rio_db_reader_free": (None, [c_void_p]),
    "rio_db_value_plan": (
        c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_uint64, c_uint32, c_void_p, c_void_p, c_void_p]),
    "rio_db_value_copy": (
        c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_uint64,
                c_void_p]),
    "rio_wal_ops_plan": (c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_void_p]),
    "rio_wal_ops_gather": (
        c_int, [c_void_p, c_uint64, c_void_p, c_uint64, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p,
                c_void_p]),
    "rio_wal_ops_encode_bound": (c_uint64, [c_uint64, c_uint64, c_uint64]),
    "rio_wal_ops_encode": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p]),
    "rio_writer_append_framed": (c_int, [c_void_p, c_void_p, c_uint64]),
}

EXPORTED = tuple(_SIGS)

_lib = None


def lib():
    """Load librio.so (in-tree). Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"librio.so not built at {LIB_PATH}: run `make -C go-sstables_amd/csrc` "
                "(or __graft_entry__.build()); the recordio GPU path has no CPU fallback")
        # One HIP runtime per process: torch bundles its own libamdhip64 under the same soname as
        # the ROCm one librio.so links. Whichever loads first is used by both; if librio's loads
        # first, torch later finds no GPU. So when torch is present (the Python mirror uses it for
        # device buffers), it is imported before the library.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            if os.environ.get("RIO_LIB_PATH") and not hasattr(L, name):
                continue  # an older experiment build (A/B timing) may predate some entry points
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def strerror(status: int) -> str:
    return lib().rio_strerror(status).decode()


_ctx = {}


def default_ctx(device: int = 0) -> int:
    """A per-device rio_ctx (created lazily; needs a GPU)."""
    if device not in _ctx:
        h = c_void_p()
        rc = lib().rio_ctx_create(device, ctypes.byref(h))
        if rc != RIO_OK:
            raise RuntimeError(f"rio_ctx_create(device={device}) failed: {strerror(rc)} "
                               "(the recordio decode path needs a HIP device)")
        _ctx[device] = h.value
    return _ctx[device]
