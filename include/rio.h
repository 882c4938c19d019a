/*
 * rio.h — C-ABI of the MI355X-native recordio decode path (v3/v4, and the legacy v1/v2 layouts).
 *
 * This is the drop-in boundary a Go `recordio` adapter (behind `//go:build cgo && rocm`) binds
 * with cgo; see INTEGRATION.md for the binding. Plain pointers and sizes only, no torch/HIP types
 * in any signature (a HIP stream is passed as `void*`). The library never retains a caller pointer
 * after a call returns.
 *
 * Reference interfaces replaced (github.com/thomasjungblut/go-sstables, paths relative to the repo):
 *   recordio.ReaderI  {Open, Close, ReadNext, SkipNext}          recordio/recordio.go:83-89
 *   recordio.ReadAtI  {Open, Close, Size, ReadNextAt, SeekNext}   recordio/recordio.go:91-105
 *   NewFileReaderWithPath / NewFileReader                         recordio/file_reader.go:490-524
 *   NewMemoryMappedReaderWithPath                                 recordio/mmap_reader.go:364-371
 *   FileReader.ReadNext v4 / v3 (sequential whole-file semantics) recordio/file_reader.go:61-131, 389-447
 *     readNextV2 / readNextV1                                     recordio/file_reader.go:322-388, 282-320
 *   MMapReader.ReadNextAt v4 / v3                                 recordio/mmap_reader.go:130-203, 298-356
 *     readNextAtV2 / readNextAtV1                                 recordio/mmap_reader.go:242-296, 205-240
 *   MMapReader.SeekNext                                           recordio/mmap_reader.go:58-128
 *   readFileHeaderFromBuffer                                      recordio/common_reader.go:22-44
 *   readRecordHeaderV1 / V2                                       recordio/common_reader.go:46-81
 *   readRecordHeaderV3 / V4 + checksumByteReader                  recordio/common_reader.go:83-151,
 *                                                                 recordio/checksum_byte_reader.go:11-60
 *   SnappyCompressor.DecompressWithBuf (golang/snappy v1.0.0)     recordio/compressor/snappy_compression.go:22-24
 *   NewSSTableReader load / validateDataFile / Scan (rio_sst_*)   sstables/sstable_reader.go:250-345, 205-238, 119-159
 *   DiskKeyIndex binarySearch (rio_index_*)                       sstables/disk_key_index.go:87-140
 *   wal.Replayer.Replay (rio_replay_*)                            wal/replayer.go:18-77
 *   SSTableStreamWriter's bloom filter: NewOptimal / Add          sstables/sstable_writer.go:78-83, 114-118, 150-154
 *     (rio_bloom_optimal, rio_bloom_add, rio_sst_bloom_add)
 *   SSTableReader.Contains / Get, SliceKeyIndex.Get in batches    sstables/sstable_reader.go:49-77,
 *     (rio_bloom_contains, rio_sst_key_prefixes, rio_sst_lookup)  sstables/slice_key_index.go:19-35
 *   SuperSSTableReader.Contains / Get / Scan* over a stack        sstables/super_sstable_reader.go:18-105
 *     (rio_sst_stack_*, rio_sst_keys_gather)
 *   FileWriter.Write + fillRecordHeaderV4 (input generator only)  recordio/file_writer.go:160-233
 */
#ifndef RIO_H
#define RIO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------ */
/* Format constants (recordio/recordio.go:11-43)                                               */
/* ------------------------------------------------------------------------------------------ */
#define RIO_VERSION1 1u
#define RIO_VERSION2 2u
#define RIO_VERSION3 3u
#define RIO_VERSION4 4u
#define RIO_MAGIC 0x130691u /* MagicNumberSeparatorLong, uvarint bytes 91 8d 4c */
#define RIO_FILE_HEADER_BYTES 8u
#define RIO_RECORD_HEADER_V1_BYTES 20u /* RecordHeaderSizeBytesV1V2: LE u32 magic, LE u64 u, LE u64 c */
#define RIO_RECORD_HEADER_V3_MAX 31u /* RecordHeaderV3MaxSizeBytes */
#define RIO_RECORD_HEADER_V4_MAX 36u /* RecordHeaderV4MaxSizeBytes */
#define RIO_COMP_NONE 0u
#define RIO_COMP_GZIP 1u
#define RIO_COMP_SNAPPY 2u
#define RIO_COMP_LZW 3u
/* Device input buffers handed to rio_device_decode must have this many readable bytes past
 * `len` (the kernels load whole aligned 16-B words around headers; bytes past `len` are never
 * interpreted). */
#define RIO_DEVICE_PAD 64u

/* ------------------------------------------------------------------------------------------ */
/* Status codes: one per error class the reference's readers distinguish.                     */
/* `rio_status_is_eof(s)` answers `errors.Is(err, io.EOF)` for the error the reference returns. */
/* ------------------------------------------------------------------------------------------ */
typedef enum rio_status {
    RIO_OK = 0,
    /* header read hit EOF before its first byte: FileReader wraps io.EOF once
     * (file_reader.go:93), MMapReader.ReadNextAt returns a bare io.EOF (mmap_reader.go:153-155) */
    RIO_EOF = 1,
    /* FileReader only: magic mismatch and every byte after the consumed magic varint is zero
     * (DirectIO padding) -> bare io.EOF (file_reader.go:76-91) */
    RIO_EOF_ZERO_TAIL = 2,
    /* io.EOF on the first byte of a later header field (nil byte / u / c / crc varint) */
    RIO_EOF_HEADER = 3,
    /* payload read classified as io.EOF: FileReader io.ReadFull read 0 bytes (file_reader.go:104-107);
     * MMapReader any short ReadAt (mmap_reader.go:175-178) */
    RIO_EOF_PAYLOAD = 4,
    RIO_ERR_UNEXPECTED_EOF = 5,   /* io.ErrUnexpectedEOF (partial varint / partial payload) */
    RIO_ERR_MAGIC = 6,            /* MagicNumberMismatchErr (common_reader.go:19) */
    RIO_ERR_HEADER_CRC = 7,       /* HeaderChecksumMismatchErr (common_reader.go:20,140-148) */
    RIO_ERR_VARINT_OVERFLOW = 8,  /* binary.ReadUvarint overflow */
    RIO_ERR_HEADER_TOO_LONG = 9,  /* "checksum byte reader out of range" (checksum_byte_reader.go:25-27) */
    RIO_ERR_DECOMPRESS = 10,      /* codec error (snappy ErrCorrupt, gzip errors) */
    RIO_ERR_VERSION = 11,         /* "version mismatch, expected a value from 1 to 4 but was N" */
    RIO_ERR_COMPRESSION_TYPE = 12,/* "unknown compression type [N]" */
    RIO_ERR_SHORT_FILE_HEADER = 13,/* fewer than 8 bytes in the file */
    RIO_ERR_INVALID_OFFSET = 14,  /* "mmap: invalid ReadAt offset N" (offset > size) */
    RIO_ERR_UNSUPPORTED = 15,     /* a request the GPU path does not serve (SeekNext on v1 files
                                     mmap_reader.go:62-64; see DESIGN.md §8 for the rest) */
    RIO_ERR_CAPACITY = 16,        /* caller-provided output arrays too small */
    RIO_ERR_ARG = 17,             /* bad argument */
    RIO_ERR_HIP = 18,             /* HIP runtime failure */
    RIO_ERR_STATE = 19,           /* reader not opened / already closed / already opened */
    RIO_ERR_IO = 20,              /* file open / mmap / read failure */
    RIO_ERR_PROTO = 21,           /* proto.Unmarshal of an IndexEntry failed (invalid wire format) */
    /* the codec returned io.EOF: gzip.NewReader on an empty payload (gzip_compression.go:56-59).
     * FileReader.ReadNext returns it bare (file_reader.go:119-121), MMapReader.ReadNextAt wraps it
     * once ("failed decompressing record", mmap_reader.go:189-191); errors.Is(err, io.EOF) holds */
    RIO_EOF_CODEC = 22,
    RIO_STATUS_COUNT_ = 22
} rio_status;

const char* rio_strerror(int status);
int rio_status_is_eof(int status);
const char* rio_build_info(void);

/* ------------------------------------------------------------------------------------------ */
/* Whole-file decode result.                                                                   */
/* Sequential semantics: `n_records` records are delivered in file order, then `status`.       */
/* A clean end is one of the RIO_EOF family. Records with index < n_records are valid even if   */
/* status is an error: the reference's ReadNext loop returns them before the error.            */
/* A record whose payload fails to decompress does not end the sequence: FileReader.ReadNext     */
/* returns the codec error for it and the next call reads the record after it (the payload was   */
/* consumed, file_reader.go:101-125), so such a record is delivered with RIO_FLAG_CORRUPT (or    */
/* RIO_FLAG_EOF for gzip's empty payload) and the records after it are decoded. Its slice of     */
/* `out` has the length its payload announced (snappy preamble, gzip ISIZE; 0 when that is       */
/* unusable) and unspecified bytes. first_bad / n_bad summarise the flagged records.             */
/* ------------------------------------------------------------------------------------------ */
typedef struct rio_file_info {
    uint32_t version;         /* file header version (1..4) */
    uint32_t compression;     /* file header compression type (0..3) */
    uint64_t n_records;       /* records delivered before `status` */
    uint64_t total_out_bytes; /* sum of decoded record lengths of those records */
    int32_t status;           /* terminal status of the ReadNext loop */
    uint32_t reserved0;
    uint64_t status_offset;   /* file offset of the record header at which `status` was raised */
    uint64_t detail0;         /* HEADER_CRC: expected crc; VERSION/COMPRESSION_TYPE: value */
    uint64_t detail1;         /* HEADER_CRC: actual crc */
    uint64_t n_chunks;        /* framing chunks used (diagnostic) */
    uint64_t n_repairs;       /* chunks whose speculative entry had to be re-walked (diagnostic) */
    uint64_t first_bad;       /* first record flagged RIO_FLAG_CORRUPT / RIO_FLAG_EOF (~0: none) */
    uint64_t n_bad;           /* records so flagged (< n_records) */
} rio_file_info;

/* Per-record flag bits (rio_decode `flags`) */
#define RIO_FLAG_NIL 0x1u     /* record written as nil: ReadNext returns nil, not []byte{} */
#define RIO_FLAG_CORRUPT 0x2u /* the payload does not decompress: ReadNext returns the codec error
                                 (snappy ErrCorrupt / the gzip reader's error) for this record */
#define RIO_FLAG_EOF 0x4u     /* gzip: empty payload, gzip.NewReader's bare io.EOF for this record
                                 (gzip_compression.go:56-59, passed through by file_reader.go:118-121) */

/* ------------------------------------------------------------------------------------------ */
/* Context: one HIP device + stream + device arenas + pinned staging. NOT thread-safe: use one  */
/* per goroutine / host thread. Independent files on different devices need no communication. */
/* ------------------------------------------------------------------------------------------ */
typedef struct rio_ctx rio_ctx;

int rio_ctx_create(int device, rio_ctx** out);
void rio_ctx_destroy(rio_ctx* ctx);
int rio_device_count(int* out);
int rio_ctx_device(const rio_ctx* ctx); /* the context's device, -1 for NULL */
/* Pooled contexts for per-file readers (the Go adapter's FileReader.Open / Close,
 * file_reader.go:26-59): rio_ctx_acquire hands out an idle context of `device` from a process-wide
 * pool (creating one when none is idle), rio_ctx_release returns it (up to 4 idle per device are
 * kept, the rest destroyed). A fresh context grows every device arena on its first file (12-16 ms
 * for a 128 MiB file against 4.7 ms warm), so a reader per file should not create one. */
int rio_ctx_acquire(int device, rio_ctx** out);
void rio_ctx_release(rio_ctx* ctx);

/* ---- host-memory two-phase API (the cgo binding: one call pair per file) --------------------
 * rio_frame: H2D copy of the file through pinned staging, device framing (record boundaries,
 * header CRC, decoded sizes) and the scan; fills `info` (sizes the caller must allocate). For a
 * gzip file rio_frame also decodes it (a record of several gzip members is larger than its last
 * member's ISIZE, the framing's size, which only the decode finds out), so the sizes are exact.
 * rio_decode: device decode of every framed record + D2H of the results into caller buffers:
 *   out      [>= info->total_out_bytes]  concatenated record bytes
 *   out_off  [n_records + 1]             record i = out[out_off[i] .. out_off[i+1])
 *   rec_off  [n_records]                 file offset of record i's header (ReadNextAt offset)
 *   flags    [n_records]                 RIO_FLAG_NIL / RIO_FLAG_CORRUPT / RIO_FLAG_EOF
 * rio_decode fills info->first_bad / n_bad (records that fail to decompress are flagged, not cut). */
int rio_frame(rio_ctx* ctx, const uint8_t* file, uint64_t len, rio_file_info* info);
int rio_decode(rio_ctx* ctx, uint8_t* out, uint64_t out_cap, uint64_t* out_off, uint64_t* rec_off,
               uint8_t* flags, uint64_t rec_cap, rio_file_info* info);
/* rio_host_register / rio_host_unregister: page-lock a host buffer the caller reuses for file images
 * (hipHostRegister). rio_frame and rio_stream_open_host then copy such an image to the device by DMA
 * in place instead of through the pinned staging pieces; results are the same either way. No
 * reference counterpart: the cgo adapter would register its read buffer pool once.
 * Unregister such a range with rio_host_unregister; a range unlocked behind the library's back is
 * detected (hipPointerGetAttributes) and copied through staging. */
int rio_host_register(const void* p, uint64_t n);
int rio_host_unregister(const void* p);

/* ---- device-resident API: the file is already in HBM; everything runs on `stream` with no host
 * synchronisation (graph-capturable). Outputs are device pointers with the layout above; the
 * result struct is written to device memory `d_info`. `d_file` must have RIO_DEVICE_PAD readable
 * bytes past `len`. If the decoded size exceeds out_cap or rec_cap, d_info->status is
 * RIO_ERR_CAPACITY with the sizes needed in d_info and nothing usable is decoded (call again with
 * outputs of that size). A gzip file whose records of several members outgrow the framing's sizes
 * reports this only after its decode: a capacity-0 probe can undersize it, so loop on CAPACITY.
 * `stream` is a hipStream_t (NULL = the ctx stream). */
/* Calls of one ctx share its device scratch. The library orders the decode calls across streams:
 * rio_device_decode, rio_device_decode_ex or rio_device_decode_batch on a stream other than the
 * previous decode call's waits (stream-ordered) for that call, and so do rio_frame and rio_decode on
 * the ctx stream. Every other call that takes a `stream` (rio_device_encode, rio_sst_*, rio_bloom_*,
 * rio_wal_ops_*, rio_device_index_search) is not ordered by the library: a sequence of them on one
 * ctx runs on one stream, and a caller that changes streams between calls sharing a ctx orders them
 * itself (an event, or a stream wait). Arenas grow on demand (hipMalloc); before capturing
 * calls into a hipGraph, size them with rio_ctx_reserve (largest file length, record count and batch
 * size to come) so that nothing is allocated during capture, and capture on the stream of the
 * previous call. */
int rio_ctx_reserve(rio_ctx* ctx, uint64_t max_file_len, uint64_t max_records, uint32_t max_batch);
/* Device bytes the ctx's framing and decode arenas hold (grow-only; no reference counterpart): constant across
 * calls after rio_ctx_reserve, whichever walk the automatic choice takes for each file. */
uint64_t rio_ctx_arena_bytes(const rio_ctx* ctx);
int rio_device_decode(rio_ctx* ctx, const uint8_t* d_file, uint64_t len, uint8_t* d_out,
                      uint64_t out_cap, uint64_t* d_out_off, uint64_t* d_rec_off, uint8_t* d_flags,
                      uint64_t rec_cap, rio_file_info* d_info, void* stream);
/* Same as rio_device_decode for a file whose 8-byte header the caller has already read (an mmap'd or
 * uploaded file): `compression` is its compression type, so only that codec's decode kernels are
 * launched (a Snappy file: 6 launches). RIO_COMP_UNKNOWN launches every decoder, as
 * rio_device_decode does. A file whose header contradicts the hint comes back as RIO_ERR_ARG. */
#define RIO_COMP_UNKNOWN 0xFFFFFFFFu
int rio_device_decode_ex(rio_ctx* ctx, const uint8_t* d_file, uint64_t len, uint32_t compression, uint8_t* d_out,
                         uint64_t out_cap, uint64_t* d_out_off, uint64_t* d_rec_off, uint8_t* d_flags, uint64_t rec_cap,
                         rio_file_info* d_info, void* stream);
/* Batch form: n_files device-resident files, file k = d_files[k] (lens[k] bytes, 16-byte aligned,
 * RIO_DEVICE_PAD readable bytes past it) decoded into its own outputs (d_out[k] ... d_info[k], as for
 * rio_device_decode). The arrays of pointers are host arrays; everything runs on `stream` without
 * host synchronisation. Replaces a loop of FileReader / MMapReader opens over a directory or shard
 * (wal/replayer.go:18-77, BASELINE configs[3]): the large-record decoder runs once across the files. */
int rio_device_decode_batch(rio_ctx* ctx, uint32_t n_files, const uint8_t* const* d_files, const uint64_t* lens,
                            uint8_t* const* d_out, const uint64_t* out_cap, uint64_t* const* d_out_off,
                            uint64_t* const* d_rec_off, uint8_t* const* d_flags, const uint64_t* rec_cap,
                            rio_file_info* const* d_info, void* stream);
/* Upper bound on records in a file of `len` bytes (the smallest record is v2's empty one, 5 bytes:
 * magic, u = 0, c = 0; v3 / v4 / v1 take 6 / 7 / 20). */
uint64_t rio_max_records(uint64_t len);
/* Kernel-timing probe for benchmarks: per-stage device milliseconds (walk, scan, placement, decode) averaged
 * over the decodes recorded since rio_ctx_set_timing; fills up to n entries, returns the count (0 when timing
 * is off). rio_ctx_set_timing(ctx, slots): record HIP events around the stages of the next `slots` calls
 * (a ring; 0 = off, the default: the events cost ~3 us each per call). */
int rio_ctx_last_stage_ms(rio_ctx* ctx, float* ms, int n);
int rio_ctx_set_timing(rio_ctx* ctx, int enable);

/* ---- sstables on the device (sstables/sstable_reader.go). Both calls work on arenas produced by
 * rio_device_decode of index.rio / data.rio, run on `stream` (NULL = ctx stream), no host sync.
 *
 * rio_sst_index_parse replaces SliceKeyIndexLoader.Load's per-record proto.Unmarshal into an
 * IndexEntry (slice_key_index.go:91-131, sstables/proto/sstable.proto:5-9). Record i of the index
 * arena (d_index_out[d_index_off[i] .. d_index_off[i+1])) -> key bytes at
 * d_index_out[d_key_off[i] .. + d_key_len[i]), valueOffset, checksum (absent fields = 0).
 * d_result[0] = first malformed record (proto error: the reference's Load fails there) or ~0.
 *
 * rio_sst_validate replaces validateDataFile (sstable_reader.go:205-238) and the
 * SSTableFullScanIterator's optional hash check (sstable_iterator.go:77-111): for every index entry,
 * the value is the data record whose file offset is valueOffset (getValueAtOffset, :85-92), its
 * CRC-64/ISO (checksumValue, :240-248) goes to d_crc_out[i]. d_result[0] = first entry whose
 * non-zero checksum mismatches (ChecksumError), d_result[1] = first entry not in the writer's
 * layout (valueOffset != data record i's offset: keep the reference reader); ~0 = none. An entry
 * outside the layout whose valueOffset is another data record's offset gets that record's CRC-64, and
 * its checksum is compared with it; one whose valueOffset is no data record's offset (every entry when
 * n_data == 0) gets d_crc_out[i] = 0 and no checksum comparison. */
int rio_sst_index_parse(rio_ctx* ctx, const uint8_t* d_index_out, const uint64_t* d_index_off, uint64_t n,
                        uint64_t* d_key_off, uint64_t* d_key_len, uint64_t* d_value_off, uint64_t* d_checksum,
                        uint64_t* d_result, void* stream);
int rio_sst_validate(rio_ctx* ctx, const uint8_t* d_data_out, const uint64_t* d_data_off,
                     const uint64_t* d_data_rec_off, uint64_t n_data, const uint64_t* d_value_off,
                     const uint64_t* d_checksum, uint64_t n_index, uint64_t* d_crc_out, uint64_t* d_result,
                     void* stream);
/* v0 tables (metadata version 0: values are protobuf DataEntry {value = 1}, sstable_reader.go:303-314,
 * sstables/proto/sstable.proto:12-14). rio_sst_data_entries replaces the proto.Unmarshal of every value
 * record (MMapProtoReader.ReadNextAt / ProtoReader.ReadNext, recordio/proto/mmap_proto_reader.go:12-24)
 * on the decoded data arena: d_view[2j], d_view[2j+1] = [begin, end) of record j's DataEntry.value in
 * d_data_out, both RIO_VALUE_NIL when the field is absent (value nil) and RIO_VALUE_BAD when the
 * record is not a valid DataEntry ("proto: cannot parse invalid wire-format data").
 * d_result[0] = first malformed record or ~0. rio_sst_validate_view is rio_sst_validate over those
 * ranges (a nil or malformed value hashes as empty). */
#define RIO_VALUE_NIL (~0ull)
#define RIO_VALUE_BAD (~0ull - 1)
int rio_sst_data_entries(rio_ctx* ctx, const uint8_t* d_data_out, const uint64_t* d_data_off, uint64_t n_data,
                         uint64_t* d_view, uint64_t* d_result, void* stream);
int rio_sst_validate_view(rio_ctx* ctx, const uint8_t* d_data_out, const uint64_t* d_data_off,
                          const uint64_t* d_data_rec_off, uint64_t n_data, const uint64_t* d_view,
                          const uint64_t* d_value_off, const uint64_t* d_checksum, uint64_t n_index,
                          uint64_t* d_crc_out, uint64_t* d_result, void* stream);

/* ---- sstables, host-memory API (the cgo binding: one call per table) ------------------------
 * rio_sst_open replaces NewSSTableReader's load (sstable_reader.go:250-345) for the tables the device
 * path handles: H2D of index.rio and data.rio, device decode of both, IndexEntry parse and the CRC-64
 * of every value on the device (the two calls above), D2H of what the iterator needs. The handle owns
 * host copies; pointers from rio_sst_entry stay valid until rio_sst_free.
 * Returns RIO_ERR_UNSUPPORTED (no handle, `info` filled) when either file is one the device path hands
 * back (none of recordio v1..v4 is; the code stays for the adapter's contract). Otherwise the
 * handle is returned and `info` says which of the reference's load errors applies: index/data status
 * outside the EOF family (reading error), first_bad_proto (proto.Unmarshal error, slice_key_index.go:
 * 107-110), first_unplaced (not the writer's layout: keep the reference reader), first_bad_crc
 * (validateDataFile's ChecksumError, sstable_reader.go:205-238, unless SkipHashCheckOnLoad), and
 * data.first_bad (a value that does not decompress: validateDataFile's ReadNextAt error). Of
 * first_bad_crc and data.first_bad the smaller entry is the one validateDataFile stops at; on a tie it
 * is the read error (a flagged value's CRC is not meaningful). */
typedef struct rio_sst_info {
    rio_file_info index;      /* ReadNext loop over index.rio */
    rio_file_info data;       /* ReadNext loop over data.rio */
    uint64_t n_entries;       /* index records = IndexEntries */
    uint64_t first_bad_proto; /* ~0 = none */
    uint64_t first_bad_crc;   /* ~0 = none */
    uint64_t first_unplaced;  /* ~0 = none */
    uint64_t index_bad;       /* first index record that does not decompress (RIO_FLAG_CORRUPT): Load's
                                 ReadNext error there, before any later index status; ~0 = none.
                                 n_entries stops at the first flagged index record (gzip's bare io.EOF
                                 ends the index cleanly, slice_key_index.go:117-126) */
    uint64_t first_bad_value; /* v0 tables: first data record that is not a valid DataEntry; ~0 = none */
} rio_sst_info;
typedef struct rio_sst rio_sst;
int rio_sst_open(rio_ctx* ctx, const uint8_t* index_file, uint64_t index_len, const uint8_t* data_file,
                 uint64_t data_len, rio_sst** out, rio_sst_info* info);
/* flags: RIO_SST_V0_VALUES for a table whose metadata version is 0 (no meta.pb.bin, or version 0):
 * values are DataEntry protos (rio_sst_data_entries), rio_sst_entry returns DataEntry.value and
 * RIO_ERR_PROTO for a malformed one; validateDataFile does not run for such tables (:205-209), so
 * first_bad_crc is left ~0 and crc still holds each value's CRC-64. */
#define RIO_SST_V0_VALUES 1u
int rio_sst_open_ex(rio_ctx* ctx, const uint8_t* index_file, uint64_t index_len, const uint8_t* data_file,
                    uint64_t data_len, uint32_t flags, rio_sst** out, rio_sst_info* info);
/* Entry i in index order (SSTableFullScanIterator.Next, sstable_iterator.go:77-111): key, the value of
 * data record i (is_nil for a nil record), the stored valueOffset and checksum and the value's CRC-64.
 * Returns RIO_OK, RIO_ERR_ARG for i >= n_entries, the data file's terminal status when data record i
 * does not exist (the scan's dataReader.ReadNext error; key and checksum are still filled), or
 * RIO_ERR_DECOMPRESS / RIO_EOF_CODEC when data record i is flagged RIO_FLAG_CORRUPT / RIO_FLAG_EOF. */
int rio_sst_entry(const rio_sst* t, uint64_t i, const uint8_t** key, uint64_t* key_len, const uint8_t** value,
                  uint64_t* value_len, int* is_nil, uint64_t* value_offset, uint64_t* checksum, uint64_t* crc);
void rio_sst_free(rio_sst* t);

/* ---- recordio v4 encoding on the device (the write side: FileWriter.Write for a batch) --------
 * Replaces a loop of FileWriter.Write (recordio/file_writer.go:189-233; compaction output,
 * sstable_merger.go:36-169): record i = d_records[d_rec_off[i] .. d_rec_off[i+1]) (RIO_DEVICE_PAD
 * readable bytes past the arena end), d_flags[i] & RIO_FLAG_NIL marks a nil record (d_flags NULL =
 * none), compression RIO_COMP_NONE or RIO_COMP_SNAPPY (golang/snappy v1.0.0 block encoding). The
 * whole v4 file (8-byte header + records) goes to d_out, byte-identical to the reference writer; record
 * i's file offset (what Write returns) to d_out_rec_off[i], the file length to *d_out_len. With
 * out_cap >= rio_encode_bound(n, total_bytes) the file always fits; otherwise nothing is written
 * when *d_out_len > out_cap. Stream-ordered, no host sync. total_bytes = d_rec_off[n]. */
uint64_t rio_encode_bound(uint64_t n_records, uint64_t total_bytes, uint32_t compression);
int rio_device_encode(rio_ctx* ctx, const uint8_t* d_records, const uint64_t* d_rec_off, const uint8_t* d_flags,
                      uint64_t n, uint64_t total_bytes, uint32_t compression, uint8_t* d_out, uint64_t out_cap,
                      uint64_t* d_out_rec_off, uint64_t* d_out_len, void* stream);
/* host-memory form (the cgo binding): H2D of the records, device encode, D2H of the file image and
 * offsets; *out_len = file length (RIO_ERR_CAPACITY when it exceeds out_cap). Synchronises. */
int rio_encode_file(rio_ctx* ctx, const uint8_t* records, const uint64_t* rec_off, const uint8_t* flags, uint64_t n,
                    uint32_t compression, uint8_t* out, uint64_t out_cap, uint64_t* out_rec_off, uint64_t* out_len);

/* ---- merge-compaction of loaded tables on the device (rio_compact.hip) -----------------------
 * Replaces SSTableMerger.Merge / MergeCompact / MergeCompactIterator (sstables/sstable_merger.go:36-169:
 * a priority queue over T scan iterators, one WriteNext per surviving key) with the reducers
 * ScanReduceLatestWins / ScanReduceLatestWinsSkipTombstones (super_sstable_reader.go:107-131, what
 * simpledb/compaction.go:119 runs for every compaction), and the IndexEntry side of
 * SSTableStreamWriter.WriteNext (sstable_writer.go:98-150). Everything works on the device arrays a
 * table load leaves behind (rio_device_decode of both files, rio_sst_index_parse, rio_sst_validate).
 * Table t of a call is views[t]; its position in the array is the reducer's context (the position
 * SuperSSTableReader.Scan assigns, super_sstable_reader.go:88-97): the highest position wins.
 * Limits: 1 <= T <= RIO_MERGE_MAX_TABLES, entries per table < 2^40, entries of all tables < 2^31
 * (RIO_ERR_UNSUPPORTED beyond). Bytes comparator only (skiplist.BytesComparator: lexicographic,
 * unsigned, a proper prefix first).
 *
 * The three calls are one sequence on one context: rio_sst_merge_plan copies the views to the
 * context and sizes the context's merge scratch (prefixes, scan inputs and outputs, scan temp: about
 * 40 bytes per input entry) for all three; rio_sst_merge_gather and rio_sst_index_encode work on the
 * last plan's views and allocate nothing. Outputs are caller buffers. All three are stream-ordered
 * (NULL = the ctx stream) and never wait for the stream (a plan waits only for the previous plan's copy
 * of its views, a host array, so the plan is not graph-capturable). The caller reads d_result (64 bytes) after the plan:
 * rio_device_encode takes its record count by value, so n_out must be known on the host; that copy
 * is the sequence's only host round trip before the output files are fetched. */
#define RIO_MERGE_MAX_TABLES 256u
#define RIO_MERGE_ENTRY_BITS 40u /* src = table << RIO_MERGE_ENTRY_BITS | entry */
#define RIO_MERGE_ALL 0u                          /* SSTableMerger.Merge: every entry, nil values too */
#define RIO_MERGE_LATEST_WINS 1u                  /* MergeCompact + ScanReduceLatestWins */
#define RIO_MERGE_LATEST_WINS_SKIP_TOMBSTONES 2u  /* MergeCompact + ScanReduceLatestWinsSkipTombstones */
typedef struct rio_sst_view {
    const uint8_t* index;      /* decoded index arena (rio_device_decode of index.rio) */
    const uint64_t* key_off;   /* [n] key i = index[key_off[i] .. + key_len[i]) (rio_sst_index_parse) */
    const uint64_t* key_len;   /* [n] */
    const uint8_t* data;       /* decoded data arena (rio_device_decode of data.rio) */
    const uint64_t* data_off;  /* [n + 1] value i = data[data_off[i] .. data_off[i + 1]) */
    const uint8_t* flags;      /* [n] RIO_FLAG_NIL marks a nil value */
    const uint64_t* crc;       /* [n] CRC-64/ISO of value i (rio_sst_validate's d_crc_out) */
    uint64_t n;                /* entries */
    uint64_t index_bytes;      /* length of the index arena: keys are clamped to it */
    uint64_t data_bytes;       /* length of the data arena: values are clamped to it */
} rio_sst_view;
/* d_result of rio_sst_merge_plan (uint64[RIO_MERGE_RESULT_WORDS]) */
#define RIO_MERGE_RESULT_WORDS 8u
#define RIO_MERGE_R_N_OUT 0u        /* surviving entries */
#define RIO_MERGE_R_VALUE_BYTES 1u  /* their value bytes */
#define RIO_MERGE_R_NULL_VALUES 2u  /* survivors with a nil value (MetaData.nullValues; RIO_MERGE_ALL only) */
#define RIO_MERGE_R_FIRST_DUP 3u    /* RIO_MERGE_ALL: first merged position whose key equals its predecessor's
                                       (WriteNext's "the same key cannot be written more than once"); ~0 = none */
#define RIO_MERGE_R_UNSORTED 4u     /* first table whose keys are not strictly ascending, or whose key / value
                                       ranges leave their arenas; ~0 = none. Nothing else of the plan is
                                       meaningful then (the caller returns RIO_ERR_UNSUPPORTED): merged
                                       positions can collide, so d_src and d_keep may be partly unwritten.
                                       rio_sst_flush_plan reuses the word for the first rejected OP */
#define RIO_MERGE_R_KEY_BYTES 5u    /* key bytes of the survivors (sizes rio_sst_index_encode's output) */
/* Plan: order all N = sum of views[t].n entries by (key, table position) and decide survival.
 *   d_src  [N] entry at merged position p = views[d_src[p] >> 40] entry (d_src[p] & (2^40 - 1))
 *   d_keep [N] 1 when position p survives the mode's reduce
 * Each table's order is checked, not trusted: every search and every later gather index is clamped
 * to its table and arena, so an unsorted or inconsistent input yields RIO_MERGE_R_UNSORTED, never an
 * out-of-range access. Returns RIO_ERR_ARG for NULL views / outputs, T = 0, T > RIO_MERGE_MAX_TABLES
 * or an unknown mode, before any device call. */
int rio_sst_merge_plan(rio_ctx* ctx, const rio_sst_view* views, uint32_t n_tables, uint32_t mode, uint64_t* d_src,
                       uint8_t* d_keep, uint64_t* d_result, void* stream);
/* Gather of the last plan's survivors (n_out = d_result[RIO_MERGE_R_N_OUT], read by the caller) into
 * the layout rio_device_encode takes:
 *   d_out_src   [n_out]      the survivors' d_src words in merged order
 *   d_values    [values_cap] values back to back; values_cap >= value bytes + RIO_DEVICE_PAD
 *   d_val_off   [n_out + 1]  value j = d_values[d_val_off[j] .. d_val_off[j + 1])
 *   d_val_flags [n_out]      RIO_FLAG_NIL for a nil value
 * A value that would pass values_cap is not copied. RIO_ERR_STATE without a plan on this context. */
int rio_sst_merge_gather(rio_ctx* ctx, const uint64_t* d_src, const uint8_t* d_keep, uint64_t n_out,
                         uint64_t* d_out_src, uint8_t* d_values, uint64_t values_cap, uint64_t* d_val_off,
                         uint8_t* d_val_flags, void* stream);
/* Index records of the output table: entry j = proto.Marshal(&IndexEntry{Key, ValueOffset, Checksum})
 * (sstable_writer.go:126-132; proto3: an empty key, offset 0 and checksum 0 are omitted, varints are
 * minimal) with the key and the CRC-64 of survivor d_out_src[j] (the value is not hashed again) and
 * ValueOffset = d_value_file_off[j], the record offsets rio_device_encode returned for the values.
 *   d_entries [entries_cap]  entries back to back; entries_cap >= rio_index_entries_bound(n_out, key bytes)
 *   d_ent_off [n_out + 1]
 * An entry that would pass entries_cap is not written. The arena and offsets then go to
 * rio_device_encode(RIO_COMP_NONE) for index.rio. */
int rio_sst_index_encode(rio_ctx* ctx, const uint64_t* d_out_src, const uint64_t* d_value_file_off, uint64_t n_out,
                         uint8_t* d_entries, uint64_t entries_cap, uint64_t* d_ent_off, void* stream);
/* host helpers: the marshalled length of one IndexEntry, and the arena bound for n of them */
uint64_t rio_index_entry_len(uint64_t key_len, uint64_t value_offset, uint64_t checksum);
uint64_t rio_index_entries_bound(uint64_t n, uint64_t key_bytes);

/* ---- memstore flush on the device (rio_flush.hip) ---------------------------------------------
 * Replaces MemStore.Flush / FlushWithTombstones (memstore/memstore.go:189-238: a walk over the skip
 * list, one WriteNext per key) for a memstore kept as an append-only log of operations in
 * application order. Op i = key keys[key_off[i] .. key_off[i + 1]) with value
 * values[val_off[i] .. val_off[i + 1]); flags[i] & RIO_FLAG_NIL marks a tombstone (Delete /
 * Tombstone: the value is nil, its range is not read). Op i is applied after op i - 1, so the last
 * op of a key is the key's state. The key arena has RIO_DEVICE_PAD readable bytes past key_bytes
 * (the contract of rio_device_encode's records). */
typedef struct rio_ops_view {
    const uint8_t* keys;       /* key arena */
    const uint64_t* key_off;   /* [n + 1] */
    const uint8_t* values;     /* value arena */
    const uint64_t* val_off;   /* [n + 1] */
    const uint8_t* flags;      /* [n] RIO_FLAG_NIL marks a tombstone */
    uint64_t n;                /* ops */
    uint64_t key_bytes;        /* length of the key arena: keys are clamped to it */
    uint64_t value_bytes;      /* length of the value arena: values are clamped to it */
} rio_ops_view;
/* Grow a device log by a batch's log. `log` is a view over arrays the caller owns, with the given capacities:
 * key_off and val_off hold ops_cap + 1 words, flags ops_cap bytes, keys keys_cap and values values_cap bytes.
 * The arrays ARE WRITTEN although the view's pointers are const. The call copies the batch's key bytes behind
 * log.key_bytes, its value bytes behind log.value_bytes and its flags behind log.n (device to device), and one
 * kernel (rio_memidx.hip) writes key_off[log.n + 1 + i] = log.key_bytes + min(batch.key_off[i + 1],
 * batch.key_bytes) for every batch op i, the same for val_off, and key_off[0] = val_off[0] = 0 for log.n = 0.
 * Afterwards the view with n = log.n + batch.n, key_bytes = log.key_bytes + batch.key_bytes and value_bytes =
 * log.value_bytes + batch.value_bytes over the same arrays is the log of the old ops followed by the batch's:
 * the caller computes it, nothing is read back.
 * Precondition: the batch is as this library's producers leave one, key_off[0] = val_off[0] = 0. Any other batch
 * gives offsets that stay inside the arenas and a log rio_mem_index_build / _extend accept or reject, never an
 * out-of-range access.
 * Stream-ordered (NULL = the ctx stream), never waits for the stream, allocates nothing. batch.n = 0 is a no-op.
 * Returns RIO_ERR_ARG for a NULL ctx / log / batch, batch.n > 0 with a NULL array on either side, log.n +
 * batch.n > ops_cap, or new key / value bytes + RIO_DEVICE_PAD above keys_cap / values_cap (the key arena keeps
 * its readable pad); RIO_ERR_UNSUPPORTED for 2^31 - 1 ops and more in all; before any device call. */
int rio_ops_append(rio_ctx* ctx, const rio_ops_view* log, uint64_t ops_cap, uint64_t keys_cap, uint64_t values_cap,
                   const rio_ops_view* batch, void* stream);
#define RIO_FLUSH_WITH_TOMBSTONES 0u /* FlushWithTombstones: latest op of every key, nil values too */
#define RIO_FLUSH_SKIP_TOMBSTONES 1u /* Flush: keys whose latest op is nil are left out */
#define RIO_FLUSH_MAX_KEY_LEN 1024u
/* Plan of a flush: order the n ops by (key, op index) with the bytes comparator (lexicographic,
 * unsigned, a proper prefix first) and keep the last op of every key; under
 * RIO_FLUSH_SKIP_TOMBSTONES a key whose last op is nil is dropped, an empty non-nil value is kept
 * (memstore.go:229).
 *   d_src  [n] op at sorted position p (table bits 0: the word rio_sst_merge_gather takes)
 *   d_keep [n] 1 when position p goes to the table
 *   d_result   the block of rio_sst_merge_plan: RIO_MERGE_R_N_OUT, _VALUE_BYTES, _NULL_VALUES and
 *              _KEY_BYTES as for a merge; RIO_MERGE_R_FIRST_DUP is always ~0; RIO_MERGE_R_UNSORTED
 *              holds the first OP (not table) whose key or value range is not monotone, leaves its
 *              arena, or whose key is longer than max_key_len; ~0 = none. Nothing else of the plan is
 *              meaningful then.
 * The plan registers ONE rio_sst_view on the context as the last plan (keys = the index arena, values
 * = the data arena, key lengths and the CRC-64 of every kept value in context scratch), so
 * rio_sst_merge_gather and rio_sst_index_encode follow it exactly as they follow rio_sst_merge_plan;
 * the op arrays must stay valid until those calls have run. The ordering is an LSD radix sort over
 * the key length and the ceil(max_key_len / 8) big-endian 8-byte chunks of the keys: max_key_len is
 * a bound on the key lengths, it sets the pass count (pass the longest key's length, 0 .. RIO_FLUSH_MAX_KEY_LEN).
 * Scratch (40 bytes per op, the sort's temp and the gather's 16 bytes per op) is sized here, nothing is allocated afterwards.
 * Stream-ordered (NULL = the ctx stream), never waits for the stream (only for the previous plan's
 * copy of its view, as rio_sst_merge_plan). Every index read back from a buffer is clamped: a wrong
 * input gives RIO_MERGE_R_UNSORTED or wrong bytes, never an out-of-range access.
 * Returns RIO_ERR_ARG for a NULL ctx / ops / d_result, an unknown mode or n > 0 with a NULL array,
 * RIO_ERR_UNSUPPORTED for n >= 2^31 - 1 or max_key_len > RIO_FLUSH_MAX_KEY_LEN, before any device call. */
int rio_sst_flush_plan(rio_ctx* ctx, const rio_ops_view* ops, uint32_t mode, uint32_t max_key_len, uint64_t* d_src,
                       uint8_t* d_keep, uint64_t* d_result, void* stream);
/* Stage milliseconds of the context's last flush plan, recorded while rio_ctx_set_timing is on: check,
 * the length pass, the chunk passes (last chunk first), keep, crc. Fills up to n entries and returns
 * the count (0 when timing is off or the log was empty). Waits for the plan's last stage. */
int rio_sst_flush_stage_ms(rio_ctx* ctx, float* ms, int n);

/* ---- WAL recovery on the device: WalMutation records to an op log (rio_walops.hip) -------------
 * Replaces the host loop of simpledb's replayAndSetupWriteAheadLog (simpledb/recovery.go:208-240):
 * proto.Unmarshal of every WAL record into a WalMutation (simpledb/proto/wal_mutation.pb.go), then
 * memStore.Upsert / Tombstone. Input: the decoded WAL files as rio_device_decode leaves them in HBM,
 * one rio_wal_segment per file in replay order; output: a rio_ops_view for rio_sst_flush_plan
 * (FlushWithTombstones, flush.go). Nothing is copied to the host but the plan's result block.
 *
 * Record rules (proto.Unmarshal into a reset message + the switch at recovery.go:224-237):
 * WalMutation is oneof { addition = 1 (UpsertMutation: 1 key string, 2 value string, 3 keyBytes,
 * 4 valueBytes); deleteTombStone = 2 (DeleteTombstoneMutation: 1 key string, 2 keyBytes) }, all wire
 * type 2. Fields in wire order; the member seen last is the oneof's; a member seen again while current
 * merges field by field (last occurrence wins), a switch to the other member starts it empty. A known
 * field with another wire type and unknown fields are skipped at both levels. Every occurrence of a
 * string field must be valid UTF-8 (Go's utf8.Valid). No member (a nil or empty record too): no op, the
 * record still counts. addition: (keyBytes, valueBytes) when keyBytes is non-empty, with an absent or
 * empty valueBytes refused as Upsert(key, nil); otherwise (key, value) as bytes, both may be empty.
 * deleteTombStone: a tombstone of keyBytes when non-empty, otherwise of key. */
typedef struct rio_wal_segment {      /* one decoded WAL file, in replay order */
    const uint8_t* out;               /* rio_device_decode's d_out; RIO_DEVICE_PAD readable bytes past out_bytes */
    const uint64_t* out_off;          /* [n + 1] */
    const uint8_t* flags;             /* [n]; RIO_FLAG_NIL = nil record (Unmarshal of nil: the empty mutation) */
    uint64_t n;                       /* records to replay (the caller has already cut at first_bad / its read error) */
    uint64_t out_bytes;               /* arena length: every range is clamped to it */
} rio_wal_segment;
#define RIO_WAL_MAX_SEGMENTS 4096u
/* d_result of rio_wal_ops_plan (uint64[RIO_WAL_RESULT_WORDS]) */
#define RIO_WAL_RESULT_WORDS 8u
#define RIO_WAL_R_N_RECORDS 0u    /* recovery.go's numRecords: every record, no-ops too */
#define RIO_WAL_R_N_OPS 1u        /* upserts + tombstones */
#define RIO_WAL_R_KEY_BYTES 2u    /* key arena length */
#define RIO_WAL_R_VALUE_BYTES 3u  /* value arena length */
#define RIO_WAL_R_MAX_KEY_LEN 4u  /* the longest key: what rio_sst_flush_plan takes as max_key_len */
#define RIO_WAL_R_FIRST_BAD 5u    /* first refused record, counted over all segments; ~0 = none. When set,
                                     nothing else in the block is meaningful: the reference fails recovery
                                     at that record and flushes nothing */
#define RIO_WAL_R_BAD_CLASS 6u    /* RIO_WAL_BAD_* of that record */
#define RIO_WAL_BAD_PROTO 1u      /* proto.Unmarshal fails: malformed wire data at either message level */
#define RIO_WAL_BAD_UTF8 2u       /* a proto3 string field (key / value) is not valid UTF-8 */
#define RIO_WAL_BAD_VALUE_NIL 3u  /* Upsert(key, nil): memstore.ValueNil (memstore.go:124) */
#define RIO_WAL_BAD_RANGE 4u      /* the segment's offsets are not monotone or leave its arena */
/* Plan: copy the segments to the context (as rio_sst_merge_plan copies its views: only the previous
 * plan's copy is waited for, so the plan is not graph-capturable), size the context's scratch for both
 * calls (68 bytes per record plus the scan's temp), parse every record (one lane per record over the
 * concatenation of the segments) and scan the op flags and the key and value lengths. The caller reads
 * d_result (64 bytes), the sequence's one host round trip, and sizes the gather's outputs from it. Of
 * several refused records the smallest index is reported. Every offset read from a buffer is clamped to
 * its arena: a wrong input gives RIO_WAL_BAD_RANGE or wrong bytes, never an out-of-range access.
 * Returns RIO_ERR_ARG for a NULL ctx / segs / d_result, n_segs = 0 or a segment with n > 0 and a NULL
 * array, RIO_ERR_UNSUPPORTED for n_segs > RIO_WAL_MAX_SEGMENTS or 2^31 - 1 records and more, before any
 * device call. Stream-ordered (NULL = the ctx stream). */
int rio_wal_ops_plan(rio_ctx* ctx, const rio_wal_segment* segs, uint32_t n_segs, uint64_t* d_result, void* stream);
/* Gather of the last plan's ops (n_ops = d_result[RIO_WAL_R_N_OPS]) into the arrays of a rio_ops_view:
 *   d_keys    [keys_cap]    keys back to back; keys_cap >= key bytes (+ RIO_DEVICE_PAD for the flush)
 *   d_key_off [n_ops + 1]
 *   d_values  [values_cap]  values back to back; a tombstone has none
 *   d_val_off [n_ops + 1]
 *   d_flags   [n_ops]       RIO_FLAG_NIL for a tombstone
 *   d_op_rec  [n_ops]       source record of each op, counted over all segments (may be NULL)
 * A key or value that would pass its cap is not copied. Allocates nothing; the segments' arrays must
 * still be valid. RIO_ERR_STATE without a plan on this context, RIO_ERR_ARG for a NULL ctx or output or
 * n_ops larger than the plan's record count. Stream-ordered (NULL = the ctx stream). */
int rio_wal_ops_gather(rio_ctx* ctx, uint64_t n_ops, uint8_t* d_keys, uint64_t keys_cap, uint64_t* d_key_off,
                       uint8_t* d_values, uint64_t values_cap, uint64_t* d_val_off, uint8_t* d_flags,
                       uint64_t* d_op_rec /* may be NULL: source record index of each op */, void* stream);

/* ---- batched writes: an op log to WalMutation records on the device (rio_walenc.hip) ------------
 * Replaces the per-mutation proto.Marshal of db.PutBytes / db.DeleteBytes (simpledb/db.go:256-347: the
 * WalMutation of db.go:258-265 / :312-318, marshalled, appended to the WAL, applied to the memstore) for a
 * batch kept as a rio_ops_view, the inverse of rio_wal_ops_plan / _gather. Record i is proto.Marshal's
 * output: deterministic field order, proto3 empty fields omitted, minimal varints, the oneof member always
 * present.
 *   upsert (flags[i] without RIO_FLAG_NIL): 0A varint(body), then 1A varint(klen) key when klen > 0 (keyBytes =
 *            3), then 22 varint(vlen) value when vlen > 0 (valueBytes = 4)
 *   delete (RIO_FLAG_NIL; the value range is not read): 12 varint(body), then 12 varint(klen) key when
 *            klen > 0 (keyBytes = 2)
 * so an empty-key upsert with an empty value is 0A 00 and an empty-key delete 12 00. The records go to
 * d_records back to back in the layout rio_device_encode takes (which frames them into a WAL file image,
 * byte-identical to FileWriter.Write):
 *   d_records [records_cap]  records_cap >= rio_wal_ops_encode_bound(n, key_bytes, value_bytes) always fits
 *                            (+ RIO_DEVICE_PAD readable bytes for rio_device_encode)
 *   d_rec_off [n + 1]        record i = d_records[d_rec_off[i] .. d_rec_off[i + 1])
 *   d_result                 uint64[RIO_WALENC_RESULT_WORDS]
 * A record whose end passes records_cap is not written; d_rec_off and d_result are complete either way.
 * Every key and value range is checked: not monotone or leaving its arena (key_bytes / value_bytes) gives
 * RIO_WALENC_R_FIRST_BAD = the smallest such op with class RIO_WAL_BAD_RANGE, nothing else is meaningful
 * then and no record byte is promised; nothing is read outside a clamped range, every store is checked
 * against records_cap. Stream-ordered (NULL = the ctx stream), no host wait; the view is passed by value
 * into the launches. Scratch (8 bytes per op and the scan's temp) is grow-only in the context: after one
 * call with n at least as large the call allocates nothing and can be captured in a graph.
 * Returns RIO_ERR_ARG for a NULL ctx / ops / d_rec_off / d_result, n > 0 with a NULL array or a NULL
 * d_records with records_cap > 0, RIO_ERR_UNSUPPORTED for n >= 2^31 - 1, before any device call. */
#define RIO_WALENC_RESULT_WORDS 8u
#define RIO_WALENC_R_N_RECORDS 0u    /* n */
#define RIO_WALENC_R_BYTES 1u        /* d_rec_off[n]: the record arena's length */
#define RIO_WALENC_R_N_UPSERTS 2u
#define RIO_WALENC_R_N_DELETES 3u
#define RIO_WALENC_R_MAX_KEY_LEN 4u  /* the longest key: what rio_sst_flush_plan takes as max_key_len */
#define RIO_WALENC_R_FIRST_BAD 5u    /* first refused OP; ~0 = none */
#define RIO_WALENC_R_BAD_CLASS 6u    /* RIO_WAL_BAD_RANGE */
/* n records of these arenas never need more: 33 = 3 tags + 3 ten-byte varints per record */
uint64_t rio_wal_ops_encode_bound(uint64_t n, uint64_t key_bytes, uint64_t value_bytes);
int rio_wal_ops_encode(rio_ctx* ctx, const rio_ops_view* ops, uint8_t* d_records, uint64_t records_cap,
                       uint64_t* d_rec_off, uint64_t* d_result, void* stream);

/* ---- bloom filters of tables, and point lookups of a loaded table (rio_bloom.hip) --------------
 * Replaces the writer's filter build (sstables/sstable_writer.go:78-83 NewOptimal, :114-118 one Add per
 * WriteNext, :150-154 WriteFile) and the reader's point lookups (sstable_reader.go:49-65 Contains: filter
 * first, then the index; :67-77 Get; slice_key_index.go:19-35 the search) with batched calls over keys that
 * are already in HBM. The filter is steakknife/bloomfilter's: m bits, k 64-bit hash keys; an element is the
 * FNV-1 64-bit hash h of the key (hash/fnv New64: basis 0xcbf29ce484222325, per byte h *= 0x100000001b3 then
 * h ^= byte); probe j is bit (h ^ hash_keys[j]) mod m, bit i being bit i & 63 of 64-bit word i >> 6. Add sets
 * all k bits, Contains needs all k. The file around the bits (gzip, header, SHA-384 trailer) is host work.
 *   bits       8 * ceil(m / 64) bytes of device memory, little-endian 64-bit words as the file holds them
 *   hash_keys  [k] device array
 * All calls are stream-ordered (NULL = the ctx stream), never synchronise with the host and allocate
 * nothing: they can be captured into a hipGraph. Every offset read from a buffer is clamped to its arena and
 * every entry index to its table: a wrong input gives wrong answers or ~0, never an out-of-range access.
 * RIO_ERR_ARG before any device call and before *ctx is read: a NULL ctx or filter, k = 0, k > RIO_BLOOM_MAX_K,
 * m < 2, and with n > 0 a NULL array (bits and hash_keys included). n = 0 is a no-op returning RIO_OK. */
#define RIO_BLOOM_MAX_K 64u
typedef struct rio_bloom_view {
    uint64_t* bits;
    const uint64_t* hash_keys;
    uint64_t m;
    uint32_t k;
} rio_bloom_view;
/* bloomfilter.NewOptimal's sizes (host): m = ceil(-max_n * ln p / ln^2 2), k = ceil(ln 2 * m / max_n);
 * (1000, 0.01) -> (9586, 7), the writer's defaults (sstable_writer.go:218-222). RIO_ERR_ARG for max_n = 0,
 * p outside (0, 1) or a NULL output. *k may exceed RIO_BLOOM_MAX_K for a tiny p: the device calls refuse it. */
int rio_bloom_optimal(uint64_t max_n, double p, uint64_t* m, uint64_t* k);
/* filter.Add(fnv64(key)) for key i = d_keys[d_key_off[i] .. d_key_off[i + 1]), i < n (sstable_writer.go:114-118).
 * ORs into the bits that are there: the caller zero-fills, several adds compose. key_bytes is the arena's
 * length; nothing past it is read. */
int rio_bloom_add(rio_ctx* ctx, const rio_bloom_view* f, const uint8_t* d_keys, const uint64_t* d_key_off, uint64_t n,
                  uint64_t key_bytes, void* stream);
/* The same for the keys of the last plan's survivors (rio_sst_merge_plan or rio_sst_flush_plan on this
 * context): d_out_src [n_out] as rio_sst_merge_gather leaves it, the keys found as rio_sst_index_encode finds
 * them. RIO_ERR_STATE without a plan (checked before the n_out = 0 no-op), RIO_ERR_ARG for n_out above the
 * plan's entry count. */
int rio_sst_bloom_add(rio_ctx* ctx, const rio_bloom_view* f, const uint64_t* d_out_src, uint64_t n_out, void* stream);
/* filter.Contains(fnv64(key)) per key (sstable_reader.go:51-60): d_hit[i] = 1 when all k bits are set, else 0. */
int rio_bloom_contains(rio_ctx* ctx, const rio_bloom_view* f, const uint8_t* d_keys, const uint64_t* d_key_off,
                       uint64_t n, uint64_t key_bytes, uint8_t* d_hit, void* stream);
/* First 8 key bytes of every entry of a loaded table, big-endian and zero-padded, into the caller's
 * d_pfx[view->n]: what rio_sst_lookup probes. A reader builds it once per table (the merge plan's own
 * prefixes live in plan scratch and do not survive the plan). */
int rio_sst_key_prefixes(rio_ctx* ctx, const rio_sst_view* view, uint64_t* d_pfx, void* stream);
/* SliceKeyIndex.Get / Contains per query key (slice_key_index.go:19-35: sort.Search, then the equality test)
 * over the table's resident keys: d_entry[i] = index of the entry whose key equals query i, or ~0. With a
 * filter (sstable_reader.go:49-65), a query the filter rejects stores ~0 without touching the index; NULL =
 * no gate (Get does not consult the filter, :67-77). Of the view only index, key_off, key_len, n and
 * index_bytes are read. The keys are taken to be strictly ascending (the writer's order; the merge plan checks it, this call does not:
 * on an unsorted table the answers are wrong, the accesses stay in range). */
int rio_sst_lookup(rio_ctx* ctx, const rio_sst_view* view, const uint64_t* d_pfx, const rio_bloom_view* f,
                   const uint8_t* d_keys, const uint64_t* d_key_off, uint64_t n, uint64_t key_bytes, uint64_t* d_entry,
                   void* stream);

/* ---- a stack of loaded tables: SuperSSTableReader on the device (rio_stack.hip) ----------------
 * Replaces SuperSSTableReader.Contains / Get (sstables/super_sstable_reader.go:18-49: the readers from newest
 * to oldest, the first table that holds the key answers) for a batch of query keys, and gives the cut points of
 * ScanStartingAt / ScanRange (slice_key_index.go:49-70) for every table of the stack; the scans themselves are
 * rio_sst_merge_plan(RIO_MERGE_LATEST_WINS) over the cut views, rio_sst_merge_gather and rio_sst_keys_gather.
 * Table t of a stack is views[t]; position is age, the highest is the newest, as for rio_sst_merge_plan.
 *
 * rio_sst_stack_create copies the views, the prefix pointers (rio_sst_key_prefixes of every table), the filters
 * (bits == NULL: that table has no filter; filters == NULL: no table has one) and the stored-checksum pointers
 * (the index entries' Checksum arrays, rio_sst_index_parse's d_checksum; an entry or the array may be NULL) to
 * device memory the stack owns, and sizes all scratch for batches of up to max_batch queries (8 bytes per
 * query and the scan's temp). It waits for that one copy. After create no stack call allocates, synchronises
 * with the host or reads a host array: every stack call can be captured into a hipGraph. The tables' arrays
 * must stay valid while the stack is used. Stack calls are stream-ordered (NULL = the stream of the context
 * the stack was created on).
 * RIO_ERR_ARG before any device call and before *ctx is read: a NULL ctx / views / d_pfx / out, T = 0,
 * T > RIO_MERGE_MAX_TABLES, max_batch = 0, a table with n > 0 and a NULL array or prefix pointer, a filter
 * (bits != NULL) with k = 0, k > RIO_BLOOM_MAX_K, m < 2 or NULL hash keys. RIO_ERR_UNSUPPORTED for a table of
 * 2^40 entries and more or max_batch >= 2^31 - 1.
 * Every table and entry number read back from a buffer is clamped to what exists, every range to its arena,
 * every store is checked against its capacity: a wrong d_src gives ~0, RIO_GET_NOT_FOUND or wrong bytes, never
 * an out-of-range access. */
typedef struct rio_sst_stack rio_sst_stack;
#define RIO_GET_VALUE 0u     /* the value's bytes are at d_val_off[i] (an empty value has length 0) */
#define RIO_GET_NOT_FOUND 1u /* no table holds the key (d_src[i] = ~0, or a word that names no entry) */
#define RIO_GET_NIL 2u       /* the newest entry's record is nil: Get returns nil without an error and does not
                                fall through to an older table */
#define RIO_GET_HOST 3u      /* the host produces the reader's error: the data record does not decompress
                                (RIO_FLAG_CORRUPT / RIO_FLAG_EOF), or the value fails its stored checksum */
int rio_sst_stack_create(rio_ctx* ctx, const rio_sst_view* views, const uint64_t* const* d_pfx,
                         const rio_bloom_view* filters, const uint64_t* const* d_stored_checksum, uint32_t n_tables,
                         uint64_t max_batch, rio_sst_stack** out, void* stream);
void rio_sst_stack_free(rio_sst_stack* stack); /* NULL is accepted */
/* d_src[i] = table << RIO_MERGE_ENTRY_BITS | entry of the newest table whose keys contain query i =
 * d_keys[d_key_off[i] .. d_key_off[i + 1]), or ~0. gated = 1 is Contains: a table whose filter rejects the key
 * is skipped without touching its index (sstable_reader.go:49-65), tables without a filter are searched.
 * gated = 0 is Get, which never asks a filter (:67-77). key_bytes is the arena's length; nothing past it is
 * read. n > max_batch is RIO_ERR_ARG, n = 0 a no-op. */
int rio_sst_stack_lookup(rio_sst_stack* stack, uint32_t gated, const uint8_t* d_keys, const uint64_t* d_key_off,
                         uint64_t n, uint64_t key_bytes, uint64_t* d_src, void* stream);
/* Per query a status byte (RIO_GET_*) and d_val_off[n + 1], the exclusive scan of the value lengths
 * (RIO_GET_VALUE: the value's length; the others 0). The host reads d_val_off[n] to size the value arena: the
 * sequence's one round trip. check_crc != 0 is EnableHashCheckOnReads: RIO_GET_HOST when the table has stored
 * checksums, the entry's is not 0 and differs from the view's crc (sstable_reader.go:99-114). */
int rio_sst_stack_value_plan(rio_sst_stack* stack, const uint64_t* d_src, uint64_t n, uint32_t check_crc,
                             uint8_t* d_status, uint64_t* d_val_off, void* stream);
/* The values back to back in query order: value i to d_values[d_val_off[i] .. d_val_off[i + 1]). A value that
 * would pass values_cap is not copied. */
int rio_sst_stack_value_copy(rio_sst_stack* stack, const uint64_t* d_src, uint64_t n, const uint64_t* d_val_off,
                             uint8_t* d_values, uint64_t values_cap, void* stream);
/* d_pos[k * T + t] = lower bound (upper = 0: entries of table t before the first key >= key k) or upper bound
 * (upper = 1: entries up to the last key <= key k) of key k in table t: where IteratorStartingAt starts and
 * IteratorBetween starts and ends (both ends inclusive). */
int rio_sst_stack_bounds(rio_sst_stack* stack, const uint8_t* d_keys, const uint64_t* d_key_off, uint64_t n_keys,
                         uint64_t key_bytes, uint32_t upper, uint64_t* d_pos, void* stream);
/* The keys of the last plan's survivors (rio_sst_merge_plan or rio_sst_flush_plan on this context), laid out as
 * rio_sst_merge_gather lays out their values: d_key_off[n_out + 1] is the scan of the key lengths, key j =
 * d_keys[d_key_off[j] .. d_key_off[j + 1]). A key that would pass keys_cap is not copied (the plan's
 * RIO_MERGE_R_KEY_BYTES sizes it). RIO_ERR_STATE without a plan, RIO_ERR_ARG for n_out above the plan's entry
 * count. Allocates nothing. */
int rio_sst_keys_gather(rio_ctx* ctx, const uint64_t* d_out_src, uint64_t n_out, uint8_t* d_keys, uint64_t keys_cap,
                        uint64_t* d_key_off, void* stream);

/* ---- batched GetBytes: memstores over the table stack (rio_memidx.hip, rio_db.hip) -------------
 * Replaces a loop of DB.GetBytes (simpledb/db.go:197-242) over a batch of keys: the table stack's Get
 * (currentSSTable().Get, :212), then the memstore pair's Get (RWMemstore.Get, simpledb/rw_memstore.go:22-36:
 * the write store, and only on its KeyNotFound the read store, the one being flushed), combined by the rules
 * of :213-241. A memstore is the op log of rio_ops_view as it lies in device memory; rio_mem_index_build
 * makes it searchable in place, without copying a key or a value.
 *
 * An index is 16 bytes per distinct key: d_order[j] = the op index of the latest op of the j-th distinct key
 * in bytes.Compare order (nil ops included: the state FlushWithTombstones would write, memstore.go:189-238),
 * d_pfx[j] = that key's first 8 bytes as a big-endian word, zero-padded (the probe word of rio_sst_key_prefixes).
 * Only the first n_keys entries of both are meaningful; n_keys is the RIO_MERGE_R_N_OUT word of d_result, the
 * block of rio_sst_flush_plan, which stays in DEVICE memory: the lookups read n_keys there and clamp it to
 * ops.n, so no host read stands between a build and a lookup, and a lookup captured into a hipGraph sees the
 * index of a later build into the same buffers. RIO_MERGE_R_UNSORTED holds the first rejected op as for the
 * flush plan (a range that leaves its arena, a key longer than max_key_len); such a log leaves n_keys = 0.
 * The build runs the flush plan's sort and keep stages under RIO_FLUSH_WITH_TOMBSTONES (not its checksums), one
 * stream compaction of the kept positions and one kernel for the prefixes. It is a plan call: it REPLACES the
 * context's last plan and leaves none (rio_sst_merge_gather / rio_sst_keys_gather / rio_sst_index_encode return
 * RIO_ERR_STATE until the next rio_sst_merge_plan / rio_sst_flush_plan); rio_sst_flush_stage_ms reports its
 * stages. Scratch (the plan's, 9 bytes per op and the compaction's temp) is sized in the call, nothing is
 * allocated afterwards. Stream-ordered (NULL = the ctx stream), never waits for the stream. The index costs one
 * sort of the whole log; a log that has grown is extended from its old index by rio_mem_index_extend.
 * Returns RIO_ERR_ARG for a NULL ctx / ops / d_result or n > 0 with a NULL array, RIO_ERR_UNSUPPORTED for
 * n >= 2^31 - 1 or max_key_len > RIO_FLUSH_MAX_KEY_LEN, before any device call. */
#define RIO_DB_MAX_MEMSTORES 2u
typedef struct rio_mem_index {
    rio_ops_view ops;        /* the log the index points into; ops.n bounds every op index read back */
    const uint64_t* order;   /* [ops.n] rio_mem_index_build's d_order */
    const uint64_t* pfx;     /* [ops.n] its d_pfx */
    const uint64_t* result;  /* its d_result (device memory) */
} rio_mem_index;
int rio_mem_index_build(rio_ctx* ctx, const rio_ops_view* ops, uint32_t max_key_len, uint64_t* d_order, uint64_t* d_pfx,
                        uint64_t* d_result, void* stream);
/* The index of a log that has grown, from the index of its first n_old ops. Precondition: d_order, d_pfx and
 * d_result hold the index of ops [0, n_old) of this same log, from rio_mem_index_build or an earlier
 * rio_mem_index_extend, and d_order / d_pfx have room for ops.n words. max_key_len bounds the keys of the new ops
 * [n_old, ops.n) and sets their sort's pass count. Afterwards the three buffers hold what
 * rio_mem_index_build(ctx, ops, L, ...) leaves for any L that bounds every key of the log: d_order[0 .. n_keys)
 * and d_pfx[0 .. n_keys) word for word, and every word of d_result, in the same buffers. n_keys stays in device
 * memory: nothing is read back, the call never waits for the stream.
 * The new ops go through the build's stages as a log of their own (sort, keep, compaction, prefixes: cost of a
 * build over the tail alone); each of their distinct keys is then ranked in the old index by binary search, one
 * scan counts the old keys the tail rewrote, and old and new entries move to their merged places (16 bytes per op
 * of scratch) and back. The old ops are not sorted again.
 * Rejection follows the build's rule, the first rejected op of the whole log: an old index that was rejected
 * stays rejected with its op; a rejected new op j (a range that leaves its arena or is not monotone, a key longer
 * than max_key_len) gives RIO_MERGE_R_UNSORTED = n_old + j and n_keys = 0, and nothing else of the index is
 * meaningful. A rejection is sticky: after it only rio_mem_index_build over the whole log helps.
 * n_old = ops.n leaves the index as it is; n_old = 0 is the build. A plan call like the build: it replaces the
 * context's last plan and leaves none. Scratch is sized in the call from ops.n and the tail's length. Every
 * index read back from a buffer is clamped (the old n_keys to n_old, the tail's to its length, an op to the log,
 * a position to [0, ops.n)): a wrong input gives a wrong index, never an out-of-range access. A lookup captured
 * into a hipGraph carries its ops.n by value and clamps n_keys to it: capture the buffers' capacity, as for a
 * rebuild in place.
 * Returns RIO_ERR_ARG for n_old > ops.n and what the build refuses, RIO_ERR_UNSUPPORTED as the build, before any
 * device call. */
int rio_mem_index_extend(rio_ctx* ctx, const rio_ops_view* ops, uint64_t n_old, uint32_t max_key_len, uint64_t* d_order,
                         uint64_t* d_pfx, uint64_t* d_result, void* stream);
/* d_mem_src[i] = store << RIO_MERGE_ENTRY_BITS | op of the newest store of idx[0 .. n_idx) that holds query i =
 * d_keys[d_key_off[i] .. d_key_off[i + 1]), or ~0. Position is age, the highest is the newest (the write store
 * after the read store), as for tables. The first store that holds the key answers, also when its op is nil:
 * a tombstone in the write store ends the search (rw_memstore.go:25-33 returns KeyTombstoned without asking the
 * read store). The indexes travel by value in the kernel's arguments: nothing is copied to the device, the call
 * can be captured into a hipGraph. key_bytes is the query arena's length; nothing past it is read. Every index
 * read back from a buffer is clamped (n_keys to ops.n, an op to [0, ops.n), ranges to their arenas): a wrong
 * input gives ~0 or a wrong op, never an out-of-range access.
 * RIO_ERR_ARG before any device call: a NULL ctx / idx, n_idx = 0 or above RIO_DB_MAX_MEMSTORES, an index with
 * a NULL result block or with ops.n > 0 and a NULL array, n > 0 with a NULL array; RIO_ERR_UNSUPPORTED for
 * n >= 2^31 - 1 or an index of 2^40 ops and more. n = 0 is a no-op. */
int rio_mem_lookup(rio_ctx* ctx, const rio_mem_index* idx, uint32_t n_idx, const uint8_t* d_keys,
                   const uint64_t* d_key_off, uint64_t n, uint64_t key_bytes, uint64_t* d_mem_src, void* stream);
/* The write store's size estimate after every op of a batch, and the op at which a loop of db.PutBytes /
 * db.DeleteBytes would rotate (simpledb/db.go:299: EstimatedSizeInBytes() > memstoreMaxSize after every put, no
 * check after a delete, db.go:311-347). store = the write store's index as rio_mem_lookup takes it (NULL or
 * ops.n = 0: an empty store), size0 = its raw estimatedSize (memstore.go:32, before the 1.15 scaling), batch = a
 * batch as WriteBatch.upload leaves it (offsets from 0). d_size[i] (batch->n words) = the raw estimatedSize after
 * op i: what a loop of RWMemstore.Upsert / RWMemstore.Delete over ops 0 .. i leaves (memstore.go:119-178,
 * rw_memstore.go:48-63) when the write store started in store's state with size0; arithmetic mod 2^64 as Go's
 * uint64. d_result is a block of RIO_SIZE_RESULT_WORDS words in DEVICE memory:
 *   RIO_SIZE_R_CUT        the first op i that is a put (not nil) with uint64(1.15 * float32(d_size[i])) > max_size,
 *                         or ~0. The expression is Go's (memstore.go:182): the u64 -> f32 conversion rounds to
 *                         nearest, one float32 multiply by float32(1.15), truncation; a product of 2^64 and more
 *                         counts as 2^64 - 1
 *   RIO_SIZE_R_SIZE       d_size[CUT]; d_size[n - 1] without a cut; size0 for n = 0
 *   RIO_SIZE_R_KEY_END    key_off[CUT + 1] (key_off[n] without a cut, 0 for n = 0): where the batch's key arena splits
 *   RIO_SIZE_R_VALUE_END  val_off[CUT + 1], the same for the value arena
 *   RIO_SIZE_R_FIRST_BAD  the first batch op the flush plan's check rejects (a range that leaves its arena or is
 *                         not monotone, a key longer than max_key_len), or ~0; 0 for a store index that was
 *                         rejected (its RIO_MERGE_R_UNSORTED set). Nothing else in the block or in d_size is
 *                         meaningful then
 * The batch goes through the flush plan's check, sort and keep stages under RIO_FLUSH_WITH_TOMBSTONES; an op's
 * predecessor is its neighbour in that order or, for the first op of a key, the store's entry found by
 * rio_mem_lookup's binary search; one inclusive sum gives the sizes, one pass the cut. It is a plan call like
 * rio_mem_index_build: it REPLACES the context's last plan and leaves none. Scratch (the plan's, 17 bytes per op,
 * the scan's temp) is sized in the call from the context's arenas. Stream-ordered (NULL = the ctx stream), never
 * waits for the stream. Every index read back from a buffer is clamped (an op to its log, n_keys to the store's
 * ops.n, ranges to their arenas): a wrong input gives wrong words, never an out-of-range access.
 * Returns RIO_ERR_ARG for a NULL ctx / batch / d_result, n > 0 with a NULL array or a NULL d_size, a store refused
 * as by rio_mem_lookup; RIO_ERR_UNSUPPORTED for n >= 2^31 - 1 or max_key_len > RIO_FLUSH_MAX_KEY_LEN, before any
 * device call. n = 0 writes the result block only. */
#define RIO_SIZE_RESULT_WORDS 8u
#define RIO_SIZE_R_CUT 0u
#define RIO_SIZE_R_SIZE 1u
#define RIO_SIZE_R_KEY_END 2u
#define RIO_SIZE_R_VALUE_END 3u
#define RIO_SIZE_R_FIRST_BAD 4u
int rio_mem_size_scan(rio_ctx* ctx, const rio_mem_index* store, uint64_t size0, const rio_ops_view* batch,
                      uint32_t max_key_len, uint64_t max_size, uint64_t* d_size, uint64_t* d_result, void* stream);
/* The combined read. A reader owns the scan's scratch for batches of up to max_batch queries (8 bytes per query
 * and the scan's temp); stack = NULL is a database without tables yet. The stack must outlive the reader. After
 * create no reader call allocates, waits for the device or reads a host array.
 * RIO_ERR_ARG for a NULL ctx / out or max_batch = 0, RIO_ERR_UNSUPPORTED for max_batch >= 2^31 - 1, before any
 * device call. */
typedef struct rio_db_reader rio_db_reader;
#define RIO_GET_MEM_VALUE 4u /* rio_db_value_plan: a memstore's value answers (an empty one too: length 0) */
int rio_db_reader_create(rio_ctx* ctx, rio_sst_stack* stack, uint64_t max_batch, rio_db_reader** out);
void rio_db_reader_free(rio_db_reader* reader); /* NULL is accepted */
/* Per query a status byte and d_val_off[n + 1], the exclusive scan of the value lengths, from d_tab_src =
 * rio_sst_stack_lookup(gated = 0)'s words (NULL without a stack: no table holds any key) and d_mem_src =
 * rio_mem_lookup's over the same idx. The table's own status is rio_sst_stack_value_plan's (check_crc as there).
 * db.go:197-242, the first rule that matches:
 *   1. the table status is RIO_GET_HOST: RIO_GET_HOST. The reference returns the table's error before it asks
 *      the memstore (:212-218), so also when a memstore holds the key
 *   2. a memstore holds the key with a non-nil op: RIO_GET_MEM_VALUE with the op's value length, 0 included
 *      (:240-241 returns the memstore's empty value without an error)
 *   3. a memstore holds the key with a nil op: RIO_GET_NOT_FOUND whatever the tables hold (:231-234)
 *   4. the table status is RIO_GET_VALUE with length > 0: RIO_GET_VALUE (:228-229)
 *   5. RIO_GET_NOT_FOUND: the table statuses NOT_FOUND and NIL, and VALUE of length 0 (:214-221, :226-227)
 * RIO_ERR_ARG: a NULL reader / idx / d_val_off, n_idx = 0 or above RIO_DB_MAX_MEMSTORES, an index refused as by
 * rio_mem_lookup, n > 0 with a NULL d_mem_src / d_status, d_tab_src given to a reader without a stack,
 * n > max_batch. */
int rio_db_value_plan(rio_db_reader* reader, const rio_mem_index* idx, uint32_t n_idx, const uint64_t* d_tab_src,
                      const uint64_t* d_mem_src, uint64_t n, uint32_t check_crc, uint8_t* d_status, uint64_t* d_val_off,
                      void* stream);
/* The values back to back in query order: value i to d_values[d_val_off[i] .. d_val_off[i + 1]), from the op
 * log's value arena (RIO_GET_MEM_VALUE) or the table's data arena (RIO_GET_VALUE). A value that would pass
 * values_cap is not copied. Arguments as for rio_db_value_plan, with its d_status and d_val_off. */
int rio_db_value_copy(rio_db_reader* reader, const rio_mem_index* idx, uint32_t n_idx, const uint64_t* d_tab_src,
                      const uint64_t* d_mem_src, const uint8_t* d_status, uint64_t n, const uint64_t* d_val_off,
                      uint8_t* d_values, uint64_t values_cap, void* stream);

/* ---- DiskKeyIndex lookups (sstables/disk_key_index.go:87-140) --------------------------------
 * Batched DiskKeyIndex.Get / Contains / IteratorStartingAt: one result per query key, each the
 * reference's binarySearch over the byte offsets of an uncompressed index.rio with every probe
 * findAt(h) = SeekNext(h) + proto.Unmarshal(IndexEntry), exactly as a freshly loaded DiskKeyIndex
 * runs it (the reference's offsetCache is per index and may keep an empty entry at an offset whose
 * probe hit io.EOF; later lookups on the same Go object then see that entry: see DESIGN.md §8).
 *   status  RIO_OK (no error; `found` tells Get / Contains), else findAt's error: SeekNext's
 *           non-EOF error (e.g. RIO_ERR_UNEXPECTED_EOF) or RIO_ERR_PROTO. RIO_ERR_UNSUPPORTED for a
 *           v1 index (SeekNext's "unsupported on files with version lower than v2", mmap_reader.go:62-64),
 *           and from rio_device_index_search for a compressed one (keep the reference index); the
 *           rio_index handle answers compressed indexes from their decoded view.
 *   offset  binarySearch's offset (IteratorStartingAt starts there; size when an io.EOF probe ended it)
 *   value_offset / checksum  IndexVal when found. */
typedef struct rio_index_hit {
    uint64_t offset;
    uint64_t value_offset;
    uint64_t checksum;
    int32_t status;
    int32_t found;
} rio_index_hit;
/* device-resident: d_file (RIO_DEVICE_PAD readable bytes past len), query i = d_keys[d_key_off[i] ..
 * d_key_off[i+1]), results to d_hits[n]; seek_len 0 = 4096 (mmap_reader.go:370); no host sync */
int rio_device_index_search(rio_ctx* ctx, const uint8_t* d_file, uint64_t len, uint64_t seek_len,
                            const uint8_t* d_keys, const uint64_t* d_key_off, uint64_t n, rio_index_hit* d_hits,
                            void* stream);
/* host-memory handle (the cgo DiskIndexLoader.Load / Get binding): the index file stays resident in
 * HBM; each search copies the keys in and the hits out (synchronises). A compressed index.rio is
 * decoded once at open (records + the SeekNext map over the file) and searched from that view
 * (disk_key_index.go:173 reads it through an MMapReader, which decompresses every record). */
typedef struct rio_index rio_index;
int rio_index_open(rio_ctx* ctx, const uint8_t* file, uint64_t len, rio_index** out);
int rio_index_search(rio_index* idx, const uint8_t* keys, const uint64_t* key_off, uint64_t n, rio_index_hit* hits);
void rio_index_free(rio_index* idx);

/* ---- ordered replay of a file list (the WAL replay adapter) ----------------------------------
 * Replaces the per-file loop of wal.Replayer.Replay (wal/replayer.go:18-77; the caller walks the
 * directory and sorts the *.wal paths as :20-37 does). A worker thread with its own context maps and
 * decodes file k+1.. on `device` while the caller consumes file k; at most `depth` (0 = 2) decoded
 * files are held ahead. `workers` (0 = 2, at most depth) threads each own a context and stream, so
 * one file's H2D overlaps another's decode and D2H. rio_replay_next hands out the files strictly in list order: it returns
 * RIO_EOF after the last one; otherwise that file's rc (RIO_OK, RIO_ERR_IO when it cannot be opened or
 * mapped, RIO_ERR_HIP) with `info` and the arrays of rio_decode (out / out_off[n+1] / flags[n]), valid
 * until the next rio_replay_next or rio_replay_free. Deliver records < info.n_records, then map
 * info.status like FileReader.ReadNext's terminal error; when info.n_bad, stop at record
 * info.first_bad instead: RIO_FLAG_EOF ends this file (replayer.go:60-63), RIO_FLAG_CORRUPT ends the
 * replay with the codec error (:65-67). A file with info.status RIO_ERR_UNSUPPORTED
 * must be re-read whole by the reference reader before any of its records is delivered. */
typedef struct rio_replay rio_replay;
int rio_replay_open(int device, const char* const* paths, uint64_t n_paths, uint32_t depth, uint32_t workers,
                    rio_replay** out);
/* The same over several GPUs of one node (one host thread + context per GPU, no
 * communication): workers_per_device workers per device, worker w on devices[w % n_devices], file i
 * to worker i % W; files are still handed out strictly in list order. A device may be listed twice
 * (two workers' contexts on one GPU). depth (0 = 2) is raised to the worker count
 * workers_per_device * n_devices (0 = 2 per device), so every worker has a file in flight. */
int rio_replay_open_devices(const int* devices, uint32_t n_devices, const char* const* paths, uint64_t n_paths,
                            uint32_t depth, uint32_t workers_per_device, rio_replay** out);
int rio_replay_next(rio_replay* r, uint64_t* index, const uint8_t** out, const uint64_t** out_off,
                    const uint8_t** flags, rio_file_info* info);
void rio_replay_free(rio_replay* r);

/* ---- windowed sequential decode of one file (FileReader.ReadNext, file_reader.go:61-131, over a
 * file larger than the staging it should take: SURVEY §8b "one cgo call per window") -----------
 * The file is framed and decoded in windows of about `window_bytes` (0 = 128 MiB; a record larger
 * than a window doubles it) cut at record boundaries: one window's H2D overlaps the previous one's
 * decode and D2H on a second context. At most `depth` (0 = 4) decoded windows are held ahead.
 * rio_stream_next hands out the windows in file order: rc RIO_OK (or RIO_ERR_IO / RIO_ERR_HIP)
 * with the window's records — out / out_off[n+1] (window-relative) / rec_off[n] (file offsets of
 * the record headers) / flags[n], valid until the next rio_stream_next or rio_stream_free — and
 * `first_record`, the file-wide index of its first record. info.status is RIO_OK while more windows
 * follow; the last window carries the file's terminal status as the whole-file rio_frame /
 * rio_decode pair reports it (status_offset a file offset; the failing record's index is
 * first_record + info.n_records). info.first_bad / n_bad cover the window's flagged records
 * (first_bad a file-wide index). RIO_EOF after the last window. RIO_ERR_UNSUPPORTED: the adapter
 * continues with the reference reader after SkipNext over the records already delivered.
 * rio_stream_open_host reads from host memory instead of a path (the caller keeps it alive until
 * rio_stream_free). */
/* ---- a file set over several GPUs (independent files sharded over the GPUs of a node,
 * the 8 tables of an SSTable set, a WAL directory decoded without ordering): rio_fileset_decode
 * assigns the files to `devices` longest-processing-time first on their sizes, runs one host thread
 * with a pooled context per device (read, H2D, device decode, D2H into page-locked blocks) and
 * returns when every file is decoded. rio_fileset_get: file i's arrays (layout as rio_replay_next,
 * plus rec_off[n]), its info, the device that decoded it; rc RIO_OK or the file's RIO_ERR_IO /
 * RIO_ERR_HIP. Valid until rio_fileset_free. A device may be listed twice. */
typedef struct rio_fileset rio_fileset;
int rio_fileset_decode(const int* devices, uint32_t n_devices, const char* const* paths, uint64_t n_paths,
                       rio_fileset** out);
int rio_fileset_get(const rio_fileset* s, uint64_t i, const uint8_t** out, const uint64_t** out_off,
                    const uint64_t** rec_off, const uint8_t** flags, rio_file_info* info, int* device);
void rio_fileset_free(rio_fileset* s);

typedef struct rio_stream rio_stream;
int rio_stream_open(int device, const char* path, uint64_t window_bytes, uint32_t depth, rio_stream** out);
int rio_stream_open_host(int device, const uint8_t* data, uint64_t len, uint64_t window_bytes, uint32_t depth,
                         rio_stream** out);
int rio_stream_next(rio_stream* s, uint64_t* first_record, const uint8_t** out, const uint64_t** out_off,
                    const uint64_t** rec_off, const uint8_t** flags, rio_file_info* info);
void rio_stream_free(rio_stream* s);

/* ---- single-record decode at an arbitrary offset (MMapReader.ReadNextAt semantics) on the
 * device; `d_file` device-resident. The decoded record is written to `d_out` (capacity out_cap);
 * *len_out / *nil_out / status go to host memory (this call synchronises). */
int rio_device_read_at(rio_ctx* ctx, const uint8_t* d_file, uint64_t len, uint64_t offset,
                       uint8_t* d_out, uint64_t out_cap, uint64_t* len_out, int* nil_out,
                       uint64_t* detail0, uint64_t* detail1);

/* ---- batched ReadNextAt on the device: n offsets of one device-resident file in one plan / copy pair, the
 * shape of rio_sst_stack_value_plan / _copy. Both calls are stream-ordered (a NULL stream is the context's own)
 * and do no host synchronisation; `d_file` is 16-byte aligned with RIO_DEVICE_PAD readable bytes past `len`.
 * Any offset value is legal, in any order, with duplicates. Per query the hit is what MMapReader.ReadNextAt
 * (mmap_reader.go:130-203) gives at that offset:
 *   status   RIO_OK, or the call's error class (a refused file header gives every hit its status);
 *   nil      1 for a nil record (RIO_OK, no bytes);
 *   len      RIO_OK: the decoded length. RIO_ERR_CAPACITY (set by the copy): the decoded length the query needs.
 *            RIO_ERR_UNSUPPORTED: a gzip / lzw record that is located but not expanded on the device: its payload
 *            is file bytes [payload_off, payload_off + len). Any other status: 0;
 *   detail0/1  RIO_ERR_HEADER_CRC: the expected / actual checksum.
 * rio_device_read_at_plan writes the hits and d_out_off[n + 1], the exclusive sum of the decoded lengths of the
 * RIO_OK non-nil hits (0 for every other hit); d_out_off[n] is the capacity the copy needs.
 * rio_device_read_at_copy writes record i to d_out + [d_out_off[i], d_out_off[i + 1]). A RIO_OK non-nil hit whose
 * range ends past out_cap becomes RIO_ERR_CAPACITY, keeps its len and writes nothing. A Snappy stream that does
 * not decode makes its hit RIO_ERR_DECOMPRESS with len 0; its range in d_out_off stays and the bytes of that range
 * are unspecified. Nothing is written outside the ranges. gzip / lzw payloads are not expanded (the hits stay RIO_ERR_UNSUPPORTED).
 * The plan's scan arenas belong to the context and only grow: a plan that needs larger ones than any before it
 * frees the old ones, which waits for the device, and two plans of one context must not be in flight on different
 * streams at once (one context serves one stream at a time for these calls, as for the other plan calls).
 * Both return RIO_OK for n == 0 without launching anything, RIO_ERR_ARG for a null or misaligned argument,
 * RIO_ERR_UNSUPPORTED for n >= 2^31 - 1, all before any device call. */
typedef struct rio_read_at_hit {
    int32_t status;
    int32_t nil;
    uint64_t len;
    uint64_t detail0, detail1;
    uint64_t hdr_len;      /* bytes of the record's header */
    uint64_t payload_off;  /* file offset of the first payload byte */
} rio_read_at_hit;
int rio_device_read_at_plan(rio_ctx* ctx, const uint8_t* d_file, uint64_t len, const uint64_t* d_offsets, uint64_t n,
                            rio_read_at_hit* d_hits, uint64_t* d_out_off, void* stream);
int rio_device_read_at_copy(rio_ctx* ctx, const uint8_t* d_file, uint64_t len, uint64_t n, rio_read_at_hit* d_hits,
                            const uint64_t* d_out_off, uint8_t* d_out, uint64_t out_cap, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Reader handles mirroring recordio.ReaderI / recordio.ReadAtI on top of the device path.     */
/* Returned data pointers: ReadNext until Close (windowed file readers: until the next        */
/* ReadNext); ReadNextAt / SeekNext as documented at their declarations. The Go adapter        */
/* slices/copies them into Go memory.                                                           */
/* ------------------------------------------------------------------------------------------ */
typedef struct rio_reader rio_reader;

int rio_reader_new_file(rio_ctx* ctx, const char* path, rio_reader** out); /* NewFileReaderWithPath */
int rio_reader_new_mmap(rio_ctx* ctx, const char* path, rio_reader** out); /* NewMemoryMappedReaderWithPath */
int rio_reader_open(rio_reader* r);
int rio_reader_close(rio_reader* r);
void rio_reader_free(rio_reader* r);
int rio_reader_header(rio_reader* r, uint32_t* version, uint32_t* compression);
uint64_t rio_reader_size(rio_reader* r);
/* detail values of the last error (HEADER_CRC: expected/actual; VERSION etc.: value) */
void rio_reader_last_detail(rio_reader* r, uint64_t* detail0, uint64_t* detail1, uint64_t* offset);
/* ReaderI. read_next on a record that does not decompress returns RIO_ERR_DECOMPRESS (RIO_EOF_CODEC
 * for gzip's empty payload) and the next call returns the record after it; skip_next passes over it. */
int rio_reader_read_next(rio_reader* r, const uint8_t** data, uint64_t* len, int* is_nil);
int rio_reader_skip_next(rio_reader* r);
/* ReadAtI (recordio.go:91-105), thread-safe: any number of threads may call these on one handle.
 * The first call decodes the whole file once; after that ReadNextAt at a record start, and SeekNext
 * (seek_len >= 4) whose scan lands on a decoded record, are a binary search on the calling thread
 * (no kernel, no lock) and *data points into the reader's decoded arena, valid until rio_reader_free.
 * Other offsets run the single-record kernels on a per-call stream; *data is then valid until the
 * calling thread's next ReadNextAt / SeekNext. Detail values are per thread (rio_reader_last_detail). */
int rio_reader_read_next_at(rio_reader* r, uint64_t offset, const uint8_t** data, uint64_t* len,
                            int* is_nil);
int rio_reader_seek_next(rio_reader* r, uint64_t offset, uint64_t* rec_offset, const uint8_t** data,
                         uint64_t* len, int* is_nil);
/* n ReadNextAt calls in one: hits[i] is what rio_reader_read_next_at(offsets[i]) returns (status, nil, len, and
 * the details of a RIO_ERR_HEADER_CRC in the hit itself), record i is (*data)[(*out_off)[i] .. (*out_off)[i + 1]),
 * in query order. Thread-safe like the calls above; *data and *out_off (n + 1 entries) are valid until the calling
 * thread's next batch call or rio_reader_free (a record that does not decode has an empty range here; hdr_len and
 * payload_off are 0 in hits answered from the index). The batch never builds the reader's decoded index: when an earlier
 * ReadNextAt / SeekNext has built it, offsets that are record starts are copied from it on the calling thread;
 * every other offset goes to one rio_device_read_at_plan / _copy pair over the reader's device copy of the file,
 * whose offsets, hits and bytes come back in three staged copies, each with its own synchronise (the pair runs a
 * second time when the reader's output arena, which only grows, was too small for the batch). gzip / lzw records that pair locates but does not expand are expanded
 * one by one, each as a small file of its own: slow, correct, and meant for the odd record, not for bulk reads of
 * such files. Returns RIO_OK (per-query statuses are in the hits), RIO_ERR_ARG, RIO_ERR_STATE (not open),
 * RIO_ERR_UNSUPPORTED (n >= 2^31 - 1) or a device failure. */
int rio_reader_read_next_at_batch(rio_reader* r, const uint64_t* offsets, uint64_t n, rio_read_at_hit* hits,
                                  const uint8_t** data, const uint64_t** out_off);
/* MMapReader.seekLen (mmap_reader.go:370, default 4096; tests shrink it to 10) */
int rio_reader_set_seek_len(rio_reader* r, uint64_t seek_len);
/* A read-only view of what the ReadAtI calls above answer from (open MMAP-mode readers; RIO_ERR_STATE
 * otherwise, RIO_ERR_ARG on a null argument): the decoded record count and the SeekNext map, every
 * 0x91 offset of the file with the end of a SeekNext walk from it. Builds the index if no call has
 * yet; nothing else does. n_records == 0 means the index was not built (a framing / decode error, a
 * refused header, a failed allocation, a decoded size over RIO_READAT_INDEX_MAX): the single-record
 * kernels answer every call and the two arrays are empty. The pointers are into the reader's index,
 * valid until rio_reader_free. (A struct tag, not a typedef: C keeps typedef and function names in
 * one namespace, and the call carries the same name.) */
#define RIO_SEEK_END_OTHER (~0ull >> 1)             /* the walk ends at a trial outside the decoded sequence */
#define RIO_SEEK_END_EOF   (RIO_SEEK_END_OTHER - 1) /* the walk runs to the file end: io.EOF */
struct rio_reader_index_info {
    uint64_t n_records;        /* decoded records the index serves; 0 = not built, the kernels answer everything */
    uint64_t n_positions;      /* K */
    const uint64_t* positions; /* P[K]: every 0x91 offset, ascending */
    const uint64_t* ends;      /* R[K]: record number < n_records, RIO_SEEK_END_EOF or RIO_SEEK_END_OTHER */
};
int rio_reader_index_info(rio_reader* r, struct rio_reader_index_info* info);
/* whole-file result of a file reader after its (lazy) device decode (RIO_ERR_STATE when windowed) */
int rio_reader_file_info(rio_reader* r, rio_file_info* info);
/* File readers decode files larger than 256 MiB in 128 MiB windows (rio_stream_*); before the first
 * ReadNext / SkipNext this sets the window (files larger than it are windowed), or ~0 for whole-file
 * decode always, or 0 for the automatic policy. Records and errors are the same either way. */
int rio_reader_set_window(rio_reader* r, uint64_t window_bytes);

/* ------------------------------------------------------------------------------------------ */
/* Input generator (host): byte-identical to FileWriter for v4 files (file_writer.go:160-233);   */
/* Snappy records use a golang/snappy v1.0.0-compatible block encoder. Not on the decode path.  */
/* ------------------------------------------------------------------------------------------ */
typedef struct rio_writer rio_writer;
int rio_writer_new(const char* path, uint32_t compression, rio_writer** out);
/* record == NULL writes a nil record; returns the record's offset in *offset */
int rio_writer_write(rio_writer* w, const uint8_t* record, uint64_t len, uint64_t* offset);
uint64_t rio_writer_size(rio_writer* w);
/* appends len bytes of already-framed records (rio_device_encode's image without its file header, or a
 * part of it cut at record boundaries) as they are; rio_writer_size grows by len */
int rio_writer_append_framed(rio_writer* w, const uint8_t* bytes, uint64_t len);
int rio_writer_close(rio_writer* w);
/* In-memory encoder used by the generators: appends one record to buf (capacity cap), returns
 * bytes written or 0 if it does not fit. record == NULL => nil record. */
uint64_t rio_encode_record_v4(uint8_t* buf, uint64_t cap, uint32_t compression,
                              const uint8_t* record, uint64_t len);
void rio_encode_file_header(uint8_t* buf8, uint32_t version, uint32_t compression);
uint64_t rio_snappy_max_encoded_len(uint64_t n);
uint64_t rio_snappy_encode(uint8_t* dst, uint64_t dst_cap, const uint8_t* src, uint64_t n);
/* Synthetic workloads of BASELINE.json. Writes a complete v4 file
 * image into buf; returns its length (0 if cap too small). kind: 0 = ref-random (one record of
 * bytes in [0,254] repeated, benchmark/recordio_read_test.go:32-42), 1 = text-like (seeded
 * Zipf words, distinct per record), 2 = random bytes distinct per record. */
uint64_t rio_generate(uint8_t* buf, uint64_t cap, uint32_t compression, uint64_t n_records,
                      uint64_t record_len, int kind, uint64_t seed, int threads);
uint64_t rio_generate_bound(uint32_t compression, uint64_t n_records, uint64_t record_len);

#ifdef __cplusplus
}
#endif
#endif /* RIO_H */
