// rio_device.h — structures shared by the HIP kernels (the .hip files) and the host runtime
// (rio_ctx.h and the files that include it). Internal to librio; the public boundary is include/rio.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rio.h"

namespace rio {

#ifdef __HIPCC__
#define RIO_HD __host__ __device__
#else
#define RIO_HD
#endif

constexpr uint64_t kNone = ~0ull;       // "no speculative entry found in this chunk"
// WalkSlot::len: decoded length | flag bits
constexpr uint64_t kNilBit = 1ull << 63;  // nil record
constexpr uint64_t kBadBit = 1ull << 62;  // payload fails already at framing (codec preamble / size)
constexpr uint64_t kEofBit = 1ull << 61;  // gzip: empty payload (gzip.NewReader's io.EOF)
constexpr uint64_t kLenMask = kEofBit - 1;
constexpr uint32_t kDescWide = 0xFFFFFFFFu;  // rec_desc z = w = kDescWide: sizes in rec_pay (rec_stream)
// lanes of the Snappy lane decoder that met a corrupt record are listed for k_finish (re-checked there)
constexpr uint32_t kFailLanes = 1024;

// Snappy decode launch shape (k_snappy_pipe): every wave owns one 64-byte sink line that absorbs
// the pipeline's placeholder loads and stores.
constexpr unsigned kSnappyBlock = 256;
// RIO_SNAPPY_GRID: the launch grid (experiment builds: make variant VDEFS=-DRIO_SNAPPY_GRID=768); the
// sink is sized for up to kSnappyGridMax workgroups whatever the variant, so a build that changes the
// grid in rio_snappy.hip alone stays inside the context's sink
#ifndef RIO_SNAPPY_GRID
#define RIO_SNAPPY_GRID 512
#endif
constexpr unsigned kSnappyGrid = RIO_SNAPPY_GRID;
constexpr unsigned kSnappyGridMax = 1024;
static_assert(kSnappyGrid <= kSnappyGridMax, "sink sized for kSnappyGridMax workgroups");
constexpr uint64_t kSinkBytes = (uint64_t)kSnappyBlock / 64 * kSnappyGridMax * 64;

// Framing chunks are at most kMaxChunkBytes long (rio_ctx_create caps RIO_CHUNK_BYTES / RIO_LANE_CHUNK_BYTES there)
constexpr uint64_t kMaxChunkBytes = 1ull << 30;

// minimum waves per SIMD for k_walk (its launch bound; the context sizes small files' chunks by it, rio_ctx.cpp).
// Round 1: 6 waves with 60 B spilled to scratch beat 5 (walk 0.210 -> 0.185 ms on C2). With the packed DPP fill
// scans and the 32-bit LEB128 packing the spills landed in the fill loop: 6 waves 0.413 ms on C3, 5 waves (96
// VGPRs, no scratch) 0.300 ms, against 0.363 before (C2 0.183 -> 0.164 ms); without a bound the compiler takes 4 waves
constexpr uint32_t kWalkOcc = 5;
// chunks per block of k_scan_blocks' first level (k_place finds a chunk's block by it)
constexpr int kScanBlock = 256;

// One walked record: 16 bytes, written by the walks with one store and read by k_place with one load.
//   len: decoded length (bits 0..60) | kEofBit | kBadBit | kNilBit. k_gz_resize / k_lzw_resize rewrite the length.
//   pos: bits 0..29  record header offset from the chunk's start (a chunk owns the records that start in it, and
//                    chunks are at most kMaxChunkBytes = 2^30 bytes);
//        bits 30..37 bytes from the record header start to the first payload byte the decoder consumes (header +
//                    snappy preamble; the low byte of frame_record's `pay`);
//        bit  38     escape: the stream length does not fit bits 39..63, which are then 0;
//        bits 39..63 stream length (the rest of frame_record's `pay`), below kSlotStreamEsc = 32 MiB.
// The decoded length keeps all of its 61 bits (a resize pass may write any size there), so of the two lengths only
// the stream length can overflow its field, and the slot takes an escape bit for it (not widths proved against
// P.len). The decoded length and the flags are always the slot's. k_place recovers an escaped record's stream
// length from the chain, not by framing the record again (frame_record inside k_place cost it 32 VGPRs, three of
// its eight waves per SIMD and 256 bytes of scratch per lane): only a record with a payload escapes, for which
// frame_record gives next = start + header + payload and pay = (payload - k) << 8 | (header + k), so its stream is
// the bytes from start + (pay & 0xFF) to the chain's next record, and that record's start is in the chunk's next
// slot or, behind the chunk's last record, in ChunkSum::exit.
struct alignas(16) WalkSlot {
    uint64_t len;
    uint64_t pos;
};
constexpr uint32_t kSlotOffBits = 30, kSlotHdrShift = 30, kSlotStreamShift = 39;
constexpr uint64_t kSlotEsc = 1ull << 38;
constexpr uint64_t kSlotStreamEsc = 1ull << (64 - kSlotStreamShift);
// rel = record start - chunk start; len_flags = decoded length | flag bits; pay = frame_record's descriptor
RIO_HD inline WalkSlot slot_pack(uint64_t rel, uint64_t len_flags, uint64_t pay) {
    const uint64_t slen = pay >> 8;
    return WalkSlot{len_flags, rel | (pay & 0xFF) << kSlotHdrShift |
                                   (slen < kSlotStreamEsc ? slen << kSlotStreamShift : kSlotEsc)};
}
RIO_HD inline uint64_t slot_rel(uint64_t pos) { return pos & ((1ull << kSlotOffBits) - 1); }
// the `pay` descriptor of a slot (with the escape bit: its low byte only)
RIO_HD inline uint64_t slot_pay(uint64_t pos) { return (pos >> kSlotStreamShift) << 8 | ((pos >> kSlotHdrShift) & 0xFF); }

// Framing chunk: a byte range [cs, ce) of the file; a chunk OWNS the records whose header starts
// in its range. Written by the walk kernel, consumed by the scan / place kernels.
struct ChunkSum {
    uint64_t entry;    // speculative first record start in [cs, ce) (kNone if none validated)
    uint64_t exit;     // first record start >= ce reached from `entry` (or err_off if status != OK)
    uint64_t bytes;    // decoded bytes of the records walked from `entry`
    uint64_t err_off;  // offset of the header that raised `status`
    uint64_t det0, det1;  // HEADER_CRC expected/actual; MAGIC: bytes consumed by the magic varint
    uint32_t count;    // records walked from `entry` (all stored in scratch)
    int32_t status;    // RIO_OK or the terminal status raised inside this chunk
};

// Key-point summary of a run of chunks: the composed chunk functions
// evaluated at the run's first speculative entry `key`; identity (pass-through) for inputs >= ce.
struct RunSum {
    uint64_t key;      // kNone: the run has no speculative entry (owns nothing unless broken)
    uint64_t out;      // chain position after the run when entered at `key`
    uint64_t cnt;      // records owned
    uint64_t bytes;    // decoded bytes owned
    uint64_t ce;       // end of the run's byte range (0 = identity element)
    uint32_t term;     // the chain terminated (status) inside the run
    uint32_t broken;   // a speculative entry did not chain: slow path required
    uint64_t term_chunk;  // chunk index that raised the terminal status
};

// Per-chunk placement decided by the scan: records [base_idx, base_idx + owned) of the file are
// this chunk's scratch slots [0, owned).
struct ChunkPlace {
    uint64_t base_idx;
    uint64_t base_bytes;
    uint64_t owned;
};

// Device-side scan state (one per decode call).
struct ScanState {
    uint32_t version, compression;
    int32_t hdr_status;     // file header status
    uint32_t slow;          // 1 => ChunkPlace array is authoritative (sequential repair ran)
    uint64_t n_records;
    uint64_t total_bytes;
    int32_t status;         // terminal status
    uint32_t zero_nonzero;  // zero-tail check result (1 = a non-zero byte found)
    uint64_t status_offset;
    uint64_t det0, det1;
    uint64_t zero_from;     // zero-tail check range start (kNone = no check)
    uint64_t n_repairs;
    uint64_t first_bad;        // first record flagged RIO_FLAG_CORRUPT / RIO_FLAG_EOF (kNone = none)
    uint64_t n_bad;            // records so flagged
    uint64_t unsupported_rec;  // first record the device path hands back (absurd gzip sizes)
    uint32_t n_fail_lanes;     // Snappy lane-decoder lanes listed in fail_lanes (> kFailLanes: all)
    uint32_t capacity_fail;
    uint32_t huge_streams;  // a record stream exceeds 32-bit positions: the wave decoder (coop_file) runs, one thread per record
    uint32_t any_mixed;     // snappy: some record is not one literal covering its output (k_place);
                            // 0 => every record is copied by k_copy_records instead of k_snappy_pipe
    uint32_t scan_ticket;   // k_scan_blocks: the last block to finish runs the top-level scan
    uint32_t finish_ticket; // k_finish: the last block to finish publishes the result
    uint32_t pipe_next;     // k_snappy_pipe: next record chunk handed to a wave that finished its own
    uint32_t gz_resize;     // gzip: some record holds several members whose output the framing's
                            // size (its last member's ISIZE) does not cover: k_gz_resize sizes them;
                            // lzw: some record's output is not its header's u (k_lzw_resize)
    uint32_t gz_redo;       // k_gz_resize / k_lzw_resize ran: the scan, placement and decoders run again
};

// Result of the single-record (ReadNextAt) kernel.
struct ReadAtResult {
    int32_t status;
    int32_t nil;
    uint64_t len;
    uint64_t det0, det1;
    uint64_t hdr_len;
    uint64_t payload_off;
};

// the batched calls hand the same fields out as rio_read_at_hit (rio.h): one layout, read either way
static_assert(sizeof(rio_read_at_hit) == sizeof(ReadAtResult) && alignof(rio_read_at_hit) == alignof(ReadAtResult) &&
                  offsetof(rio_read_at_hit, status) == offsetof(ReadAtResult, status) &&
                  offsetof(rio_read_at_hit, nil) == offsetof(ReadAtResult, nil) &&
                  offsetof(rio_read_at_hit, len) == offsetof(ReadAtResult, len) &&
                  offsetof(rio_read_at_hit, detail0) == offsetof(ReadAtResult, det0) &&
                  offsetof(rio_read_at_hit, detail1) == offsetof(ReadAtResult, det1) &&
                  offsetof(rio_read_at_hit, hdr_len) == offsetof(ReadAtResult, hdr_len) &&
                  offsetof(rio_read_at_hit, payload_off) == offsetof(ReadAtResult, payload_off),
              "rio_read_at_hit is ReadAtResult");

// rio_seek.hip / rio_snappy.hip: a batch of ReadNextAt queries on one file (rio_device_read_at_plan / _copy)
struct ReadAtParams {
    const uint8_t* file;      // 16-byte aligned, RIO_DEVICE_PAD readable bytes past len
    uint64_t len;
    const uint64_t* offsets;  // [n] (plan)
    uint64_t n;
    ReadAtResult* hits;       // [n]
    uint64_t* tmp;            // [n + 1] scan input (plan)
    uint64_t* out_off;        // [n + 1] written by the plan, read by the copy
    uint8_t* out;             // (copy)
    uint64_t out_cap;
    uint8_t* sink;            // [kSinkBytes] the context's sink arena (Snappy copy)
};

// Launch configuration passed from the host runtime.
struct FrameParams {
    const uint8_t* file;
    uint64_t len;
    uint64_t chunk_bytes;
    uint64_t n_chunks;
    uint64_t slots;  // scratch slots per chunk
    WalkSlot* scratch;       // [n_chunks * slots] the walked records of each chunk
    // internal per-record payload descriptor [rec_cap]: bits 0..7 = bytes from the record header
    // start to the first payload byte the decoder consumes (header + snappy preamble), bits 8..63
    // = length of the consumed payload stream (snappy element stream / raw payload). Written for
    // gzip / lzw files and for records rec_desc cannot describe (see rec_stream)
    uint64_t* rec_pay;
    // internal per-record decode descriptor [rec_cap] (Snappy decode): x,y = file offset of the
    // element stream (lo, hi), z = stream length, w = decoded length
    uint4* rec_desc;
    uint8_t* sink;           // [kSinkBytes] placeholder-store target of the Snappy decode pipeline
    uint64_t* fail_lanes;    // [2 * kFailLanes] record ranges [r0, r1) of lanes that met a corrupt record
    // Snappy: files whose mean decoded record is at least this many bytes (and files past 32-bit
    // lane positions) take the wave-per-record decoder k_snappy_coop instead of k_snappy_pipe
    uint64_t coop_min;
    // the file header's compression type as the host knows it (RIO_COMP_UNKNOWN: every decoder is
    // launched and exits unless the file is its own); k_finish rejects a file that contradicts it
    uint32_t comp_hint;
    uint32_t zero_done;  // the zero-tail check already ran (host API phase A): k_place skips it
    uint32_t walk_lane;  // framing by k_walk_lane (one lane per chunk) instead of k_walk (one wave per chunk)
    uint64_t* walk_hint; // page-locked host word: the decode's mean bytes per record (finalize_info), read by
                         // the context when it picks the next decode's walk (null: not recorded)
    uint32_t redo;       // redo round of this codec (RIO_COMP_GZIP: k_gz_resize onwards, RIO_COMP_LZW:
                         // k_lzw_resize onwards; 0: first round): the kernel exits unless the file is
                         // that codec's and its resize kernel ran
    ChunkSum* chunks;
    RunSum* block_runs;      // [n_blocks] (scan level 1 output)
    RunSum* chunk_excl;      // [n_chunks] exclusive within-block prefix
    ChunkPlace* place;       // [n_chunks]
    uint64_t* block_in;      // [n_blocks] chain position entering each block
    RunSum* block_excl;      // [n_blocks] exclusive prefix over blocks
    uint64_t n_blocks;
    ScanState* state;
    // outputs
    uint8_t* out;
    uint64_t out_cap;
    uint64_t* out_off;
    uint64_t* rec_off;
    uint8_t* flags;
    uint64_t rec_cap;
    rio_file_info* info;  // device copy of the public result
};

// Files of one rio_device_decode_batch call, passed by value to the batched decode kernel (the
// kernel argument holds them all: no H2D copy, no host sync, graph-capturable).
constexpr uint32_t kMaxBatch = 16;
struct FrameBatch {
    FrameParams f[kMaxBatch];
    uint32_t n;
};

// rio_encode.hip: recordio v4 encoding of a batch of records (rio_device_encode)
struct EncParams {
    const uint8_t* rec;        // records arena
    const uint64_t* rec_off;   // [n + 1]
    const uint8_t* flags;      // [n] RIO_FLAG_NIL, or null
    uint64_t n;
    uint32_t compression;
    uint8_t* scratch;          // compressed payloads, record i at scr_off[i]
    uint64_t* scr_off;         // [n + 1]
    uint64_t* clen;            // [n] payload length in the file (c for snappy, u for none)
    uint16_t* gtab;            // global tables: kMaxTable entries per lane of k_snappy_encode<false>
    uint8_t* hdr;              // [n][kHdrSlot] header bytes; hdr[i * kHdrSlot + 63] = header length
    uint64_t* size;            // [n + 1] exclusive scan of the record sizes = file offsets - 8
    uint64_t* tmp;             // [n + 1] scan inputs (payload bounds, then record sizes)
    uint8_t* out;
    uint64_t out_cap;
    uint64_t* out_rec_off;     // [n] file offset of each record (what Write returns)
    uint64_t* out_len;         // [1] file length
    uint32_t lds_small;        // records <= 1 KiB on the LDS-table kernel
};

// rio_compact.hip: merge-compaction of loaded tables (rio_sst_merge_plan / _gather, rio_sst_index_encode)
struct MergeParams {
    const rio_sst_view* views;  // [T] device copy of the caller's views
    const uint64_t* base;       // [T + 1] number of table t's first entry among all N input entries
    uint32_t T;
    uint32_t mode;              // RIO_MERGE_*
    uint64_t N;
    uint64_t* pfx;              // [N] first 8 key bytes, big-endian, zero-padded
    uint64_t* src;              // [N] table << RIO_MERGE_ENTRY_BITS | entry, in merged order
    uint8_t* keep;              // [N]
    uint64_t* result;           // [RIO_MERGE_RESULT_WORDS]
};
struct GatherParams {
    const rio_sst_view* views;
    uint32_t T;
    uint64_t N, n_out;
    const uint64_t* src;        // [N] the plan's order
    const uint8_t* keep;        // [N]
    uint64_t* tmp;              // [max(N, n_out) + 1] scan input
    uint64_t* opos;             // [N + 1] exclusive scan of keep
    uint64_t* out_src;          // [n_out]
    uint8_t* values;
    uint64_t values_cap;
    uint64_t* val_off;          // [n_out + 1]
    uint8_t* val_flags;         // [n_out]
};
struct EntryParams {
    const rio_sst_view* views;
    uint32_t T;
    uint64_t n_out;
    const uint64_t* out_src;    // [n_out]
    const uint64_t* file_off;   // [n_out] ValueOffset of each entry
    uint64_t* tmp;              // [n_out + 1] scan input
    uint8_t* entries;
    uint64_t entries_cap;
    uint64_t* ent_off;          // [n_out + 1]
};

// rio_flush.hip: ordering and latest-wins reduce of a memstore's op log (rio_sst_flush_plan)
struct FlushParams {
    rio_ops_view ops;
    uint32_t mode;              // RIO_FLUSH_*
    uint32_t max_key_len;       // bound on the key lengths: ceil(max_key_len / 8) chunk passes
    uint64_t* key_len;          // [n] clamped key lengths (the registered view's key_len)
    uint64_t* crc;              // [n] CRC-64/ISO of the kept values, by op (the registered view's crc)
    uint64_t* dig[2];           // [n] a pass's digits and the sort's reordered copy of them
    uint32_t* perm[2];          // [n] op indices in the order so far, in and out of a pass
    void* cub;                  // radix sort temp
    size_t cub_bytes;
    uint64_t* src;              // [n] op at sorted position p
    uint8_t* keep;              // [n]
    uint64_t* result;           // [RIO_MERGE_RESULT_WORDS]
};
constexpr uint32_t kFlushMaxStages = (RIO_FLUSH_MAX_KEY_LEN + 7) / 8 + 1 + 3;  // check, passes, keep, crc

// rio_walops.hip: WalMutation records of decoded WAL files to an op log (rio_wal_ops_plan / _gather)
constexpr uint8_t kWalNoOp = 0, kWalUpsert = 1, kWalTombstone = 2;
struct WalParams {
    const rio_wal_segment* segs;  // [S] device copy of the caller's segments
    const uint64_t* base;         // [S + 1] number of segment s's first record among all N records
    uint32_t S;
    uint64_t N;
    // per record, written by the plan (context scratch)
    uint32_t* rec;                // [N] kWal* | segment << 8
    uint64_t* koff;               // [N] key range in the segment's arena (offset; the length is klen)
    uint64_t* voff;               // [N] value range
    uint64_t* klen;               // [N + 1] scan inputs: 0 for a record without an op
    uint64_t* vlen;               // [N + 1]
    uint64_t* isop;               // [N + 1]
    uint64_t* opos;               // [N + 1] exclusive scans: op number, key and value arena offsets
    uint64_t* kdst;               // [N + 1]
    uint64_t* vdst;               // [N + 1]
    uint64_t* meta;               // [2] smallest (bad record << 3 | class), longest key
    uint64_t* result;             // [RIO_WAL_RESULT_WORDS]
    // the gather's outputs
    uint64_t n_ops;
    uint8_t* keys;
    uint64_t keys_cap;
    uint64_t* key_off;            // [n_ops + 1]
    uint8_t* values;
    uint64_t values_cap;
    uint64_t* val_off;            // [n_ops + 1]
    uint8_t* flags;               // [n_ops]
    uint64_t* op_rec;             // [n_ops] or null
};

// rio_walenc.hip: an op log to WalMutation records (rio_wal_ops_encode)
struct WalEncParams {
    rio_ops_view ops;             // by value: nothing is copied to the device beforehand
    uint8_t* records;             // record arena
    uint64_t records_cap;
    uint64_t* rec_off;            // [n + 1] the caller's: exclusive scan of len
    uint64_t* len;                // [n + 1] scan input (context scratch): record lengths, item n = 0
    uint64_t* meta;               // [4] smallest (bad op << 3 | class), longest key, upserts, deletes
    uint64_t* result;             // [RIO_WALENC_RESULT_WORDS]
};

// rio_bloom.hip: bloom filter build / query and the point lookup of a loaded table (rio_bloom_*, rio_sst_lookup)
struct BloomParams {
    rio_bloom_view f;             // the filter (bits == null: rio_sst_lookup without a gate)
    // keys of an arena (rio_bloom_add / rio_bloom_contains / rio_sst_lookup's queries)
    const uint8_t* keys;
    const uint64_t* key_off;      // [n + 1]
    uint64_t n;
    uint64_t key_bytes;           // arena length: every key is clamped to it
    // keys of the last plan's survivors (rio_sst_bloom_add): n survivors
    const rio_sst_view* views;
    uint32_t T;
    const uint64_t* out_src;      // [n]
    uint8_t* hit;                 // [n] rio_bloom_contains
};
struct LookupParams {
    rio_sst_view v;               // the table, by value: nothing is copied to the device beforehand
    const uint64_t* pfx;          // [v.n] rio_sst_key_prefixes
    uint64_t* entry;              // [n] entry index or ~0
};

// rio_stack.hip: a stack of loaded tables (rio_sst_stack_*). The four tables live in device memory the stack
// owns; every kernel reads them at wave-uniform addresses
struct StackParams {
    const rio_sst_view* views;          // [T]
    const uint64_t* const* pfx;         // [T] rio_sst_key_prefixes of table t
    const rio_bloom_view* filters;      // [T] bits == null: table t has no filter
    const uint64_t* const* stored;      // [T] the index entries' stored checksums, or null
    uint32_t T;
    uint32_t flag;                      // lookup: gated; value plan: check_crc; bounds: upper
    // queries of an arena (lookup, bounds)
    const uint8_t* keys;
    const uint64_t* key_off;            // [n + 1]
    uint64_t n;
    uint64_t key_bytes;
    uint64_t* src;                      // [n] lookup's output, the value calls' input
    uint8_t* status;                    // [n] RIO_GET_*
    uint64_t* tmp;                      // [n + 1] scan input (stack scratch)
    uint64_t* val_off;                  // [n + 1]
    uint8_t* values;
    uint64_t values_cap;
    uint64_t* pos;                      // [n * T] bounds
};
// rio_sst_keys_gather: keys of a plan's survivors
struct KeysParams {
    const rio_sst_view* views;
    uint32_t T;
    uint64_t n_out;
    const uint64_t* out_src;            // [n_out]
    uint64_t* tmp;                      // [n_out + 1] scan input
    uint8_t* keys;
    uint64_t keys_cap;
    uint64_t* key_off;                  // [n_out + 1]
};

// rio_memidx.hip: a memstore's index (rio_mem_index_build) and the lookup over up to two of them (rio_mem_lookup)
struct MemBuildParams {
    rio_ops_view ops;
    const uint64_t* src;                // [n] the flush plan's order
    const uint8_t* keep;                // [n] its keep flags
    uint64_t* order;                    // [n] src compacted by keep
    uint64_t* pfx;                      // [n] key prefixes of order's ops
    uint64_t* n_sel;                    // [1] the compaction's count (scratch; the result block's word is read)
    uint64_t* result;                   // [RIO_MERGE_RESULT_WORDS] the plan's, on the device
};
// rio_mem_index_extend: A = the index of ops [0, n_old) in order / pfx / result, B = the index of the tail
// [n_old, ops.n) in context scratch (op words relative to n_old); the merged index returns to order / pfx / result
struct MemExtendParams {
    rio_ops_view ops;                   // the whole log
    uint64_t n_old, t;                  // t = ops.n - n_old > 0
    uint64_t* order;                    // [ops.n] A, then the merged index
    uint64_t* pfx;                      // [ops.n]
    uint64_t* result;                   // [RIO_MERGE_RESULT_WORDS] A's, then the merged index's
    const uint64_t* b_order;            // [t] B
    const uint64_t* b_pfx;              // [t]
    const uint64_t* b_result;           // [RIO_MERGE_RESULT_WORDS] the tail plan's, sealed
    uint64_t* lb;                       // [t + 1] A keys below B[j]; nA from nB on
    uint64_t* eq;                       // [t + 1] 1 when A[lb[j]] is B[j]'s key (the scan's input)
    uint64_t* e;                        // [t + 1] exclusive scan of eq
    uint64_t* m_order;                  // [ops.n] the merged copy
    uint64_t* m_pfx;                    // [ops.n]
    uint64_t* drop;                     // [4] sums over the dropped A entries: count, value bytes, nil values, key bytes
};
// rio_ops_append: the offsets of a batch rebased behind a log's
struct OpsRebaseParams {
    uint64_t* key_off;                  // the log's, [log_n + n + 1] and more
    uint64_t* val_off;
    const uint64_t* b_key_off;          // the batch's, [n + 1]
    const uint64_t* b_val_off;
    uint64_t log_n, n;                  // n > 0
    uint64_t log_key_bytes, log_value_bytes, b_key_bytes, b_value_bytes;
};
struct MemLookupParams {
    rio_mem_index i0, i1;               // by value: store 0 and, when n_idx = 2, the newer store 1
    uint32_t n_idx;
    const uint8_t* keys;
    const uint64_t* key_off;            // [n + 1]
    uint64_t n;
    uint64_t key_bytes;
    uint64_t* src;                      // [n] store << RIO_MERGE_ENTRY_BITS | op, or ~0
};
// rio_memsize.hip: the running size estimate of a batch over a write store (rio_mem_size_scan)
struct MemSizeParams {
    rio_mem_index store;                // by value; store.ops.n = 0: an empty store
    rio_ops_view batch;
    uint64_t size0, max_size;
    const uint64_t* src;                // [n] the batch plan's order
    const uint8_t* keep;                // [n] its keep flags
    const uint64_t* plan;               // [RIO_MERGE_RESULT_WORDS] its result block
    uint64_t* delta;                    // [n] what op i adds to the size, mod 2^64; size0 rides on op 0
    uint64_t* size;                     // [n] d_size: the inclusive sum of delta
    uint64_t* cut;                      // [1] the first over-limit put, or ~0
    uint64_t* result;                   // [RIO_SIZE_RESULT_WORDS]
};
// rio_db.hip: the combined read (rio_db_value_plan / rio_db_value_copy)
struct DbParams {
    rio_mem_index i0, i1;
    uint32_t n_idx;
    const rio_sst_view* views;          // [T] the stack's tables; T = 0: a reader without a stack
    const uint64_t* const* stored;      // [T]
    uint32_t T;
    uint32_t check_crc;
    const uint64_t* tab_src;            // [n] or null
    const uint64_t* mem_src;            // [n]
    uint64_t n;
    uint8_t* status;                    // [n] RIO_GET_*
    uint64_t* tmp;                      // [n + 1] scan input (reader scratch)
    uint64_t* val_off;                  // [n + 1]
    uint8_t* values;
    uint64_t values_cap;
};

// protobuf varint length, and proto.Marshal's size of an IndexEntry {key = 1, valueOffset = 2, checksum = 3}:
// proto3 omits an empty key and zero scalars (sstables/proto/sstable.proto:5-9)
RIO_HD inline uint32_t pb_varint_len(uint64_t v) {
    uint32_t n = 1;
    while (v >= 0x80) {
        v >>= 7;
        n++;
    }
    return n;
}
// v as a varint at p (pb_varint_len(v) bytes); returns the byte behind it
RIO_HD inline uint8_t* pb_put_varint(uint8_t* p, uint64_t v) {
    while (v >= 0x80) {
        *p++ = (uint8_t)(v | 0x80);
        v >>= 7;
    }
    *p++ = (uint8_t)v;
    return p;
}
RIO_HD inline uint64_t pb_index_entry_len(uint64_t key_len, uint64_t value_off, uint64_t checksum) {
    return (key_len ? 1 + pb_varint_len(key_len) + key_len : 0) + (value_off ? 1 + pb_varint_len(value_off) : 0) +
           (checksum ? 1 + pb_varint_len(checksum) : 0);
}

#ifdef __HIPCC__
// A record whose payload does not decode: flag it for ReadNext (RIO_FLAG_CORRUPT) and count it.
// Only the thread that decoded record i writes its flag byte.
__device__ inline void mark_bad(const FrameParams& P, uint64_t i, uint8_t flag = RIO_FLAG_CORRUPT) {
    P.flags[i] = (uint8_t)(P.flags[i] | flag);
    atomicMin((unsigned long long*)&P.state->first_bad, (unsigned long long)i);
    atomicAdd((unsigned long long*)&P.state->n_bad, 1ull);
}
// Record i's consumed stream (snappy element stream / raw payload): file offset and length. k_place
// writes rec_pay only for gzip / lzw files (their kernels keep markers in it) and for records whose
// sizes do not fit rec_desc's 32-bit fields (rec_desc then holds the kDescWide sentinel).
__device__ inline void rec_stream(const FrameParams& P, uint64_t i, uint64_t& start, uint64_t& slen) {
    const uint4 d = P.rec_desc[i];
    if (d.z == kDescWide && d.w == kDescWide) {
        const uint64_t pay = P.rec_pay[i];
        start = P.rec_off[i] + (pay & 0xFF);
        slen = pay >> 8;
    } else {
        start = ((uint64_t)d.y << 32) | d.x;
        slen = d.z;
    }
}
#endif

}  // namespace rio
