// rio_ctx.h — the context of librio's host runtime: struct rio_ctx and the few helpers that more than one of the
// runtime's files needs (rio_ctx.cpp, rio_decode.cpp, rio_reader.cpp, rio_tables.cpp, rio_index.cpp, rio_encoder.cpp).
// Internal to librio; rio_replay.cpp and rio_writer.cpp reach the context only through rio_host.h.
//
// Ownership. Every device arena is a DevBuf and every DevBuf frees itself; a feature's events and page-locked
// memory are freed by the destructor of the nested struct that holds them. Nothing is released from a list.
// The invariant this rests on: no arena is freed, and no host vector that an async copy reads is destroyed, before
// the synchronisations of rio_ctx_destroy (the context's stream, the order event, the plan uploads). So
// rio_ctx_destroy synchronises first and deletes last, a destructor never runs on a live context, and no DevBuf
// has static storage duration (its hipFree would run after the HIP runtime's teardown).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <vector>

#include "rio_host.h"
#include "rio_launch.h"

#define HIP_TRY(x)                                  \
    do {                                            \
        hipError_t e_ = (x);                        \
        if (e_ != hipSuccess) return RIO_ERR_HIP;   \
    } while (0)

namespace rio {

inline int hip_status(hipError_t e) { return e == hipSuccess ? RIO_OK : RIO_ERR_HIP; }

// statuses of a file whose header was refused, and those after which no record was framed at all
inline bool header_refused(int s) {
    return s == RIO_ERR_VERSION || s == RIO_ERR_COMPRESSION_TYPE || s == RIO_ERR_SHORT_FILE_HEADER;
}
inline bool nothing_framed(int s) { return header_refused(s) || s == RIO_ERR_UNSUPPORTED; }

inline uint64_t env_u64(const char* name, uint64_t dflt) {
    const char* v = getenv(name);
    if (!v || !*v) return dflt;
    return strtoull(v, nullptr, 0);
}

// A grow-only device allocation that frees itself.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        release();
        size_t want = std::max<size_t>(n, 256);
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

// framing scratch + per-record decode descriptors of one file (a ctx has one set per file of a batch)
struct FileArenas {
    // meta: the scan state, the file info, the lanes' failure list, the block and chunk summaries and the chunk
    // placements of one call in one allocation (state and block summaries first, 256-byte aligned parts)
    DevBuf scratch, rec_pay, rec_desc, meta;
    uint64_t bytes() const {
        return scratch.cap + rec_pay.cap + rec_desc.cap + meta.cap;
    }
};

// A plan's table (views or segments, then their bases) on the device, with the host copy it is uploaded from.
struct PlanUpload {
    DevBuf dev;
    std::vector<uint64_t> host;
    hipEvent_t ev = nullptr;  // recorded after the last upload's copy of `host`
    ~PlanUpload() {
        wait();
        if (ev) hipEventDestroy(ev);
    }
    // `fresh` (already sized into `dev`) goes up on stream s. The host copy lives here until the next upload,
    // which waits for this upload's copy of it (not for the stream): the copy may read it after the call returns
    hipError_t upload(std::vector<uint64_t>& fresh, hipStream_t s) {
        hipError_t e = ev ? hipEventSynchronize(ev) : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) return e;
        host.swap(fresh);
        e = hipMemcpyAsync(dev.p, host.data(), host.size() * 8, hipMemcpyHostToDevice, s);
        return e != hipSuccess ? e : hipEventRecord(ev, s);
    }
    void wait() const {
        if (ev) hipEventSynchronize(ev);
    }
};

}  // namespace rio

// One member per feature; a feature's entry points are in the file named beside it.
struct rio_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // reader handles sharing this ctx take this around every device use (rio_reader_*)
    std::mutex mu;

    // timing ring (empty by default): slot i holds the 5 stage events of the i-th decode since rio_ctx_set_timing
    struct Timing {
        std::vector<std::array<hipEvent_t, 5>> ring;
        uint64_t cursor = 0;
        hipEvent_t* next_events() {
            if (ring.empty()) return nullptr;
            return ring[cursor++ % ring.size()].data();
        }
        hipEvent_t* same_events() {  // phase B of the call whose phase A took the last slot
            if (ring.empty() || cursor == 0) return nullptr;
            return ring[(cursor - 1) % ring.size()].data();
        }
        void set_ring(size_t n) {
            for (auto& s : ring)
                for (auto& e : s) hipEventDestroy(e);
            ring.assign(n, {});
            for (auto& s : ring)
                for (auto& e : s) hipEventCreate(&e);
            cursor = 0;
        }
        ~Timing() { set_ring(0); }
    } timing;

    // framing (rio_ctx.cpp: ctx_frame_params)
    struct Framing {
        uint64_t chunk_bytes = 32768;
        bool chunk_auto = true;  // RIO_CHUNK_BYTES unset: larger wave-walk chunks for large records (kBigRecordChunk)
        // framing walk (RIO_WALK_LANE): 0 k_walk (one wave per chunk_bytes chunk), 1 k_walk_lane (one lane per
        // lane_chunk_bytes chunk, RIO_LANE_CHUNK_BYTES), 2 auto (default): the lane walk when the context's
        // previous decode had records of kLaneWalkMin..kLaneWalkMax bytes on average (512 B and up on files of 1 GiB and
        // more; walk_hint, written by that decode's finalize_info into page-locked host memory: no host
        // synchronisation), else the wave walk
        uint32_t walk_mode = 2;
        uint64_t lane_chunk_bytes = 16384;
        uint64_t lane_walk_min = 512;  // kLaneWalkSmallMin (RIO_LANE_WALK_MIN)
        uint64_t walk_slots = 5120;    // resident k_walk waves: CUs x 4 SIMDs x kWalkOcc (wave_chunk_bytes)
        uint64_t* walk_hint = nullptr;
        uint64_t coop_min = ~0ull >> 8;
        rio::FileArenas fa;                                   // the single-file calls
        std::vector<std::unique_ptr<rio::FileArenas>> batch;  // rio_device_decode_batch: one set per file
        rio::DevBuf sink;
        ~Framing() {
            if (walk_hint) hipHostFree(walk_hint);
        }
    } fr;

    // host two-phase API and single-record reads (rio_decode.cpp, rio_reader.cpp)
    struct HostApi {
        rio::DevBuf file, out, out_off, rec_off, flags, readat_out, readat_res, seek_off;
        // last host-API framing (rio_frame -> rio_decode)
        rio::FrameParams last{};
        bool framed = false;
        bool predecoded = false;  // gzip: rio_frame decoded the file already (ctx arenas hold the result)
        rio_file_info frame_info{};
    } host;

    // rio_device_read_at_plan (rio_decode.cpp): the scan input (n + 1 words) and the scan temp; grow-only
    struct ReadAtBatch {
        rio::DevBuf tmp, cub;
    } rab;

    // rio_sst_open (rio_tables.cpp): parsed index fields (4 x n), per-entry CRC-64, kernel results, v0 value ranges
    struct Sst {
        rio::DevBuf fields, crc, res, view;
    } sst;

    // rio_device_encode (rio_encoder.cpp): compressed payloads, their offsets and lengths, hash tables, headers,
    // record sizes, scan temp; rio_encode_file: records, offsets, flags, file image, record offsets
    struct Encode {
        rio::DevBuf scr, scr_off, clen, tab, hdr, size, tmp, cub;
        rio::DevBuf rec, rec_off, flags, out, out_off, len;
    } enc;

    // index search (rio_index.cpp): key prefixes, indices, permutation, radix sort temp
    struct Query {
        rio::DevBuf pfx, pfx_out, idx, perm, tmp;
    } q;

    // rio_sst_merge_* and rio_sst_flush_plan (rio_tables.cpp): the last plan's views + table bases, key prefixes,
    // scan input, keep-flag scan, scan temp
    struct Merge {
        rio::PlanUpload views;
        rio::DevBuf pfx, tmp, opos, cub;
        uint32_t T = 0;
        uint64_t N = 0;
        bool planned = false;
    } mrg;

    // rio_sst_flush_plan: key lengths and value CRCs (the registered view's arrays, alive until the next plan),
    // digits (2 x n), permutations (2 x n), radix sort temp; stage events while timing is on
    struct Flush {
        rio::DevBuf len, crc, dig, perm, cub;
        std::vector<hipEvent_t> ev;
        uint32_t stages = 0;
        ~Flush() {
            for (hipEvent_t e : ev) hipEventDestroy(e);
        }
    } fl;

    // rio_mem_index_build (rio_db_host.cpp): the plan's order and keep flags, the compaction's temp and its count
    // rio_mem_index_extend: the tail's index, ranks and result block in one allocation (ext); the merged copy
    // rio_mem_size_scan: the batch's deltas, the cut word and the batch plan's result block in one allocation (size)
    struct MemIndex {
        rio::DevBuf src, keep, cub, n_sel, ext, merged, size;
    } mem;

    // rio_wal_ops_plan (rio_tables.cpp): the last plan's segments + record bases, the per-record scratch
    // (WalParams, one allocation), scan temp; P holds the scratch pointers for the gather
    struct WalOps {
        rio::PlanUpload segs;
        rio::DevBuf scr, cub;
        rio::WalParams P{};
        bool planned = false;
    } wal;

    // rio_wal_ops_encode (rio_tables.cpp): the scan input (n + 1 words) and the 4 meta words in one allocation,
    // scan temp; grow-only, so a call with no more ops than an earlier one allocates nothing
    struct WalEnc {
        rio::DevBuf scr, cub;
    } walenc;

    // the two pinned staging pieces of h2d_staged / d2h_staged / h2d_fill and the event behind each piece's DMA
    struct Staging {
        uint8_t* pinned[2] = {nullptr, nullptr};
        hipEvent_t ev[2] = {};
        ~Staging() {
            for (int i = 0; i < 2; i++) {
                if (pinned[i]) hipHostFree(pinned[i]);
                if (ev[i]) hipEventDestroy(ev[i]);
            }
        }
    } stage;

    // the decode calls share the framing arenas: a call on another stream than the previous one waits
    // for it (ev, completed with or recorded after every such call)
    struct Order {
        hipEvent_t ev = nullptr;
        hipStream_t stream = nullptr;
        bool valid = false;
        ~Order() {
            if (ev) hipEventDestroy(ev);
        }
    } order;

    ~rio_ctx() {
        if (stream) hipStreamDestroy(stream);
    }
};

// a stack of loaded tables (rio_super.cpp); rio_db_host.cpp's reader reads its tables
struct rio_sst_stack {
    int device = 0;
    hipStream_t stream = nullptr;  // the creating context's, for calls with a NULL stream
    uint32_t T = 0;
    uint64_t max_batch = 0;
    rio::DevBuf tables, tmp, cub;       // views | prefix pointers | filters | stored-checksum pointers; scan input; scan temp
    rio::StackParams P{};               // the four table pointers and T
};

namespace rio {

// the stream of an entry point's `void* stream` argument: the caller's, or the context's own for null
inline hipStream_t stream_of(const rio_ctx* ctx, void* stream) {
    return stream ? static_cast<hipStream_t>(stream) : ctx->stream;
}

// rio_tables.cpp: rio_sst_flush_plan after its argument checks; with_crc = false leaves the checksum stage out
int flush_plan(rio_ctx* ctx, const rio_ops_view* ops, uint32_t mode, uint32_t max_key_len, uint64_t* d_src, uint8_t* d_keep,
               uint64_t* d_result, void* stream, bool with_crc);

// rio_ctx.cpp
int ctx_frame_params(rio_ctx* ctx, const uint8_t* d_file, uint64_t len, FrameParams& P, FileArenas& A,
                     bool reserve_all = false);
int order_before(rio_ctx* ctx, hipStream_t s);
int order_event(rio_ctx* ctx, hipEvent_t& e);
void order_mark(rio_ctx* ctx, hipStream_t s);
int order_after(rio_ctx* ctx, hipStream_t s);
int h2d_staged(rio_ctx* c, void* dst, const uint8_t* src, uint64_t n);
int d2h_staged(rio_ctx* c, uint8_t* dst, const void* src, uint64_t n);
int h2d_fill(rio_ctx* c, void* dst, uint64_t n, FillFn fill, void* user);

}  // namespace rio
