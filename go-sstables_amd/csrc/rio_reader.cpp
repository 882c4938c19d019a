// rio_reader.cpp — the reader handles of librio (include/rio.h), which mirror recordio.ReaderI / recordio.ReadAtI:
//   FileReader  Open/ReadNext/SkipNext/Close   recordio/file_reader.go:26-172, 272-279
//   MMapReader  Open/ReadNextAt/SeekNext/Size  recordio/mmap_reader.go:25-203, 358-371
// Every decode runs on the device (rio_place.hip, rio_seek.hip); host code only moves bytes, parses the
// 8-byte file header at Open (readFileHeaderFromBuffer, common_reader.go:22-44) and iterates the
// decoded arena.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <string>

#include "rio_ctx.h"

using namespace rio;

// ------------------------------------------------------------------------------------------
// single-record decode (ReadNextAt) / seek (SeekNext) on a device-resident file
// ------------------------------------------------------------------------------------------
static int read_at_impl(rio_ctx* ctx, const uint8_t* d_file, uint64_t len, uint64_t offset, bool seek,
                        uint64_t seek_len, ReadAtResult* res, uint64_t* rec_offset) {
    rio_ctx::HostApi& H = ctx->host;
    HIP_TRY(H.readat_res.ensure(sizeof(ReadAtResult)));
    HIP_TRY(H.seek_off.ensure(8));
    if (H.readat_out.cap == 0) HIP_TRY(H.readat_out.ensure(1 << 20));
    for (int attempt = 0; attempt < 2; attempt++) {
        if (seek)
            HIP_TRY(launch_seek_next(d_file, len, offset, seek_len, H.readat_out.as<uint8_t>(), H.readat_out.cap,
                                     H.readat_res.as<ReadAtResult>(), H.seek_off.as<uint64_t>(), ctx->stream));
        else
            HIP_TRY(launch_read_at(d_file, len, offset, H.readat_out.as<uint8_t>(), H.readat_out.cap,
                                   H.readat_res.as<ReadAtResult>(), ctx->stream));
        HIP_TRY(hipMemcpyAsync(res, H.readat_res.p, sizeof(ReadAtResult), hipMemcpyDeviceToHost, ctx->stream));
        if (rec_offset) HIP_TRY(hipMemcpyAsync(rec_offset, H.seek_off.p, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (res->status != RIO_ERR_CAPACITY) return RIO_OK;
        HIP_TRY(H.readat_out.ensure(res->len + 16));
    }
    return RIO_OK;
}

// ------------------------------------------------------------------------------------------
// reader handles
// ------------------------------------------------------------------------------------------
// MMapReader's view of a decoded file: the FileReader sequence of records (rio_frame + rio_decode,
// once per reader) and the SeekNext map (build_seek_map, rio_seek.hip: every 0x91 position P[k]
// and the record R[k] a SeekNext walk reaching it ends at). ReadNextAt at a record start and SeekNext
// whose walk ends at a decoded record are answered from here by binary search on the calling thread:
// no kernel, no lock, no copy (the data pointer stays valid until rio_reader_free).
struct ReadAtIndex {
    std::vector<uint8_t> out, flags;
    std::vector<uint64_t> out_off, rec_off, P, R;
    uint64_t n = 0;
    // record index i with rec_off[i] == off, or n
    uint64_t find(uint64_t off) const {
        const uint64_t i = (uint64_t)(std::lower_bound(rec_off.begin(), rec_off.begin() + n, off) - rec_off.begin());
        return i < n && rec_off[i] == off ? i : n;
    }
    // ReadNextAt's result for record i (mmap_reader.go:130-203; the FileReader decoded the same bytes)
    int record(uint64_t i, const uint8_t** data, uint64_t* len, int* is_nil) const {
        if (flags[i] & RIO_FLAG_CORRUPT) return RIO_ERR_DECOMPRESS;
        if (flags[i] & RIO_FLAG_EOF) return RIO_EOF_CODEC;
        const bool nil = (flags[i] & RIO_FLAG_NIL) != 0;
        if (is_nil) *is_nil = nil ? 1 : 0;
        if (len) *len = nil ? 0 : out_off[i + 1] - out_off[i];
        if (data) *data = out.data() + out_off[i];
        return RIO_OK;
    }
};

struct rio_reader {
    rio_ctx* ctx = nullptr;
    std::string path;
    bool mmap_mode = false;
    std::atomic<bool> open{false}, closed{false};
    int fd = -1;
    const uint8_t* map = nullptr;
    uint64_t size = 0;
    uint32_t version = 0, compression = 0;
    std::mutex mu;
    // FILE mode: whole-file decode result
    bool decoded = false;
    int decode_rc = RIO_OK;
    rio_file_info info{};
    std::vector<uint8_t> out, flags;
    std::vector<uint64_t> out_off, rec_off;
    uint64_t cursor = 0;
    bool past_end = false;
    // windowed decode (rio_stream) for files larger than `window`: ReadNext walks the current
    // window's view, then fetches the next; the whole-file decode is the one-window case
    uint64_t window = 0;  // 0: automatic (kAutoWindow above kAutoWindowFrom), ~0: never
    rio_stream* stream = nullptr;
    const uint8_t* w_out = nullptr;
    const uint64_t* w_off = nullptr;
    const uint8_t* w_flags = nullptr;
    uint64_t w_n = 0;
    bool w_last = true;
    // MMAP mode
    bool on_device = false;
    DevBuf dfile;
    std::atomic<uint64_t> seek_len{4096};
    // MMAP mode: the device arenas of a batch (rio_reader_read_next_at_batch), used under mu and the context's lock
    DevBuf b_offsets, b_hits, b_out_off, b_out;
    // MMAP mode: the decoded file (built on the first ReadNextAt / SeekNext, then read-only)
    std::atomic<const ReadAtIndex*> ix{nullptr};
    std::unique_ptr<ReadAtIndex> ix_own;
};

// details of the last failed reader call, per calling thread (ReadAtI is used concurrently)
struct LastDetail {
    uint64_t d0 = 0, d1 = 0, off = 0;
};
static thread_local LastDetail tl_det;

static int reader_new(rio_ctx* ctx, const char* path, bool mm, rio_reader** out) {
    if (!ctx || !path || !out) return RIO_ERR_ARG;
    *out = nullptr;
    // NewFileReader / mmap.Open fail on a missing file (file_reader.go:507, mmap_reader.go:366)
    int fd = ::open(path, O_RDONLY);
    if (fd < 0) return RIO_ERR_IO;
    auto* r = new rio_reader();
    r->ctx = ctx;
    r->path = path;
    r->mmap_mode = mm;
    r->fd = fd;
    struct stat st;
    if (fstat(fd, &st) == 0) r->size = (uint64_t)st.st_size;
    *out = r;
    return RIO_OK;
}

extern "C" int rio_reader_new_file(rio_ctx* ctx, const char* path, rio_reader** out) {
    return reader_new(ctx, path, false, out);
}
extern "C" int rio_reader_new_mmap(rio_ctx* ctx, const char* path, rio_reader** out) {
    return reader_new(ctx, path, true, out);
}

extern "C" int rio_reader_open(rio_reader* r) {
    if (!r) return RIO_ERR_ARG;
    std::lock_guard<std::mutex> g(r->mu);
    if (r->open) return RIO_ERR_STATE;    // "already opened"
    if (r->closed) return RIO_ERR_STATE;  // "already closed"
    struct stat st;
    if (fstat(r->fd, &st) != 0) return RIO_ERR_IO;
    r->size = (uint64_t)st.st_size;
    if (r->size) {
        void* m = mmap(nullptr, r->size, PROT_READ, MAP_PRIVATE, r->fd, 0);
        if (m == MAP_FAILED) return RIO_ERR_IO;
        r->map = static_cast<const uint8_t*>(m);
    }
    if (r->size < RIO_FILE_HEADER_BYTES) return RIO_ERR_SHORT_FILE_HEADER;
    const uint8_t* f = r->map;
    r->version = f[0] | (uint32_t)f[1] << 8 | (uint32_t)f[2] << 16 | (uint32_t)f[3] << 24;
    r->compression = f[4] | (uint32_t)f[5] << 8 | (uint32_t)f[6] << 16 | (uint32_t)f[7] << 24;
    if (r->version > RIO_VERSION4 || r->version < RIO_VERSION1) {
        tl_det.d0 = r->version;
        return RIO_ERR_VERSION;
    }
    if (r->compression > RIO_COMP_LZW) {
        tl_det.d0 = r->compression;
        return RIO_ERR_COMPRESSION_TYPE;
    }
    r->open = true;
    return RIO_OK;
}

extern "C" int rio_reader_close(rio_reader* r) {
    if (!r) return RIO_ERR_ARG;
    std::lock_guard<std::mutex> g(r->mu);
    r->closed = true;
    r->open = false;
    if (r->map) munmap(const_cast<uint8_t*>(r->map), r->size);
    r->map = nullptr;
    if (r->stream) rio_stream_free(r->stream);
    r->stream = nullptr;
    r->w_n = 0;
    r->dfile.release();
    r->b_offsets.release();
    r->b_hits.release();
    r->b_out_off.release();
    r->b_out.release();
    r->on_device = false;
    return RIO_OK;
}

extern "C" void rio_reader_free(rio_reader* r) {
    if (!r) return;
    rio_reader_close(r);
    if (r->fd >= 0) ::close(r->fd);
    delete r;
}

extern "C" int rio_reader_header(rio_reader* r, uint32_t* version, uint32_t* compression) {
    if (!r) return RIO_ERR_ARG;
    if (version) *version = r->version;
    if (compression) *compression = r->compression;
    return r->open ? RIO_OK : RIO_ERR_STATE;
}

extern "C" uint64_t rio_reader_size(rio_reader* r) { return r ? r->size : 0; }

extern "C" void rio_reader_last_detail(rio_reader* r, uint64_t* d0, uint64_t* d1, uint64_t* off) {
    if (!r) return;
    if (d0) *d0 = tl_det.d0;
    if (d1) *d1 = tl_det.d1;
    if (off) *off = tl_det.off;
}

// files past 32 MiB are read window by window (rio_stream_*): one window's H2D overlaps earlier windows'
// decode and D2H, where the one-shot pair moves the whole file in, then all records out (round 4)
constexpr uint64_t kAutoWindowFrom = 32ull << 20, kAutoWindow = 128ull << 20;

static uint64_t reader_window(const rio_reader* r) {
    if (r->window == ~0ull) return 0;
    const uint64_t w = r->window ? r->window : kAutoWindow;
    const uint64_t from = r->window ? w : kAutoWindowFrom;
    return r->size > RIO_FILE_HEADER_BYTES + from ? w : 0;
}

// the next window of a streamed file becomes the reader's view
static int stream_fetch(rio_reader* r) {
    uint64_t first = 0;
    const uint8_t *o = nullptr, *fl = nullptr;
    const uint64_t *off = nullptr, *ro = nullptr;
    rio_file_info fi{};
    int rc = rio_stream_next(r->stream, &first, &o, &off, &ro, &fl, &fi);
    if (rc == RIO_EOF) rc = RIO_ERR_STATE;  // the last window was taken already (not reached: w_last)
    if (rc) return rc;
    r->w_out = o;
    r->w_off = off;
    r->w_flags = fl;
    r->w_n = fi.n_records;
    r->w_last = fi.status != RIO_OK;
    r->cursor = 0;
    r->info = fi;
    return RIO_OK;
}

static int file_decode(rio_reader* r) {
    if (r->decoded) return r->decode_rc;
    r->decoded = true;
    if (const uint64_t w = reader_window(r)) {
        int rc = rio_stream_open(r->ctx->device, r->path.c_str(), w, 4, &r->stream);
        if (!rc) rc = stream_fetch(r);
        // a file the device path does not decode is refused at its first window, as below
        if (!rc && r->info.status == RIO_ERR_UNSUPPORTED && r->w_n == 0) rc = RIO_ERR_UNSUPPORTED;
        return r->decode_rc = rc;
    }
    rio_file_info fi{};
    std::lock_guard<std::mutex> cg(r->ctx->mu);
    int rc = rio_frame(r->ctx, r->map, r->size, &fi);
    if (rc) return r->decode_rc = rc;
    if (fi.status == RIO_ERR_UNSUPPORTED) return r->decode_rc = RIO_ERR_UNSUPPORTED;
    r->out.resize(fi.total_out_bytes + 1);
    r->out_off.resize(fi.n_records + 1);
    r->rec_off.resize(fi.n_records + 1);
    r->flags.resize(fi.n_records + 1);
    rc = rio_decode(r->ctx, r->out.data(), fi.total_out_bytes, r->out_off.data(), r->rec_off.data(), r->flags.data(),
                    fi.n_records, &fi);
    if (rc) return r->decode_rc = rc;
    r->info = fi;
    r->w_out = r->out.data();
    r->w_off = r->out_off.data();
    r->w_flags = r->flags.data();
    r->w_n = fi.n_records;
    r->w_last = true;
    return r->decode_rc = RIO_OK;
}

// ReadNext / SkipNext (under the reader's lock): decode on first use, then position the view on the next record:
// `have` if there is one, else the view holds the terminal info
static int view_advance(rio_reader* r, bool& have) {
    if (!r->open || r->closed || r->mmap_mode) return RIO_ERR_STATE;
    if (int rc = file_decode(r)) return rc;
    if (r->past_end) return RIO_EOF;
    while (r->cursor >= r->w_n && !r->w_last) {
        const int rc = stream_fetch(r);
        if (rc) return rc;
    }
    have = r->cursor < r->w_n;
    return RIO_OK;
}

extern "C" int rio_reader_set_window(rio_reader* r, uint64_t window_bytes) {
    if (!r) return RIO_ERR_ARG;
    std::lock_guard<std::mutex> g(r->mu);
    if (r->decoded) return RIO_ERR_STATE;
    r->window = window_bytes;
    return RIO_OK;
}

extern "C" int rio_reader_file_info(rio_reader* r, rio_file_info* info) {
    if (!r || !info) return RIO_ERR_ARG;
    std::lock_guard<std::mutex> g(r->mu);
    if (!r->open || r->closed || r->mmap_mode) return RIO_ERR_STATE;
    int rc = file_decode(r);
    if (rc) return rc;
    if (r->stream) return RIO_ERR_STATE;  // windowed: the whole-file totals are not known up front
    *info = r->info;
    return RIO_OK;
}

// terminal status as ReadNext reports it
static int terminal(rio_reader* r) {
    tl_det.d0 = r->info.detail0;
    tl_det.d1 = r->info.detail1;
    tl_det.off = r->info.status_offset;
    return r->info.status;
}

extern "C" int rio_reader_read_next(rio_reader* r, const uint8_t** data, uint64_t* len, int* is_nil) {
    if (!r) return RIO_ERR_ARG;
    std::lock_guard<std::mutex> g(r->mu);
    if (data) *data = nullptr;
    if (len) *len = 0;
    if (is_nil) *is_nil = 0;
    bool have = false;
    if (int rc = view_advance(r, have)) return rc;
    if (!have) return terminal(r);
    const uint64_t i = r->cursor++;
    // a record whose payload does not decompress: ReadNext returns the codec error (or gzip's bare
    // io.EOF for an empty payload) and the next call goes on with the record after it
    if (r->w_flags[i] & (RIO_FLAG_CORRUPT | RIO_FLAG_EOF)) {
        tl_det.d0 = tl_det.d1 = 0;
        tl_det.off = r->info.status_offset;
        return (r->w_flags[i] & RIO_FLAG_EOF) ? RIO_EOF_CODEC : RIO_ERR_DECOMPRESS;
    }
    if (data) *data = r->w_out + r->w_off[i];
    if (len) *len = r->w_off[i + 1] - r->w_off[i];
    if (is_nil) *is_nil = (r->w_flags[i] & RIO_FLAG_NIL) ? 1 : 0;
    return RIO_OK;
}

// FileReader.SkipNext (file_reader.go:133-172): header parse + seek, no payload read, no
// zero-tail check. Divergence (documented): a nil record in a compressed file is skipped by its
// true extent, not by c bytes (the reference's :151-157 quirk).
extern "C" int rio_reader_skip_next(rio_reader* r) {
    if (!r) return RIO_ERR_ARG;
    std::lock_guard<std::mutex> g(r->mu);
    bool have = false;
    if (int rc = view_advance(r, have)) return rc;
    if (have) {
        r->cursor++;
        return RIO_OK;
    }
    const int s = terminal(r);
    switch (s) {
    case RIO_EOF_ZERO_TAIL: return RIO_ERR_MAGIC;  // SkipNext does not test for a zero tail
    case RIO_ERR_UNEXPECTED_EOF:  // detail0 == 1: raised by the payload read, else inside a header varint
        if (r->info.detail0 != 1) return s;
        [[fallthrough]];
    case RIO_EOF_PAYLOAD:  // header parsed fine: SkipNext seeks past the payload
        r->past_end = true;
        return RIO_OK;
    default: return s;
    }
}

// ---- ReadAtI (MMapReader.ReadNextAt / SeekNext, mmap_reader.go:58-203) -----------------------
// The file is decoded once (rio_frame + rio_decode on the reader's ctx) into a ReadAtIndex. A
// ReadNextAt at a record start, and a SeekNext whose scan meets only bytes that cannot form a marker
// before a record's header, are answered from it on the calling thread (binary search, no kernel, no
// lock). Everything else (offsets inside records or past the decoded sequence, scans over 0x91
// bytes) runs the single-record kernels (k_read_at / k_seek_next) under the reader's lock, exactly
// as before; for gzip files those kernels locate the record and the host serves the payload from the
// index when the offset is a record start.
// Largest decoded size (and record count) the index is built for: a file past it keeps n = 0 and
// every ReadNextAt / SeekNext takes the single-record kernels (no whole-file host copy, no
// first-call decode of a huge file). The framing's sizes are what the records claim, so a damaged
// header cannot make this allocate more than the cap. RIO_READAT_INDEX_MAX overrides (bytes).
static uint64_t readat_index_cap() {
    static const uint64_t cap = env_u64("RIO_READAT_INDEX_MAX", 4ull << 30);
    return cap;
}

static void build_readat_index(rio_reader* r, ReadAtIndex& x) {
    rio_ctx* ctx = r->ctx;
    std::lock_guard<std::mutex> cg(ctx->mu);
    rio_file_info fi{};
    if (rio_frame(ctx, r->map, r->size, &fi) != RIO_OK) return;
    const uint64_t n0 = fi.n_records;
    if (fi.total_out_bytes > readat_index_cap() || n0 > readat_index_cap() / 16) return;
    try {
        x.out.assign(fi.total_out_bytes + 1, 0);
        x.out_off.assign(n0 + 1, 0);
        x.rec_off.assign(n0 + 1, 0);
        x.flags.assign(n0 + 1, 0);
    } catch (const std::bad_alloc&) {  // never through the C-ABI: the kernels answer instead
        x = ReadAtIndex{};
        return;
    }
    if (rio_decode(ctx, x.out.data(), fi.total_out_bytes, x.out_off.data(), x.rec_off.data(), x.flags.data(), n0, &fi) !=
        RIO_OK)
        return;
    if (header_refused(fi.status)) return;
    const uint64_t n = std::min<uint64_t>(fi.n_records, n0);
    // the device file, record offsets and flags of the decode are still in the ctx arenas
    if (build_seek_map(ctx->host.file.as<uint8_t>(), r->size, ctx->host.rec_off.as<uint64_t>(),
                       ctx->host.flags.as<uint8_t>(), n, x.P, x.R, ctx->stream))
        return;
    x.n = n;  // published only complete: a failed build leaves n = 0 (every call takes the kernels)
}

static const ReadAtIndex* readat_index(rio_reader* r) {
    if (const ReadAtIndex* x = r->ix.load(std::memory_order_acquire)) return x;
    std::lock_guard<std::mutex> g(r->mu);
    if (const ReadAtIndex* x = r->ix.load(std::memory_order_relaxed)) return x;
    auto x = std::make_unique<ReadAtIndex>();
    if (r->open && !r->closed) build_readat_index(r, *x);
    r->ix.store(x.get(), std::memory_order_release);
    r->ix_own = std::move(x);
    return r->ix_own.get();
}

static int ensure_on_device(rio_reader* r) {
    if (r->on_device) return RIO_OK;
    HIP_TRY(hipSetDevice(r->ctx->device));
    HIP_TRY(r->dfile.ensure(r->size + RIO_DEVICE_PAD));
    int rc = h2d_staged(r->ctx, r->dfile.p, r->map, r->size);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(r->dfile.as<uint8_t>() + r->size, 0, RIO_DEVICE_PAD, r->ctx->stream));
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    r->on_device = true;
    return RIO_OK;
}

// record bytes of a kernel-path result: valid until this thread's next ReadNextAt / SeekNext
static thread_local std::vector<uint8_t> tl_rec;

// the single-record kernels (ReadNextAt at `offset`, or SeekNext scanning from it); *res_out gets the
// kernel's result (a gzip / lzw record it located but did not expand: payload_off, len)
static int readat_kernel(rio_reader* r, uint64_t offset, bool seek, uint64_t seek_len, uint64_t* ro_out,
                         const uint8_t** data, uint64_t* len, int* is_nil, ReadAtResult* res_out = nullptr) {
    std::lock_guard<std::mutex> g(r->mu);
    if (!r->open || r->closed) return RIO_ERR_STATE;
    std::lock_guard<std::mutex> cg(r->ctx->mu);
    int rc = ensure_on_device(r);
    if (rc) return rc;
    ReadAtResult res{};
    uint64_t ro = 0;
    rc = read_at_impl(r->ctx, r->dfile.as<uint8_t>(), r->size, offset, seek, seek_len, &res, seek ? &ro : nullptr);
    if (rc) return rc;
    if (ro_out) *ro_out = ro;
    if (res_out) *res_out = res;
    tl_det.d0 = res.det0;
    tl_det.d1 = res.det1;
    if (res.status != RIO_OK) return res.status;
    if (is_nil) *is_nil = res.nil;
    if (len) *len = res.nil ? 0 : res.len;
    tl_rec.resize(res.len + 1);
    if (!res.nil && res.len)
        HIP_TRY(hipMemcpy(tl_rec.data(), r->ctx->host.readat_out.p, res.len, hipMemcpyDeviceToHost));
    if (data) *data = tl_rec.data();
    return RIO_OK;
}

// A gzip / lzw record the whole-file decode never reached (MMapReader.ReadNextAt decodes any record
// start, mmap_reader.go:130-203, e.g. one after a header that fails its CRC, where FileReader stops):
// the single-record kernel located it (res: payload_off, len = payload bytes), and it is decoded here
// as a file of its own (the 8-byte file header, then the record's header and payload) through the
// whole-file path on the reader's context: the same inflate / lzw kernels, Go's multistream and size
// rules included. ReadNextAt's result for it: the record, or the codec's error class.
static thread_local std::vector<uint8_t> tl_x_out, tl_x_flags;
static thread_local std::vector<uint64_t> tl_x_off, tl_x_rec;
static int readat_expand(rio_reader* r, uint64_t rec, const ReadAtResult& res, const uint8_t** data, uint64_t* len,
                         int* is_nil) {
    const uint64_t end = res.payload_off + res.len;
    if (!r->map || res.nil || res.len == 0 || res.payload_off <= rec || end > r->size) return RIO_ERR_UNSUPPORTED;
    std::vector<uint8_t> img(RIO_FILE_HEADER_BYTES + (end - rec));
    memcpy(img.data(), r->map, RIO_FILE_HEADER_BYTES);
    memcpy(img.data() + RIO_FILE_HEADER_BYTES, r->map + rec, end - rec);
    std::lock_guard<std::mutex> g(r->mu);
    if (!r->open || r->closed) return RIO_ERR_STATE;
    std::lock_guard<std::mutex> cg(r->ctx->mu);
    rio_file_info fi{};
    int rc = rio_frame(r->ctx, img.data(), img.size(), &fi);
    if (rc) return rc;
    if (fi.n_records == 0) return RIO_ERR_UNSUPPORTED;  // (the kernel framed it: not reached)
    const uint64_t n = fi.n_records;
    // the sizes are what the (possibly damaged) headers claim: an lzw u may be 4096x its payload.
    // Bounded like the index (readat_index_cap), and an allocation failure is a status, never an
    // exception through the C-ABI
    if (fi.total_out_bytes > readat_index_cap() || n > readat_index_cap() / 16) return RIO_ERR_CAPACITY;
    try {
        tl_x_out.resize(fi.total_out_bytes + 1);
        tl_x_off.resize(n + 1);
        tl_x_rec.resize(n);
        tl_x_flags.resize(n);
    } catch (const std::exception&) {
        return RIO_ERR_CAPACITY;
    }
    rc = rio_decode(r->ctx, tl_x_out.data(), fi.total_out_bytes, tl_x_off.data(), tl_x_rec.data(), tl_x_flags.data(), n,
                    &fi);
    if (rc) return rc;
    if (fi.n_records == 0 || fi.status == RIO_ERR_UNSUPPORTED) return RIO_ERR_UNSUPPORTED;
    if (tl_x_flags[0] & RIO_FLAG_CORRUPT) return RIO_ERR_DECOMPRESS;
    if (tl_x_flags[0] & RIO_FLAG_EOF) return RIO_EOF_CODEC;
    if (is_nil) *is_nil = 0;
    if (len) *len = tl_x_off[1] - tl_x_off[0];
    if (data) *data = tl_x_out.data() + tl_x_off[0];
    return RIO_OK;
}

static int readat_check(rio_reader* r, const uint8_t** data, uint64_t* len, int* is_nil, bool seek) {
    if (data) *data = nullptr;
    if (len) *len = 0;
    if (is_nil) *is_nil = 0;
    if (!r->open || r->closed) return RIO_ERR_STATE;
    // SeekNext: "unsupported on files with version lower than v2" (mmap_reader.go:62-64)
    if (seek && r->version < RIO_VERSION2) return RIO_ERR_UNSUPPORTED;
    return RIO_OK;
}

extern "C" int rio_reader_read_next_at(rio_reader* r, uint64_t offset, const uint8_t** data, uint64_t* len,
                                       int* is_nil) {
    if (!r) return RIO_ERR_ARG;
    if (int rc = readat_check(r, data, len, is_nil, false)) return rc;
    tl_det = LastDetail{0, 0, offset};
    const ReadAtIndex* x = readat_index(r);
    const uint64_t i = x->find(offset);
    if (i < x->n) return x->record(i, data, len, is_nil);
    ReadAtResult res{};
    const int rc = readat_kernel(r, offset, false, 0, nullptr, data, len, is_nil, &res);
    const bool expand = r->compression == RIO_COMP_GZIP || r->compression == RIO_COMP_LZW;
    if (rc == RIO_ERR_UNSUPPORTED && expand) return readat_expand(r, offset, res, data, len, is_nil);
    return rc;
}

// ---- a batch of ReadNextAt calls (rio_reader_read_next_at_batch) ----------------------------------
// The queries that the reader's device copy of the file answers: one rio_device_read_at_plan / _copy pair under the
// reader's and the context's lock, the hits, offsets and bytes copied back through the context's staging. The output
// arena only grows; a batch that needs more than it holds comes back RIO_ERR_CAPACITY with its need in out_off[m]
// and runs once more.
static int batch_on_device(rio_reader* r, const std::vector<uint64_t>& offs, std::vector<rio_read_at_hit>& hits,
                           std::vector<uint64_t>& out_off, std::vector<uint8_t>& out) {
    const uint64_t m = offs.size();
    std::lock_guard<std::mutex> g(r->mu);
    if (!r->open || r->closed) return RIO_ERR_STATE;
    rio_ctx* ctx = r->ctx;
    std::lock_guard<std::mutex> cg(ctx->mu);
    int rc = ensure_on_device(r);
    if (rc) return rc;
    HIP_TRY(r->b_offsets.ensure(m * 8));
    HIP_TRY(r->b_hits.ensure(m * sizeof(rio_read_at_hit)));
    HIP_TRY(r->b_out_off.ensure((m + 1) * 8));
    if (r->b_out.cap == 0) HIP_TRY(r->b_out.ensure(1 << 20));
    if ((rc = h2d_staged(ctx, r->b_offsets.p, reinterpret_cast<const uint8_t*>(offs.data()), m * 8))) return rc;
    hits.resize(m);
    out_off.resize(m + 1);
    for (int attempt = 0; attempt < 2; attempt++) {
        rc = rio_device_read_at_plan(ctx, r->dfile.as<uint8_t>(), r->size, r->b_offsets.as<uint64_t>(), m,
                                     r->b_hits.as<rio_read_at_hit>(), r->b_out_off.as<uint64_t>(), nullptr);
        if (!rc)
            rc = rio_device_read_at_copy(ctx, r->dfile.as<uint8_t>(), r->size, m, r->b_hits.as<rio_read_at_hit>(),
                                         r->b_out_off.as<uint64_t>(), r->b_out.as<uint8_t>(), r->b_out.cap, nullptr);
        if (!rc) rc = d2h_staged(ctx, reinterpret_cast<uint8_t*>(out_off.data()), r->b_out_off.p, (m + 1) * 8);
        if (rc) return rc;
        if (out_off[m] <= r->b_out.cap) break;
        if (attempt) return RIO_ERR_CAPACITY;  // (the same file and offsets: not reached)
        HIP_TRY(r->b_out.ensure(out_off[m] + 16));
    }
    if ((rc = d2h_staged(ctx, reinterpret_cast<uint8_t*>(hits.data()), r->b_hits.p, m * sizeof(rio_read_at_hit)))) return rc;
    out.resize(out_off[m] + 1);
    return out_off[m] ? d2h_staged(ctx, out.data(), r->b_out.p, out_off[m]) : RIO_OK;
}

// the calling thread's last batch: what *data / *out_off point into, and the device path's results before they are
// merged with the index's and the expanded records
struct BatchResult {
    std::vector<uint8_t> data, dev_data, x_data;
    std::vector<uint64_t> off, dev_offsets, dev_off, x_off;
    std::vector<rio_read_at_hit> dev_hits;
    std::vector<uint64_t> dev_query;  // the query each device hit answers
    std::vector<uint64_t> x_query;    // the queries expanded one by one, in x_off's order
    std::vector<const uint8_t*> src;  // per query: its record's bytes (null: none)
};
static thread_local BatchResult tl_batch;

extern "C" int rio_reader_read_next_at_batch(rio_reader* r, const uint64_t* offsets, uint64_t n, rio_read_at_hit* hits,
                                             const uint8_t** data, const uint64_t** out_off) {
    if (!r || !data || !out_off || (n && (!offsets || !hits))) return RIO_ERR_ARG;
    *data = nullptr;
    *out_off = nullptr;
    if (n >= (1ull << 31) - 1) return RIO_ERR_UNSUPPORTED;
    if (!r->open || r->closed) return RIO_ERR_STATE;
    BatchResult& B = tl_batch;
    try {
        B.off.assign(n + 1, 0);
        B.src.assign(n, nullptr);
        B.dev_offsets.clear();
        B.dev_query.clear();
        B.x_data.clear();
        B.x_off.assign(1, 0);
        B.x_query.clear();
        // record starts of an index some earlier call built: from it, on this thread. The batch builds none
        const ReadAtIndex* x = r->ix.load(std::memory_order_acquire);
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t j = x && x->n ? x->find(offsets[i]) : 0;
            if (x && j < x->n) {
                rio_read_at_hit h{};
                int nil = 0;
                h.status = x->record(j, &B.src[i], &h.len, &nil);
                h.nil = nil;
                if (h.status != RIO_OK) B.src[i] = nullptr;
                hits[i] = h;
            } else {
                B.dev_offsets.push_back(offsets[i]);
                B.dev_query.push_back(i);
            }
        }
        const uint64_t m = B.dev_offsets.size();
        if (m) {
            if (int rc = batch_on_device(r, B.dev_offsets, B.dev_hits, B.dev_off, B.dev_data)) return rc;
            const bool expand = r->compression == RIO_COMP_GZIP || r->compression == RIO_COMP_LZW;
            for (uint64_t k = 0; k < m; k++) {
                const uint64_t i = B.dev_query[k];
                rio_read_at_hit h = B.dev_hits[k];
                if (h.status == RIO_OK && !h.nil) B.src[i] = B.dev_data.data() + B.dev_off[k];
                if (h.status == RIO_ERR_UNSUPPORTED && expand) {
                    // located, not expanded: as a file of its own, one record at a time (takes the locks itself)
                    ReadAtResult res{};
                    res.len = h.len;
                    res.payload_off = h.payload_off;
                    const uint8_t* d = nullptr;
                    uint64_t l = 0;
                    int nil = 0;
                    h.status = readat_expand(r, offsets[i], res, &d, &l, &nil);
                    h.len = h.status == RIO_OK ? l : 0;
                    if (h.status == RIO_OK) {
                        B.x_data.insert(B.x_data.end(), d, d + l);
                        B.x_off.push_back(B.x_data.size());
                        B.x_query.push_back(i);
                    }
                }
                hits[i] = h;
            }
            // expanded records were appended while x_data grew: their pointers now
            for (uint64_t t = 0; t < B.x_query.size(); t++) B.src[B.x_query[t]] = B.x_data.data() + B.x_off[t];
        }
        for (uint64_t i = 0; i < n; i++)
            B.off[i + 1] = B.off[i] + (hits[i].status == RIO_OK && !hits[i].nil ? hits[i].len : 0);
        if (m == n && B.off == B.dev_off) {
            B.data.swap(B.dev_data);  // every query answered on the device: its arena is the result as it stands
        } else {
            B.data.resize(B.off[n] + 1);
            for (uint64_t i = 0; i < n; i++)
                if (B.off[i + 1] > B.off[i]) memcpy(B.data.data() + B.off[i], B.src[i], B.off[i + 1] - B.off[i]);
        }
    } catch (const std::exception&) {  // an allocation failure is a status, never an exception through the C-ABI
        return RIO_ERR_CAPACITY;
    }
    *data = B.data.data();
    *out_off = B.off.data();
    return RIO_OK;
}

extern "C" int rio_reader_seek_next(rio_reader* r, uint64_t offset, uint64_t* rec_offset, const uint8_t** data,
                                    uint64_t* len, int* is_nil) {
    if (!r) return RIO_ERR_ARG;
    if (rec_offset) *rec_offset = 0;
    if (int rc = readat_check(r, data, len, is_nil, true)) return rc;
    tl_det = LastDetail{0, 0, offset};
    const uint64_t seek_len = r->seek_len.load(std::memory_order_relaxed);
    const ReadAtIndex* x = readat_index(r);
    uint64_t s = offset;  // the scan's position: a fresh SeekNext from s continues it exactly
    // with windows of >= 4 bytes the walk is fixed by the first 0x91 at or after s (build_seek_map).
    // Not at 3: mmap_reader.go:89-98 leaves the window once ix >= numRead, also right after the third
    // marker byte, so with seekLen 3 every marker ends the scan in io.EOF (k_seek_next reproduces it)
    if (seek_len >= 4 && s <= r->size && x->n) {
        const uint64_t k = (uint64_t)(std::lower_bound(x->P.begin(), x->P.end(), s) - x->P.begin());
        if (k < x->P.size() && x->R[k] < x->n) {  // else the single-record kernel answers (kSeekOther / io.EOF walks)
            const uint64_t i = x->R[k];
            if (rec_offset) *rec_offset = x->rec_off[i];
            tl_det.off = x->rec_off[i];
            return x->record(i, data, len, is_nil);
        }
    }
    for (;;) {
        uint64_t ro = 0;
        ReadAtResult res{};
        const int rc = readat_kernel(r, s, true, seek_len, &ro, data, len, is_nil, &res);
        if (rec_offset) *rec_offset = ro;
        tl_det.off = rc == RIO_ERR_INVALID_OFFSET ? offset : ro;
        // gzip / lzw: the kernel stops at a trial whose payload needs expanding; a record start is served
        // from the decoded index, any other record is expanded on its own (readat_expand); an io.EOF-class
        // trial (an empty gzip payload) continues the scan as mmap_reader.go:105-114 does
        const bool expand = r->compression == RIO_COMP_GZIP || r->compression == RIO_COMP_LZW;
        if (rc != RIO_ERR_UNSUPPORTED || !expand) return rc;
        const uint64_t i = x->find(ro);
        int rx;
        if (i < x->n) {
            rx = x->record(i, data, len, is_nil);
        } else {
            rx = readat_expand(r, ro, res, data, len, is_nil);
        }
        if (rx == RIO_EOF_CODEC) {
            s = ro + 3;
            continue;
        }
        return rx;
    }
}

extern "C" int rio_reader_index_info(rio_reader* r, struct rio_reader_index_info* info) {
    if (!r || !info) return RIO_ERR_ARG;
    *info = {};
    if (!r->open || r->closed || !r->mmap_mode) return RIO_ERR_STATE;
    const ReadAtIndex* x = readat_index(r);
    if (x->n == 0) return RIO_OK;  // not built: whatever a failed build left in P / R is not shown
    info->n_records = x->n;
    info->n_positions = x->P.size();
    info->positions = x->P.data();
    info->ends = x->R.data();
    return RIO_OK;
}

extern "C" int rio_reader_set_seek_len(rio_reader* r, uint64_t seek_len) {
    if (!r || seek_len == 0) return RIO_ERR_ARG;
    r->seek_len.store(seek_len, std::memory_order_relaxed);
    return RIO_OK;
}
