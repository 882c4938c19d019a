// rio_ctx.cpp — the context of librio's host runtime (include/rio.h): status strings, HIP contexts (device, stream,
// grow-only device arenas), the framing parameters of a file, stream ordering between the decode calls, and the
// pinned staging every host <-> device copy goes through. The state itself is declared in rio_ctx.h.
#include <algorithm>
#include <cstring>
#include <iterator>
#include <map>

#include "rio_ctx.h"
#include "rio_host.h"

using namespace rio;

// ------------------------------------------------------------------------------------------
// status helpers
// ------------------------------------------------------------------------------------------
extern "C" const char* rio_strerror(int s) {
    switch (s) {
    case RIO_OK: return "ok";
    case RIO_EOF: return "EOF";
    case RIO_EOF_ZERO_TAIL: return "EOF (zero-padded tail)";
    case RIO_EOF_HEADER: return "EOF inside record header";
    case RIO_EOF_PAYLOAD: return "EOF reading record payload";
    case RIO_ERR_UNEXPECTED_EOF: return "unexpected EOF";
    case RIO_ERR_MAGIC: return "magic number mismatch";
    case RIO_ERR_HEADER_CRC: return "header checksum mismatch";
    case RIO_ERR_VARINT_OVERFLOW: return "binary: varint overflows a 64-bit integer";
    case RIO_ERR_HEADER_TOO_LONG: return "checksum byte reader out of range";
    case RIO_ERR_DECOMPRESS: return "snappy: corrupt input";
    case RIO_ERR_VERSION: return "version mismatch";
    case RIO_ERR_COMPRESSION_TYPE: return "unknown compression type";
    case RIO_ERR_SHORT_FILE_HEADER: return "not enough bytes in the file header";
    case RIO_ERR_INVALID_OFFSET: return "mmap: invalid ReadAt offset";
    case RIO_ERR_UNSUPPORTED: return "not supported by the GPU decode path";
    case RIO_ERR_CAPACITY: return "output capacity too small";
    case RIO_ERR_ARG: return "invalid argument";
    case RIO_ERR_HIP: return "HIP runtime error";
    case RIO_ERR_STATE: return "reader state error";
    case RIO_ERR_IO: return "I/O error";
    case RIO_ERR_PROTO: return "proto: cannot parse invalid wire-format data";
    case RIO_EOF_CODEC: return "EOF from the codec (empty gzip payload)";
    default: return "unknown status";
    }
}

extern "C" int rio_status_is_eof(int s) {
    return s == RIO_EOF || s == RIO_EOF_ZERO_TAIL || s == RIO_EOF_HEADER || s == RIO_EOF_PAYLOAD || s == RIO_EOF_CODEC;
}

extern "C" const char* rio_build_info(void) { return "librio gfx950 recordio v3/v4 decode"; }

extern "C" uint64_t rio_max_records(uint64_t len) {
    return len <= RIO_FILE_HEADER_BYTES ? 1 : (len - RIO_FILE_HEADER_BYTES) / 5 + 1;  // v2's 5-byte empty record
}

// ------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------
// mean bytes per record for which the auto walk takes k_walk_lane (round 5 A/B on MI355X, 16 KiB lane chunks:
// 1 KiB incompressible records walk 0.269 -> 0.142 ms; 48-byte and 36 KiB records slower, so those keep k_walk)
constexpr uint64_t kLaneWalkMin = 768, kLaneWalkMax = 8192, kLaneWalkChunks = 32768;
// 512..767-byte records take the lane walk on files of kLaneWalkSmallChunks lane chunks and more. With three 8-byte slot
// stores per record C2's 561-byte records in 535 MiB measured even against the wave walk, and this was 65536
// (profiles/r5/r5be_lane_walk_min_ab.txt); with one 16-byte slot store per record the lane walk frames C2 0.025 ms faster
// (walk + scan + place 0.178 -> 0.153 ms, value 448.9 -> 463.5 GiB/s, medians of five alternated runs, lines "c2 parent" /
// "c2 new" of profiles/r7/r7b_slots_ab.txt), so the class takes it from the same file size as the larger records.
// Lane chunk: 16 KiB like theirs; 12 KiB framed another 0.010 ms faster with a value inside the run-to-run spread,
// 8 KiB and 24 KiB slower (lines "lane8k" / "lane12k" / "lane24k" there). RIO_LANE_WALK_MIN overrides kLaneWalkSmallMin.
// Measured again with the shorter hop of round 15 (lines "new@8192" / "new@12288" / "new@16384" of
// profiles/r15/r15a_lane_hops_ab.txt, two rounds): C2 464.1 / 467.0 / 470.8 GiB/s; the smaller chunks still walk faster
// (0.092 / 0.090 / 0.097 ms) and still give it back in the scan, the placement and the decoder, so 16 KiB and these
// thresholds stay. A chunk that is no power of two (16 656 bytes, the parent build, one run) walked 0.118 against 0.113 ms:
// the lanes' common 16 KiB stride is not what holds the walk.
constexpr uint64_t kLaneWalkSmallMin = 512, kLaneWalkSmallChunks = 32768;
// records of more than kLaneWalkMax bytes on average: wave-walk chunks of at least kBigRecordChunk (a 32 KiB chunk holds
// at most a few such records and the placement runs a wave per chunk with most lanes idle: C4 place 0.123 -> 0.076 ms,
// walk 0.61 -> 0.585, +1.2 %, profiles/r5/r5bl_c4_chunk_ab.txt); not when RIO_CHUNK_BYTES sets the size
constexpr uint64_t kBigRecordChunk = 65536;
// Small files walk smaller chunks: the smallest multiple of 4 KiB (the walk's fill round) whose chunk count fits one round
// of resident walk waves (CUs x 4 SIMDs x kWalkOcc, k_walk's launch bound in rio_device.h: 5 120 on MI355X), at least kSmallFileChunkMin; files
// that need more than one round at the default size keep it. A 32 MiB file's 1 024 default chunks were one wave per SIMD,
// each walking 32 KiB as a chain of dependent fill rounds; a chunk count just past one round runs a second round for a
// few waves (round 6 on MI355X: 32 MiB of 1 KiB records 0.117 -> 0.084 ms at 8 KiB chunks; 100 MB 0.171 -> 0.15 ms at
// 20 KiB (5 059 waves), against 16 KiB (6 100: two rounds) and 19 KiB (5 325); profiles/r6/r6j_small_file_chunks.txt)
constexpr uint64_t kSmallFileChunkMin = 8192;
static uint64_t wave_chunk_bytes(const rio_ctx* ctx, uint64_t len) {
    const uint64_t cb = ctx->fr.chunk_bytes;
    if (!ctx->fr.chunk_auto) return cb;
    const uint64_t slots = ctx->fr.walk_slots;
    const uint64_t want = ((len + slots - 1) / slots + 4095) & ~4095ull;
    return std::min(cb, std::max(want, kSmallFileChunkMin));
}

// bytes of a file's framing arenas at chunk size cb: scratch (the 16-byte slots) and meta
struct ArenaSizes {
    uint64_t n_chunks, slots, n_blocks, scratch, meta;
};
static ArenaSizes arena_sizes(uint64_t len, uint64_t cb) {
    ArenaSizes z;
    z.n_chunks = len > RIO_FILE_HEADER_BYTES ? (len - RIO_FILE_HEADER_BYTES + cb - 1) / cb : 0;
    z.slots = cb / 5 + 1;  // records starting in a chunk: the smallest is v2's 5 bytes
    z.n_blocks = (z.n_chunks + 255) / 256;
    const uint64_t nc = std::max<uint64_t>(z.n_chunks, 1), nb = std::max<uint64_t>(z.n_blocks, 1);
    z.scratch = nc * z.slots * sizeof(WalkSlot);
    auto al = [](uint64_t x) { return (x + 255) & ~255ull; };
    z.meta = al(sizeof(ScanState)) + al(sizeof(rio_file_info)) + 2 * al(nb * sizeof(RunSum)) +
             al(2 * kFailLanes * sizeof(uint64_t)) + al(nc * sizeof(ChunkSum)) + al(nc * sizeof(RunSum)) +
             al(nc * sizeof(ChunkPlace));
    return z;
}

// reserve_all: size the arenas for every chunk size the automatic walk choice can pick for a file of len bytes
// (wave chunks, lane chunks, big-record wave chunks), not only the one the current hint selects, so a later call
// whose hint flips the walk never grows an arena (rio_ctx_reserve's promise)
int rio::ctx_frame_params(rio_ctx* ctx, const uint8_t* d_file, uint64_t len, FrameParams& P, FileArenas& A,
                          bool reserve_all) {
    const rio_ctx::Framing& F = ctx->fr;
    memset(&P, 0, sizeof P);
    P.file = d_file;
    P.len = len;
    // the lane walk reads ~64 bytes per record and is latency-bound per lane; the wave walk reads every
    // byte (HBM-bound on records of ~1 KiB and more) and frames candidates 64 at a time (the better one for
    // small records, and for very large ones, whose chunks hold no header and the lane walk scans)
    // (and only with lanes to fill the chip: a file of fewer than kLaneWalkChunks lane chunks leaves the lane
    // walk's one-chain-per-lane latency exposed, C1's 103 MB: walk 0.076 -> 0.179 ms)
    bool lane = F.walk_mode == 1;
    if (F.walk_mode == 2 && F.walk_hint && len / F.lane_chunk_bytes >= kLaneWalkChunks) {
        const uint64_t m = *reinterpret_cast<volatile uint64_t*>(F.walk_hint);
        const uint64_t chunks = len / F.lane_chunk_bytes;
        lane = (m >= kLaneWalkMin && m <= kLaneWalkMax) ||
               (m >= F.lane_walk_min && m < kLaneWalkMin && chunks >= kLaneWalkSmallChunks);
    }
    uint64_t cb = lane ? F.lane_chunk_bytes : wave_chunk_bytes(ctx, len);
    if (!lane && F.chunk_auto && F.walk_hint && *reinterpret_cast<volatile uint64_t*>(F.walk_hint) > kLaneWalkMax)
        cb = std::max<uint64_t>(cb, kBigRecordChunk);
    P.walk_lane = lane ? 1u : 0u;
    P.walk_hint = F.walk_hint;
    P.chunk_bytes = cb;
    P.coop_min = F.coop_min;
    P.comp_hint = RIO_COMP_UNKNOWN;
    P.zero_done = 0;
    const ArenaSizes z = arena_sizes(len, cb);
    P.n_chunks = z.n_chunks;
    P.slots = z.slots;
    P.n_blocks = z.n_blocks;
    const uint64_t nc = std::max<uint64_t>(P.n_chunks, 1), nb = std::max<uint64_t>(P.n_blocks, 1);
    uint64_t scr = z.scratch, meta_need = z.meta;
    if (reserve_all) {
        for (uint64_t c : {wave_chunk_bytes(ctx, len), F.chunk_bytes, F.lane_chunk_bytes,
                           std::max<uint64_t>(F.chunk_bytes, kBigRecordChunk)}) {
            const ArenaSizes y = arena_sizes(len, c);
            scr = std::max(scr, y.scratch);
            meta_need = std::max(meta_need, y.meta);
        }
    }
    HIP_TRY(A.scratch.ensure(scr));
    auto al = [](uint64_t x) { return (x + 255) & ~255ull; };
    const uint64_t o_info = al(sizeof(ScanState)), o_brun = o_info + al(sizeof(rio_file_info));
    const uint64_t o_bexc = o_brun + al(nb * sizeof(RunSum)), o_fail = o_bexc + al(nb * sizeof(RunSum));
    const uint64_t o_chk = o_fail + al(2 * kFailLanes * sizeof(uint64_t)), o_cexc = o_chk + al(nc * sizeof(ChunkSum));
    const uint64_t o_place = o_cexc + al(nc * sizeof(RunSum)), meta_bytes = o_place + al(nc * sizeof(ChunkPlace));
    HIP_TRY(A.meta.ensure(std::max(meta_bytes, meta_need)));
    HIP_TRY(ctx->fr.sink.ensure(kSinkBytes));
    uint8_t* const mb = A.meta.as<uint8_t>();
    P.sink = F.sink.as<uint8_t>();
    P.fail_lanes = reinterpret_cast<uint64_t*>(mb + o_fail);
    P.scratch = A.scratch.as<WalkSlot>();
    P.chunks = reinterpret_cast<ChunkSum*>(mb + o_chk);
    P.chunk_excl = reinterpret_cast<RunSum*>(mb + o_cexc);
    P.place = reinterpret_cast<ChunkPlace*>(mb + o_place);
    P.block_runs = reinterpret_cast<RunSum*>(mb + o_brun);
    P.block_excl = reinterpret_cast<RunSum*>(mb + o_bexc);
    P.state = reinterpret_cast<ScanState*>(mb);
    P.info = reinterpret_cast<rio_file_info*>(mb + o_info);
    return RIO_OK;
}

extern "C" int rio_device_count(int* out) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    if (out) *out = n;
    return n > 0 ? RIO_OK : RIO_ERR_HIP;
}

extern "C" int rio_ctx_create(int device, rio_ctx** out) {
    if (!out) return RIO_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return RIO_ERR_HIP;
    if (device < 0 || device >= n) return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(device));
    auto* c = new rio_ctx();
    rio_ctx::Framing& F = c->fr;
    c->device = device;
    F.chunk_bytes = env_u64("RIO_CHUNK_BYTES", 32768);
    F.chunk_auto = std::getenv("RIO_CHUNK_BYTES") == nullptr;
    // k_walk's candidate bounds take 32-bit differences inside a chunk (magic_mask): chunks stay below
    // 1 GiB, and a walked record's slot holds its offset inside its chunk in 30 bits; anything outside
    // [64, 1 GiB] or not a multiple of 16 falls back to the default
    static_assert(kMaxChunkBytes == 1ull << 30 && kMaxChunkBytes <= 1ull << kSlotOffBits,
                  "the chunk cap bounds WalkSlot's chunk-relative offsets and k_walk's 32-bit differences");
    if (F.chunk_bytes < 64 || F.chunk_bytes > kMaxChunkBytes || (F.chunk_bytes & 15)) F.chunk_bytes = 32768;
    F.walk_mode = (uint32_t)std::min<uint64_t>(env_u64("RIO_WALK_LANE", 2), 2);
    F.lane_chunk_bytes = env_u64("RIO_LANE_CHUNK_BYTES", 16384);
    F.lane_walk_min = env_u64("RIO_LANE_WALK_MIN", kLaneWalkSmallMin);
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
        F.walk_slots = (uint64_t)cus * 4 * kWalkOcc;
    if (F.lane_chunk_bytes < 64 || F.lane_chunk_bytes > kMaxChunkBytes || (F.lane_chunk_bytes & 15))
        F.lane_chunk_bytes = 16384;
    if (hipHostMalloc(reinterpret_cast<void**>(&F.walk_hint), sizeof(uint64_t), hipHostMallocPortable) != hipSuccess) {
        (void)hipGetLastError();
        F.walk_hint = nullptr;  // no hint: the wave walk
    } else {
        *F.walk_hint = 0;
    }
    F.coop_min = env_u64("RIO_COOP_MIN", ~0ull >> 8);  // k_snappy_coop: wide files only
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return RIO_ERR_HIP;
    }
    // no stage events until rio_ctx_set_timing asks for them: the five timing events of a call cost a C2 step
    // 1.5 % and a C1-size step 13 % (profiles/r5/r5az_event_cost.txt)
    c->timing.set_ring(0);
    *out = c;
    return RIO_OK;
}

extern "C" int rio_ctx_device(const rio_ctx* c) { return c ? c->device : -1; }

// The synchronisations stand here, before the delete: the destructors behind it only free (rio_ctx.h).
extern "C" void rio_ctx_destroy(rio_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    if (c->order.ev) hipEventSynchronize(c->order.ev);  // the last device-API call may have run on a caller's stream
    c->mrg.views.wait();                                // the last plan's view copy reads its host vector
    c->wal.segs.wait();                                 // the last plan's segment copy reads its host vector
    delete c;
}

// slots == 0 disables stage events; slots == n keeps the events of the last n decodes
extern "C" int rio_ctx_set_timing(rio_ctx* c, int slots) {
    if (!c || slots < 0) return RIO_ERR_ARG;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    c->timing.set_ring((size_t)slots);
    return RIO_OK;
}

// Mean per-stage device milliseconds over the decodes recorded in the ring:
// [0] header + walk, [1] scan + zero-tail check, [2] placement, [3] decode kernels.
extern "C" int rio_ctx_last_stage_ms(rio_ctx* c, float* ms, int n) {
    if (!c || !ms || c->timing.ring.empty() || c->timing.cursor == 0) return 0;
    const uint64_t used = std::min<uint64_t>(c->timing.cursor, c->timing.ring.size());
    double acc[4] = {0, 0, 0, 0};
    for (uint64_t s = 0; s < used; s++) {
        auto& e = c->timing.ring[s];
        hipEventSynchronize(e[4]);
        for (int k = 0; k < 4; k++) {
            float v = 0;
            hipEventElapsedTime(&v, e[k], e[k + 1]);
            acc[k] += v;
        }
    }
    int k = std::min(n, 4);
    for (int i = 0; i < k; i++) ms[i] = (float)(acc[i] / (double)used);
    return k;
}

// ------------------------------------------------------------------------------------------
// stream ordering of the decode calls
// ------------------------------------------------------------------------------------------
// The decode calls of one ctx use the same scratch arenas: a call on a stream other than the
// previous call's waits for that call first (stream-ordered, no host synchronisation).
int rio::order_before(rio_ctx* ctx, hipStream_t s) {
    if (ctx->order.valid && ctx->order.stream != s) HIP_TRY(hipStreamWaitEvent(s, ctx->order.ev, 0));
    return RIO_OK;
}
// the device-resident calls hand the order event to their last kernel (k_finish) as its completion event instead
// of recording it behind the call: no marker packet between this call and the next (profiles/r5/r5bi_order_event_ab.txt)
int rio::order_event(rio_ctx* ctx, hipEvent_t& e) {
    if (!ctx->order.ev) HIP_TRY(hipEventCreateWithFlags(&ctx->order.ev, hipEventDisableTiming));
    e = ctx->order.ev;
    return RIO_OK;
}
void rio::order_mark(rio_ctx* ctx, hipStream_t s) {
    ctx->order.stream = s;
    ctx->order.valid = true;
}
int rio::order_after(rio_ctx* ctx, hipStream_t s) {
    hipEvent_t e;
    if (int rc = order_event(ctx, e)) return rc;
    HIP_TRY(hipEventRecord(e, s));
    order_mark(ctx, s);
    return RIO_OK;
}

extern "C" int rio_ctx_reserve(rio_ctx* ctx, uint64_t max_file_len, uint64_t max_records, uint32_t max_batch) {
    if (!ctx || max_batch > kMaxBatch) return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    FrameParams P;
    if (int rc = ctx_frame_params(ctx, nullptr, max_file_len, P, ctx->fr.fa, true)) return rc;
    HIP_TRY(ctx->fr.fa.rec_pay.ensure((max_records + 1) * 8));
    HIP_TRY(ctx->fr.fa.rec_desc.ensure((max_records + 1) * 16));
    while (ctx->fr.batch.size() < max_batch) ctx->fr.batch.emplace_back(new FileArenas());
    for (uint32_t j = 0; j < max_batch; j++) {
        FileArenas& A = *ctx->fr.batch[j];
        if (int rc = ctx_frame_params(ctx, nullptr, max_file_len, P, A, true)) return rc;
        HIP_TRY(A.rec_pay.ensure((max_records + 1) * 8));
        HIP_TRY(A.rec_desc.ensure((max_records + 1) * 16));
    }
    hipEvent_t e;
    return order_event(ctx, e);
}
extern "C" uint64_t rio_ctx_arena_bytes(const rio_ctx* ctx) {
    if (!ctx) return 0;
    uint64_t t = ctx->fr.sink.cap + ctx->fr.fa.bytes();
    for (auto& a : ctx->fr.batch) t += a->bytes();
    return t;
}

// ------------------------------------------------------------------------------------------
// pinned staging and the page-lock registry
// ------------------------------------------------------------------------------------------
constexpr size_t kStage = 32ull << 20;  // pinned staging piece

static int ensure_pinned(rio_ctx* c) {
    for (int i = 0; i < 2; i++) {
        if (!c->stage.pinned[i]) {
            HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->stage.pinned[i]), kStage, hipHostMallocDefault));
            HIP_TRY(hipEventCreateWithFlags(&c->stage.ev[i], hipEventDisableTiming));
        }
    }
    return RIO_OK;
}

// Page-locked host ranges this library knows: rio_host_register's ranges and PinnedPool's
// blocks, base -> bytes. A DMA straight from host memory needs ALL of [p, p + n) page-locked; a
// pointer attribute only describes p itself.
namespace {
std::mutex g_pin_mu;
std::map<uintptr_t, uint64_t> g_pin;
bool pinned_known(uintptr_t a, uint64_t n) {
    std::lock_guard<std::mutex> g(g_pin_mu);
    auto it = g_pin.upper_bound(a);
    if (it == g_pin.begin()) return false;
    --it;
    return a >= it->first && a - it->first <= it->second && n <= it->second - (a - it->first);
}
}  // namespace
void rio::note_pinned(const void* p, uint64_t n) {
    std::lock_guard<std::mutex> g(g_pin_mu);
    g_pin[reinterpret_cast<uintptr_t>(p)] = n;
}
void rio::forget_pinned(const void* p) {
    std::lock_guard<std::mutex> g(g_pin_mu);
    g_pin.erase(reinterpret_cast<uintptr_t>(p));
}

// true when all of [p, p + n) is page-locked host memory: a range this library registered or
// allocated, or one allocation HIP reports (hipHostMalloc / hipHostRegister by the caller) that
// covers the whole range. The copy then goes by DMA directly, without the staging pieces; anything
// else (a partly registered image, a range running past its registration) takes the staging path.
// The probes' errors on pageable memory are cleared so a later hipGetLastError (kernel launch
// check) does not see them.
bool rio::is_host_pinned(const void* p, uint64_t n) {
    if (!p || n < (1u << 20)) return false;  // small copies: staging costs nothing
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    hipPointerAttribute_t at{};
    bool ok = hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost;
    // the registry covers whole ranges the library locked itself, but only while HIP still reports the memory
    // page-locked: a range the caller unregistered with hipHostUnregister directly (or freed) is forgotten here
    // instead of being taken for DMA-able memory
    if (pinned_known(a, n)) {
        (void)hipGetLastError();
        if (ok) return true;
        std::lock_guard<std::mutex> g(g_pin_mu);
        auto it = g_pin.upper_bound(a);
        if (it != g_pin.begin()) g_pin.erase(std::prev(it));
        return false;
    }
    if (ok) {
        void* base = nullptr;
        size_t sz = 0;
        ok = hipMemGetAddressRange(&base, &sz, const_cast<void*>(p)) == hipSuccess && base &&
             reinterpret_cast<uintptr_t>(base) <= a && a - reinterpret_cast<uintptr_t>(base) <= sz &&
             n <= sz - (a - reinterpret_cast<uintptr_t>(base));
    }
    (void)hipGetLastError();
    return ok;
}

// pageable host -> device through two pinned staging pieces (copy of piece k+1 overlaps the DMA
// of piece k): h2d_fill with the host pool's copy as the producer; pinned sources go directly
static int fill_from_host(void* src, uint8_t* dst, uint64_t off, uint64_t n) {
    HostPool::get().copy(dst, static_cast<const uint8_t*>(src) + off, n);
    return RIO_OK;
}
int rio::h2d_staged(rio_ctx* c, void* dst, const uint8_t* src, uint64_t n) {
    if (is_host_pinned(src, n)) return hip_status(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, c->stream));
    return h2d_fill(c, dst, n, fill_from_host, const_cast<uint8_t*>(src));
}

// device -> pageable host through pinned staging (the DMA of piece k+1 overlaps the copy out of piece k);
// pinned destinations directly
int rio::d2h_staged(rio_ctx* c, uint8_t* dst, const void* src, uint64_t n) {
    if (is_host_pinned(dst, n)) {
        HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, c->stream));
        return hip_status(hipStreamSynchronize(c->stream));
    }
    int rc = ensure_pinned(c);
    if (rc) return rc;
    uint64_t o = 0, prev_o = 0, prev_m = 0;
    for (int k = 0; o < n || prev_m; k ^= 1) {  // one more round than pieces: the last piece's copy out
        const uint64_t m = std::min<uint64_t>(kStage, n - o);
        if (m) {
            HIP_TRY(hipEventSynchronize(c->stage.ev[k]));
            HIP_TRY(hipMemcpyAsync(c->stage.pinned[k], static_cast<const uint8_t*>(src) + o, m, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipEventRecord(c->stage.ev[k], c->stream));
        }
        if (prev_m) {
            HIP_TRY(hipEventSynchronize(c->stage.ev[k ^ 1]));
            HostPool::get().copy(dst + prev_o, c->stage.pinned[k ^ 1], prev_m);
        }
        prev_o = o;
        prev_m = m;
        o += m;
    }
    return RIO_OK;
}

// host producer -> device through the two pinned staging pieces: producing piece k+1 overlaps
// the DMA of piece k (the pieces are filled in order)
int rio::h2d_fill(rio_ctx* c, void* dst, uint64_t n, FillFn fill, void* user) {
    int rc = ensure_pinned(c);
    if (rc) return rc;
    uint64_t o = 0;
    int k = 0;
    while (o < n) {
        const uint64_t m = std::min<uint64_t>(kStage, n - o);
        HIP_TRY(hipEventSynchronize(c->stage.ev[k]));
        if ((rc = fill(user, c->stage.pinned[k], o, m))) {
            (void)hipStreamSynchronize(c->stream);  // the other piece's DMA may still read staging
            return rc;
        }
        HIP_TRY(hipMemcpyAsync(static_cast<uint8_t*>(dst) + o, c->stage.pinned[k], m, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipEventRecord(c->stage.ev[k], c->stream));
        o += m;
        k ^= 1;
    }
    return RIO_OK;
}

// page-lock a caller's host buffer (a file image it reuses): the H2D of rio_frame / rio_stream_open_host
// then reads it by DMA in place instead of through the staging pieces
extern "C" int rio_host_register(const void* p, uint64_t n) {
    if (!p || !n) return RIO_ERR_ARG;
    HIP_TRY(hipHostRegister(const_cast<void*>(p), n, hipHostRegisterDefault));
    rio::note_pinned(p, n);
    return RIO_OK;
}
extern "C" int rio_host_unregister(const void* p) {
    if (!p) return RIO_ERR_ARG;
    rio::forget_pinned(p);
    HIP_TRY(hipHostUnregister(const_cast<void*>(p)));
    return RIO_OK;
}
