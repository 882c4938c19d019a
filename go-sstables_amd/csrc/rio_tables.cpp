// rio_tables.cpp — the SSTable entry points of librio (include/rio.h): index parse and value validation, the
// host-memory table handle, and what writes a table on the device: merge-compaction, bloom filters and point
// lookups, the memstore flush and the WAL ops.
//
// In every entry point of merge, bloom, flush and WAL ops all argument checks stand before the first read of *ctx:
// a call refused on its arguments touches neither the context nor the device. tests/test_compact_host.py,
// tests/test_bloom_host.py, tests/test_memstore_host.py and tests/test_wal_mutation_host.py make such calls on a
// machine without a GPU, where no context can be created, and pass a placeholder for ctx. Keep that order; where
// checks also follow it, a marker says where the first read of *ctx stands.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rio_ctx.h"

using namespace rio;

// ------------------------------------------------------------------------------------------
// sstables: index parse + value validation on decoded arenas (rio_sstable.hip)
// ------------------------------------------------------------------------------------------
extern "C" int rio_sst_index_parse(rio_ctx* ctx, const uint8_t* d_index_out, const uint64_t* d_index_off, uint64_t n,
                                   uint64_t* d_key_off, uint64_t* d_key_len, uint64_t* d_value_off,
                                   uint64_t* d_checksum, uint64_t* d_result, void* stream) {
    if (!ctx || !d_index_off || !d_result || (n && (!d_index_out || !d_key_off || !d_key_len || !d_value_off || !d_checksum)))
        return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    return hip_status(launch_sst_index(d_index_out, d_index_off, n, d_key_off, d_key_len, d_value_off, d_checksum,
                                       d_result, stream_of(ctx, stream)));
}

extern "C" int rio_sst_validate(rio_ctx* ctx, const uint8_t* d_data_out, const uint64_t* d_data_off,
                                const uint64_t* d_data_rec_off, uint64_t n_data, const uint64_t* d_value_off,
                                const uint64_t* d_checksum, uint64_t n_index, uint64_t* d_crc_out, uint64_t* d_result,
                                void* stream) {
    if (!ctx || !d_result || (n_index && (!d_value_off || !d_checksum || !d_crc_out || !d_data_off || !d_data_rec_off)))
        return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    return hip_status(launch_sst_validate(d_data_out, d_data_off, d_data_rec_off, n_data, d_value_off, d_checksum,
                                          n_index, d_crc_out, d_result, stream_of(ctx, stream)));
}

extern "C" int rio_sst_data_entries(rio_ctx* ctx, const uint8_t* d_data_out, const uint64_t* d_data_off, uint64_t n_data,
                                    uint64_t* d_view, uint64_t* d_result, void* stream) {
    if (!ctx || !d_data_off || !d_result || (n_data && (!d_data_out || !d_view))) return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    return hip_status(launch_sst_data_entry(d_data_out, d_data_off, n_data, d_view, d_result, stream_of(ctx, stream)));
}

extern "C" int rio_sst_validate_view(rio_ctx* ctx, const uint8_t* d_data_out, const uint64_t* d_data_off,
                                     const uint64_t* d_data_rec_off, uint64_t n_data, const uint64_t* d_view,
                                     const uint64_t* d_value_off, const uint64_t* d_checksum, uint64_t n_index,
                                     uint64_t* d_crc_out, uint64_t* d_result, void* stream) {
    if (!ctx || !d_result ||
        (n_index && (!d_value_off || !d_checksum || !d_crc_out || !d_data_off || !d_data_rec_off || !d_view)))
        return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    return hip_status(launch_sst_validate(d_data_out, d_data_off, d_data_rec_off, n_data, d_value_off, d_checksum,
                                          n_index, d_crc_out, d_result, stream_of(ctx, stream), d_view));
}

// ------------------------------------------------------------------------------------------
// sstables: merge-compaction of loaded tables (rio_compact.hip)
// ------------------------------------------------------------------------------------------
extern "C" uint64_t rio_index_entry_len(uint64_t key_len, uint64_t value_offset, uint64_t checksum) {
    return pb_index_entry_len(key_len, value_offset, checksum);
}

extern "C" uint64_t rio_index_entries_bound(uint64_t n, uint64_t key_bytes) {
    // per entry: three tags, the key length (< 2^40: at most 6 bytes) and two 10-byte varints
    return key_bytes + 29 * n + 64;
}

extern "C" int rio_sst_merge_plan(rio_ctx* ctx, const rio_sst_view* views, uint32_t n_tables, uint32_t mode,
                                  uint64_t* d_src, uint8_t* d_keep, uint64_t* d_result, void* stream) {
    if (!ctx || !views || !d_result || n_tables == 0 || n_tables > RIO_MERGE_MAX_TABLES ||
        mode > RIO_MERGE_LATEST_WINS_SKIP_TOMBSTONES)
        return RIO_ERR_ARG;
    static_assert(sizeof(rio_sst_view) % 8 == 0, "views and bases share one uint64 buffer");
    const size_t vw = sizeof(rio_sst_view) / 8 * n_tables;
    std::vector<uint64_t> host(vw + n_tables + 1);
    memcpy(host.data(), views, vw * 8);
    uint64_t N = 0;
    for (uint32_t t = 0; t < n_tables; t++) {
        const rio_sst_view& v = views[t];
        if (v.n && (!v.index || !v.key_off || !v.key_len || !v.data_off || !v.flags || !v.crc)) return RIO_ERR_ARG;
        if (v.n >> RIO_MERGE_ENTRY_BITS) return RIO_ERR_UNSUPPORTED;
        host[vw + t] = N;
        N += v.n;
    }
    host[vw + n_tables] = N;
    if (N >= (1ull << 31) - 1) return RIO_ERR_UNSUPPORTED;
    if (N && (!d_src || !d_keep)) return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    rio_ctx::Merge& M = ctx->mrg;
    M.planned = false;
    HIP_TRY(M.views.dev.ensure(host.size() * 8));
    HIP_TRY(M.pfx.ensure(N * 8 + 8));
    HIP_TRY(M.tmp.ensure(N * 8 + 8));
    HIP_TRY(M.opos.ensure(N * 8 + 8));
    HIP_TRY(M.cub.ensure(std::max<size_t>(scan_cub_bytes(N), 256)));
    hipStream_t s = stream_of(ctx, stream);
    HIP_TRY(M.views.upload(host, s));
    MergeParams P{};
    P.views = M.views.dev.as<rio_sst_view>();
    P.base = M.views.dev.as<uint64_t>() + vw;
    P.T = n_tables;
    P.mode = mode;
    P.N = N;
    P.pfx = M.pfx.as<uint64_t>();
    P.src = d_src;
    P.keep = d_keep;
    P.result = d_result;
    HIP_TRY(launch_merge_plan(P, s));
    M.T = n_tables;
    M.N = N;
    M.planned = true;
    return RIO_OK;
}

extern "C" int rio_sst_merge_gather(rio_ctx* ctx, const uint64_t* d_src, const uint8_t* d_keep, uint64_t n_out,
                                    uint64_t* d_out_src, uint8_t* d_values, uint64_t values_cap, uint64_t* d_val_off,
                                    uint8_t* d_val_flags, void* stream) {
    if (!ctx || !d_val_off || !d_values || (n_out && (!d_out_src || !d_val_flags))) return RIO_ERR_ARG;
    // from here on *ctx is read
    const rio_ctx::Merge& M = ctx->mrg;
    if (!M.planned) return RIO_ERR_STATE;
    if (n_out > M.N || (M.N && (!d_src || !d_keep))) return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    GatherParams P{};
    P.views = M.views.dev.as<rio_sst_view>();
    P.T = M.T;
    P.N = M.N;
    P.n_out = n_out;
    P.src = d_src;
    P.keep = d_keep;
    P.tmp = M.tmp.as<uint64_t>();
    P.opos = M.opos.as<uint64_t>();
    P.out_src = d_out_src;
    P.values = d_values;
    P.values_cap = values_cap;
    P.val_off = d_val_off;
    P.val_flags = d_val_flags;
    return hip_status(launch_merge_gather(P, M.cub.p, M.cub.cap, stream_of(ctx, stream)));
}

extern "C" int rio_sst_index_encode(rio_ctx* ctx, const uint64_t* d_out_src, const uint64_t* d_value_file_off,
                                    uint64_t n_out, uint8_t* d_entries, uint64_t entries_cap, uint64_t* d_ent_off,
                                    void* stream) {
    if (!ctx || !d_ent_off || !d_entries || (n_out && (!d_out_src || !d_value_file_off))) return RIO_ERR_ARG;
    // from here on *ctx is read
    const rio_ctx::Merge& M = ctx->mrg;
    if (!M.planned) return RIO_ERR_STATE;
    if (n_out > M.N) return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    EntryParams P{};
    P.views = M.views.dev.as<rio_sst_view>();
    P.T = M.T;
    P.n_out = n_out;
    P.out_src = d_out_src;
    P.file_off = d_value_file_off;
    P.tmp = M.tmp.as<uint64_t>();
    P.entries = d_entries;
    P.entries_cap = entries_cap;
    P.ent_off = d_ent_off;
    return hip_status(launch_index_entries(P, M.cub.p, M.cub.cap, stream_of(ctx, stream)));
}

// ------------------------------------------------------------------------------------------
// bloom filters and point lookups of a loaded table (rio_bloom.hip)
// ------------------------------------------------------------------------------------------
// bloomfilter.NewOptimal (OptimalM / OptimalK): sstable_writer.go:79 sizes every table's filter with it
extern "C" int rio_bloom_optimal(uint64_t max_n, double p, uint64_t* m, uint64_t* k) {
    if (!m || !k || max_n == 0 || !(p > 0.0 && p < 1.0)) return RIO_ERR_ARG;
    const double ln2 = 0.693147180559945309417232121458176568;  // Go's math.Ln2
    const double dm = std::ceil(-(double)max_n * std::log(p) / (ln2 * ln2));
    if (!(dm < 18446744073709551616.0)) return RIO_ERR_ARG;
    *m = (uint64_t)dm;
    *k = (uint64_t)std::ceil(ln2 * (double)*m / (double)max_n);
    return RIO_OK;
}

static bool bloom_view_ok(const rio_bloom_view* f) {
    return f && f->k >= 1 && f->k <= RIO_BLOOM_MAX_K && f->m >= 2;
}

// n keys against filter f (null: no gate, bits stays null)
static BloomParams bloom_keys(const rio_bloom_view* f, const uint8_t* d_keys, const uint64_t* d_key_off, uint64_t n,
                              uint64_t key_bytes) {
    BloomParams P{};
    if (f) P.f = *f;
    P.keys = d_keys;
    P.key_off = d_key_off;
    P.n = n;
    P.key_bytes = key_bytes;
    return P;
}

extern "C" int rio_bloom_add(rio_ctx* ctx, const rio_bloom_view* f, const uint8_t* d_keys, const uint64_t* d_key_off,
                             uint64_t n, uint64_t key_bytes, void* stream) {
    if (!ctx || !bloom_view_ok(f)) return RIO_ERR_ARG;
    if (n == 0) return RIO_OK;
    if (!f->bits || !f->hash_keys || !d_keys || !d_key_off) return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    return hip_status(launch_bloom_add(bloom_keys(f, d_keys, d_key_off, n, key_bytes), false, stream_of(ctx, stream)));
}

extern "C" int rio_sst_bloom_add(rio_ctx* ctx, const rio_bloom_view* f, const uint64_t* d_out_src, uint64_t n_out,
                                 void* stream) {
    if (!ctx || !bloom_view_ok(f) || (n_out && (!f->bits || !f->hash_keys || !d_out_src))) return RIO_ERR_ARG;
    // from here on *ctx is read
    const rio_ctx::Merge& M = ctx->mrg;
    if (!M.planned) return RIO_ERR_STATE;
    if (n_out > M.N) return RIO_ERR_ARG;
    if (n_out == 0) return RIO_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    BloomParams P{};
    P.f = *f;
    P.n = n_out;
    P.views = M.views.dev.as<rio_sst_view>();
    P.T = M.T;
    P.out_src = d_out_src;
    return hip_status(launch_bloom_add(P, true, stream_of(ctx, stream)));
}

extern "C" int rio_bloom_contains(rio_ctx* ctx, const rio_bloom_view* f, const uint8_t* d_keys, const uint64_t* d_key_off,
                                  uint64_t n, uint64_t key_bytes, uint8_t* d_hit, void* stream) {
    if (!ctx || !bloom_view_ok(f)) return RIO_ERR_ARG;
    if (n == 0) return RIO_OK;
    if (!f->bits || !f->hash_keys || !d_keys || !d_key_off || !d_hit) return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    BloomParams P = bloom_keys(f, d_keys, d_key_off, n, key_bytes);
    P.hit = d_hit;
    return hip_status(launch_bloom_contains(P, stream_of(ctx, stream)));
}

extern "C" int rio_sst_key_prefixes(rio_ctx* ctx, const rio_sst_view* view, uint64_t* d_pfx, void* stream) {
    if (!ctx || !view) return RIO_ERR_ARG;
    if (view->n == 0) return RIO_OK;
    if (!d_pfx || !view->index || !view->key_off || !view->key_len) return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    return hip_status(launch_sst_key_prefixes(*view, d_pfx, stream_of(ctx, stream)));
}

extern "C" int rio_sst_lookup(rio_ctx* ctx, const rio_sst_view* view, const uint64_t* d_pfx, const rio_bloom_view* f,
                              const uint8_t* d_keys, const uint64_t* d_key_off, uint64_t n, uint64_t key_bytes,
                              uint64_t* d_entry, void* stream) {
    if (!ctx || !view || (f && !bloom_view_ok(f))) return RIO_ERR_ARG;
    if (n == 0) return RIO_OK;
    if (!d_keys || !d_key_off || !d_entry || (f && (!f->bits || !f->hash_keys)) ||
        (view->n && (!d_pfx || !view->index || !view->key_off || !view->key_len)))
        return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    LookupParams Q{};
    Q.v = *view;
    Q.pfx = d_pfx;
    Q.entry = d_entry;
    return hip_status(launch_sst_lookup(bloom_keys(f, d_keys, d_key_off, n, key_bytes), Q, stream_of(ctx, stream)));
}

// ------------------------------------------------------------------------------------------
// memstore flush: order an op log and keep the latest op of every key (rio_flush.hip)
// ------------------------------------------------------------------------------------------
extern "C" int rio_sst_flush_plan(rio_ctx* ctx, const rio_ops_view* ops, uint32_t mode, uint32_t max_key_len,
                                  uint64_t* d_src, uint8_t* d_keep, uint64_t* d_result, void* stream) {
    if (!ctx || !ops || !d_result || mode > RIO_FLUSH_SKIP_TOMBSTONES) return RIO_ERR_ARG;
    const uint64_t n = ops->n;
    if (n && (!ops->keys || !ops->key_off || !ops->values || !ops->val_off || !ops->flags || !d_src || !d_keep))
        return RIO_ERR_ARG;
    if (n >= (1ull << 31) - 1 || max_key_len > RIO_FLUSH_MAX_KEY_LEN) return RIO_ERR_UNSUPPORTED;
    return flush_plan(ctx, ops, mode, max_key_len, d_src, d_keep, d_result, stream, true);
}

int rio::flush_plan(rio_ctx* ctx, const rio_ops_view* ops, uint32_t mode, uint32_t max_key_len, uint64_t* d_src,
                    uint8_t* d_keep, uint64_t* d_result, void* stream, bool with_crc) {
    const uint64_t n = ops->n;
    // from here on *ctx is read
    HIP_TRY(hipSetDevice(ctx->device));
    rio_ctx::Merge& M = ctx->mrg;
    rio_ctx::Flush& F = ctx->fl;
    M.planned = false;
    // the one-table view of the log the gather and the index encode work on, then its bases {0, n}
    constexpr size_t vw = sizeof(rio_sst_view) / 8;
    std::vector<uint64_t> host(vw + 2);
    HIP_TRY(M.views.dev.ensure(host.size() * 8));
    HIP_TRY(M.tmp.ensure(n * 8 + 8));
    HIP_TRY(M.opos.ensure(n * 8 + 8));
    HIP_TRY(M.cub.ensure(std::max<size_t>(scan_cub_bytes(n), 256)));
    HIP_TRY(F.len.ensure(n * 8 + 8));
    HIP_TRY(F.crc.ensure(n * 8 + 8));
    HIP_TRY(F.dig.ensure(2 * n * 8 + 16));
    HIP_TRY(F.perm.ensure(2 * n * 4 + 16));
    HIP_TRY(F.cub.ensure(std::max<size_t>(flush_cub_bytes(n, max_key_len), 256)));
    rio_sst_view v{};
    v.index = ops->keys;
    v.key_off = ops->key_off;
    v.key_len = F.len.as<uint64_t>();
    v.data = ops->values;
    v.data_off = ops->val_off;
    v.flags = ops->flags;
    v.crc = F.crc.as<uint64_t>();
    v.n = n;
    v.index_bytes = ops->key_bytes;
    v.data_bytes = ops->value_bytes;
    memcpy(host.data(), &v, sizeof v);
    host[vw] = 0;
    host[vw + 1] = n;
    hipStream_t s = stream_of(ctx, stream);
    HIP_TRY(M.views.upload(host, s));
    hipEvent_t* ev = nullptr;
    if (!ctx->timing.ring.empty()) {  // rio_ctx_set_timing: stage events (rio_sst_flush_stage_ms)
        while (F.ev.size() < kFlushMaxStages + 1) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            F.ev.push_back(e);
        }
        ev = F.ev.data();
    }
    FlushParams P{};
    P.ops = *ops;
    P.mode = mode;
    P.max_key_len = max_key_len;
    P.key_len = F.len.as<uint64_t>();
    P.crc = F.crc.as<uint64_t>();
    P.dig[0] = F.dig.as<uint64_t>();
    P.dig[1] = P.dig[0] + n + 1;
    P.perm[0] = F.perm.as<uint32_t>();
    P.perm[1] = P.perm[0] + n + 1;
    P.cub = F.cub.p;
    P.cub_bytes = F.cub.cap;
    P.src = d_src;
    P.keep = d_keep;
    P.result = d_result;
    F.stages = 0;
    uint32_t stages = 0;
    HIP_TRY(launch_flush_plan(P, s, ev, &stages, with_crc));
    F.stages = ev ? stages : 0;
    M.T = 1;
    M.N = n;
    M.planned = true;
    return RIO_OK;
}

extern "C" int rio_sst_flush_stage_ms(rio_ctx* ctx, float* ms, int n) {
    if (!ctx || !ms || n <= 0) return 0;
    const rio_ctx::Flush& F = ctx->fl;
    const uint32_t k = std::min<uint32_t>(F.stages, (uint32_t)n);
    if (!k || F.ev.size() < (size_t)F.stages + 1) return 0;
    if (hipEventSynchronize(F.ev[F.stages]) != hipSuccess) return 0;
    for (uint32_t i = 0; i < k; i++)
        if (hipEventElapsedTime(&ms[i], F.ev[i], F.ev[i + 1]) != hipSuccess) return 0;
    return (int)k;
}

// ------------------------------------------------------------------------------------------
// WAL recovery: WalMutation records of decoded WAL files to an op log (rio_walops.hip)
// ------------------------------------------------------------------------------------------
extern "C" int rio_wal_ops_plan(rio_ctx* ctx, const rio_wal_segment* segs, uint32_t n_segs, uint64_t* d_result,
                                void* stream) {
    if (!ctx || !segs || !d_result || n_segs == 0) return RIO_ERR_ARG;
    if (n_segs > RIO_WAL_MAX_SEGMENTS) return RIO_ERR_UNSUPPORTED;
    static_assert(sizeof(rio_wal_segment) % 8 == 0, "segments and bases share one uint64 buffer");
    const size_t sw = sizeof(rio_wal_segment) / 8 * n_segs;
    std::vector<uint64_t> host(sw + n_segs + 1);
    memcpy(host.data(), segs, sw * 8);
    uint64_t N = 0;
    for (uint32_t t = 0; t < n_segs; t++) {
        const rio_wal_segment& g = segs[t];
        if (g.n && (!g.out || !g.out_off || !g.flags)) return RIO_ERR_ARG;
        if (g.n >= (1ull << 31) - 1) return RIO_ERR_UNSUPPORTED;
        host[sw + t] = N;
        N += g.n;
        if (N >= (1ull << 31) - 1) return RIO_ERR_UNSUPPORTED;
    }
    host[sw + n_segs] = N;
    // from here on *ctx is read
    HIP_TRY(hipSetDevice(ctx->device));
    rio_ctx::WalOps& W = ctx->wal;
    W.planned = false;
    // the scratch of both calls, sized here and nowhere later: 8 uint64 arrays of N + 1, the two meta words, and
    // a 32-bit word per record (kind and segment)
    const size_t words = 8 * (N + 1) + 2;
    HIP_TRY(W.segs.dev.ensure(host.size() * 8));
    HIP_TRY(W.scr.ensure(words * 8 + 4 * (N + 1)));
    HIP_TRY(W.cub.ensure(std::max<size_t>(scan_cub_bytes(N), 256)));
    hipStream_t s = stream_of(ctx, stream);
    HIP_TRY(W.segs.upload(host, s));
    WalParams P{};
    P.segs = W.segs.dev.as<rio_wal_segment>();
    P.base = W.segs.dev.as<uint64_t>() + sw;
    P.S = n_segs;
    P.N = N;
    uint64_t* w = W.scr.as<uint64_t>();
    uint64_t** arrays[8] = {&P.koff, &P.voff, &P.klen, &P.vlen, &P.isop, &P.opos, &P.kdst, &P.vdst};
    for (uint64_t** a : arrays) {
        *a = w;
        w += N + 1;
    }
    P.meta = w;
    P.rec = reinterpret_cast<uint32_t*>(w + 2);
    P.result = d_result;
    HIP_TRY(launch_wal_plan(P, W.cub.p, W.cub.cap, s));
    W.P = P;
    W.planned = true;
    return RIO_OK;
}

extern "C" int rio_wal_ops_gather(rio_ctx* ctx, uint64_t n_ops, uint8_t* d_keys, uint64_t keys_cap, uint64_t* d_key_off,
                                  uint8_t* d_values, uint64_t values_cap, uint64_t* d_val_off, uint8_t* d_flags,
                                  uint64_t* d_op_rec, void* stream) {
    if (!ctx || !d_key_off || !d_val_off || (n_ops && (!d_keys || !d_values || !d_flags))) return RIO_ERR_ARG;
    // from here on *ctx is read
    if (!ctx->wal.planned) return RIO_ERR_STATE;
    if (n_ops > ctx->wal.P.N) return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    WalParams P = ctx->wal.P;
    P.result = nullptr;
    P.n_ops = n_ops;
    P.keys = d_keys;
    P.keys_cap = keys_cap;
    P.key_off = d_key_off;
    P.values = d_values;
    P.values_cap = values_cap;
    P.val_off = d_val_off;
    P.flags = d_flags;
    P.op_rec = d_op_rec;
    return hip_status(launch_wal_gather(P, stream_of(ctx, stream)));
}

// ------------------------------------------------------------------------------------------
// batched writes: an op log to WalMutation records (rio_walenc.hip)
// ------------------------------------------------------------------------------------------
extern "C" uint64_t rio_wal_ops_encode_bound(uint64_t n, uint64_t key_bytes, uint64_t value_bytes) {
    // per record: the member's, the key's and the value's tag, and three varints of at most 10 bytes
    return key_bytes + value_bytes + 33 * n;
}

extern "C" int rio_wal_ops_encode(rio_ctx* ctx, const rio_ops_view* ops, uint8_t* d_records, uint64_t records_cap,
                                  uint64_t* d_rec_off, uint64_t* d_result, void* stream) {
    if (!ctx || !ops || !d_rec_off || !d_result || (records_cap && !d_records)) return RIO_ERR_ARG;
    const uint64_t n = ops->n;
    if (n && (!ops->keys || !ops->key_off || !ops->values || !ops->val_off || !ops->flags)) return RIO_ERR_ARG;
    if (n >= (1ull << 31) - 1) return RIO_ERR_UNSUPPORTED;
    // from here on *ctx is read
    HIP_TRY(hipSetDevice(ctx->device));
    rio_ctx::WalEnc& W = ctx->walenc;
    HIP_TRY(W.scr.ensure((n + 1 + 4) * 8));
    HIP_TRY(W.cub.ensure(std::max<size_t>(scan_cub_bytes(n), 256)));
    WalEncParams P{};
    P.ops = *ops;
    P.records = d_records;
    P.records_cap = records_cap;
    P.rec_off = d_rec_off;
    P.meta = W.scr.as<uint64_t>();  // the meta words first: their place does not move with n
    P.len = P.meta + 4;
    P.result = d_result;
    return hip_status(launch_walenc(P, W.cub.p, W.cub.cap, stream_of(ctx, stream)));
}

// ------------------------------------------------------------------------------------------
// sstables: host-memory table handle (the cgo NewSSTableReader binding)
// ------------------------------------------------------------------------------------------
struct rio_sst {
    std::vector<uint8_t> index, data, index_flags, data_flags;
    std::vector<uint64_t> index_off, index_rec_off, data_off, data_rec_off;
    std::vector<uint64_t> key_off, key_len, value_off, checksum, crc;
    std::vector<uint64_t> view;  // v0 tables: DataEntry.value ranges per data record (rio_sst_data_entries)
    bool v0 = false;
    rio_sst_info info{};
};

// rio_frame + rio_decode into host vectors; the device arenas (ctx->host.out, out_off, rec_off) keep
// the decoded file until the next decode on this ctx
static int sst_decode_host(rio_ctx* ctx, const uint8_t* file, uint64_t len, std::vector<uint8_t>& out,
                           std::vector<uint64_t>& off, std::vector<uint64_t>& rec_off, std::vector<uint8_t>& flags,
                           rio_file_info& info) {
    int rc = rio_frame(ctx, file, len, &info);
    if (rc) return rc;
    const uint64_t n = info.n_records;
    out.assign(info.total_out_bytes + 1, 0);
    off.assign(n + 1, 0);
    rec_off.assign(n + 1, 0);
    flags.assign(n + 1, 0);
    rc = rio_decode(ctx, out.data(), info.total_out_bytes, off.data(), rec_off.data(), flags.data(), n, &info);
    if (rc) return rc;
    off.resize(info.n_records + 1);
    return RIO_OK;
}

extern "C" int rio_sst_open(rio_ctx* ctx, const uint8_t* index_file, uint64_t index_len, const uint8_t* data_file,
                            uint64_t data_len, rio_sst** out, rio_sst_info* info) {
    return rio_sst_open_ex(ctx, index_file, index_len, data_file, data_len, 0, out, info);
}

extern "C" int rio_sst_open_ex(rio_ctx* ctx, const uint8_t* index_file, uint64_t index_len, const uint8_t* data_file,
                               uint64_t data_len, uint32_t flags, rio_sst** out, rio_sst_info* info) {
    if (!ctx || !out || !info || (!index_file && index_len) || (!data_file && data_len)) return RIO_ERR_ARG;
    *out = nullptr;
    memset(info, 0, sizeof *info);
    HIP_TRY(hipSetDevice(ctx->device));
    rio_ctx::HostApi& H = ctx->host;
    rio_ctx::Sst& S = ctx->sst;
    auto* t = new rio_sst();
    t->v0 = (flags & RIO_SST_V0_VALUES) != 0;
    rio_sst_info& I = t->info;
    I.first_bad_proto = I.first_bad_crc = I.first_unplaced = I.index_bad = I.first_bad_value = ~0ull;
    int rc = sst_decode_host(ctx, index_file, index_len, t->index, t->index_off, t->index_rec_off, t->index_flags, I.index);
    uint64_t n = 0;
    if (!rc && !nothing_framed(I.index.status)) {
        // the index arena is on the device (H.out / H.out_off): parse it there
        n = I.index.n_records;
        // an index record that does not decompress ends Load's ReadNext loop (slice_key_index.go:
        // 117-126): ErrCorrupt fails the load there, gzip's bare io.EOF ends the index cleanly
        if (I.index.n_bad && I.index.first_bad < n) {
            if (t->index_flags[I.index.first_bad] & RIO_FLAG_CORRUPT) I.index_bad = I.index.first_bad;
            n = I.index.first_bad;
        }
        const uint64_t nn = std::max<uint64_t>(n, 1);
        if (S.fields.ensure(nn * 32) || S.crc.ensure(nn * 8) || S.res.ensure(32)) rc = RIO_ERR_HIP;
        uint64_t* f = S.fields.as<uint64_t>();
        uint64_t* res = S.res.as<uint64_t>();
        if (!rc && launch_sst_index(H.out.as<uint8_t>(), H.out_off.as<uint64_t>(), n, f, f + nn, f + 2 * nn,
                                    f + 3 * nn, res, ctx->stream) != hipSuccess)
            rc = RIO_ERR_HIP;
        t->key_off.assign(nn, 0);
        t->key_len.assign(nn, 0);
        t->value_off.assign(nn, 0);
        t->checksum.assign(nn, 0);
        t->crc.assign(nn, 0);
        std::vector<uint64_t>* dst[4] = {&t->key_off, &t->key_len, &t->value_off, &t->checksum};
        for (int k = 0; k < 4 && !rc; k++)
            rc = d2h_staged(ctx, reinterpret_cast<uint8_t*>(dst[k]->data()), f + k * nn, nn * 8);
        if (!rc) rc = d2h_staged(ctx, reinterpret_cast<uint8_t*>(&I.first_bad_proto), res, 8);
        if (!rc) {
            // key offsets are absolute into the index arena, which t->index mirrors
            rc = sst_decode_host(ctx, data_file, data_len, t->data, t->data_off, t->data_rec_off, t->data_flags, I.data);
        }
        if (!rc && !nothing_framed(I.data.status)) {
            const uint64_t* view = nullptr;
            if (t->v0) {  // DataEntry values: their ranges in the data arena, then hashed as such
                const uint64_t nd = std::max<uint64_t>(I.data.n_records, 1);
                if (S.view.ensure(nd * 16)) rc = RIO_ERR_HIP;
                if (!rc && launch_sst_data_entry(H.out.as<uint8_t>(), H.out_off.as<uint64_t>(), I.data.n_records,
                                                 S.view.as<uint64_t>(), res + 3, ctx->stream) != hipSuccess)
                    rc = RIO_ERR_HIP;
                t->view.assign(2 * nd, 0);
                if (!rc) rc = d2h_staged(ctx, reinterpret_cast<uint8_t*>(t->view.data()), S.view.p, nd * 16);
                if (!rc) rc = d2h_staged(ctx, reinterpret_cast<uint8_t*>(&I.first_bad_value), res + 3, 8);
                view = S.view.as<uint64_t>();
            }
            if (!rc && launch_sst_validate(H.out.as<uint8_t>(), H.out_off.as<uint64_t>(), H.rec_off.as<uint64_t>(),
                                           I.data.n_records, f + 2 * nn, f + 3 * nn, n, S.crc.as<uint64_t>(),
                                           res + 1, ctx->stream, view) != hipSuccess)
                rc = RIO_ERR_HIP;
            if (!rc) rc = d2h_staged(ctx, reinterpret_cast<uint8_t*>(t->crc.data()), S.crc.p, nn * 8);
            uint64_t vr[2] = {~0ull, ~0ull};
            if (!rc) rc = d2h_staged(ctx, reinterpret_cast<uint8_t*>(vr), res + 1, 16);
            I.first_bad_crc = t->v0 ? ~0ull : vr[0];  // validateDataFile returns at once for v0 (:205-209)
            I.first_unplaced = vr[1];
        }
    }
    I.n_entries = n;
    *info = I;
    if (rc) {
        delete t;
        return rc;
    }
    if (I.index.status == RIO_ERR_UNSUPPORTED || I.data.status == RIO_ERR_UNSUPPORTED) {
        delete t;
        return RIO_ERR_UNSUPPORTED;
    }
    *out = t;
    return RIO_OK;
}

extern "C" int rio_sst_entry(const rio_sst* t, uint64_t i, const uint8_t** key, uint64_t* key_len,
                             const uint8_t** value, uint64_t* value_len, int* is_nil, uint64_t* value_offset,
                             uint64_t* checksum, uint64_t* crc) {
    if (!t || i >= t->info.n_entries) return RIO_ERR_ARG;
    if (key) *key = t->index.data() + t->key_off[i];
    if (key_len) *key_len = t->key_len[i];
    if (value_offset) *value_offset = t->value_off[i];
    if (checksum) *checksum = t->checksum[i];
    if (crc) *crc = t->crc[i];
    if (value) *value = nullptr;
    if (value_len) *value_len = 0;
    if (is_nil) *is_nil = 0;
    if (i >= t->info.data.n_records) return t->info.data.status == RIO_OK ? RIO_EOF : t->info.data.status;
    if (t->data_flags[i] & (RIO_FLAG_CORRUPT | RIO_FLAG_EOF))  // the scan's ReadNext error for this value
        return (t->data_flags[i] & RIO_FLAG_EOF) ? RIO_EOF_CODEC : RIO_ERR_DECOMPRESS;
    if (t->v0) {  // DataEntry.value of data record i
        const uint64_t b = t->view[2 * i], e = t->view[2 * i + 1];
        const bool nil = b == RIO_VALUE_NIL || b == RIO_VALUE_BAD;
        if (value) *value = nil ? nullptr : t->data.data() + b;
        if (value_len) *value_len = nil ? 0 : e - b;
        if (is_nil) *is_nil = b == RIO_VALUE_NIL ? 1 : 0;
        return b == RIO_VALUE_BAD ? RIO_ERR_PROTO : RIO_OK;
    }
    const bool nil = (t->data_flags[i] & RIO_FLAG_NIL) != 0;
    if (value) *value = nil ? nullptr : t->data.data() + t->data_off[i];
    if (value_len) *value_len = t->data_off[i + 1] - t->data_off[i];
    if (is_nil) *is_nil = nil ? 1 : 0;
    return RIO_OK;
}

extern "C" void rio_sst_free(rio_sst* t) { delete t; }
