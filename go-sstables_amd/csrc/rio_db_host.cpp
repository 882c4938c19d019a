// rio_db_host.cpp — the entry points of the memstore index and of the combined read (include/rio.h: rio_mem_index_build,
// rio_mem_index_extend, rio_ops_append, rio_mem_lookup, rio_mem_size_scan, rio_db_*; kernels in rio_memidx.hip,
// rio_memsize.hip and rio_db.hip).
//
// As in rio_super.cpp, all argument checks stand before the first read of *ctx, *reader or of any device state: a
// call refused on its arguments touches none (tests/test_db_get_host.py makes such calls on a machine without a
// GPU). rio_mem_index_build, rio_mem_index_extend and rio_mem_size_scan size their scratch in the call, as the plan
// they run does; rio_ops_append allocates nothing; after rio_db_reader_create no reader call allocates, waits for the device or hands a host array to an asynchronous copy, and rio_mem_lookup
// never does: the launch parameters travel by value.
#include <cstring>

#include "rio_ctx.h"

using namespace rio;

struct rio_db_reader {
    int device = 0;
    hipStream_t stream = nullptr;  // the creating context's, for calls with a NULL stream
    uint64_t max_batch = 0;
    DevBuf tmp, cub;               // scan input; scan temp
    // the stack's tables (T = 0 without a stack)
    const rio_sst_view* views = nullptr;
    const uint64_t* const* stored = nullptr;
    uint32_t T = 0;
};

namespace {

// RIO_OK, or why idx[0 .. n_idx) cannot be searched; reads nothing on the device
int check_indexes(const rio_mem_index* idx, uint32_t n_idx) {
    if (!idx || n_idx == 0 || n_idx > RIO_DB_MAX_MEMSTORES) return RIO_ERR_ARG;
    for (uint32_t s = 0; s < n_idx; s++) {
        const rio_mem_index& I = idx[s];
        if (!I.result) return RIO_ERR_ARG;
        if (I.ops.n && (!I.order || !I.pfx || !I.ops.keys || !I.ops.key_off || !I.ops.values || !I.ops.val_off || !I.ops.flags))
            return RIO_ERR_ARG;
        if (I.ops.n >> RIO_MERGE_ENTRY_BITS) return RIO_ERR_UNSUPPORTED;
    }
    return RIO_OK;
}

DbParams db_params(const rio_db_reader* r, const rio_mem_index* idx, uint32_t n_idx, const uint64_t* d_tab_src,
                   const uint64_t* d_mem_src, uint64_t n) {
    DbParams P{};
    P.i0 = idx[0];
    P.i1 = idx[n_idx > 1 ? 1 : 0];
    P.n_idx = n_idx;
    P.views = r->views;
    P.stored = r->stored;
    P.T = r->T;
    P.tab_src = d_tab_src;
    P.mem_src = d_mem_src;
    P.n = n;
    P.tmp = r->tmp.as<uint64_t>();
    return P;
}

hipStream_t stream_of(const rio_db_reader* r, void* stream) {
    return stream ? static_cast<hipStream_t>(stream) : r->stream;
}

}  // namespace

extern "C" int rio_mem_index_build(rio_ctx* ctx, const rio_ops_view* ops, uint32_t max_key_len, uint64_t* d_order,
                                   uint64_t* d_pfx, uint64_t* d_result, void* stream) {
    if (!ctx || !ops || !d_result) return RIO_ERR_ARG;
    const uint64_t n = ops->n;
    if (n && (!ops->keys || !ops->key_off || !ops->values || !ops->val_off || !ops->flags || !d_order || !d_pfx))
        return RIO_ERR_ARG;
    if (n >= (1ull << 31) - 1 || max_key_len > RIO_FLUSH_MAX_KEY_LEN) return RIO_ERR_UNSUPPORTED;
    // from here on *ctx is read
    HIP_TRY(hipSetDevice(ctx->device));
    rio_ctx::MemIndex& X = ctx->mem;
    HIP_TRY(X.src.ensure(n * 8 + 8));
    HIP_TRY(X.keep.ensure(n + 8));
    HIP_TRY(X.n_sel.ensure(8));
    HIP_TRY(X.cub.ensure(std::max<size_t>(mem_index_cub_bytes(n), 256)));
    const int rc = flush_plan(ctx, ops, RIO_FLUSH_WITH_TOMBSTONES, max_key_len, X.src.as<uint64_t>(), X.keep.as<uint8_t>(),
                              d_result, stream, false);
    // the plan's view has no checksums and its order lives in this call's scratch: no gather may follow it
    ctx->mrg.planned = false;
    if (rc != RIO_OK || n == 0) return rc;
    MemBuildParams P{};
    P.ops = *ops;
    P.src = X.src.as<uint64_t>();
    P.keep = X.keep.as<uint8_t>();
    P.order = d_order;
    P.pfx = d_pfx;
    P.n_sel = X.n_sel.as<uint64_t>();
    P.result = d_result;
    return hip_status(launch_mem_index(P, X.cub.p, X.cub.cap, rio::stream_of(ctx, stream)));
}

extern "C" int rio_mem_index_extend(rio_ctx* ctx, const rio_ops_view* ops, uint64_t n_old, uint32_t max_key_len,
                                    uint64_t* d_order, uint64_t* d_pfx, uint64_t* d_result, void* stream) {
    if (!ctx || !ops || !d_result) return RIO_ERR_ARG;
    const uint64_t n = ops->n;
    if (n_old > n) return RIO_ERR_ARG;
    if (n && (!ops->keys || !ops->key_off || !ops->values || !ops->val_off || !ops->flags || !d_order || !d_pfx))
        return RIO_ERR_ARG;
    if (n >= (1ull << 31) - 1 || max_key_len > RIO_FLUSH_MAX_KEY_LEN) return RIO_ERR_UNSUPPORTED;
    if (n_old == n) return RIO_OK;
    if (n_old == 0) return rio_mem_index_build(ctx, ops, max_key_len, d_order, d_pfx, d_result, stream);
    // from here on *ctx is read
    HIP_TRY(hipSetDevice(ctx->device));
    const uint64_t t = n - n_old;
    rio_ctx::MemIndex& X = ctx->mem;
    HIP_TRY(X.src.ensure(t * 8 + 8));
    HIP_TRY(X.keep.ensure(t + 8));
    HIP_TRY(X.n_sel.ensure(8));
    HIP_TRY(X.cub.ensure(std::max<size_t>(mem_extend_cub_bytes(t), 256)));
    // ext: the tail's order and prefixes (t words each), lb, eq and e (t + 1 each), its result block, the drop sums
    HIP_TRY(X.ext.ensure((5 * t + 3 + RIO_MERGE_RESULT_WORDS + 4) * 8));
    HIP_TRY(X.merged.ensure(2 * n * 8));
    uint64_t* w = X.ext.as<uint64_t>();
    uint64_t* b_order = w;
    uint64_t* b_pfx = b_order + t;
    uint64_t* lb = b_pfx + t;
    uint64_t* eq = lb + t + 1;
    uint64_t* e = eq + t + 1;
    uint64_t* b_result = e + t + 1;
    uint64_t* drop = b_result + RIO_MERGE_RESULT_WORDS;
    // the tail as a log of its own: the offsets are absolute, the arenas the same
    rio_ops_view tail = *ops;
    tail.key_off += n_old;
    tail.val_off += n_old;
    tail.flags += n_old;
    tail.n = t;
    const int rc = flush_plan(ctx, &tail, RIO_FLUSH_WITH_TOMBSTONES, max_key_len, X.src.as<uint64_t>(), X.keep.as<uint8_t>(),
                              b_result, stream, false);
    ctx->mrg.planned = false;  // as the build: no gather may follow this plan
    if (rc != RIO_OK) return rc;
    hipStream_t s = rio::stream_of(ctx, stream);
    MemBuildParams B{};
    B.ops = tail;
    B.src = X.src.as<uint64_t>();
    B.keep = X.keep.as<uint8_t>();
    B.order = b_order;
    B.pfx = b_pfx;
    B.n_sel = X.n_sel.as<uint64_t>();
    B.result = b_result;
    HIP_TRY(launch_mem_index(B, X.cub.p, X.cub.cap, s));
    MemExtendParams P{};
    P.ops = *ops;
    P.n_old = n_old;
    P.t = t;
    P.order = d_order;
    P.pfx = d_pfx;
    P.result = d_result;
    P.b_order = b_order;
    P.b_pfx = b_pfx;
    P.b_result = b_result;
    P.lb = lb;
    P.eq = eq;
    P.e = e;
    P.m_order = X.merged.as<uint64_t>();
    P.m_pfx = P.m_order + n;
    P.drop = drop;
    return hip_status(launch_mem_extend(P, X.cub.p, X.cub.cap, s));
}

extern "C" int rio_ops_append(rio_ctx* ctx, const rio_ops_view* log, uint64_t ops_cap, uint64_t keys_cap, uint64_t values_cap,
                              const rio_ops_view* batch, void* stream) {
    if (!ctx || !log || !batch) return RIO_ERR_ARG;
    const uint64_t n = batch->n;
    if (n == 0) return RIO_OK;
    if (!batch->keys || !batch->key_off || !batch->values || !batch->val_off || !batch->flags || !log->keys || !log->key_off ||
        !log->values || !log->val_off || !log->flags)
        return RIO_ERR_ARG;
    // each sum is checked against a capacity before it can wrap
    if (log->n > ops_cap || n > ops_cap - log->n) return RIO_ERR_ARG;
    if (keys_cap < RIO_DEVICE_PAD || log->key_bytes > keys_cap - RIO_DEVICE_PAD ||
        batch->key_bytes > keys_cap - RIO_DEVICE_PAD - log->key_bytes)
        return RIO_ERR_ARG;
    if (values_cap < RIO_DEVICE_PAD || log->value_bytes > values_cap - RIO_DEVICE_PAD ||
        batch->value_bytes > values_cap - RIO_DEVICE_PAD - log->value_bytes)
        return RIO_ERR_ARG;
    if (log->n + n >= (1ull << 31) - 1) return RIO_ERR_UNSUPPORTED;
    // from here on *ctx is read
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = rio::stream_of(ctx, stream);
    if (batch->key_bytes)
        HIP_TRY(hipMemcpyAsync(const_cast<uint8_t*>(log->keys) + log->key_bytes, batch->keys, batch->key_bytes,
                               hipMemcpyDeviceToDevice, s));
    if (batch->value_bytes)
        HIP_TRY(hipMemcpyAsync(const_cast<uint8_t*>(log->values) + log->value_bytes, batch->values, batch->value_bytes,
                               hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(const_cast<uint8_t*>(log->flags) + log->n, batch->flags, n, hipMemcpyDeviceToDevice, s));
    OpsRebaseParams P{};
    P.key_off = const_cast<uint64_t*>(log->key_off);
    P.val_off = const_cast<uint64_t*>(log->val_off);
    P.b_key_off = batch->key_off;
    P.b_val_off = batch->val_off;
    P.log_n = log->n;
    P.n = n;
    P.log_key_bytes = log->key_bytes;
    P.log_value_bytes = log->value_bytes;
    P.b_key_bytes = batch->key_bytes;
    P.b_value_bytes = batch->value_bytes;
    return hip_status(launch_ops_rebase(P, s));
}

extern "C" int rio_mem_lookup(rio_ctx* ctx, const rio_mem_index* idx, uint32_t n_idx, const uint8_t* d_keys,
                              const uint64_t* d_key_off, uint64_t n, uint64_t key_bytes, uint64_t* d_mem_src,
                              void* stream) {
    if (!ctx) return RIO_ERR_ARG;
    const int rc = check_indexes(idx, n_idx);
    if (rc != RIO_OK) return rc;
    if (n && (!d_keys || !d_key_off || !d_mem_src)) return RIO_ERR_ARG;
    if (n >= (1ull << 31) - 1) return RIO_ERR_UNSUPPORTED;
    if (n == 0) return RIO_OK;
    // from here on *ctx is read
    HIP_TRY(hipSetDevice(ctx->device));
    MemLookupParams P{};
    P.i0 = idx[0];
    P.i1 = idx[n_idx > 1 ? 1 : 0];
    P.n_idx = n_idx;
    P.keys = d_keys;
    P.key_off = d_key_off;
    P.n = n;
    P.key_bytes = key_bytes;
    P.src = d_mem_src;
    return hip_status(launch_mem_lookup(P, rio::stream_of(ctx, stream)));
}

extern "C" int rio_mem_size_scan(rio_ctx* ctx, const rio_mem_index* store, uint64_t size0, const rio_ops_view* batch,
                                 uint32_t max_key_len, uint64_t max_size, uint64_t* d_size, uint64_t* d_result,
                                 void* stream) {
    if (!ctx || !batch || !d_result) return RIO_ERR_ARG;
    const uint64_t n = batch->n;
    if (n && (!batch->keys || !batch->key_off || !batch->values || !batch->val_off || !batch->flags || !d_size))
        return RIO_ERR_ARG;
    if (store) {
        const int rc = check_indexes(store, 1);
        if (rc != RIO_OK) return rc;
    }
    if (n >= (1ull << 31) - 1 || max_key_len > RIO_FLUSH_MAX_KEY_LEN) return RIO_ERR_UNSUPPORTED;
    // from here on *ctx is read
    HIP_TRY(hipSetDevice(ctx->device));
    MemSizeParams P{};
    if (store) P.store = *store;  // else ops.n = 0: an empty store
    P.batch = *batch;
    P.size0 = size0;
    P.max_size = max_size;
    P.size = d_size;
    P.result = d_result;
    rio_ctx::MemIndex& X = ctx->mem;
    if (n) {
        HIP_TRY(X.src.ensure(n * 8 + 8));
        HIP_TRY(X.keep.ensure(n + 8));
        // size: the deltas (n words), the cut word, the batch plan's result block
        HIP_TRY(X.size.ensure((n + 1 + RIO_MERGE_RESULT_WORDS) * 8));
        HIP_TRY(X.cub.ensure(std::max<size_t>(mem_size_cub_bytes(n), 256)));
        P.src = X.src.as<uint64_t>();
        P.keep = X.keep.as<uint8_t>();
        P.delta = X.size.as<uint64_t>();
        P.cut = P.delta + n;
        uint64_t* plan = P.cut + 1;
        P.plan = plan;
        const int rc = flush_plan(ctx, batch, RIO_FLUSH_WITH_TOMBSTONES, max_key_len, X.src.as<uint64_t>(), X.keep.as<uint8_t>(),
                                  plan, stream, false);
        if (rc != RIO_OK) return rc;
    }
    ctx->mrg.planned = false;  // as the index build: no gather may follow this plan
    return hip_status(launch_mem_size(P, X.cub.p, X.cub.cap, rio::stream_of(ctx, stream)));
}

extern "C" int rio_db_reader_create(rio_ctx* ctx, rio_sst_stack* stack, uint64_t max_batch, rio_db_reader** out) {
    if (!ctx || !out || max_batch == 0) return RIO_ERR_ARG;
    *out = nullptr;
    if (max_batch >= (1ull << 31) - 1) return RIO_ERR_UNSUPPORTED;
    // from here on *ctx and *stack are read
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<rio_db_reader> r(new rio_db_reader());
    r->device = ctx->device;
    r->stream = ctx->stream;
    r->max_batch = max_batch;
    if (stack) {
        if (stack->device != ctx->device) return RIO_ERR_ARG;
        r->views = stack->P.views;
        r->stored = stack->P.stored;
        r->T = stack->P.T;
    }
    HIP_TRY(r->tmp.ensure(max_batch * 8 + 8));
    HIP_TRY(r->cub.ensure(std::max<size_t>(scan_cub_bytes(max_batch), 256)));
    *out = r.release();
    return RIO_OK;
}

extern "C" void rio_db_reader_free(rio_db_reader* reader) {
    if (!reader) return;
    hipSetDevice(reader->device);
    delete reader;
}

extern "C" int rio_db_value_plan(rio_db_reader* reader, const rio_mem_index* idx, uint32_t n_idx, const uint64_t* d_tab_src,
                                 const uint64_t* d_mem_src, uint64_t n, uint32_t check_crc, uint8_t* d_status,
                                 uint64_t* d_val_off, void* stream) {
    if (!reader || !d_val_off) return RIO_ERR_ARG;
    const int rc = check_indexes(idx, n_idx);
    if (rc != RIO_OK) return rc;
    if (n && (!d_mem_src || !d_status)) return RIO_ERR_ARG;
    // from here on *reader is read
    if (n > reader->max_batch || (d_tab_src && !reader->T)) return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(reader->device));
    DbParams P = db_params(reader, idx, n_idx, d_tab_src, d_mem_src, n);
    P.check_crc = check_crc ? 1 : 0;
    P.status = d_status;
    P.val_off = d_val_off;
    return hip_status(launch_db_value_plan(P, reader->cub.p, reader->cub.cap, stream_of(reader, stream)));
}

extern "C" int rio_db_value_copy(rio_db_reader* reader, const rio_mem_index* idx, uint32_t n_idx, const uint64_t* d_tab_src,
                                 const uint64_t* d_mem_src, const uint8_t* d_status, uint64_t n, const uint64_t* d_val_off,
                                 uint8_t* d_values, uint64_t values_cap, void* stream) {
    if (!reader) return RIO_ERR_ARG;
    const int rc = check_indexes(idx, n_idx);
    if (rc != RIO_OK) return rc;
    if (n && (!d_mem_src || !d_status || !d_val_off || !d_values)) return RIO_ERR_ARG;
    // from here on *reader is read
    if (n > reader->max_batch || (d_tab_src && !reader->T)) return RIO_ERR_ARG;
    if (n == 0) return RIO_OK;
    HIP_TRY(hipSetDevice(reader->device));
    DbParams P = db_params(reader, idx, n_idx, d_tab_src, d_mem_src, n);
    P.status = const_cast<uint8_t*>(d_status);
    P.val_off = const_cast<uint64_t*>(d_val_off);
    P.values = d_values;
    P.values_cap = values_cap;
    return hip_status(launch_db_value_copy(P, stream_of(reader, stream)));
}
