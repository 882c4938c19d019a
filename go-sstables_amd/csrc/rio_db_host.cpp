// rio_db_host.cpp — the entry points of the memstore index and of the combined read (include/rio.h: rio_mem_index_build,
// rio_mem_lookup, rio_db_*; kernels in rio_memidx.hip and rio_db.hip).
//
// As in rio_super.cpp, all argument checks stand before the first read of *ctx, *reader or of any device state: a
// call refused on its arguments touches none (tests/test_db_get_host.py makes such calls on a machine without a
// GPU). rio_mem_index_build sizes its scratch in the call, as the plan it runs does; after rio_db_reader_create no
// reader call allocates, waits for the device or hands a host array to an asynchronous copy, and rio_mem_lookup
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
    HIP_TRY(r->cub.ensure(std::max<size_t>(db_cub_bytes(max_batch), 256)));
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
