// rio_super.cpp — the entry points of a stack of loaded tables (include/rio.h: rio_sst_stack_*, rio_stack.hip)
// and rio_sst_keys_gather.
//
// As in rio_tables.cpp, all argument checks stand before the first read of *ctx or of the stack's device state:
// a call refused on its arguments touches neither (tests/test_super_host.py makes such calls on a machine
// without a GPU). After rio_sst_stack_create nothing here allocates, waits for the device or hands a host array
// to an asynchronous copy: the launch parameters travel by value.
#include <cstring>

#include "rio_ctx.h"

using namespace rio;

namespace {

hipStream_t stream_of(const rio_sst_stack* st, void* stream) {
    return stream ? static_cast<hipStream_t>(stream) : st->stream;
}

StackParams keys_params(const rio_sst_stack* st, const uint8_t* d_keys, const uint64_t* d_key_off, uint64_t n,
                        uint64_t key_bytes) {
    StackParams P = st->P;
    P.keys = d_keys;
    P.key_off = d_key_off;
    P.n = n;
    P.key_bytes = key_bytes;
    return P;
}

}  // namespace

extern "C" int rio_sst_stack_create(rio_ctx* ctx, const rio_sst_view* views, const uint64_t* const* d_pfx,
                                    const rio_bloom_view* filters, const uint64_t* const* d_stored_checksum,
                                    uint32_t n_tables, uint64_t max_batch, rio_sst_stack** out, void* stream) {
    if (!ctx || !views || !d_pfx || !out || n_tables == 0 || n_tables > RIO_MERGE_MAX_TABLES || max_batch == 0)
        return RIO_ERR_ARG;
    *out = nullptr;
    static_assert(sizeof(rio_sst_view) % 8 == 0 && sizeof(rio_bloom_view) % 8 == 0, "the tables share one uint64 buffer");
    constexpr size_t vw = sizeof(rio_sst_view) / 8, fw = sizeof(rio_bloom_view) / 8;
    const size_t T = n_tables;
    std::vector<uint64_t> host(T * (vw + fw + 2), 0);
    uint64_t* h_views = host.data();
    uint64_t* h_pfx = h_views + T * vw;
    uint64_t* h_flt = h_pfx + T;
    uint64_t* h_stored = h_flt + T * fw;
    for (uint32_t t = 0; t < n_tables; t++) {
        const rio_sst_view& v = views[t];
        if (v.n && (!d_pfx[t] || !v.index || !v.key_off || !v.key_len || !v.data_off || !v.flags || !v.crc))
            return RIO_ERR_ARG;
        if (v.n >> RIO_MERGE_ENTRY_BITS) return RIO_ERR_UNSUPPORTED;
        if (filters && filters[t].bits) {
            const rio_bloom_view& f = filters[t];
            if (f.k < 1 || f.k > RIO_BLOOM_MAX_K || f.m < 2 || !f.hash_keys) return RIO_ERR_ARG;
            memcpy(h_flt + t * fw, &f, sizeof f);
        }
        memcpy(h_views + t * vw, &v, sizeof v);
        h_pfx[t] = reinterpret_cast<uint64_t>(d_pfx[t]);
        h_stored[t] = d_stored_checksum ? reinterpret_cast<uint64_t>(d_stored_checksum[t]) : 0;
    }
    if (max_batch >= (1ull << 31) - 1) return RIO_ERR_UNSUPPORTED;
    // from here on *ctx is read
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<rio_sst_stack> st(new rio_sst_stack());
    st->device = ctx->device;
    st->stream = ctx->stream;
    st->T = n_tables;
    st->max_batch = max_batch;
    HIP_TRY(st->tables.ensure(host.size() * 8));
    HIP_TRY(st->tmp.ensure(max_batch * 8 + 8));
    HIP_TRY(st->cub.ensure(std::max<size_t>(scan_cub_bytes(max_batch), 256)));
    hipStream_t s = rio::stream_of(ctx, stream);
    HIP_TRY(hipMemcpyAsync(st->tables.p, host.data(), host.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // `host` is read by that copy; the only wait of the stack's life
    uint64_t* d = st->tables.as<uint64_t>();
    st->P.views = reinterpret_cast<const rio_sst_view*>(d);
    st->P.pfx = reinterpret_cast<const uint64_t* const*>(d + T * vw);
    st->P.filters = reinterpret_cast<const rio_bloom_view*>(d + T * vw + T);
    st->P.stored = reinterpret_cast<const uint64_t* const*>(d + T * (vw + fw) + T);
    st->P.T = n_tables;
    st->P.tmp = st->tmp.as<uint64_t>();
    *out = st.release();
    return RIO_OK;
}

extern "C" void rio_sst_stack_free(rio_sst_stack* stack) {
    if (!stack) return;
    hipSetDevice(stack->device);
    delete stack;
}

extern "C" int rio_sst_stack_lookup(rio_sst_stack* stack, uint32_t gated, const uint8_t* d_keys,
                                    const uint64_t* d_key_off, uint64_t n, uint64_t key_bytes, uint64_t* d_src,
                                    void* stream) {
    if (!stack || gated > 1) return RIO_ERR_ARG;
    if (n && (!d_keys || !d_key_off || !d_src)) return RIO_ERR_ARG;
    // from here on *stack is read
    if (n > stack->max_batch) return RIO_ERR_ARG;
    if (n == 0) return RIO_OK;
    HIP_TRY(hipSetDevice(stack->device));
    StackParams P = keys_params(stack, d_keys, d_key_off, n, key_bytes);
    P.flag = gated;
    P.src = d_src;
    return hip_status(launch_stack_lookup(P, stream_of(stack, stream)));
}

extern "C" int rio_sst_stack_value_plan(rio_sst_stack* stack, const uint64_t* d_src, uint64_t n, uint32_t check_crc,
                                        uint8_t* d_status, uint64_t* d_val_off, void* stream) {
    if (!stack || !d_val_off || (n && (!d_src || !d_status))) return RIO_ERR_ARG;
    // from here on *stack is read
    if (n > stack->max_batch) return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(stack->device));
    StackParams P = stack->P;
    P.flag = check_crc ? 1 : 0;
    P.n = n;
    P.src = const_cast<uint64_t*>(d_src);
    P.status = d_status;
    P.val_off = d_val_off;
    return hip_status(launch_stack_value_plan(P, stack->cub.p, stack->cub.cap, stream_of(stack, stream)));
}

extern "C" int rio_sst_stack_value_copy(rio_sst_stack* stack, const uint64_t* d_src, uint64_t n,
                                        const uint64_t* d_val_off, uint8_t* d_values, uint64_t values_cap,
                                        void* stream) {
    if (!stack || (n && (!d_src || !d_val_off || !d_values))) return RIO_ERR_ARG;
    // from here on *stack is read
    if (n > stack->max_batch) return RIO_ERR_ARG;
    if (n == 0) return RIO_OK;
    HIP_TRY(hipSetDevice(stack->device));
    StackParams P = stack->P;
    P.n = n;
    P.src = const_cast<uint64_t*>(d_src);
    P.val_off = const_cast<uint64_t*>(d_val_off);
    P.values = d_values;
    P.values_cap = values_cap;
    return hip_status(launch_stack_value_copy(P, stream_of(stack, stream)));
}

extern "C" int rio_sst_stack_bounds(rio_sst_stack* stack, const uint8_t* d_keys, const uint64_t* d_key_off,
                                    uint64_t n_keys, uint64_t key_bytes, uint32_t upper, uint64_t* d_pos, void* stream) {
    if (!stack || upper > 1) return RIO_ERR_ARG;
    if (n_keys && (!d_keys || !d_key_off || !d_pos)) return RIO_ERR_ARG;
    if (n_keys >= (1ull << 31) - 1) return RIO_ERR_UNSUPPORTED;
    if (n_keys == 0) return RIO_OK;
    // from here on *stack is read
    HIP_TRY(hipSetDevice(stack->device));
    StackParams P = keys_params(stack, d_keys, d_key_off, n_keys, key_bytes);
    P.flag = upper;
    P.pos = d_pos;
    return hip_status(launch_stack_bounds(P, stream_of(stack, stream)));
}

extern "C" int rio_sst_keys_gather(rio_ctx* ctx, const uint64_t* d_out_src, uint64_t n_out, uint8_t* d_keys,
                                   uint64_t keys_cap, uint64_t* d_key_off, void* stream) {
    if (!ctx || !d_key_off || (n_out && (!d_out_src || !d_keys))) return RIO_ERR_ARG;
    // from here on *ctx is read
    const rio_ctx::Merge& M = ctx->mrg;
    if (!M.planned) return RIO_ERR_STATE;
    if (n_out > M.N) return RIO_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    KeysParams P{};
    P.views = M.views.dev.as<rio_sst_view>();
    P.T = M.T;
    P.n_out = n_out;
    P.out_src = d_out_src;
    P.tmp = M.tmp.as<uint64_t>();
    P.keys = d_keys;
    P.keys_cap = keys_cap;
    P.key_off = d_key_off;
    return hip_status(launch_keys_gather(P, M.cub.p, M.cub.cap, rio::stream_of(ctx, stream)));
}
